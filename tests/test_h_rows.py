"""The zeroed LSTM output rows a recurrence plan keeps (nnet/_plans.py: _h_rows), on the CPU: the buffer protocol needs
`torch.zeros` only.

The contract: when a run has written its frames into the rows _h_rows handed it, every other frame of those rows is exactly
zero, whoever wrote in between -- an eager call, which asks _h_rows again, or a replay of a captured graph, which writes
through the address it was handed at capture time and asks nobody.  A run is stood in for by writing a
non-zero value into the frames its walk covers (graph_interleave_cases.written_frames), a capture by keeping what _h_rows
returned, a replay by writing into that.

The sequences are those of the two defects the contract was fixed for: (A) capture short, run long, replay short -- the
clear of the kept buffer was a host-side action that no capture records; (B) run short, replay long, run short -- the host's
record of the last geometry does not learn of a replay.  On the code before the fix both fail at the step named in the
assertion message."""
import itertools

import pytest
import torch

import graph_interleave_cases as G
from puresound_amd.nnet import _plans

LD = 128
F = 3                                        # rows of the 2-D map: F rows of LD frames, pad frames between them
SHORT, LONG, OTHER = 3, 127, 100             # utterance lengths inside one 128-frame row


def _geometry(t, pass_="intra"):
    """DPRNNblock2D.forward_padded's two walks over F rows of LD frames that hold t frames each -> (frames, walk)"""
    frames = (F - 1) * LD + t
    return (frames, (t, 1, F, LD)) if pass_ == "intra" else (frames, (F, LD, t, 1))


class _Plan:
    """A recurrence plan and the stand-ins for what runs on it."""

    def __init__(self, n=2, hidden=4, dirs=1):
        self.rnn = dict(D=dirs, H=hidden)
        self.x = torch.zeros(n, 5, F * LD)
        self.count = itertools.count(1)

    def ask(self, t, pass_="intra", lane=0):
        frames, walk = _geometry(t, pass_)
        buf = _plans._h_rows(self.rnn, self.x, frames, *walk, lane)
        assert buf is not None and buf.shape == (self.x.shape[0], self.rnn["D"] * self.rnn["H"], F * LD)
        return walk, buf

    @staticmethod
    def write(walk, buf, value):
        buf[..., torch.tensor(G.written_frames(walk))] = float(value)

    def ran(self, what, walk, buf):
        """A run wrote its frames: what follows it reads the whole span."""
        self.write(walk, buf, next(self.count))
        ok, bad = G.pad_frames_are_zero(buf, walk)
        assert ok, f"{what}: {bad} values in the pad frames of its LSTM output rows are not zero"

    def eager(self, t, pass_="intra", lane=0, what=None):
        walk, buf = self.ask(t, pass_, lane)
        self.ran(what or f"eager call at T = {t}", walk, buf)
        return walk, buf

    def capture(self, t, pass_="intra", lane=0, warmups=3):
        """graphs.capture: the warm-ups run, the capture only records -> the graph (what a replay writes, and where)"""
        for _ in range(warmups):
            self.eager(t, pass_, lane, what=f"warm-up at T = {t}")
        return self.ask(t, pass_, lane)

    def replay(self, graph, what):
        self.ran(what, *graph)


def test_every_frame_written_needs_no_kept_rows():
    p = _Plan()
    assert _plans._h_rows(p.rnn, p.x, F * LD, LD, 1, F, LD) is None          # q * steps covers the span
    assert "h_rows" not in p.rnn


def test_written_frames_are_the_walks_of_the_two_passes():
    for t in (1, SHORT, LONG):
        want = sorted(f * LD + i for f in range(F) for i in range(t))
        assert G.written_frames(_geometry(t, "intra")[1]) == want
        assert G.written_frames(_geometry(t, "inter")[1]) == want
        assert max(want) < _geometry(t)[0] and len(want) < _geometry(t)[0]   # pad frames inside the span


@pytest.mark.parametrize("pass_", ["intra", "inter"])
@pytest.mark.parametrize("longer", ["eager", "capture"])
def test_defect_a_replay_of_the_short_graph_behind_a_longer_call(pass_, longer):
    p = _Plan()
    short = p.capture(SHORT, pass_)
    p.replay(short, "first replay of the short graph")
    if longer == "eager":
        p.eager(LONG, pass_)
    else:
        p.replay(p.capture(LONG, pass_), "first replay of the long graph")
    p.replay(short, f"replay of the short graph behind the longer {longer} call")


@pytest.mark.parametrize("pass_", ["intra", "inter"])
def test_defect_b_eager_call_behind_a_replay_the_host_never_saw(pass_):
    p = _Plan()
    long_ = p.capture(LONG, pass_)
    p.replay(long_, "first replay of the long graph")
    p.eager(SHORT, pass_)
    p.replay(long_, "replay of the long graph behind the short eager call")
    p.eager(SHORT, pass_, what="short eager call directly behind the long graph's replay")


def test_the_schedule_of_the_gpu_test_on_the_buffer_protocol():
    """graph_interleave_cases.PART_A with lengths standing for the shapes; `c` is a third length inside the same row here (on
    the GPU it is another row length, which shares no buffer with `a` and `b`: the easier case)."""
    p, other = _Plan(n=2), _Plan(n=1)
    other.rnn = p.rnn
    graphs = {}
    for i, (kind, shape, _) in enumerate(G.PART_A):
        if kind == "churn":
            continue
        plan = other if shape == "b1" else p
        t = {"a": SHORT, "b": LONG, "b1": LONG, "c": OTHER}[shape]
        if kind == "eager":
            plan.eager(t, what=G.describe(i))
        else:
            if shape not in graphs:
                graphs[shape] = plan.capture(t)
            plan.replay(graphs[shape], G.describe(i))


def test_lanes_and_batches_keep_rows_of_their_own():
    p = _Plan()
    _, a = p.eager(SHORT, lane=0)
    _, b = p.eager(SHORT, lane=1)
    assert a.data_ptr() != b.data_ptr()
    assert p.ask(SHORT, lane=0)[1] is a and p.ask(SHORT, lane=1)[1] is b      # kept from call to call
    q = _Plan(n=3)
    q.rnn = p.rnn
    _, c = q.eager(SHORT)
    assert c.shape[0] == 3 and c is not a
    assert p.ask(SHORT, lane=0)[1] is a


def test_a_dropped_buffer_is_never_handed_out_again_and_every_kept_one_is_listed():
    """More geometries than a lane keeps: the oldest leaves the plan, and the graph that pinned it keeps writing rows that
    nobody else is handed.  (_tensors_in is what PlanCache.cached_tensors, and so a capture's pin, walks a plan with.)"""
    def listed():
        kept = []
        _plans._tensors_in(p.rnn, set(), kept)
        return kept

    p = _Plan()
    pinned = p.capture(SHORT)
    assert any(k is pinned[1] for k in listed())
    for t in range(10, 10 + _plans.H_ROWS_KEPT):
        _, buf = p.eager(t)
        assert len(listed()) <= _plans.H_ROWS_KEPT and any(k is buf for k in listed())
    assert not any(k is pinned[1] for k in listed())
    p.replay(pinned, "replay of a graph whose rows have left the plan")
    _, again = p.eager(SHORT)
    assert again is not pinned[1]
    assert [g for _, g, _ in G.kept_rows({"plan": p.rnn})][-1] == (_geometry(SHORT)[0],) + _geometry(SHORT)[1]
    for t in range(10 + _plans.H_ROWS_KEPT - 1, 9, -1):                       # and the others once more, newest first
        p.eager(t)
    p.replay(pinned, "replay of the pinned graph at the end")


def test_large_rows_stay_under_the_byte_budget(monkeypatch):
    """Rows of a full batch are past a gigabyte each: beside the buffer in use a lane keeps only what fits H_ROWS_BYTES, so at
    such shapes it holds one buffer, as before, and a pinned one still keeps its zeros."""
    p = _Plan()
    one = 4 * p.x.shape[0] * p.rnn["D"] * p.rnn["H"] * F * LD
    monkeypatch.setattr(_plans, "H_ROWS_BYTES", 2 * one)
    pinned = p.capture(SHORT)
    _, b = p.eager(LONG)
    assert p.ask(SHORT)[1] is pinned[1] and p.ask(LONG)[1] is b               # two fit
    _, c = p.eager(OTHER)
    kept = [buf for _, _, buf in G.kept_rows({"plan": p.rnn})]
    assert len(kept) == 2 and kept[-1] is c and not any(k is pinned[1] for k in kept)
    monkeypatch.setattr(_plans, "H_ROWS_BYTES", one // 2)                       # less than one buffer: the one in use stays
    _, d = p.eager(SHORT)
    kept = [buf for _, _, buf in G.kept_rows({"plan": p.rnn})]
    assert len(kept) == 1 and kept[0] is d
    p.replay(pinned, "replay of the pinned graph")
    p.eager(LONG)
