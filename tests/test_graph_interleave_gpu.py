"""Captured graphs against later calls on the same model (graph_interleave_cases.py has the schedules and the shapes).

A captured graph holds raw addresses of what the model keeps between calls -- packed-weight plans, PlanCache's kept scratch,
the zeroed LSTM output rows of _plans._h_rows -- and every other replay test replays right behind its capture.  Here other
lengths, other batches, eager calls, other captures, other sessions and freed memory full of NaN come in between.

Part A: GraphedInference on the eight presets of edge_length_cases, both arithmetics.  `served` is graphed and also called
eagerly, `plain` only ever runs eager inference and is the reference (one eager model equals freshly built ones bit for bit:
test_edge_lengths_gpu.py::test_one_model_object_walks_the_ladder).  Every step of PART_A is torch.equal to plain.inference of
the same input -- graphs.py promises bit identity, so there is no tolerance -- and behind the steps that say so every kept
h_rows buffer of the served model has exact zeros outside the frames its geometry writes.

Part B: a streaming session with graphs on a model that meanwhile serves offline calls at other shapes, a second session at
another width that is stepped and dropped, and the NaN churn: the streamed samples and flush() are torch.equal to an
undisturbed session on a model of the same weights, the offline results to that model's, the second session's samples to
an undisturbed session of its own.  One preset per streamer class, and StreamingSkiM's frame graph on stream_tiny (whose
state lives in the module: its "second session" is the stateless step_chunk API at another width).

No test here empties the allocator's cache or deletes a model between a capture and a replay: inside the caching allocator
a graph that reads or writes freed memory gives wrong numbers, which the NaN churn shows; once the block is back with the
driver the same replay is a memory fault.  The ownership these tests confirm was established by reading ("Who
owns what a captured graph reads")."""
import pytest
import torch

import cases
import edge_length_cases as E
import graph_interleave_cases as G
from detweights import det_state_dict, det_wave

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def PA():
    import puresound_amd.nnet as PA
    from puresound_amd import hip
    hip.lib()  # fail loudly if the extension is missing
    return PA


def nan_churn(dev):
    """NaN-filled blocks through torch's caching allocator (the fixture of test_edge_lengths_gpu.py, as a function to call
    between steps): what is handed out next -- scratch, outputs, and any block a graph still writes after its owner let go
    of it -- holds NaN."""
    junk = [torch.full((1 << 22,), NAN, device=dev) for _ in range(16)]
    junk += [torch.full((n,), NAN, device=dev) for n in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20)]
    del junk


def check_kept_rows(model, where):
    """Every kept h_rows buffer of the model's plans: exact zeros in every frame its geometry's walk does not write
    -> how many buffers were looked at."""
    from puresound_amd.nnet._plans import PlanCache
    torch.cuda.synchronize()
    seen = 0
    for mod in model.modules():
        if isinstance(mod, PlanCache):
            for lane, (t, *walk), buf in G.kept_rows([plan for _, plan in (mod._plans or {}).values()]):
                frames = G.written_frames(walk)
                assert frames[-1] < t <= buf.shape[-1], (where, t, walk, tuple(buf.shape))
                ok, bad = G.pad_frames_are_zero(buf, walk)
                assert ok, (f"{where}: {bad} non-zero values in the pad frames of {type(mod).__name__}'s kept LSTM rows "
                            f"{tuple(buf.shape)}, lane {lane}, t = {t}, walk = {tuple(walk)}")
                seen += 1
    return seen


def _fresh(PA, dev, name, prec=None):
    model = cases.build(PA.NS, name).eval()
    model.load_state_dict(E.weights(name)[0])
    model.to(dev)
    return model if prec is None else model.set_gemm_precision(prec)


def _infer(model, noisy, enroll):
    return model.inference(noisy) if enroll is None else model.inference(noisy, enroll)


# ---------------------------------------------------------------------------------------------------------------------
# Part A
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", G.PRECISIONS)
@pytest.mark.parametrize("name", G.PRESETS)
def test_graphed_inference_between_other_calls_on_the_model(PA, dev, name, prec):
    from puresound_amd.graphs import GraphedInference
    served, plain = _fresh(PA, dev, name, prec), _fresh(PA, dev, name, prec)
    fast = GraphedInference(served)
    assert not fast._stochastic()               # (a model GraphedInference runs eagerly would empty the case)
    looked_at = 0
    for i, (kind, shape, rows) in enumerate(G.PART_A):
        if kind == "churn":
            nan_churn(dev)
            continue
        noisy, enroll = (None if v is None else v.to(dev) for v in G.step_input(name, shape, i))
        t, batch = G.SHAPES[shape]
        graphs_before = len(fast._graphs)
        if kind == "graph":
            got = fast(noisy) if enroll is None else fast(noisy, enroll)
        else:
            got = _infer(served, noisy, enroll)
            assert len(fast._graphs) == graphs_before, "an eager call dropped the graphs: nothing is replayed behind it"
        want = _infer(plain, noisy, enroll)
        torch.cuda.synchronize()
        assert want.shape == (batch, E.out_length(name, t)) and bool(torch.isfinite(want).all()), G.describe(i)
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), f"{name} [{prec}] {G.describe(i)}"
        assert torch.equal(got, want), (f"{name} [{prec}] {G.describe(i)}: differs from the eager model by "
                                        f"{float((got - want).abs().max()):.3e}")
        if rows:
            looked_at += check_kept_rows(served, f"{name} [{prec}] {G.describe(i)}")
    assert len(fast._graphs) == 3               # a, b, b1 and nothing else: every other graph step was a replay
    print(f"{name} [{prec}]: {len(G.PART_A) - 1} steps equal the eager model; {looked_at} kept-row buffers checked")
    if name in ("ns_dpcrn_short", "ns_dparn_short"):
        assert looked_at > 0, "no kept LSTM rows on a preset whose intra pass leaves pad frames: the check saw nothing"


# (hidden, N, Q): lstm_m4_kernel<128, CONTIG>, lstm_m4_kernel<64, CONTIG>, and N * Q = 4096 sequences for lstm_mfma_kernel<64, CONTIG>
@pytest.mark.parametrize("hidden,n,q", [(128, 2, 8), (64, 2, 8), (64, 64, 64)])
def test_partial_store_group_leaves_zeros_behind_the_last_step(dev, hidden, n, q):
    """What the kept-rows check found on an eager-only model: the forward LSTM kernels that store h' in 16-byte groups of
    four steps end a pass of 4 k + 1 .. 4 k + 3 steps in a partial group, whose store reaches the pad frames behind the last
    step -- with zeros, not with what a register held.  Rows of zeros going in, as _h_rows hands them out."""
    from puresound_amd import hip
    stride = 8
    ldt = hip.padded_frames(q * stride)
    gx = (det_wave(960 + hidden, n * 4 * hidden, ldt).reshape(n, 4 * hidden, ldt) * 2.0).to(dev)
    whh_t = (det_wave(961, hidden, 4 * hidden).reshape(1, hidden, 4 * hidden) * 0.3).to(dev)
    for steps in (5, 6, 7, 8):
        walk = (q, stride, steps, 1)
        out = torch.zeros(n, hidden, ldt, device=dev)
        hout, _ = hip.lstm(gx, whh_t, hidden, 1, *walk, out=out)
        torch.cuda.synchronize()
        assert hout.data_ptr() == out.data_ptr()
        written = out[..., torch.tensor(G.written_frames(walk), device=dev)]
        assert bool(torch.isfinite(written).all()) and float(written.abs().min(dim=1).values.max()) > 0.0, steps
        ok, bad = G.pad_frames_are_zero(out, walk)
        assert ok, f"H = {hidden}, {n * q} sequences of {steps} steps: {bad} non-zero values in frames no step wrote"


# ---------------------------------------------------------------------------------------------------------------------
# Part B
# ---------------------------------------------------------------------------------------------------------------------
def _session(cls, model, streams, enroll):
    s = cls(model)
    if enroll is None:
        s.init_streams(streams, use_graph=True)
    else:
        s.init_streams(streams, enroll=enroll, use_graph=True)
    return s


def _second_input(name, dev, k):
    """the second session's OTHER_HOPS hops of OTHER_STREAMS streams (other samples at each visit k), and its enrolment"""
    _, hop = E.win_hop(name)
    x = (det_wave(930 + k, G.OTHER_STREAMS, G.OTHER_HOPS * hop) * E.AMP).to(dev)
    e = (det_wave(940 + k, G.OTHER_STREAMS, E.L_ENROLL) * E.AMP).to(dev) if E.has_enrolment(name) else None
    return x, e


def _second_session(cls, model, name, dev, k):
    """a session of another width: built, stepped hop by hop (graphs of one hop) and in one chunk, dropped -> its samples"""
    _, hop = E.win_hop(name)
    x, e = _second_input(name, dev, k)
    s = _session(cls, model, G.OTHER_STREAMS, e)
    half = G.OTHER_HOPS // 2
    outs = [s.step(x[:, i * hop:(i + 1) * hop]) for i in range(half)]
    outs.append(s.step_chunk(x[:, half * hop:]))
    outs.append(s.flush())
    assert s._graphs, "the second session ran no graph"
    del s
    return torch.cat([o for o in outs if o is not None], dim=1)


def _offline_input(name, dev, k):
    t, batch = G.OFFLINE[k]
    noisy, enroll = E.inputs(name, E.length_of(name, t), batch)
    return noisy.to(dev), (None if enroll is None else enroll.to(dev))


@pytest.mark.parametrize("cls_name,name", G.STREAMERS)
def test_streaming_session_while_the_model_serves_other_calls(PA, dev, cls_name, name):
    import puresound_amd.streaming as S
    cls = getattr(S, cls_name)
    _, hop = E.win_hop(name)
    m1, m2 = _fresh(PA, dev, name), _fresh(PA, dev, name)
    x, enroll = (None if v is None else v.to(dev) for v in E.inputs(name, G.HOPS * hop, G.STREAMS))
    chunk = G.CHUNK_HOPS * hop
    n_chunks = G.HOPS // G.CHUNK_HOPS

    def stream(model, between=None):
        s = _session(cls, model, G.STREAMS, enroll)
        outs = []
        for i in range(n_chunks):
            outs.append(s.step_chunk(x[:, i * chunk:(i + 1) * chunk]))
            if between is not None and i + 1 in G.thirds(n_chunks):
                between(G.thirds(n_chunks).index(i + 1))
        assert G.CHUNK_HOPS in s._graphs, "the session ran no graph of the chunk's length"
        outs.append(s.flush())
        torch.cuda.synchronize()
        return torch.cat(outs, dim=1)

    y_ref = stream(m1)
    assert bool(torch.isfinite(y_ref).all()) and y_ref.shape[1] > (G.HOPS - 8) * hop
    offline, second = {}, {}

    def between(k):
        offline[k] = _infer(m2, *_offline_input(name, dev, k))
        second[k] = _second_session(cls, m2, name, dev, k)
        nan_churn(dev)

    y = stream(m2, between)
    assert sorted(offline) == sorted(second) == [0, 1]
    assert torch.equal(y, y_ref), (f"{cls_name} on {name}: the session whose model served other calls differs from the "
                                   f"undisturbed one by {float((y - y_ref).abs().max()):.3e}, first at sample "
                                   f"{int((y != y_ref).any(0).nonzero()[0])} of {y.shape[1]}")
    for k in (0, 1):
        want = _infer(m1, *_offline_input(name, dev, k))
        assert torch.equal(offline[k], want), (f"{cls_name} on {name}: offline call {k} (T, B = {G.OFFLINE[k]}) between the "
                                               f"chunks differs by {float((offline[k] - want).abs().max()):.3e}")
        own = _second_session(cls, m1, name, dev, k)
        assert own.shape[1] > 0 and torch.equal(second[k], own), (
            f"{cls_name} on {name}: second session {k} differs by {float((second[k] - own).abs().max()):.3e}")


def test_streaming_skim_frame_graph_while_the_module_serves_other_calls(PA, dev):
    """StreamingSkiM keeps its streaming state in the module itself, so one object carries one session: the calls in between
    are the offline forward at another batch and length and the stateless step_chunk API at another width."""
    name = "stream_tiny"
    c = cases.CASES[name]
    ch, e, k = c["args"][0], c["kw"]["embed_dim"], c["kw"]["seg_size"]
    frames, b = G.HOPS, G.STREAMS

    def build():
        m = cases.build(PA.NS, name).eval()
        m.load_state_dict(det_state_dict(m))
        return m.to(dev)

    m1, m2 = build(), build()
    xs = det_wave(950, b * ch, frames).reshape(b, ch, frames).to(dev)
    ds = det_wave(951, b, e).to(dev)
    off = [(det_wave(952, 4 * ch, 47).reshape(4, ch, 47).to(dev), det_wave(953, 4, e).to(dev)),
           (det_wave(954, ch, 7).reshape(1, ch, 7).to(dev), det_wave(955, 1, e).to(dev))]
    seg = [(det_wave(956 + i, G.OTHER_STREAMS * k, ch).reshape(G.OTHER_STREAMS, k, ch).to(dev),
            det_wave(958 + i, G.OTHER_STREAMS, e).to(dev)) for i in range(2)]

    def stream(m, between=None):
        m.init_status(streams=b, use_graph=True)
        outs = []
        for f in range(frames):
            outs.append(m.step_frame(xs[..., f].reshape(b, -1, 1), ds))
            if between is not None and f + 1 in G.thirds(frames):
                between(G.thirds(frames).index(f + 1))
        assert m._graph is not None
        torch.cuda.synchronize()
        return torch.cat(outs, dim=-1)

    y_ref = stream(m1)
    assert bool(torch.isfinite(y_ref).all())
    offline, chunked = {}, {}

    def between(i):
        offline[i] = m2(*off[i])
        chunked[i] = m2.step_chunk(seg[i][0], embed=seg[i][1])[0]
        nan_churn(dev)

    y = stream(m2, between)
    assert torch.equal(y, y_ref), f"the frame graph differs by {float((y - y_ref).abs().max()):.3e}"
    for i in range(2):
        assert torch.equal(offline[i], m1(*off[i])), i
        assert torch.equal(chunked[i], m1.step_chunk(seg[i][0], embed=seg[i][1])[0]), i
