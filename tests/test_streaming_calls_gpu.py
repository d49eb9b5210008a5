"""What the hop-by-hop streamers hand to the C ABI: every call that step / step_chunk / flush / close make, with every argument,
against a ledger recorded from commit ae04f6f, before the streamers of the free-encoder models got one session base
(streaming/_free.py) and the step wrappers of hip.py one argument list per pair of entries.  A wrapper that passes an argument
to the block entry and not to its slot twin, or a session that launches in another order, differs from the ledger in a line.

A proxy around hip.lib() writes one line per call: the entry's name and its arguments in order; integers and floats as values,
pointers as `set` or `null`, structs behind a pointer (ps_prologue, ps_dprnn_pass, ps_skim_block, ps_skim_state, the ring-pair
table) field by field in the same way.  The calls of init_streams / init_slots / open (the speaker net) are not recorded.

Sessions, all eager (use_graph=False) and of B = 3 columns, on the smallest models the streamers' own GPU tests build.
Block: the priming hops one by one, a chunk of 5 hops, a chunk of 17 (16 + 1 where a launch takes 16 hops at most), flush.
Slots: capacity 3, open(1), a chunk of 5 hops, end(1, 2), two single hops, the model's delay in hops where it has one,
close(1).  StreamingSeparator has no slot sessions, so ns_dpcrn_short has the block session only.

streaming_calls.txt: the 3318 calls of the 15 sessions are 198 distinct lines, so the file names each distinct line once
(`c<i> <line>`) and gives a session as the sequence of those names, a run of a repeated stretch as `<n>*(c.. c..)`.  The test
expands a session to its lines and compares line by line.

`python tests/test_streaming_calls_gpu.py --record` writes streaming_calls.txt from the tree it runs in."""
import contextlib
import ctypes as C
import os
import re
import sys
import textwrap
import time

import pytest
import torch

import conftest  # noqa: F401  (run as a script: it puts the repository and tests/golden on sys.path)
from detweights import det_wave
from test_streaming_long_run_gpu import _streamer, _takes_enrolment
from test_streaming_tcn_gpu import CLN
from test_streaming_tcn_gpu import _model as _tcn_model

pytestmark = pytest.mark.gpu
LEDGER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "streaming_calls.txt")
B = 3
MODELS = ["tcn_tiny", "tcn_tiny_cln", "dprnn_cfg4_tse", "skim_tiny_k", "skim_vad", "unet_small_nodelay", "unet_small", "dpcrn"]
CASES = [(m, kind) for m in MODELS for kind in ("block", "slots") if (m, kind) != ("dpcrn", "slots")]


def _show(value, kind) -> str:
    """One argument (or struct field) of ctypes type `kind` as the ledger has it."""
    if isinstance(value, C.Array) and not issubclass(kind, C.Array):     # a table of structs behind a pointer
        return "[" + ", ".join(_show(v, kind._type_) for v in value) + "]"
    if hasattr(value, "_obj"):                                           # C.byref(struct)
        value, kind = value._obj, type(value._obj)
    if issubclass(kind, C.Structure):
        return "{" + ", ".join(f"{name}={_show(getattr(value, name), k)}" for name, k in kind._fields_) + "}"
    if issubclass(kind, C.Array):
        return "[" + ", ".join(_show(v, kind._type_) for v in value) + "]"
    if kind is C.c_void_p or issubclass(kind, C._Pointer):
        return "set" if value else "null"
    if kind in (C.c_float, C.c_double):
        return repr(float(value))
    return str(int(value))


class Recorder:
    """hip.lib()'s stand-in: the library, with a line per call while `on`."""

    def __init__(self, real, signatures):
        self.real, self.signatures, self.on, self.lines = real, signatures, False, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not self.on:
            return fn

        def call(*args):
            kinds = self.signatures[name][1]
            assert len(kinds) == len(args), name
            self.lines.append(" ".join([name] + [_show(a, k) for a, k in zip(args, kinds)]))
            return fn(*args)
        call.__name__ = name
        return call

    @contextlib.contextmanager
    def recording(self):
        self.on = True
        try:
            yield
        finally:
            self.on = False


def _new_streamer(model, dev):
    from puresound_amd import streaming as S
    if model == "tcn_tiny_cln":
        return S.StreamingConvTasNet(_tcn_model("tiny_free_relu_causal", dev, **CLN)[0])
    if model == "skim_vad":
        from test_streaming_skim_gpu import _model
        return S.StreamingSkiMExtractor(_model("tse_skim_vad_short", dev)[0])
    return _streamer(model, dev)


def ledger_of(model, kind, dev, patch):
    """The lines of one session; `patch(name, value)` replaces an attribute of puresound_amd.hip."""
    from puresound_amd import _abi, hip
    s = _new_streamer(model, dev)
    rec = Recorder(hip.lib(), _abi.SIGNATURES)
    patch("lib", lambda: rec)
    hop, D = s.hop_length, s.delay_frames
    enrol = lambda n: ({"enroll": det_wave(31, n, 3000).to(dev)} if _takes_enrolment(s) else {})  # noqa: E731
    x = det_wave(32, B, 17 * hop).to(dev)
    feed = lambda hops: x[:, :hops * hop].contiguous()  # noqa: E731
    if kind == "block":
        s.init_streams(B, use_graph=False, **enrol(B))
        with rec.recording():
            for _ in range(s.prime_hops):
                assert s.step(feed(1)) is None
            assert s.step_chunk(feed(5)).shape == (B, 5 * hop)
            assert s.step_chunk(feed(17)).shape == (B, 17 * hop)
            s.flush()
    else:
        s.init_slots(B, use_graph=False)
        s.open(1, **{k: v[0] for k, v in enrol(1).items()})
        with rec.recording():
            s.step_chunk(feed(5))
        s.end(1, 2)
        with rec.recording():
            s.step(feed(1))
            s.step(feed(1))
            if D:
                s.step_chunk(feed(D))
            s.close(1)
    torch.cuda.synchronize(dev)
    return rec.lines


def _runs(seq):
    """A sequence of names -> tokens, a stretch that repeats at once as `n*(names)` (greedy, not nested)."""
    out, i = [], 0
    while i < len(seq):
        best = (0, 1, 1)                                               # (names covered beyond one copy, period, copies)
        for p in range(1, min(120, (len(seq) - i) // 2) + 1):
            n = 1
            while seq[i + n * p:i + (n + 1) * p] == seq[i:i + p]:
                n += 1
            if n > 1:
                best = max(best, ((n - 1) * p, p, n))
        _, p, n = best
        out.append(seq[i] if n == 1 else f"{n}*({' '.join(seq[i:i + p])})")
        i += p * n
    return out


def write_ledger(sessions, path=LEDGER):
    """sessions: {"model kind": lines}"""
    names = {}
    for lines in sessions.values():
        for ln in lines:
            names.setdefault(ln, f"c{len(names)}")
    with open(path, "w") as f:
        f.write("".join(f"{name} {ln}\n" for ln, name in names.items()))
        for key, lines in sessions.items():
            f.write(f"\n== {key}\n" + textwrap.fill(" ".join(_runs([names[ln] for ln in lines])), 120,
                                                    break_long_words=False, break_on_hyphens=False) + "\n")


def read_ledger(path=LEDGER):
    """-> {"model kind": lines}"""
    with open(path) as f:
        table, *sessions = f.read().split("\n== ")
    calls = dict(line.split(" ", 1) for line in table.splitlines() if line)
    want = {}
    for text in sessions:
        key, _, body = text.partition("\n")
        want[key] = []
        for n, group, single in re.findall(r"(\d+)\*\(([^)]*)\)|(c\d+)", body):
            want[key] += [calls[c] for c in group.split()] * int(n) if n else [calls[single]]
    return want


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def want():
    return read_ledger()


@pytest.mark.parametrize("model,kind", CASES, ids=[f"{m}-{k}" for m, k in CASES])
def test_calls(dev, want, monkeypatch, model, kind):
    from puresound_amd import hip
    t0 = time.perf_counter()
    lines = ledger_of(model, kind, dev, lambda name, value: monkeypatch.setattr(hip, name, value))
    print(f"streaming_calls {model} {kind}: {len(lines)} calls, {time.perf_counter() - t0:.2f} s")
    expected = want[f"{model} {kind}"]
    for k, (got, exp) in enumerate(zip(lines, expected)):
        assert got == exp, f"call {k}"
    assert len(lines) == len(expected) > 0


def test_the_ledger_has_both_entries_of_every_step_wrapper(want):
    """The seven wrappers that pick one of two entries: each entry is called in some session of the ledger."""
    called = {line.split()[0] for lines in want.values() for line in lines}
    for stem in ("conv2d_step", "istft_step", "dwconv_step", "gated_tcn_step", "free_decode_step", "dprnn_block_step",
                 "skim_block_step"):
        assert {f"ps_{stem}_f32", f"ps_{stem}_slots_f32"} <= called, stem


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    from puresound_amd import hip as _hip
    device, real = torch.device("cuda:0"), _hip.lib
    recorded = {}
    for case in CASES:
        start = time.perf_counter()
        recorded[f"{case[0]} {case[1]}"] = ledger_of(*case, device, lambda name, value: setattr(_hip, name, value))
        _hip.lib = real
        print(f"{case}: {len(recorded[f'{case[0]} {case[1]}'])} calls, {time.perf_counter() - start:.2f} s", flush=True)
    write_ledger(recorded)
