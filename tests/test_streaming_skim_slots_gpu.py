"""Slot sessions of StreamingSkiMExtractor on the MI355X (init_slots / open / end / close): ps_skim_block_step_slots_f32
against the fp64 frame loop of tests/skim_slots_ref.py and against its sibling, and the streamer: streams that begin and end
on their own against offline inference, against an init_streams(1, ...) session of each stream and against each other
(isolation and slot re-use), bit for bit, graph against eager.  The driver of a slot session (_run_slots) is the one of the
Conv-TasNet slot tests; the spans of the kernel cases are those of the DPRNN slot tests."""
import ctypes as C

import numpy as np
import pytest
import torch

import skim_slots_ref as RS
import skim_step_ref as R
from conftest import rel_max
from detweights import det_state_dict, det_wave
from test_streaming_dprnn_slots_gpu import _check_against_offline, _chunks, _cycled_spans, _fp32, _offline, _tiled_spans
from test_streaming_long_run_gpu import same_bits_at_a_small_counter
from test_streaming_skim import _build
from test_streaming_skim_gpu import _Mods, _cols
from test_streaming_slots_gpu import _run_slots, _zero

pytestmark = pytest.mark.gpu
SCHEDULE = (1, 3, 8, 16, 37)
NAN = float("nan")
I32_MAX = 2 ** 31 - 1
KERNEL_SHAPES = [(16, 8, 5), (128, 256, 5)]        # one gate row per thread; four, and 128 KB of LDS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def H():
    from puresound_amd import hip
    hip.lib()
    return hip


@pytest.fixture(autouse=True)
def _nan_in_the_allocator_cache(dev):
    """Scratch from torch.empty holds NaN, not a fresh process' zeros: uninitialised memory that reaches a result fails."""
    junk = [torch.full((1 << 22,), float("nan"), device=dev) for _ in range(16)]
    junk += [torch.full((n,), float("nan"), device=dev) for n in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20)]
    del junk
    yield


# -------------------------------------------------------------------------------------------------------------------------
# the kernel
# -------------------------------------------------------------------------------------------------------------------------
_BLOCKS = {}
MEM_KEYS = ("mh_h", "mc_h", "mh_c", "mc_c")


def _block(c, h, film, mem, dev, H):
    """make_block's block at (C, H) with skim_step_ref.kernel_case's seed (make_block's scales) and its device pack."""
    key = (c, h, film, mem)
    if key not in _BLOCKS:
        blk = R.make_block(c, h, 17 * c + h, film, mem)
        _BLOCKS[key] = (blk, H.pack_skim_block(_Mods(blk, c, h), 0, dev))
    return _BLOCKS[key]


def _rand(shape, seed):
    g = np.random.Generator(np.random.Philox(key=seed))
    return torch.tensor(g.uniform(-1.0, 1.0, shape), dtype=torch.float64)


def _case(c, h, k, b, c0, variant, dev, H):
    """Random inputs, states and banks (a missed reset, a wrong slot or a store by a dead column shows) in fp64 and on the
    device, NaN past column B there."""
    film, incoming, mem = R.VARIANTS[variant]
    blk, pk = _block(c, h, film, mem, dev, H)
    t_len, ns = 3 * k + 11, R.slots_needed(16, k)
    seed = 100000 * c + 1000 * b + c0 + 7 * list(R.VARIANTS).index(variant)
    ref = dict(x=_rand((t_len, b, c), seed), state=R.new_state(b, h, mem),
               rs=_rand((b, c), seed + 11) if film else None, rb=_rand((b, c), seed + 12) if film else None,
               bank_in=(_rand((ns, b, h), seed + 13), _rand((ns, b, h), seed + 14)) if incoming else None,
               bank_out=(_rand((ns, b, h), seed + 15), _rand((ns, b, h), seed + 16)) if mem else None)
    for n, name in enumerate(sorted(ref["state"])):
        ref["state"][name] = _rand((b, h), seed + 1 + n)
    ldb = H.padded_frames(b)
    d = dict(state={name: _cols(t, ldb, dev) for name, t in ref["state"].items()},
             terms=(_cols(ref["rs"], ldb, dev), _cols(ref["rb"], ldb, dev)) if film else None,
             bank_in=tuple(_cols(t, ldb, dev) for t in ref["bank_in"]) if incoming else None,
             bank_out=tuple(_cols(t, ldb, dev) for t in ref["bank_out"]) if mem else None)
    assert H.skim_block_step_ok(c, h, k) and ns == H.skim_bank_slots(16, k)
    return blk, pk, t_len, ns, ref, d


def _launch(H, pk, xin, counter, d, k, b, n, out, span=None):
    mem = None if d["bank_out"] is None else tuple(d["state"][name] for name in MEM_KEYS)
    H.skim_block_step(xin, counter, pk, (d["state"]["seg_h"], d["state"]["seg_c"]), k, b, n, out, terms=d["terms"],
                      bank_in=d["bank_in"], mem_state=mem, bank_out=d["bank_out"], span=span)


def _xin(H, xs, c, n, b, dev):
    ld = H.padded_frames(n * b)
    xin = torch.full((1, c, ld), NAN, device=dev)
    xin[0, :, :n * b] = xs.permute(2, 0, 1).reshape(c, n * b).float().to(dev)
    return xin, ld


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_slot_kernel(dev, H, c, h, k, b, c0, spans, variant, want_ends=None):
    """rel_max of the live outputs, of every state and of the outgoing banks against the fp64 slot loop under 1e-5 (the bound
    of this kernel family; the same loop in torch fp32 with make_block's scales: 2.8e-6, tests/test_streaming_skim.py), and
    per launch what must keep its bits."""
    blk, pk, t_len, ns, ref, d = _case(c, h, k, b, c0, variant, dev, H)
    x, state = ref["x"], ref["state"]
    mem = d["bank_out"] is not None
    live = torch.tensor([[lo <= c0 + f < hi for (lo, hi) in spans] for f in range(t_len)])   # [T, B]
    span = torch.tensor(spans, dtype=torch.int32, device=dev)
    counter = torch.tensor([c0], dtype=torch.int32, device=dev)
    inputs = [t for t in (d["terms"] or ()) + (d["bank_in"] or ())]
    inputs0 = [t.clone() for t in inputs]
    got_live, want_live, t, ends_seen = [], [], 0, set()
    for n in _chunks(t_len):
        want, _, wr = RS.block_step_slots(x[t:t + n], c0 + t, k, blk, state, spans, ref["rs"], ref["rb"], ref["bank_in"],
                                          ref["bank_out"])
        xs = x[t:t + n].clone()
        xs[~live[t:t + n]] = NAN                                                    # dead frames carry NaN
        xin, ld = _xin(H, xs, c, n, b, dev)
        out = torch.full((1, c, ld), 7.0, device=dev)
        st0 = {name: v.clone() for name, v in d["state"].items()}
        out0 = [v.clone() for v in d["bank_out"]] if mem else []
        _launch(H, pk, xin, counter, d, k, b, n, out, span)
        torch.cuda.synchronize()
        assert int(counter[0]) == c0 + t                                            # read, never written
        assert bool((out[0, :, n * b:] == 7.0).all())                               # columns past the chunk are not written
        got = out[0, :, :n * b].reshape(c, n, b).permute(1, 2, 0).cpu()
        assert bool(torch.isfinite(got).all()), t                                   # every y column of the chunk, dead ones too
        got_live.append(got[live[t:t + n]])
        want_live.append(want[live[t:t + n]])
        idle = (~live[t:t + n].any(dim=0)).to(dev)                                  # columns with no live frame in this launch
        quiet = torch.tensor([len(w) == 0 for w in wr], device=dev)                 # columns with no segment end in it
        for name, v in d["state"].items():
            assert _bits(v[:, :b][:, idle], st0[name][:, :b][:, idle]), (name, t)
            if name in MEM_KEYS:
                assert _bits(v[:, :b][:, quiet], st0[name][:, :b][:, quiet]), (name, t)
            assert bool(torch.isnan(v[:, b:]).all()), name
        for v, v0 in zip(d["bank_out"] or (), out0):
            assert _bits(v[:, :, :b][:, :, quiet], v0[:, :, :b][:, :, quiet]), t
            spared = torch.tensor([[slot not in w for w in wr] for slot in range(ns)], device=dev)   # [NS, B]: bank slots
            assert _bits(v[:, :, :b].transpose(1, 2)[spared], v0[:, :, :b].transpose(1, 2)[spared]), t   # not visited
            assert bool(torch.isnan(v[:, :, b:]).all())
        ends_seen |= {(t + f, col) for f in range(n) for col, (lo, hi) in enumerate(spans)
                      if lo <= c0 + t + f < hi and (c0 + t + f - lo) % k == k - 1}
        counter += n
        t += n
    for v, v0 in zip(inputs, inputs0):                                              # inputs: the same bits, NaN included
        assert _bits(v, v0)
    errs = {"out": rel_max(torch.cat(got_live).numpy(), torch.cat(want_live).numpy())}
    for name, r in state.items():
        errs[name] = rel_max(d["state"][name][:, :b].t().cpu().numpy(), r.numpy())
    if mem:
        for name, v, r in zip(("out_h", "out_c"), d["bank_out"], ref["bank_out"]):
            errs[name] = rel_max(v[:, :, :b].transpose(1, 2).cpu().numpy(), r.numpy())
    print(f"skim_block_step_slots C={c} H={h} K={k} B={b} c0={c0} {variant}: rel_max " +
          " ".join(f"{name} {v:.2e}" for name, v in errs.items()))
    assert max(errs.values()) < 1e-5, errs
    frames_with_ends = {f for f, _ in ends_seen}
    assert len(frames_with_ends) >= 2                                               # (segment ends were met)
    if want_ends is not None:
        want_ends(ends_seen, frames_with_ends)


@pytest.mark.parametrize("variant", list(R.VARIANTS))
@pytest.mark.parametrize("start", ["0", "3K+2"])
@pytest.mark.parametrize("b", [3, 70])
@pytest.mark.parametrize("c,h,k", KERNEL_SHAPES)
def test_block_step_slots_kernel(dev, H, c, h, k, b, start, variant):
    """(a) chunk lengths 1, 2, ..., 16 over 3K + 11 frames; the spans cycled over the columns: empty, all live, birth inside
    a chunk off the segment grid, death inside a chunk, both inside one chunk, birth on the grid, a span of K - 2 frames."""
    c0 = {"0": 0, "3K+2": 3 * k + 2}[start]
    _check_slot_kernel(dev, H, c, h, k, b, c0, _cycled_spans(k, c0, b), variant)


@pytest.mark.parametrize("variant", list(R.VARIANTS))
@pytest.mark.parametrize("c,h,k", KERNEL_SHAPES)
def test_one_tile_whose_columns_end_their_segments_at_different_frames(dev, H, c, h, k, variant):
    """(b) B = 16 born at 16 consecutive frames with K = 5: at most frames some but not all columns of the tile hand over, so
    a hand-over that stores for the wrong columns -- under the tid % 16 mapping of its loads and cell or under the tid / 16
    mapping of its bank store -- changes bits that must stay (the MemLSTM states and bank columns of the others)."""
    c0 = 3 * k + 2
    spans = [(c0 + i, I32_MAX) for i in range(16)]

    def mixed(ends, frames):
        per_frame = [len([1 for f, _ in ends if f == g]) for g in frames]
        assert all(0 < n < 16 for n in per_frame) and len(frames) > 3 * k
    _check_slot_kernel(dev, H, c, h, k, 16, c0, spans, variant, mixed)


@pytest.mark.parametrize("c,h,k", KERNEL_SHAPES)
def test_block_step_slots_kernel_with_dead_tiles(dev, H, c, h, k):
    """(c) the cycled spans put a live column into every tile: here whole tiles are dead, for all frames or for some."""
    _check_slot_kernel(dev, H, c, h, k, 40, 3 * k + 2, _tiled_spans(k, 3 * k + 2, 40), "middle")


@pytest.mark.parametrize("variant", ["middle", "plain"])
@pytest.mark.parametrize("c,h,k", KERNEL_SHAPES)
def test_all_live_span_is_the_sibling_bit_for_bit(dev, H, c, h, k, variant):
    b = 70
    blk, pk, t_len, ns, ref, da = _case(c, h, k, b, 0, variant, dev, H)
    _, _, _, _, _, db = _case(c, h, k, b, 0, variant, dev, H)
    span = torch.tensor([(0, I32_MAX)] * b, dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    t = 0
    for n in _chunks(t_len):
        xin, ld = _xin(H, ref["x"][t:t + n], c, n, b, dev)
        ya, yb = torch.full((1, c, ld), 7.0, device=dev), torch.full((1, c, ld), 7.0, device=dev)
        _launch(H, pk, xin, counter, da, k, b, n, ya)
        _launch(H, pk, xin, counter, db, k, b, n, yb, span)
        assert torch.equal(ya, yb), t
        for name in da["state"]:
            assert torch.equal(da["state"][name][:, :b], db["state"][name][:, :b]), (name, t)
        for va, vb in zip(da["bank_out"], db["bank_out"]):
            assert torch.equal(va[:, :, :b], vb[:, :, :b]), t
        counter += n
        t += n
    assert bool(torch.isfinite(ya[0, :, :n * b]).all())


def test_block_step_slots_kernel_refusals(dev, H):
    """(d) a null or misaligned span (PS_E_INVALID) and a shape without a kernel (PS_E_UNSUPPORTED): nothing is written."""
    from puresound_amd import _abi
    z = lambda *shape: torch.zeros(*shape, device=dev)  # noqa: E731

    def attempt(c, h, k, b, span_ptr, rc, word):
        blk = R.make_block(c, h, 1, film=False, mem=False)
        pk = H.pack_skim_block(_Mods(blk, c, h), 0, dev)
        ld = ldb = H.padded_frames(b)
        x, out = z(1, c, ld), torch.full((1, c, ld), 7.0, device=dev)
        states = [torch.full((h, ldb), 3.0, device=dev) for _ in range(2)]
        st = _abi.SkimState()
        st.seg_h, st.seg_c = H.ptr(states[0]), H.ptr(states[1])
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        got = H.lib().ps_skim_block_step_slots_f32(H.ptr(x), H.ptr(out), H.ptr(counter), span_ptr, C.byref(pk["struct"]),
                                                   C.byref(st), c, h, k, 0, b, 1, ld, ldb, H.stream_ptr(dev))
        torch.cuda.synchronize()
        assert got == rc
        assert word in H.lib().ps_last_error().decode()
        assert bool((out == 7.0).all()) and all(bool((s == 3.0).all()) for s in states)

    buf = torch.zeros(2 * 2 + 2, dtype=torch.int32, device=dev)
    assert buf.data_ptr() % 8 == 0
    attempt(16, 8, 5, 2, None, -1, "span")
    attempt(16, 8, 5, 2, buf.data_ptr() + 4, -1, "span")
    attempt(128, 512, 150, 2, buf.data_ptr(), -3, "LDS")
    assert not H.skim_block_step_ok(128, 512, 150)
    # through the wrapper: a contiguous [2, 2] view that begins 4 bytes into its storage, then a span of another shape
    blk = R.make_block(16, 8, 1, film=False, mem=False)
    pk = H.pack_skim_block(_Mods(blk, 16, 8), 0, dev)
    ld = ldb = H.padded_frames(2)
    out = torch.full((1, 16, ld), 7.0, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match=r"rc=-1.*span"):
        H.skim_block_step(z(1, 16, ld), counter, pk, (z(8, ldb), z(8, ldb)), 5, 2, 1, out, span=buf[1:5].view(2, 2))
    with pytest.raises(RuntimeError, match=r"span must be a contiguous int32 \[2, 2\]"):
        H.skim_block_step(z(1, 16, ld), counter, pk, (z(8, ldb), z(8, ldb)), 5, 2, 1, out, span=buf[:6].view(3, 2))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# -------------------------------------------------------------------------------------------------------------------------
# the streamer
# -------------------------------------------------------------------------------------------------------------------------
_MODELS = {}
NAMES = ["tse_skim_vad_short", "tse_skim_causal_short", "tiny_k"]
VAD = "tse_skim_vad_short"


def _model(name, dev):
    """The two presets (K = 150) and tse_skim_vad_short with segments of 5 frames."""
    if name not in _MODELS:
        import cases
        import puresound_amd.nnet as PA
        m = _build(VAD, seg_size=5) if name == "tiny_k" else cases.build(PA.NS, name).eval()
        sd = det_state_dict(m)
        m.load_state_dict(sd)
        _MODELS[name] = (m.to(dev), sd)
    return _MODELS[name]


def _streams(s, dev, plan, seed):
    """plan: (slot, start hop, length in hops, chunks between the stream's end and its close) -> stream dicts with a
    deterministic signal and an enrolment of their own."""
    out = []
    for i, (slot, start, hops, linger) in enumerate(plan):
        x = det_wave(seed + 2 * i, 1, hops * s.hop_length)[0].to(dev)
        e = det_wave(seed + 2 * i + 1, 1, 3000 + 100 * i)[0].to(dev)
        out.append(dict(id=i, slot=slot, start=start, x=x, e=e, hops=hops, linger=linger))
    return out


def _block_session(s, x, k=16, **how):
    """x [1, L] through an init_streams(1, ...) session in chunks of k hops ‖ flush() -> [L_out]."""
    hop = s.hop_length
    s.init_streams(1, **how)
    outs = [s.step_chunk(x[:, i:i + k * hop].contiguous()) for i in range(0, x.shape[1], k * hop)]
    return torch.cat(outs + [s.flush()], dim=1)[0]


# four streams in four slots, opened at the call boundaries 0, 4, 12 and 66 of the schedule: their births differ pairwise by
# no multiple of 150 and no multiple of 5; every stream is longer than two segments of 150 frames
PLAN = [(0, 0, 345, 0), (1, 3, 331, 2), (2, 10, 322, 0), (3, 66, 310, 1)]


@pytest.mark.parametrize("name", NAMES)
def test_staggered_streams_match_offline_and_their_own_sessions(dev, name):
    """(e) every slot over slot_output_range: model.inference of its stream alone within 1e-4, and the bits of an
    init_streams(1, enroll=...) session of that stream."""
    from puresound_amd.streaming import StreamingSkiMExtractor
    model, _ = _model(name, dev)
    s = StreamingSkiMExtractor(model)
    seg = model.masker.seg_size
    assert seg == (5 if name == "tiny_k" else 150)
    streams = _streams(s, dev, PLAN, seed=500)
    assert all(st["hops"] - s.prime_hops > 2 * seg for st in streams)              # two segment ends of its own, at least
    graphs = []
    with _fp32(model):
        ys, opened_at = _run_slots(s, 4, streams, SCHEDULE, probe=lambda s_: graphs.append(dict(s_._graphs)))
        refs = _offline(model, streams)
        at = sorted(opened_at.values())
        assert at == [0, 4, 12, 66]
        assert all((b - a) % 150 and (b - a) % 5 for i, a in enumerate(at) for b in at[i + 1:])
        _check_against_offline(s, streams, ys, refs)
        for a, b in zip(graphs, graphs[1:]):                                       # open / end / close never replaced a graph
            assert all(b[k] is g for k, g in a.items())
        for st in streams:
            r = s.slot_output_range(st["x"].numel(), s.win_length, s.hop_length)
            alone = _block_session(s, st["x"][None], enroll=st["e"][None])
            assert torch.equal(ys[st["id"]][r.start:r.stop], alone), st["id"]
    assert float(ys[0].abs().max()) > 1e-3


def test_slot_session_is_the_block_session_bit_for_bit(dev):
    """The same B streams opened together at hop 0 and never ended early, against an init_streams session."""
    from puresound_amd.streaming import StreamingSkiMExtractor
    model, _ = _model(VAD, dev)
    s = StreamingSkiMExtractor(model)
    b, hops, k = 4, 333, 8
    hop, lat = s.hop_length, s.latency_samples
    x = det_wave(610, b, hops * hop).to(dev)
    d = model.inference_tse_embedding(det_wave(611, b, 3000).to(dev))
    pieces = [x[:, i * hop:min(i + k, hops) * hop].contiguous() for i in range(0, hops, k)]
    s.init_streams(b, embed=d)
    block = torch.cat([s.step_chunk(p) for p in pieces] + [s.flush()], dim=1)
    s.init_slots(b)
    for i in range(b):
        s.open(i, embed=d[i:i + 1])
    outs = [s.step_chunk(p) for p in pieces]
    slots = torch.cat(outs + [torch.stack([s.close(i) for i in range(b)])], dim=1)
    assert s.active == []
    assert slots.shape[1] == block.shape[1] + lat
    assert torch.equal(slots[:, :lat], torch.full_like(slots[:, :lat], _zero(s)))
    assert torch.equal(slots[:, lat:], block)
    assert float(block.abs().max()) > 1e-3 and not torch.equal(block[0], block[1])


def test_isolation_bit_for_bit(dev):
    """Slot 1's whole output does not depend on what slots 0, 2, 3 do: idle with NaN input, or opening, ending and re-opening
    around it with other audio and other embeddings."""
    from puresound_amd.streaming import StreamingSkiMExtractor
    model, _ = _model(VAD, dev)
    s = StreamingSkiMExtractor(model)
    alone = _streams(s, dev, [(1, 3, 400, 1)], seed=700)
    crowd = alone + _streams(s, dev, [(0, 0, 60, 0), (2, 1, 150, 2), (3, 9, 31, 0), (0, 100, 90, 1), (3, 77, 200, 0),
                                      (2, 250, 120, 0), (0, 260, 100, 0)], seed=720)
    for i, st in enumerate(crowd):
        st["id"] = i
    ya, _ = _run_slots(s, 4, alone, SCHEDULE)
    yb, _ = _run_slots(s, 4, crowd, SCHEDULE)
    assert len(yb) == 8
    assert ya[0].numel() >= 400 * s.hop_length + s.latency_samples
    assert torch.equal(ya[0], yb[0])
    assert float(ya[0].abs().max()) > 1e-3


@pytest.mark.parametrize("name", [VAD, "tiny_k"])
def test_reused_slot_does_not_see_its_predecessor(dev, name):
    """Stream A then stream B (another enrolment) in slot 0, against stream B in a fresh session opened at the same counter
    value (a dummy in slot 1 advances it): the same bits.  A SegLSTM or MemLSTM state, a bank slot or a FiLM term that
    open() left behind would show."""
    from puresound_amd.streaming import StreamingSkiMExtractor
    model, _ = _model(name, dev)
    s = StreamingSkiMExtractor(model)
    a, b = _streams(s, dev, [(0, 0, 350, 0), (0, 360, 320, 0)], seed=800)
    dummy = _streams(s, dev, [(1, 0, 350, 0)], seed=810)[0]
    dummy["id"] = 2
    with _fp32(model):
        y1, at1 = _run_slots(s, 2, [a, b], SCHEDULE)
        y2, at2 = _run_slots(s, 2, [dummy, b], SCHEDULE)
        refs = _offline(model, [b])
    assert at1[b["id"]] == at2[b["id"]] > 350
    assert torch.equal(y1[b["id"]], y2[b["id"]])
    _check_against_offline(s, [b], y1, refs)


def test_open_with_the_embedding_is_open_with_the_enrolment(dev):
    from puresound_amd.streaming import StreamingSkiMExtractor
    model, _ = _model(VAD, dev)
    s = StreamingSkiMExtractor(model)
    hop, hops = s.hop_length, 170
    x = det_wave(640, 1, hops * hop).to(dev)
    e = det_wave(641, 1, 3000).to(dev)
    d = model.inference_tse_embedding(e)
    assert tuple(d.shape) == (1, 192, 1)
    ys = []
    for how in (dict(enroll=e[0]), dict(enroll=e), dict(embed=d), dict(embed=d[:, :, 0].contiguous()), dict(embed=d[0, :, 0])):
        s.init_slots(2)
        s.open(1, **how)
        chunk = torch.full((2, hops * hop), NAN, device=dev)
        chunk[1] = x[0]
        ys.append(torch.cat([s.step_chunk(chunk)[1], s.close(1)]))
    assert all(torch.equal(ys[0], y) for y in ys[1:])
    assert float(ys[0].abs().max()) > 1e-3


@pytest.mark.parametrize("name", [VAD, "tiny_k"])
def test_graph_and_eager_are_bit_identical(dev, name):
    from puresound_amd.streaming import StreamingSkiMExtractor
    model, _ = _model(name, dev)
    s = StreamingSkiMExtractor(model)
    streams = _streams(s, dev, [(0, 0, 330, 0), (1, 5, 100, 2), (2, 5, 133, 0), (1, 150, 90, 0)], seed=900)
    yg, _ = _run_slots(s, 3, streams, SCHEDULE, use_graph=True)
    assert len(s._graphs) > 0
    ye, _ = _run_slots(s, 3, streams, SCHEDULE, use_graph=False)
    assert len(s._graphs) == 0
    for i in yg:
        assert torch.equal(yg[i], ye[i]), i


@pytest.mark.parametrize("name", [VAD, "tiny_k"])
def test_end_inside_a_chunk(dev, name):
    """A stream with 5 hops left in a 16-hop chunk padded with NaN: finite output equal to offline; the slot's output hops
    after the end carry the tail, then constrain(0)."""
    from puresound_amd.streaming import StreamingSkiMExtractor
    model, _ = _model(name, dev)
    s = StreamingSkiMExtractor(model)
    st = _streams(s, dev, [(1, 0, 16 * 4 + 5, 0)], seed=950)[0]
    hop, lat = s.hop_length, s.latency_samples
    with _fp32(model):
        s.init_slots(2)
        s.open(1, st["e"])
        outs = []
        for i in range(6):
            chunk = torch.full((2, 16 * hop), NAN, device=dev)
            piece = st["x"][i * 16 * hop:(i + 1) * 16 * hop]
            chunk[1, :piece.numel()] = piece
            if i == 4:
                s.end(1, 5)
            outs.append(s.step_chunk(chunk)[1])
        last = s.close(1)
        refs = _offline(model, [st])
    y = torch.cat(outs + [last])
    _check_against_offline(s, [st], {st["id"]: y}, refs)
    after = torch.cat(outs[4:])[5 * hop:]                     # the slot's output past the stream's last input hop
    assert float((after[:lat] - _zero(s)).abs().max()) > 0    # the tail: the last frame's overlap
    assert torch.equal(after[lat:], torch.full_like(after[lat:], _zero(s)))
    assert torch.equal(last, torch.full_like(last, _zero(s)))


def test_changed_weights_refresh_the_open_slots_terms(dev):
    """Weights loaded in the middle of a slot session: the open slot's FiLM terms follow them, as an init_streams(1, ...)
    session's do -- the same bits after the change as that session's."""
    from puresound_amd.streaming import StreamingSkiMExtractor
    model, sd = _model(VAD, dev)
    s = StreamingSkiMExtractor(model)
    hop = s.hop_length
    x = det_wave(660, 1, 40 * hop).to(dev)
    d = model.inference_tse_embedding(det_wave(661, 1, 3000).to(dev))
    changed = {k: v.clone() for k, v in sd.items()}
    key = "masker.seg_input_fusion.0.cond_bias.weight"
    changed[key] = changed[key] * 1.5
    try:
        s.init_streams(1, embed=d)
        a = [s.step_chunk(x[:, :17 * hop].contiguous())]
        model.load_state_dict(changed)
        a.append(s.step_chunk(x[:, 17 * hop:].contiguous()))
        model.load_state_dict(sd)
        s.init_slots(3)
        s.open(2, embed=d)
        pad = lambda t: torch.cat([torch.full((2, t.shape[1]), NAN, device=dev), t])  # noqa: E731
        terms = s._terms[0][1][:, 2].clone()
        b = [s.step_chunk(pad(x[:, :hop]))[2], s.step_chunk(pad(x[:, hop:17 * hop]))[2]]
        model.load_state_dict(changed)
        b.append(s.step_chunk(pad(x[:, 17 * hop:]))[2])
        assert not torch.equal(s._terms[0][1][:, 2], terms)
    finally:
        model.load_state_dict(sd)
    assert torch.equal(torch.cat(b)[s.latency_samples:], torch.cat(a, dim=1)[0])


def test_errors_name_the_way_out(dev, H):
    from puresound_amd.streaming import StreamingSkiMExtractor, skim
    model, _ = _model(VAD, dev)
    s = StreamingSkiMExtractor(model)
    hop = s.hop_length
    e = det_wave(5, 1, 3000)[0].to(dev)
    d = model.inference_tse_embedding(e[None])
    x = det_wave(6, 2, 16 * hop).to(dev)

    def raises(exc, words, fn, *a, **kw):
        with pytest.raises(exc) as info:
            fn(*a, **kw)
        assert words.lower() in str(info.value).lower(), str(info.value)

    raises(RuntimeError, "init_slots()", s.step, x[:, :hop])
    for fn, a in ((s.open, (0, e)), (s.end, (0, 1)), (s.close, (0,))):
        raises(RuntimeError, "init_slots()", fn, *a)
    # the slot calls in a block session, flush in a slot session
    s.init_streams(2, embed=torch.cat([d, d]))
    for fn, a in ((s.open, (0, e)), (s.end, (0, 1)), (s.close, (0,))):
        raises(RuntimeError, "init_slots()", fn, *a)
    assert s.active == []
    s.init_slots(2)
    raises(RuntimeError, "close(slot)", s.flush)
    # slots
    raises(IndexError, "0 .. 1", s.open, 2, e)
    raises(IndexError, "0 .. 1", s.close, -1)
    raises(RuntimeError, "open(0)", s.end, 0, 1)
    raises(RuntimeError, "open(1)", s.close, 1)
    # enrolment and embedding
    raises(ValueError, "exactly one of enroll [L'] and embed [192]", s.open, 0)
    raises(ValueError, "exactly one of enroll [L'] and embed [192]", s.open, 0, e, d)
    raises(RuntimeError, "ROCm device", s.open, 0, e.cpu())
    raises(RuntimeError, "ROCm device", s.open, 0, embed=d.cpu())
    raises(ValueError, "[L'] or [1, L']", s.open, 0, det_wave(7, 2, 3000).to(dev))
    raises(ValueError, "[192], [1, 192] or [1, 192, 1]", s.open, 0, embed=torch.cat([d, d]))
    raises(ValueError, "[192], [1, 192] or [1, 192, 1]", s.open, 0, embed=d[0, :100, 0])
    # nothing above opened anything or launched
    assert s.active == [] and s.frames == 0 and int(s._span.abs().sum()) == 0
    s.open(0, e)
    raises(RuntimeError, "close(0)", s.open, 0, embed=d)
    # fewer than win samples: flush()'s rule, per slot
    raises(RuntimeError, "more hops", s.close, 0)
    out = s.step(x[:, :hop])
    assert out.shape == (2, hop)
    raises(RuntimeError, "1 more hops", s.close, 0)
    raises(ValueError, ">= 0", s.end, 0, -1)
    s.end(0, 3)
    raises(RuntimeError, "ended already", s.end, 0, 1)
    raises(RuntimeError, "step them first", s.close, 0)
    s.step_chunk(x[:, :3 * hop].contiguous())
    assert s.close(0).shape == (s.win_length - hop,)
    assert s.active == []
    # the int32 frame counter: the core's check with the slot session's way out, once (the streamer's own does not double up)
    s.open(1, embed=d)
    near = skim.FRAME_LIMIT - 20
    s._counter.fill_(near)
    s.frames = near
    s._span[1, 0] = near                                       # (a stream that is live here)
    # ... and what it returns here is what it returns at a small counter that agrees with `near` modulo K * NS
    y = same_bits_at_a_small_counter(s, H, near, 1, x[:, :8 * hop].contiguous())
    assert bool(torch.isfinite(y).all()) and s.frames == near + 8 and int(s._counter) == near + 8
    with pytest.raises(RuntimeError) as info:
        s.step_chunk(x)
    assert "init_slots()" in str(info.value) and "init_streams()" not in str(info.value)
    assert s.frames == near + 8 and int(s._counter) == near + 8
    s.step_chunk(x[:, :12 * hop].contiguous())
    assert s.frames == skim.FRAME_LIMIT
    raises(RuntimeError, "2**31 - 1", s.step, x[:, :hop].contiguous())
    raises(RuntimeError, "init_slots()", s.open, 0, e)
    assert s.close(1).shape == (s.win_length - hop,)
    # a block session keeps its own way out at the limit
    s.init_streams(2, embed=torch.cat([d, d]))
    s.frames = skim.FRAME_LIMIT
    s._hops = s.prime_hops
    raises(RuntimeError, "init_streams()", s.step, x[:, :hop].contiguous())


def test_a_masker_without_an_embedding_opens_with_neither(dev):
    """A plain causal SkiM separator in slots: open(slot), against its own block session, bit for bit."""
    import puresound_amd.nnet as PA
    from puresound_amd.streaming import StreamingSkiMExtractor
    if "plain" not in _MODELS:
        m = PA.SoTaskWrapModule(PA.FreeEncDec(32, 16, 16, output_active=True),
                                PA.SkiM(16, 8, 16, n_blocks=2, seg_size=5, causal=True), verbose=False).eval()
        m.load_state_dict(det_state_dict(m))
        _MODELS["plain"] = (m.to(dev), None)
    model, _ = _MODELS["plain"]
    s = StreamingSkiMExtractor(model)
    hop, hops = s.hop_length, 57
    x = det_wave(680, 1, hops * hop).to(dev)
    with pytest.raises(ValueError, match="pass neither enroll nor embed"):
        s.init_slots(2)
        s.open(0, enroll=x[0])
    assert s.active == []
    s.step(torch.full((2, hop), NAN, device=dev))                                   # slot 1 is born at frame 2: off the grid
    s.open(1)
    chunk = torch.full((2, hops * hop), NAN, device=dev)
    chunk[1] = x[0]
    y = torch.cat([s.step_chunk(chunk)[1], s.close(1)])
    assert torch.equal(y[s.latency_samples:], _block_session(s, x))
    assert float(y.abs().max()) > 1e-3


def test_model_left_intact(dev):
    import cases
    from puresound_amd.streaming import StreamingSkiMExtractor
    model, _ = _model(VAD, dev)
    c = cases.CASES[VAD]
    x = det_wave(c["seed"], c["B"], c["L"]).to(dev)
    e = det_wave(c["seed"] + 1, c["B"], c["L_enroll"]).to(dev)
    precision = model.masker.gemm_precision
    before = model.inference(x, e)
    params = [p.detach().clone() for p in model.parameters()]
    s = StreamingSkiMExtractor(model)
    streams = _streams(s, dev, [(0, 0, 120, 0), (1, 3, 60, 1), (1, 80, 70, 0)], seed=1000)
    _run_slots(s, 2, streams, (4,))
    _run_slots(s, 2, streams, SCHEDULE, use_graph=False)
    assert model.masker.gemm_precision == precision
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), params))
    assert torch.equal(model.inference(x, e), before)
