"""Slot sessions of StreamingDPRNN on the MI355X (init_slots / open / end / close): ps_dprnn_block_step_slots_f32 against the
fp64 frame loop of tests/dprnn_slots_ref.py and against its sibling, and the streamer: streams that begin and end on their
own against offline inference, against the block session and against each other (isolation and slot re-use), bit for bit,
graph against eager.  The driver of a slot session (_run_slots) is the one of the Conv-TasNet slot tests."""
import contextlib

import numpy as np
import pytest
import torch

import cases
import dprnn_slots_ref as RS
import dprnn_step_ref as R
from conftest import rel_max
from detweights import det_state_dict, det_wave
from test_streaming_long_run_gpu import same_bits_at_a_small_counter
from test_streaming_slots_gpu import _run_slots, _zero

pytestmark = pytest.mark.gpu
TOL = 1e-4
SCHEDULE = (1, 3, 8, 16, 37)
NAN = float("nan")
I32_MAX = 2 ** 31 - 1


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
_PASSES = {}
STATE_KEYS = ("h_intra", "c_intra", "h_bank", "c_bank")


def _passes(c, h, dev, H):
    """The two passes of one block at (C, H): torch modules (for the reference) and their device packs, made once."""
    if (c, h) not in _PASSES:
        intra, inter = R.make_pass(c, h, 11 * c + h), R.make_pass(c, h, 13 * c + h)
        _PASSES[(c, h)] = (intra, inter, H.pack_dprnn_pass(*intra, dev), H.pack_dprnn_pass(*inter, dev))
    return _PASSES[(c, h)]


def _rand(shape, seed):
    g = np.random.Generator(np.random.Philox(key=seed))
    return torch.tensor(g.uniform(-1.0, 1.0, shape), dtype=torch.float64)


def _chunks(total, k_max=16):
    """Chunk lengths 1, 2, ..., k_max, 1, 2, ... covering `total` frames (they begin at 0, 1, 3, 6, 10, 15, 21, ...)."""
    out, k = [], 1
    while sum(out) < total:
        out.append(min(k, total - sum(out)))
        k = k % k_max + 1
    return out


def _cycled_spans(k, c0, b):
    """Offsets from the starting counter c0: empty; all live; birth inside the chunk 6 .. 9 at a frame that is no multiple of
    K (7 and 3K + 9); death inside the chunk 10 .. 14; birth and death inside the chunk 15 .. 20; birth at the next multiple
    of K; a span of K - 2 frames."""
    base = [(0, 0), (c0, I32_MAX), (c0 + 7, I32_MAX), (c0, c0 + 12), (c0 + 16, c0 + 19), ((c0 // k + 1) * k, I32_MAX),
            (c0 + 3, c0 + 3 + k - 2)]
    assert (c0 + 7) % k and base[5][0] % k == 0
    return [base[i % len(base)] for i in range(b)]


def _tiled_spans(k, c0, b):
    """Whole tiles of 16 columns that are dead for a while: tile 0 never lives, tile 1 is born at offset 7 and dies at 30,
    tile 2 (ragged) lives from offset 2 except one column."""
    return [(0, 0) if col < 16 else (c0 + 7, c0 + 30) if col < 32 else (c0 + 2, I32_MAX) if col != 35 else (0, 0)
            for col in range(b)]


def _device_states(state, h, b, ldb, dev):
    st = {}
    for key, t in state.items():                       # columns past B hold NaN: never read, never written
        full = torch.full(t.shape[:-2] + (h, ldb), NAN, device=dev)
        full[..., :b] = t.transpose(-1, -2).float().to(dev)
        st[key] = full
    return st


def _check_slot_kernel(dev, H, c, h, k, b, c0, spans):
    t_len = 3 * k + 11
    intra, inter, pk_intra, pk_inter = _passes(c, h, dev, H)
    seed = 100000 * c + 1000 * b + c0
    x = _rand((t_len, b, c), seed)
    state = dict(h_intra=_rand((b, h), seed + 1), c_intra=_rand((b, h), seed + 2),      # random: a missed reset or a wrong
                 h_bank=_rand((k, b, h), seed + 3), c_bank=_rand((k, b, h), seed + 4))  # slot shows
    live = torch.tensor([[lo <= c0 + f < hi for (lo, hi) in spans] for f in range(t_len)])   # [T, B]
    assert H.dprnn_block_step_ok(c, h, k)
    ldb = H.padded_frames(b)
    st = _device_states(state, h, b, ldb, dev)
    st_first = {key: t.clone() for key, t in st.items()}
    span = torch.tensor(spans, dtype=torch.int32, device=dev)
    counter = torch.tensor([c0], dtype=torch.int32, device=dev)
    got_live, want_live, seen, t = [], [], [set() for _ in spans], 0
    for n in _chunks(t_len):
        want, vis = RS.block_step_slots(x[t:t + n], c0 + t, k, intra, inter, state, spans)
        seen = [a | v for a, v in zip(seen, vis)]
        xs = x[t:t + n].clone()
        xs[~live[t:t + n]] = NAN                                                    # dead frames carry NaN
        ld = H.padded_frames(n * b)
        xin = torch.full((1, c, ld), NAN, device=dev)
        xin[0, :, :n * b] = xs.permute(2, 0, 1).reshape(c, n * b).float().to(dev)
        out = torch.full((1, c, ld), 7.0, device=dev)
        st0 = {key: v.clone() for key, v in st.items()}
        H.dprnn_block_step(xin, counter, pk_intra, pk_inter, st["h_intra"], st["c_intra"], st["h_bank"], st["c_bank"], b, n,
                           out=out, span=span)
        torch.cuda.synchronize()
        assert int(counter[0]) == c0 + t                                            # read, never written
        assert bool((out[0, :, n * b:] == 7.0).all())                               # columns past the chunk are not written
        got = out[0, :, :n * b].reshape(c, n, b).permute(1, 2, 0).cpu()
        assert bool(torch.isfinite(got).all()), t                                   # every y column of the chunk, dead ones too
        got_live.append(got[live[t:t + n]])
        want_live.append(want[live[t:t + n]])
        idle = (~live[t:t + n].any(dim=0)).to(dev)                                  # columns with no live frame in this launch
        for key in STATE_KEYS:
            assert torch.equal(st[key][..., :b][..., idle], st0[key][..., :b][..., idle]), (key, t)
            assert bool(torch.isnan(st[key][..., b:]).all()), key
        counter += n
        t += n
    errs = {"out": rel_max(torch.cat(got_live).numpy(), torch.cat(want_live).numpy())}
    for key, ref in state.items():
        errs[key] = rel_max(st[key][..., :b].transpose(-1, -2).cpu().numpy(), ref.numpy())
    print(f"dprnn_block_step_slots C={c} H={h} K={k} B={b} c0={c0}: rel_max " +
          " ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    assert max(errs.values()) < 1e-5, errs
    for col in range(b):                                                            # bank slots not visited: the same bits
        for p in set(range(k)) - seen[col]:
            for key in ("h_bank", "c_bank"):
                assert torch.equal(st[key][p, :, col], st_first[key][p, :, col]), (key, p, col)
    assert any(len(s) == k for s in seen)                                           # (a column went round its banks)


@pytest.mark.parametrize("start", ["0", "3K+2"])
@pytest.mark.parametrize("b", [3, 70])
@pytest.mark.parametrize("c,h,k", [(16, 8, 5), (128, 64, 20)])
def test_block_step_slots_kernel(dev, H, c, h, k, b, start):
    c0 = {"0": 0, "3K+2": 3 * k + 2}[start]
    _check_slot_kernel(dev, H, c, h, k, b, c0, _cycled_spans(k, c0, b))


@pytest.mark.parametrize("c,h,k", [(16, 8, 5), (128, 64, 20)])
def test_block_step_slots_kernel_with_dead_tiles(dev, H, c, h, k):
    """(the cycled spans put a live column into every tile: here whole tiles are dead, for all frames or for some)"""
    _check_slot_kernel(dev, H, c, h, k, 40, 3 * k + 2, _tiled_spans(k, 3 * k + 2, 40))


@pytest.mark.parametrize("c,h,k", [(16, 8, 5), (128, 64, 20)])
def test_all_live_span_is_the_sibling_bit_for_bit(dev, H, c, h, k):
    b, t_len = 70, 3 * k + 11
    intra, inter, pk_intra, pk_inter = _passes(c, h, dev, H)
    seed = 7000 + c
    x = _rand((t_len, b, c), seed)
    state = dict(h_intra=_rand((b, h), seed + 1), c_intra=_rand((b, h), seed + 2),
                 h_bank=_rand((k, b, h), seed + 3), c_bank=_rand((k, b, h), seed + 4))
    ldb = H.padded_frames(b)
    sa, sb = _device_states(state, h, b, ldb, dev), _device_states(state, h, b, ldb, dev)
    span = torch.tensor([(0, I32_MAX)] * b, dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    t = 0
    for n in _chunks(t_len):
        ld = H.padded_frames(n * b)
        xin = torch.full((1, c, ld), NAN, device=dev)
        xin[0, :, :n * b] = x[t:t + n].permute(2, 0, 1).reshape(c, n * b).float().to(dev)
        ya, yb = torch.full((1, c, ld), 7.0, device=dev), torch.full((1, c, ld), 7.0, device=dev)
        H.dprnn_block_step(xin, counter, pk_intra, pk_inter, *(sa[key] for key in STATE_KEYS), b, n, out=ya)
        H.dprnn_block_step(xin, counter, pk_intra, pk_inter, *(sb[key] for key in STATE_KEYS), b, n, out=yb, span=span)
        assert torch.equal(ya, yb), t
        for key in STATE_KEYS:
            assert torch.equal(sa[key][..., :b], sb[key][..., :b]), (key, t)
        counter += n
        t += n
    assert bool(torch.isfinite(ya[0, :, :n * b]).all())


def test_block_step_slots_kernel_refusals(dev, H):
    """A null or misaligned span (PS_E_INVALID) and a shape without a kernel (PS_E_UNSUPPORTED): nothing is written."""
    import ctypes as C
    z = lambda *shape: torch.zeros(*shape, device=dev)  # noqa: E731

    def attempt(c, h, k, b, span_ptr, rc, word):
        intra, inter = R.make_pass(c, h, 1), R.make_pass(c, h, 2)
        pi, pe = H.pack_dprnn_pass(*intra, dev), H.pack_dprnn_pass(*inter, dev)
        ld, ldb = H.padded_frames(b), H.padded_frames(b)
        x, out = z(1, c, ld), torch.full((1, c, ld), 7.0, device=dev)
        states = [torch.full(s, 3.0, device=dev) for s in ((h, ldb), (h, ldb), (k, h, ldb), (k, h, ldb))]
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        got = H.lib().ps_dprnn_block_step_slots_f32(H.ptr(x), H.ptr(out), H.ptr(counter), span_ptr, C.byref(pi["struct"]),
                                                    C.byref(pe["struct"]), *(H.ptr(s) for s in states), c, h, k, b, 1, ld, ldb,
                                                    H.stream_ptr(dev))
        torch.cuda.synchronize()
        assert got == rc
        assert word in H.lib().ps_last_error().decode()
        assert bool((out == 7.0).all()) and all(bool((s == 3.0).all()) for s in states)

    buf = torch.zeros(2 * 2 + 2, dtype=torch.int32, device=dev)
    assert buf.data_ptr() % 8 == 0
    attempt(16, 8, 5, 2, None, -1, "span")
    attempt(16, 8, 5, 2, buf.data_ptr() + 4, -1, "span")
    attempt(512, 128, 4, 2, buf.data_ptr(), -3, "LDS")
    assert not H.dprnn_block_step_ok(512, 128, 4)
    # through the wrapper: a contiguous [2, 2] view that begins 4 bytes into its storage
    intra, inter = R.make_pass(16, 8, 1), R.make_pass(16, 8, 2)
    ld = ldb = H.padded_frames(2)
    out = torch.full((1, 16, ld), 7.0, device=dev)
    with pytest.raises(RuntimeError, match=r"rc=-1.*span"):
        H.dprnn_block_step(z(1, 16, ld), torch.zeros(1, dtype=torch.int32, device=dev), H.pack_dprnn_pass(*intra, dev),
                           H.pack_dprnn_pass(*inter, dev), z(8, ldb), z(8, ldb), z(5, 8, ldb), z(5, 8, ldb), 2, 1, out=out,
                           span=buf[1:5].view(2, 2))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# -------------------------------------------------------------------------------------------------------------------------
# the streamer
# -------------------------------------------------------------------------------------------------------------------------
_MODELS = {}
NAMES = ["cfg4_short", "cfg4_tse_short"]


def _model(name, dev):
    if name not in _MODELS:
        import puresound_amd.nnet as PA
        m = cases.build(PA.NS, name).eval()
        sd = det_state_dict(m)
        m.load_state_dict(sd)
        _MODELS[name] = (m.to(dev), sd)
    return _MODELS[name]


def _streams(model, s, dev, plan, seed):
    """plan: (slot, start hop, length in hops, chunks between the stream's end and its close) -> stream dicts with a
    deterministic signal and, for an enrolment-seeded model, an enrolment of its own."""
    out = []
    for i, (slot, start, hops, linger) in enumerate(plan):
        x = det_wave(seed + 2 * i, 1, hops * s.hop_length)[0].to(dev)
        e = det_wave(seed + 2 * i + 1, 1, 3000 + 100 * i)[0].to(dev) if model.embedding_free_tse else None
        out.append(dict(id=i, slot=slot, start=start, x=x, e=e, hops=hops, linger=linger))
    return out


@contextlib.contextmanager
def _fp32(model):
    """The arrangement of test_long_streams_match_offline_fp32: the model computes in exact fp32 while the streams run (the
    enrolment pass of open()) and for the offline call, and is put back after."""
    before = model.masker.gemm_precision
    model.set_gemm_precision("fp32")
    try:
        yield
    finally:
        model.set_gemm_precision(before)


def _offline(model, streams):
    """model.inference of every stream alone (inside _fp32)."""
    return {st["id"]: (model.inference(st["x"][None], st["e"][None]) if st["e"] is not None
                       else model.inference(st["x"][None]))[0] for st in streams}


def _check_against_offline(s, streams, ys, refs):
    lat = s.latency_samples
    for st in streams:
        y, ref = ys[st["id"]], refs[st["id"]]
        r = s.slot_output_range(st["x"].numel(), s.win_length, s.hop_length)
        assert (r.start, len(r)) == (lat, ref.numel())
        assert bool(torch.isfinite(y).all()), st["id"]
        err = rel_max(y[r.start:r.stop].cpu().numpy(), ref.cpu().numpy())
        print(f"stream {st['id']} (slot {st['slot']}, {st['hops']} hops): rel_max against offline {err:.3e}")
        assert err <= TOL, (st["id"], err)
        rest = torch.cat([y[:r.start], y[r.stop:]])
        assert torch.equal(rest, torch.full_like(rest, _zero(s))), st["id"]


# six streams in four slots; slots 1 and 3 are used twice.  No start and no length is a multiple of the segment (20 frames) or
# of a chunk length of the schedule
PLAN = [(0, 0, 400, 0), (1, 5, 100, 2), (2, 5, 233, 0), (3, 17, 47, 1), (1, 150, 211, 3), (3, 90, 105, 0)]


@pytest.mark.parametrize("name", NAMES)
def test_staggered_streams_match_offline(dev, name):
    from puresound_amd.streaming import StreamingDPRNN
    model, _ = _model(name, dev)
    s = StreamingDPRNN(model)
    assert s.model.masker.seg_size == 20
    streams = _streams(model, s, dev, PLAN, seed=500)
    graphs = []

    def probe(s_):
        graphs.append(dict(s_._graphs))

    with _fp32(model):
        ys, opened_at = _run_slots(s, 4, streams, SCHEDULE, probe=probe)    # (asserts constrain(0) of idle slots fed NaN)
        refs = _offline(model, streams)
    assert len(ys) == 6
    assert any(t % 20 for t in opened_at.values())                           # opened off the segment grid
    _check_against_offline(s, streams, ys, refs)
    # graphs: one per distinct piece length (37 = 16 + 16 + 5), and open / end / close never replaced one
    assert sorted(s._graphs) == [1, 3, 5, 8, 16]
    for a, b in zip(graphs, graphs[1:]):
        assert all(b[k] is g for k, g in a.items())
    assert all(s._graphs[k] is g for k, g in graphs[-1].items())


def test_slot_session_is_the_block_session_bit_for_bit(dev):
    """The same B streams opened together at hop 0 and never ended early, against an init_streams session."""
    from puresound_amd.streaming import StreamingDPRNN
    model, _ = _model("cfg4_short", dev)
    s = StreamingDPRNN(model)
    b, hops, k = 4, 203, 8
    hop, lat = s.hop_length, s.latency_samples
    x = det_wave(610, b, hops * hop).to(dev)
    pieces = [x[:, i * hop:min(i + k, hops) * hop].contiguous() for i in range(0, hops, k)]
    s.init_streams(b)
    block = torch.cat([s.step_chunk(p) for p in pieces] + [s.flush()], dim=1)
    s.init_slots(b)
    for i in range(b):
        s.open(i)
    outs = [s.step_chunk(p) for p in pieces]
    slots = torch.cat(outs + [torch.stack([s.close(i) for i in range(b)])], dim=1)
    assert s.active == []
    assert slots.shape[1] == block.shape[1] + lat
    assert torch.equal(slots[:, :lat], torch.full_like(slots[:, :lat], _zero(s)))
    assert torch.equal(slots[:, lat:], block)
    assert float(block.abs().max()) > 1e-3


def test_each_slot_is_a_block_session_of_its_stream_bit_for_bit(dev):
    """Enrolment-seeded: every slot of a full session against an init_streams(1, enroll_i) session of that stream alone (one
    enrolment per batch on both sides, so the enrolment pass runs on the same shapes)."""
    from puresound_amd.streaming import StreamingDPRNN
    model, _ = _model("cfg4_tse_short", dev)
    s = StreamingDPRNN(model)
    b, hops, k = 4, 203, 8
    hop, lat = s.hop_length, s.latency_samples
    x = det_wave(620, b, hops * hop).to(dev)
    e = [det_wave(621 + i, 1, 3000 + 160 * i).to(dev) for i in range(b)]
    cut = lambda t: [t[:, i * hop:min(i + k, hops) * hop].contiguous() for i in range(0, hops, k)]  # noqa: E731
    s.init_slots(b)
    for i in range(b):
        s.open(i, e[i][0])
    outs = [s.step_chunk(p) for p in cut(x)]
    slots = torch.cat(outs + [torch.stack([s.close(i) for i in range(b)])], dim=1)
    for i in range(b):
        s.init_streams(1, e[i])
        block = torch.cat([s.step_chunk(p) for p in cut(x[i:i + 1])] + [s.flush()], dim=1)
        assert torch.equal(slots[i, lat:], block[0]), i
    assert not torch.equal(slots[0], slots[1])


def test_isolation_bit_for_bit(dev):
    """Slot 1's whole output does not depend on what slots 0, 2, 3 do: idle with NaN input, or opening, ending and re-opening
    around it."""
    from puresound_amd.streaming import StreamingDPRNN
    model, _ = _model("cfg4_tse_short", dev)
    s = StreamingDPRNN(model)
    mine = (1, 3, 400, 1)
    alone = _streams(model, s, dev, [mine], seed=700)
    crowd = alone + _streams(model, s, dev, [(0, 0, 60, 0), (2, 1, 150, 2), (3, 9, 31, 0), (0, 100, 90, 1), (3, 77, 200, 0),
                                             (2, 250, 120, 0), (0, 260, 100, 0)], seed=720)
    for i, st in enumerate(crowd):
        st["id"] = i
    ya, _ = _run_slots(s, 4, alone, SCHEDULE)
    yb, _ = _run_slots(s, 4, crowd, SCHEDULE)
    assert len(yb) == 8
    assert ya[0].numel() >= 400 * s.hop_length + s.latency_samples
    assert torch.equal(ya[0], yb[0])
    assert float(ya[0].abs().max()) > 1e-3


def test_reused_slot_does_not_see_its_predecessor(dev):
    """Stream A then stream B in slot 0, against stream B in a fresh session opened at the same counter value (a dummy in
    slot 1 advances it): the same bits.  A bank slot or an intra state that open() left behind would show."""
    from puresound_amd.streaming import StreamingDPRNN
    model, _ = _model("cfg4_tse_short", dev)
    s = StreamingDPRNN(model)
    a, b = _streams(model, s, dev, [(0, 0, 350, 0), (0, 360, 320, 0)], seed=800)
    dummy = _streams(model, s, dev, [(1, 0, 350, 0)], seed=810)[0]
    dummy["id"] = 2
    with _fp32(model):
        y1, at1 = _run_slots(s, 2, [a, b], SCHEDULE)
        y2, at2 = _run_slots(s, 2, [dummy, b], SCHEDULE)
        refs = _offline(model, [b])
    assert at1[b["id"]] == at2[b["id"]] > 350
    assert torch.equal(y1[b["id"]], y2[b["id"]])
    _check_against_offline(s, [b], y1, refs)


@pytest.mark.parametrize("name", NAMES)
def test_graph_and_eager_are_bit_identical(dev, name):
    from puresound_amd.streaming import StreamingDPRNN
    model, _ = _model(name, dev)
    s = StreamingDPRNN(model)
    plan = [(0, 0, 300, 0), (1, 5, 100, 2), (2, 5, 133, 0), (1, 150, 90, 0)]
    streams = _streams(model, s, dev, plan, seed=900)
    yg, _ = _run_slots(s, 3, streams, SCHEDULE, use_graph=True)
    assert len(s._graphs) > 0
    ye, _ = _run_slots(s, 3, streams, SCHEDULE, use_graph=False)
    assert len(s._graphs) == 0
    for i in yg:
        assert torch.equal(yg[i], ye[i]), i


@pytest.mark.parametrize("name", NAMES)
def test_end_inside_a_chunk(dev, name):
    """A stream with 5 hops left in a 16-hop chunk padded with NaN: finite output equal to offline; the slot's output hops
    after the end carry the tail, then constrain(0)."""
    from puresound_amd.streaming import StreamingDPRNN
    model, _ = _model(name, dev)
    s = StreamingDPRNN(model)
    st = _streams(model, s, dev, [(1, 0, 16 * 4 + 5, 0)], seed=950)[0]
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
    assert float(after[:lat].abs().max()) > 0                 # the tail: the last frame's overlap
    assert torch.equal(after[lat:], torch.full_like(after[lat:], _zero(s)))
    assert torch.equal(last, torch.full_like(last, _zero(s)))


def test_errors_name_the_way_out(dev, H):
    from puresound_amd.streaming import StreamingDPRNN, dprnn
    model, _ = _model("cfg4_tse_short", dev)
    plain, _ = _model("cfg4_short", dev)
    s = StreamingDPRNN(model)
    hop = s.hop_length
    e = det_wave(5, 1, 3000)[0].to(dev)
    x = det_wave(6, 2, 8 * hop).to(dev)

    def raises(exc, words, fn, *a):
        with pytest.raises(exc) as info:
            fn(*a)
        assert words.lower() in str(info.value).lower(), str(info.value)

    raises(RuntimeError, "init_slots()", s.step, x[:, :hop])
    # the slot calls in a block session, flush in a slot session
    s.init_streams(2, det_wave(7, 2, 3000).to(dev))
    for fn, a in ((s.open, (0, e)), (s.end, (0, 1)), (s.close, (0,))):
        raises(RuntimeError, "init_slots", fn, *a)
    assert s.active == []
    s.init_slots(2)
    raises(RuntimeError, "close(slot)", s.flush)
    # slots
    raises(IndexError, "0 .. 1", s.open, 2, e)
    raises(IndexError, "0 .. 1", s.close, -1)
    raises(RuntimeError, "open(0)", s.end, 0, 1)
    raises(RuntimeError, "open(1)", s.close, 1)
    # enrolment
    raises(ValueError, "pass enroll", s.open, 0)
    raises(RuntimeError, "ROCm device", s.open, 0, e.cpu())
    raises(ValueError, "[L']", s.open, 0, det_wave(7, 2, 3000).to(dev))
    sp = StreamingDPRNN(plain)
    sp.init_slots(1)
    raises(ValueError, "pass no enroll", sp.open, 0, e)
    # nothing above opened anything or launched
    assert s.active == [] and s.frames == 0 and int(s._span.abs().sum()) == 0
    s.open(0, e)
    raises(RuntimeError, "close(0)", s.open, 0, e)
    # fewer than win samples: flush()'s rule, per slot
    raises(RuntimeError, "more hops", s.close, 0)
    out = s.step(x[:, :hop])
    assert out.shape == (2, hop)
    raises(RuntimeError, "1 more hops", s.close, 0)
    raises(RuntimeError, "more hops", s.end, 0, 0)
    raises(ValueError, ">= 0", s.end, 0, -1)
    s.end(0, 3)
    raises(RuntimeError, "ended already", s.end, 0, 1)
    raises(RuntimeError, "step them first", s.close, 0)
    s.step_chunk(x[:, :3 * hop].contiguous())
    assert s.close(0).shape == (s.win_length - hop,)
    assert s.active == []
    # the int32 frame counter
    s.open(1, e)
    near = dprnn.FRAME_LIMIT - 20
    s._counter.fill_(near)
    s.frames = near
    s._span[1, 0] = near                                       # (a stream that is live here)
    # ... and what it returns here is what it returns at a small counter that agrees with `near` modulo the segment size
    y = same_bits_at_a_small_counter(s, H, near, 1, x[:, :8 * hop].contiguous())
    assert bool(torch.isfinite(y).all()) and s.frames == near + 8 and int(s._counter) == near + 8
    raises(RuntimeError, "init_slots()", s.step_chunk, det_wave(8, 2, 16 * hop).to(dev))
    assert s.frames == near + 8 and int(s._counter) == near + 8
    s.step_chunk(x[:, :8 * hop].contiguous())
    s.step_chunk(x[:, :4 * hop].contiguous())
    assert s.frames == dprnn.FRAME_LIMIT
    raises(RuntimeError, "2**31 - 1", s.step, x[:, :hop].contiguous())
    raises(RuntimeError, "init_slots()", s.open, 0, e)
    assert s.close(1).shape == (s.win_length - hop,)
    # a block session keeps its own way out at the limit
    s.init_streams(2, det_wave(7, 2, 3000).to(dev))
    s.frames = dprnn.FRAME_LIMIT
    s._hops = s.prime_hops
    raises(RuntimeError, "init_streams()", s.step, x[:, :hop].contiguous())


def test_model_left_intact(dev):
    from puresound_amd.streaming import StreamingDPRNN
    name = "cfg4_tse_short"
    model, _ = _model(name, dev)
    c = cases.CASES[name]
    x = det_wave(c["seed"], c["B"], c["L"]).to(dev)
    e = det_wave(c["seed"] + 1, c["B"], c["L_enroll"]).to(dev)
    precision = model.masker.gemm_precision
    before = model.inference(x, e)
    params = [p.detach().clone() for p in model.parameters()]
    s = StreamingDPRNN(model)
    streams = _streams(model, s, dev, [(0, 0, 120, 0), (1, 3, 60, 1), (1, 80, 70, 0)], seed=1000)
    _run_slots(s, 2, streams, (4,))
    _run_slots(s, 2, streams, SCHEDULE, use_graph=False)
    assert model.masker.gemm_precision == precision
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), params))
    assert torch.equal(model.inference(x, e), before)
