"""Slot sessions of StreamingSeparator on the MI355X (init_slots / open / end / close for the causal DPCRN / DPARN noise
suppressors): ps_state_gate_slots_f32 against torch.where on poisoned buffers, and sessions whose streams join, end and leave
on their own against a block session of each stream at the session's width (bit for bit), the offline model and the
reference goldens."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import rel_max
from detweights import det_wave
from test_streaming_long_run_gpu import FRAME_LIMIT, same_bits_at_a_small_counter
from test_streaming_spectral_gpu import NS, TOL, _model, _stream

pytestmark = pytest.mark.gpu
MAX = 2 ** 31 - 1
NAN = float("nan")
HOP, WIN = 128, 512
E_INVALID = -1


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
    junk = [torch.full((1 << 22,), NAN, device=dev) for _ in range(8)]
    junk += [torch.full((n,), NAN, device=dev) for n in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20)]
    del junk
    yield


def _i32(span, dev):
    return span.to(torch.int32).to(dev).contiguous()


def _misaligned(span, dev):
    flat = torch.zeros(span.numel() + 1, dtype=torch.int32, device=dev)
    flat[1:] = span.to(torch.int32).reshape(-1).to(dev)
    view = flat[1:].view(-1, 2)
    assert view.data_ptr() % 8 == 4 and view.is_contiguous()
    return view


# ---- ps_state_gate_slots_f32 --------------------------------------------------------------------------------------------
def _payload(rows, ld, seed, dev):
    """[rows, ld] fp32 whose every element is a NaN with a payload of its own (odd rows: +/- inf in every fourth column), so
    that a kept element is kept in every bit and a product with 0 would not give 0."""
    idx = torch.arange(rows * ld, dtype=torch.int64).view(rows, ld)
    bits = 0x7fc00000 | ((idx * 2654435761 + seed) % 0x3fffff + 1)
    bits[1::2, 0::4] = 0x7f800000                                        # +inf
    bits[1::2, 2::8] = 0xff800000 - (1 << 32)                            # -inf
    return bits.to(torch.int32).to(dev).view(torch.float32)


def _gate_patterns(g):
    """(span, whether frame g is live in it): idle; live throughout (death INT32_MAX); born exactly at g; born one frame
    later; dead exactly at g; dead from the next frame on; a single frame at g; a single frame before g; a finite live stream."""
    return [((0, 0), False), ((0, MAX), True), ((g, MAX), True), ((g + 1, MAX), False), ((0, g), False), ((0, g + 1), True),
            ((g, g + 1), True), ((g - 1, g), False), ((g - 2, g + 5), True)]


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("b", [1, 5, 130])
def test_state_gate_kernel(dev, H, b, shift):
    ld = H.padded_frames(b)
    for t in (9, FRAME_LIMIT - 1):
        g = t - shift
        counter = torch.full((1,), t, dtype=torch.int32, device=dev)
        patterns = _gate_patterns(g)
        for turn in range(len(patterns) if b < len(patterns) else 2):   # every pattern meets every column as the turns go by
            picked = [patterns[(i + turn) % len(patterns)] for i in range(b)]
            span = torch.tensor([p for p, _ in picked], dtype=torch.int64)
            live = (span[:, 0] <= g) & (g < span[:, 1])
            assert live.tolist() == [v for _, v in picked]
            dead = torch.zeros(ld, dtype=torch.bool)
            dead[:b] = ~live                                             # the pad columns b .. ld are never dead
            dead = dead.to(dev)
            xs = [_payload(1, ld, 11 + turn, dev), _payload(21, ld, 12 + turn, dev)]     # two tensors of different rows
            before = [x.view(torch.int32).clone() for x in xs]
            H.state_gate(xs, counter, _i32(span, dev), b, shift=shift)
            for x, was in zip(xs, before):
                want = torch.where(dead[None, :], torch.zeros_like(was), was)          # (int32: an exact +0, kept bits)
                assert torch.equal(x.view(torch.int32), want), (t, turn)
                assert bool(torch.isnan(was[:, dead].view(torch.float32)).logical_or(
                    torch.isinf(was[:, dead].view(torch.float32))).all())              # what died held NaN / inf
        # every stream live: nothing changes, whatever the buffers hold
        xs = [_payload(1, ld, 31, dev), _payload(21, ld, 32, dev)]
        before = [x.view(torch.int32).clone() for x in xs]
        H.state_gate(xs, counter, _i32(torch.tensor([(0, MAX)] * b), dev), b, shift=shift)
        assert all(torch.equal(x.view(torch.int32), was) for x, was in zip(xs, before)), t
        assert int(counter) == t                                         # the gate only reads the counter


def test_state_gate_takes_the_streamers_state_shape(dev, H):
    """[1, H, F * ld]: H * F rows of ld columns, the stream the column within a row (nnet/dpcrn.py forward_step)."""
    b, hid, f = 5, 3, 4
    ld = H.padded_frames(b)
    x = _payload(hid * f, ld, 5, dev).view(1, hid, f * ld)
    was = x.view(torch.int32).clone()
    span = torch.tensor([(0, MAX), (0, 0), (7, MAX), (0, 6), (6, 7)])
    counter = torch.full((1,), 7, dtype=torch.int32, device=dev)
    H.state_gate([x], counter, _i32(span, dev), b)                       # shift = 1: frame 6
    dead = torch.zeros(ld, dtype=torch.bool)
    dead[:b] = torch.tensor([False, True, True, True, False])
    want = torch.where(dead.to(dev)[None, :], torch.zeros_like(was.view(hid * f, ld)), was.view(hid * f, ld))
    assert torch.equal(x.view(torch.int32).view(hid * f, ld), want)


def test_state_gate_refuses_bad_arguments_and_writes_nothing(dev, H):
    from puresound_amd import _abi
    b = 5
    ld = H.padded_frames(b)
    x1, x2 = _payload(1, ld, 1, dev), _payload(21, ld, 2, dev)
    before = [x.view(torch.int32).clone() for x in (x1, x2)]
    span = torch.tensor([(0, 0)] * b)                                    # every column dead: a launch would zero them all
    good, bad = _i32(span, dev), _misaligned(span, dev)
    counter = torch.full((1,), 9, dtype=torch.int32, device=dev)
    sp, st = _abi.ptr, _abi.stream_ptr(dev)

    def table(*rows):
        tab = (_abi.StateRows * len(rows))()
        for e, (p, r) in zip(tab, rows):
            e.x, e.rows = p, r
        return tab

    two = table((sp(x1), 1), (sp(x2), 21))
    big = table(*[(sp(x1), 1)] * (_abi.PS_MAX_RING_PAIRS + 1))
    gate = H.lib().ps_state_gate_slots_f32
    c, g = sp(counter), sp(good)
    refused = [  # (words of the message, arguments)
        ("8-byte aligned", (two, 2, c, None, 1, b, ld, st)),
        ("8-byte aligned", (two, 2, c, sp(bad), 1, b, ld, st)),
        ("counter (device int) is required", (two, 2, None, g, 1, b, ld, st)),
        ("shift >= 0", (two, 2, c, g, -1, b, ld, st)),
        ("1 .. 32 states", (None, 2, c, g, 1, b, ld, st)),
        ("1 .. 32 states", (two, 0, c, g, 1, b, ld, st)),
        ("1 .. 32 states", (big, _abi.PS_MAX_RING_PAIRS + 1, c, g, 1, b, ld, st)),
        ("state 1", (table((sp(x1), 1), (None, 21)), 2, c, g, 1, b, ld, st)),
        ("state 1", (table((sp(x1), 1), (sp(x2) + 4, 20)), 2, c, g, 1, b, ld, st)),      # misaligned
        ("state 0", (table((sp(x1), 0), (sp(x2), 21)), 2, c, g, 1, b, ld, st)),
        ("state 1", (table((sp(x1), 1), (sp(x2), -3)), 2, c, g, 1, b, ld, st)),
        ("B=0", (two, 2, c, g, 1, 0, ld, st)),
        ("B=-1", (two, 2, c, g, 1, -1, ld, st)),
        ("ld=4", (two, 2, c, g, 1, b, 4, st)),                           # ld < B
        ("ld=6", (two, 2, c, g, 1, b, 6, st)),                           # ld % 4
    ]
    for k, (words, args) in enumerate(refused):
        assert gate(*args) == E_INVALID, (k, words)
        assert words in H.lib().ps_last_error().decode(), (k, words, H.lib().ps_last_error().decode())
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        H.state_gate([x1, x2], counter, bad, b)
    with pytest.raises(RuntimeError, match="shift >= 0"):
        H.state_gate([x1, x2], counter, good, b, shift=-1)
    with pytest.raises(RuntimeError, match="1 .. 32 states"):
        H.state_gate([], counter, good, b)
    torch.cuda.synchronize()
    assert all(torch.equal(x.view(torch.int32), was) for x, was in zip((x1, x2), before))
    assert int(counter) == 9
    H.state_gate([x1, x2], counter, good, b)                             # (and the same call with good arguments runs)
    assert bool((x1[:, :b] == 0).all()) and bool((x2[:, :b] == 0).all())
    assert torch.equal(x2.view(torch.int32)[:, b:], before[1][:, b:])


# ---- sessions -----------------------------------------------------------------------------------------------------------
_REFS = {}


def _wave(seed, hops):
    return det_wave(seed, 1, hops * HOP)[0]


def _fp32_inference(model, x):
    model.set_gemm_precision("fp32")
    try:
        return model.inference(x)
    finally:
        model.set_gemm_precision("fp16x2")


def _block_row(key, model, x, capacity, row, dev):
    """Row `row` of an init_streams(capacity) block session fed x from frame 0 (the other rows: silence), emitted samples ‖
    flush(); computed once per key and left unchanged."""
    if key not in _REFS:
        from puresound_amd.streaming import StreamingSeparator
        xs = torch.zeros(capacity, x.shape[0], device=dev)
        xs[row] = x.to(dev)
        _REFS[key] = _stream(StreamingSeparator(model), xs, 5, use_graph=False)[row].clone()
    return _REFS[key]


def _offline(key, model, x, dev):
    if key not in _REFS:
        _REFS[key] = _fp32_inference(model, x[None].to(dev))[0].clone()
    return _REFS[key]


def _run_slots(s, capacity, streams, split, dev, use_graph=True, use_step=False, between=None):
    """streams: dicts(slot, at, x [L], linger).  The session runs in calls of at most `split` hops, cut where a stream opens
    or closes; every row that is idle, or past its stream's last input hop, is fed NaN.  A stream with linger = n > 0 is
    ended ahead (end(slot, hops left) before the call that holds its last input hop -- the call may go on past it) and closed n
    hops after its last input hop; one without is closed right after it, with no end().  between(t) runs before the call
    that starts at hop t.  -> per stream its outputs from open() on ‖ close()."""
    s.init_slots(capacity, use_graph=use_graph)
    plan = []
    for i, st in enumerate(streams):
        hops = st["x"].shape[0] // HOP
        plan.append(dict(i=i, slot=st["slot"], at=st["at"], hops=hops, linger=st.get("linger", 0),
                         close_at=st["at"] + hops + st.get("linger", 0), ended=False))
    total = max(p["close_at"] for p in plan)
    ys = [[] for _ in streams]
    t = 0
    while True:
        for p in plan:
            if p["close_at"] == t:
                ys[p["i"]].append(s.close(p["slot"]))
        for p in plan:
            if p["at"] == t:
                s.open(p["slot"])
        if t == total:
            break
        if between is not None:
            between(t)
        events = [e for p in plan for e in (p["at"], p["close_at"]) if e > t]
        k = min([split] + [e - t for e in events])
        chunk = torch.full((capacity, k * HOP), NAN, device=dev)
        live = [p for p in plan if p["at"] <= t < p["close_at"]]
        for p in live:
            fed = t - p["at"]
            n = max(min(k, p["hops"] - fed), 0)
            if n:
                chunk[p["slot"], :n * HOP] = streams[p["i"]]["x"][fed * HOP:(fed + n) * HOP].to(dev)
            if p["linger"] and not p["ended"] and p["hops"] - fed <= k:  # the stream's last input hop is in this call
                s.end(p["slot"], p["hops"] - fed)
                p["ended"] = True
        out = s.step(chunk) if (use_step and k == 1) else s.step_chunk(chunk)
        assert out.shape == (capacity, k * HOP)
        for p in live:
            ys[p["i"]].append(out[p["slot"]])
        idle = [c for c in range(capacity) if c not in [p["slot"] for p in live]]
        assert bool((out[idle] == 0).all())                              # an idle column emits constrain(0)
        t += k
    assert s.active == []
    return [torch.cat(y) for y in ys]


def _scenario(capacity):
    """Streams born at hops 0, 5 and 9, of 30, 4 (one frame: the shortest a stream may be) and 11 hops; the slot of the
    one-frame stream is closed at hop 9 and reopened there with a fourth stream, which is ended ahead and closed two hops
    late.  capacity 17: the slots lie on both sides of column 16."""
    a, b, c = (0, 1, 2) if capacity == 3 else (0, 16, 5)
    return [dict(slot=a, at=0, x=_wave(101, 30)),
            dict(slot=b, at=5, x=_wave(102, 4)),
            dict(slot=c, at=9, x=_wave(103, 11)),
            dict(slot=b, at=9, x=_wave(104, 7), linger=2)]


def _check_stream(s, y, st, model, name, capacity, i, dev):
    samples = st["x"].shape[0]
    r = s.slot_output_range(samples, WIN, HOP)
    linger = st.get("linger", 0) * HOP
    assert (r.start, y.shape[0]) == (WIN - HOP, r.stop + linger), i
    assert bool((y[:r.start] == 0).all()) and bool((y[r.stop:] == 0).all()), i     # the window fills / the tail has left
    mine = y[r.start:r.stop]
    block = _block_row((name, capacity, i), model, st["x"], capacity, st["slot"], dev)
    assert torch.equal(mine, block), f"stream {i} in slot {st['slot']} is not its row of init_streams({capacity})"
    ref = _offline((name, "offline", i), model, st["x"], dev)
    assert ref.shape == mine.shape
    sl = slice(16, samples - 16)
    err = rel_max(mine[sl].cpu().numpy(), ref[sl].cpu().numpy())
    print(f"spectral_slots {name} capacity={capacity} stream {i} ({samples // HOP} hops): rel_max vs inference {err:.2e}")
    assert err <= TOL, i


@pytest.mark.parametrize("capacity", [3, 17])
@pytest.mark.parametrize("name", NS)
def test_each_slot_is_its_stream(dev, name, capacity):
    from puresound_amd.streaming import StreamingSeparator
    model, _ = _model(name, dev)
    s = StreamingSeparator(model)
    assert (s.delay_frames, s.prime_hops, s.latency_samples) == (0, 3, WIN - HOP)
    streams = _scenario(capacity)
    ys = _run_slots(s, capacity, streams, 5, dev)
    for i, (st, y) in enumerate(zip(streams, ys)):
        _check_stream(s, y, st, model, name, capacity, i, dev)


@pytest.mark.parametrize("name", NS)
def test_golden_stream_in_a_slot_opened_at_hop_5(dev, golden_dir, name):
    from puresound_amd.streaming import StreamingSeparator
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    model, _ = _model(name, dev)
    x = det_wave(1234, 2, 4000)[:, :3968].contiguous()                   # as test_streamed_matches_reference_golden builds it
    s = StreamingSeparator(model)
    ys = _run_slots(s, 3, [dict(slot=0, at=5, x=x[0]), dict(slot=2, at=5, x=x[1])], 8, dev)
    r = s.slot_output_range(x.shape[1], WIN, HOP)
    sl = slice(16, g["wav"].shape[1] - 16)
    for row, y in enumerate(ys):
        mine = y[r.start:r.stop].cpu().numpy()
        assert mine.shape == g["wav"][row].shape
        assert rel_max(mine[sl], g["wav"][row, sl]) <= 1e-4, row


@pytest.mark.parametrize("name", NS)
def test_graph_eager_step_and_chunk_splits_give_the_same_bits(dev, name):
    from puresound_amd.streaming import StreamingSeparator
    model, _ = _model(name, dev)
    s = StreamingSeparator(model)
    streams = _scenario(3)
    runs = {(split, graph): _run_slots(s, 3, streams, split, dev, use_graph=graph, use_step=split == 1)
            for graph in (True, False) for split in (1, 4, 16)}
    base = runs[(1, True)]
    for key, ys in runs.items():
        for i, (a, c) in enumerate(zip(ys, base)):
            assert torch.equal(a, c), (key, i)


@pytest.mark.parametrize("name", NS)
def test_full_session_opened_before_hop_0_is_the_block_session(dev, name):
    from puresound_amd.streaming import StreamingSeparator
    model, _ = _model(name, dev)
    s = StreamingSeparator(model)
    x = det_wave(71, 3, HOP * 23)
    block = _stream(s, x.to(dev), 5)                                     # emitted samples ‖ flush()
    ys = _run_slots(s, 3, [dict(slot=i, at=0, x=x[i]) for i in range(3)], 5, dev)
    r = s.slot_output_range(x.shape[1], WIN, HOP)
    for i in range(3):
        assert bool((ys[i][:r.start] == 0).all())                        # the block session's priming hops: constrain(0) here
        assert torch.equal(ys[i][r.start:r.stop], block[i]), i


def test_the_rules_of_a_slot_session(dev, H):
    from puresound_amd.streaming import StreamingSeparator
    model, _ = _model("ns_dpcrn_short", dev)
    s = StreamingSeparator(model)
    x = det_wave(302, 2, 16 * HOP).to(dev)
    feed = lambda a, b: x[:, a * HOP:b * HOP].contiguous()  # noqa: E731

    def raises(kind, words, fn, *args, **kw):
        with pytest.raises(kind) as info:
            fn(*args, **kw)
        assert words in str(info.value), str(info.value)

    # a block session answers the slot calls with the core's RuntimeError
    s.init_streams(2)
    for call in (lambda: s.open(0), lambda: s.end(0, 0), lambda: s.close(0)):
        raises(RuntimeError, "init_slots()", call)
    s.init_slots(2)
    assert s.active == []
    raises(ValueError, "pass no enroll", s.open, 0, enroll=det_wave(7, 1, 3000)[0].to(dev))
    raises(RuntimeError, "is idle", s.close, 0)
    raises(RuntimeError, "is idle", s.end, 0, 0)
    raises(IndexError, "out of range", s.open, 2)
    assert s.active == [] and s.frames == 0 and int(s._span.abs().sum()) == 0     # nothing above opened or launched anything
    s.open(0)
    raises(RuntimeError, "close(0)", s.open, 0)
    raises(RuntimeError, "close(slot)", s.flush)
    # fewer than n_fft samples: flush()'s rule, per slot
    raises(RuntimeError, "more hops", s.close, 0)
    assert s.step(feed(0, 1)).shape == (2, HOP)                          # from the first hop on
    raises(RuntimeError, "a stream needs 512", s.close, 0)
    raises(RuntimeError, "3 more hops", s.end, 0, 0)
    raises(ValueError, ">= 0", s.end, 0, -1)
    s.end(0, 3)
    raises(RuntimeError, "ended already", s.end, 0, 1)
    raises(RuntimeError, "step them first", s.close, 0)
    s.step_chunk(feed(1, 4))
    assert s.close(0).shape == (WIN - HOP,) and s.active == []
    raises(RuntimeError, "is idle", s.close, 0)

    # the int32 frame counter: near 2^31 / hop (the sample index passes an int) and up to the limit, the bits of the same
    # chunk at a small counter; then _run and open refuse with the slot wording, and nothing has moved
    s.open(1)
    for near, hops in ((2 ** 31 // HOP - 3, 8), (FRAME_LIMIT - 4, 4)):
        s._counter.fill_(near)
        s.frames = near
        s._span[1, 0] = near
        y = same_bits_at_a_small_counter(s, H, near, 1, feed(0, hops))
        assert bool(torch.isfinite(y).all()) and s.frames == near + hops == int(s._counter)
    assert s.frames == FRAME_LIMIT
    raises(RuntimeError, "init_slots()", s.step, feed(0, 1))
    raises(RuntimeError, "2**31 - 1", s.step_chunk, feed(0, 2))
    raises(RuntimeError, "init_slots()", s.open, 0)
    assert s.frames == FRAME_LIMIT == int(s._counter) and s.active == [1]
    assert s.close(1).shape == (WIN - HOP,)


@pytest.mark.parametrize("name", NS)
def test_sessions_do_not_disturb_each_other_and_the_model_is_left_intact(dev, name):
    from puresound_amd.streaming import StreamingSeparator
    model, _ = _model(name, dev)
    x = det_wave(9, 2, HOP * 24).to(dev)
    before = model.inference(x)
    s = StreamingSeparator(model)
    first = _stream(s, x, 4)
    _run_slots(s, 3, _scenario(3)[1:], 4, dev)
    _run_slots(s, 3, _scenario(3)[1:], 1, dev, use_graph=False, use_step=True)
    assert torch.equal(_stream(s, x, 4), first)
    assert all(m.gemm_precision == "fp16x2" for m in model.masker.modules() if hasattr(m, "_plan_get"))
    assert torch.equal(model.inference(x), before)


def test_parameter_update_in_a_running_slot_session_carries_the_state_as_the_block_session_does(dev):
    """An in-place update between two calls drops graphs and packs; the rings, the carried LSTM states and the overlap-add tail
    stay, exactly as in a block session updated at the same frame: a full slot session remains its block twin bit for bit
    across the update, and both differ from the run without it."""
    from puresound_amd.streaming import StreamingSeparator
    base, _ = _model("ns_dpcrn_short", dev)
    x = det_wave(41, 3, HOP * 20)
    at = 10                                                              # hops before the update (a multiple of the call length)

    def update(model):
        with torch.no_grad():
            for p in model.masker.parameters():
                p.mul_(0.9)

    # the block twin: init_streams(3), `at` hops, the update, the rest, flush
    m_block = copy.deepcopy(base)
    sb = StreamingSeparator(m_block)
    sb.init_streams(3)
    outs = [sb.step_chunk(x[:, :at * HOP].contiguous().to(dev))]
    update(m_block)
    outs += [sb.step_chunk(x[:, at * HOP:].contiguous().to(dev)), sb.flush()]
    block = torch.cat(outs, dim=1)

    m_slots = copy.deepcopy(base)
    ss = StreamingSeparator(m_slots)
    seen = {}

    def between(t):
        if t == at:
            seen["graphs"], seen["packs"] = dict(ss._graphs), ss._packs
            update(m_slots)

    streams = [dict(slot=i, at=0, x=x[i]) for i in range(3)]
    ys = _run_slots(ss, 3, streams, 5, dev, between=between)
    assert seen["graphs"] and seen["packs"] is not None and ss._packs is not seen["packs"]
    assert all(ss._graphs.get(k) is not g for k, g in seen["graphs"].items())      # dropped, captured again
    r = ss.slot_output_range(x.shape[1], WIN, HOP)
    for i in range(3):
        assert torch.equal(ys[i][r.start:r.stop], block[i]), i
    plain = _run_slots(StreamingSeparator(base), 3, streams, 5, dev)
    cut = r.start + (at - 3) * HOP                                       # the samples of the frames before the update
    assert torch.equal(plain[0][:cut], ys[0][:cut]) and not torch.equal(plain[0][cut:], ys[0][cut:])
