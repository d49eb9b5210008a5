"""Slot sessions of StreamingConvTasNet on the MI355X (init_slots / open / end / close): streams that begin and end on their own
against offline inference, against the block session, against each other (isolation and slot re-use, bit for bit), graph
against eager, and unit checks of ps_dwconv_step_slots_f32 / ps_free_decode_step_slots_f32."""
import contextlib
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
from conftest import rel_max
from detweights import det_state_dict, det_wave
from test_streaming_long_run_gpu import same_bits_at_a_small_counter

pytestmark = pytest.mark.gpu
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


_MODELS = {}
CLN = dict(tcn_norm="cLN", dconv_norm="cLN")
MODELS = [("cfg3_causal_short", {}), ("tiny_free_relu_causal", {}), ("tiny_free_relu_causal", CLN)]
MODEL_IDS = ["cfg3_causal_short", "tiny_free_relu_causal", "tiny_free_relu_causal-cLN"]


def _case(name, masker_kw):
    c = copy.deepcopy(cases.CASES[name])
    c["masker"].update(masker_kw)
    return c


def _model(name, dev, **masker_kw):
    key = (name, tuple(sorted(masker_kw.items())))
    if key not in _MODELS:
        import puresound_amd.nnet as PA
        saved = cases.CASES[name]
        cases.CASES[name] = _case(name, masker_kw)
        try:
            m = cases.build(PA.NS, name).eval()
        finally:
            cases.CASES[name] = saved
        sd = det_state_dict(m)
        m.load_state_dict(sd)
        _MODELS[key] = (m.to(dev), sd)
    return _MODELS[key]


def _zero(s):
    """constrain(0): what an idle slot returns."""
    return 0.5 if s._out_mode == "sigmoid" else 0.0


def _streams(model, s, dev, plan, seed):
    """plan: (slot, start hop, length in hops, chunks between the stream's end and its close) -> stream dicts with a
    deterministic signal and, for a speaker model, an enrolment of its own."""
    out = []
    for i, (slot, start, hops, linger) in enumerate(plan):
        x = det_wave(seed + 2 * i, 1, hops * s.hop_length)[0].to(dev)
        e = det_wave(seed + 2 * i + 1, 1, 3000 + 100 * i)[0].to(dev) if model.speaker_net is not None else None
        out.append(dict(id=i, slot=slot, start=start, x=x, e=e, hops=hops, linger=linger))
    return out


def _run_slots(s, capacity, streams, schedule, use_graph=True, fill=NAN, probe=None):
    """Drive a slot session: stream i is opened in its slot at the first call boundary at or after its start hop, fed from
    there, ended (end(slot, hops left)) before the call that carries its last hop, and closed `linger` calls later.  Input
    of idle slots and after a stream's end is `fill`.  -> {id: y}, y = every output of the slot from open to close ‖ close();
    checks on the way that idle slots return constrain(0) exactly.  probe(s): called after every open / end / close."""
    hop = s.hop_length
    s.init_slots(capacity, use_graph=use_graph)
    probe = probe or (lambda _s: None)
    pending = sorted(streams, key=lambda st: st["start"])
    live, ys, opened_at = {}, {}, {}
    t = j = 0
    while pending or live:
        for slot, st in list(live.items()):
            if st["ended"]:
                if st["left"] == 0:
                    ys[st["id"]].append(s.close(slot))
                    probe(s)
                    del live[slot]
                    assert slot not in s.active
                else:
                    st["left"] -= 1
        for st in [p for p in pending if p["start"] <= t and p["slot"] not in live]:
            pending.remove(st)
            s.open(st["slot"], st["e"])
            probe(s)
            live[st["slot"]] = dict(st, pos=0, ended=False, left=st["linger"])
            ys[st["id"]] = []
            opened_at[st["id"]] = t
        assert sorted(live) == s.active
        k = schedule[j % len(schedule)]
        j += 1
        chunk = torch.full((capacity, k * hop), fill, device=s.device)
        for slot, st in live.items():
            rem = st["hops"] - st["pos"]
            n = min(rem, k)
            chunk[slot, :n * hop] = st["x"][st["pos"] * hop:(st["pos"] + n) * hop]
            if rem <= k and not st["ended"]:
                s.end(slot, rem)
                probe(s)
                st["ended"] = True
            st["pos"] += n
        out = s.step_chunk(chunk) if k > 1 else s.step(chunk)
        assert out.shape == (capacity, k * hop)
        for slot in range(capacity):
            if slot in live:
                ys[live[slot]["id"]].append(out[slot])
            else:
                assert torch.equal(out[slot], torch.full_like(out[slot], _zero(s))), (t, slot)
        t += k
    assert s.frames == t
    return {i: torch.cat(y) for i, y in ys.items()}, opened_at


@contextlib.contextmanager
def _fp32(model):
    """The arrangement of test_long_streams_match_offline_fp32: the model computes in exact fp32 while the streams run (the
    enrolment embedding of open()) and for the offline call, and is put back after."""
    model.set_gemm_precision("fp32")
    try:
        yield
    finally:
        model.set_gemm_precision("fp16x2")


def _offline(model, streams):
    """model.inference of every stream alone (inside _fp32)."""
    return {st["id"]: (model.inference(st["x"][None], st["e"][None]) if st["e"] is not None
                       else model.inference(st["x"][None]))[0] for st in streams}


def _check_against_offline(s, streams, ys, refs, bound=1e-5):
    lat = s.latency_samples
    for st in streams:
        y, ref = ys[st["id"]], refs[st["id"]]
        r = s.slot_output_range(st["x"].numel(), s.win_length, s.hop_length)
        assert (r.start, len(r)) == (lat, ref.numel())
        assert bool(torch.isfinite(y).all()), st["id"]
        err = rel_max(y[r.start:r.stop].cpu().numpy(), ref.cpu().numpy())
        print(f"stream {st['id']} (slot {st['slot']}, {st['hops']} hops): rel_max against offline {err:.3e}")
        assert err <= bound, (st["id"], err)
        rest = torch.cat([y[:r.start], y[r.stop:]])
        assert torch.equal(rest, torch.full_like(rest, _zero(s))), st["id"]


# six streams in four slots; slots 1 and 3 are used twice.  1500 hops wrap the preset's largest ring (288 slots) five times, 47
# and 100 hops are shorter than it; no start and no length is a multiple of a chunk length of the schedule
PLAN = [(0, 0, 1500, 0), (1, 5, 100, 2), (2, 5, 333, 0), (3, 17, 47, 1), (1, 200, 611, 3), (3, 90, 205, 0)]


@pytest.mark.parametrize("name,kw", MODELS, ids=MODEL_IDS)
def test_staggered_streams_match_offline(dev, name, kw):
    from puresound_amd.streaming import StreamingConvTasNet
    model, _ = _model(name, dev, **kw)
    s = StreamingConvTasNet(model)
    streams = _streams(model, s, dev, PLAN, seed=500)
    graphs = []

    def probe(s_):
        graphs.append(dict(s_._graphs))

    with _fp32(model):
        ys, opened_at = _run_slots(s, 4, streams, SCHEDULE, probe=probe)
        refs = _offline(model, streams)
    assert len(ys) == 6
    assert any(t % k for t in opened_at.values() for k in SCHEDULE[1:])         # opened off the chunk grid
    _check_against_offline(s, streams, ys, refs)
    # graphs: one per distinct piece length (37 = 16 + 16 + 5), and open / end / close never replaced one
    assert sorted(s._graphs) == [1, 3, 5, 8, 16]
    for a, b in zip(graphs, graphs[1:]):
        assert all(b[k] is g for k, g in a.items())
    assert all(s._graphs[k] is g for k, g in graphs[-1].items())


@pytest.mark.parametrize("name,kw", MODELS, ids=MODEL_IDS)
def test_slot_session_matches_block_session(dev, name, kw):
    """The same B streams opened together at hop 0 and never ended early, against an init_streams session."""
    from puresound_amd.streaming import StreamingConvTasNet
    model, _ = _model(name, dev, **kw)
    s = StreamingConvTasNet(model)
    b, hops, k = 4, 203, 8
    hop, lat = s.hop_length, s.latency_samples
    x = det_wave(610, b, hops * hop).to(dev)
    e = det_wave(611, b, 3500).to(dev) if model.speaker_net is not None else None
    pieces = [x[:, i * hop:min(i + k, hops) * hop].contiguous() for i in range(0, hops, k)]
    s.init_streams(b, e)
    block = torch.cat([s.step_chunk(p) for p in pieces] + [s.flush()], dim=1)
    s.init_slots(b)
    for i in range(b):
        s.open(i, None if e is None else e[i])
    outs = [s.step_chunk(p) for p in pieces]
    slots = torch.cat(outs + [torch.stack([s.close(i) for i in range(b)])], dim=1)
    assert s.active == []
    assert slots.shape[1] == block.shape[1] + lat
    assert torch.equal(slots[:, :lat], torch.full_like(slots[:, :lat], _zero(s)))
    err = rel_max(slots[:, lat:].cpu().numpy(), block.cpu().numpy())
    print(f"slot session against block session: rel_max {err:.3e}")
    assert err <= 1e-6


def test_isolation_bit_for_bit(dev):
    """Slot 1's whole output does not depend on what slots 0, 2, 3 do: idle with NaN input, or opening, ending and re-opening
    around it."""
    from puresound_amd.streaming import StreamingConvTasNet
    model, _ = _model("cfg3_causal_short", dev)
    s = StreamingConvTasNet(model)
    mine = (1, 3, 400, 1)
    alone = _streams(model, s, dev, [mine], seed=700)
    crowd = alone + _streams(model, s, dev, [(0, 0, 60, 0), (2, 1, 150, 2), (3, 9, 31, 0), (0, 100, 90, 1), (3, 77, 200, 0),
                                             (2, 250, 120, 0), (0, 260, 100, 0)], seed=720)
    for i, st in enumerate(crowd):
        st["id"] = i
    ya, _ = _run_slots(s, 4, alone, SCHEDULE)             # (_run_slots asserts the idle slots' constrain(0) under NaN input)
    yb, _ = _run_slots(s, 4, crowd, SCHEDULE)
    assert len(yb) == 8
    assert ya[0].numel() >= 400 * s.hop_length + s.latency_samples
    assert torch.equal(ya[0], yb[0])
    assert float(ya[0].abs().max()) > 1e-3


def test_reused_slot_does_not_see_its_predecessor(dev):
    """Stream A then stream B in slot 0, against stream B in a fresh session opened at the same counter value (a dummy in
    slot 1 advances it): the same bits."""
    from puresound_amd.streaming import StreamingConvTasNet
    model, _ = _model("cfg3_causal_short", dev)
    s = StreamingConvTasNet(model)
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


@pytest.mark.parametrize("name,kw", MODELS, ids=MODEL_IDS)
def test_graph_and_eager_are_bit_identical(dev, name, kw):
    from puresound_amd.streaming import StreamingConvTasNet
    model, _ = _model(name, dev, **kw)
    s = StreamingConvTasNet(model)
    plan = [(0, 0, 300, 0), (1, 5, 100, 2), (2, 5, 133, 0), (1, 150, 90, 0)]
    streams = _streams(model, s, dev, plan, seed=900)
    yg, _ = _run_slots(s, 3, streams, SCHEDULE, use_graph=True)
    assert len(s._graphs) > 0
    ye, _ = _run_slots(s, 3, streams, SCHEDULE, use_graph=False)
    assert len(s._graphs) == 0
    for i in yg:
        assert torch.equal(yg[i], ye[i]), i


@pytest.mark.parametrize("name,kw", MODELS, ids=MODEL_IDS)
def test_end_inside_a_chunk(dev, name, kw):
    """A stream with 5 hops left in a 16-hop chunk padded with NaN: finite output equal to offline; the slot's output hops
    after the end carry the tail, then constrain(0)."""
    from puresound_amd.streaming import StreamingConvTasNet
    model, _ = _model(name, dev, **kw)
    s = StreamingConvTasNet(model)
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
    from puresound_amd.streaming import StreamingConvTasNet
    from puresound_amd.streaming import tcn
    model, _ = _model("cfg3_causal_short", dev)
    plain, _ = _model("tiny_free_relu_causal", dev)
    s = StreamingConvTasNet(model)
    hop = s.hop_length
    e = det_wave(5, 1, 3000)[0].to(dev)
    x = det_wave(6, 2, 8 * hop).to(dev)

    def raises(exc, words, fn, *a):
        with pytest.raises(exc) as info:
            fn(*a)
        assert words.lower() in str(info.value).lower(), str(info.value)

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
    sp = StreamingConvTasNet(plain)
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
    # the int32 frame counter: refuse before g % R could go negative
    s.open(1, e)
    near = tcn.FRAME_LIMIT - 20
    s._counter.fill_(near)
    s.frames = near
    s._span[1, 0] = near                                       # (a stream that is live here)
    # ... and what it returns here is what it returns at a small counter that agrees with `near` modulo every ring
    y = same_bits_at_a_small_counter(s, H, near, 1, x[:, :8 * hop].contiguous())
    assert bool(torch.isfinite(y).all()) and s.frames == near + 8 and int(s._counter) == near + 8
    raises(RuntimeError, "init_slots()", s.step_chunk, det_wave(8, 2, 16 * hop).to(dev))
    assert s.frames == near + 8 and int(s._counter) == near + 8
    s.step_chunk(x[:, :8 * hop].contiguous())
    s.step_chunk(x[:, :4 * hop].contiguous())
    assert s.frames == tcn.FRAME_LIMIT
    raises(RuntimeError, "2**31 - 1", s.step, x[:, :hop].contiguous())
    raises(RuntimeError, "init_slots()", s.open, 0, e)
    assert s.close(1).shape == (s.win_length - hop,)


def test_model_left_intact(dev):
    from puresound_amd.streaming import StreamingConvTasNet
    model, _ = _model("cfg3_causal_short", dev)
    c = cases.CASES["cfg3_causal_short"]
    x = det_wave(c["seed"], c["B"], c["L"]).to(dev)
    e = det_wave(c["seed"] + 1, c["B"], c["L_enroll"]).to(dev)
    before = model.inference(x, e)
    params = [p.detach().clone() for p in model.parameters()]
    plans = [m.plan(dev) for stack in model.masker.tcn_list for m in stack]
    s = StreamingConvTasNet(model)
    streams = _streams(model, s, dev, [(0, 0, 120, 0), (1, 3, 60, 1), (1, 80, 70, 0)], seed=1000)
    _run_slots(s, 2, streams, (4,))
    _run_slots(s, 2, streams, SCHEDULE, use_graph=False)
    assert all(m.gemm_precision == "fp16x2" for stack in model.masker.tcn_list for m in stack)
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), params))
    assert all(a is b for a, b in zip(plans, [m.plan(dev) for stack in model.masker.tcn_list for m in stack]))
    assert torch.equal(model.inference(x, e), before)


# -------------------------------------------------------------------------------------------------------------------------
# kernel units
# -------------------------------------------------------------------------------------------------------------------------
def _rand(shape, seed):
    g = np.random.Generator(np.random.Philox(key=seed))
    return torch.tensor(g.uniform(-1.0, 1.0, shape), dtype=torch.float64)


def _chunks(total, k_max=16):
    """Chunk lengths 1, 2, ..., k_max, 1, 2, ... covering `total` frames."""
    out, k = [], 1
    while sum(out) < total:
        out.append(min(k, total - sum(out)))
        k = k % k_max + 1
    return out


def _live(spans, t_len):
    """[B, T] bool: frame g of stream b is live."""
    g = torch.arange(t_len).view(1, -1)
    sp = torch.tensor(spans)
    return (g >= sp[:, 0:1]) & (g < sp[:, 1:2])


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("d", [1, 3, 128])
@pytest.mark.parametrize("p", [2, 3, 5])
def test_dwconv_step_slots_kernel(dev, H, p, d, affine):
    from puresound_amd._abi import PS_NORM_AFFINE
    h = 6
    r = (p - 1) * d + 16
    t_len = r + 200                                     # the ring wraps
    # per stream: empty, birth inside a chunk (frame 8 of the 4-frame chunk 6 .. 9), death inside a chunk, birth older
    # than the ring, birth and death inside one chunk (21 .. 27), a span that begins after the ring has wrapped, a span
    # shorter than the ring, all live
    spans = [(0, 0), (8, I32_MAX), (0, t_len - 3), (0, I32_MAX), (23, 26), (r + 30, r + 150), (5, 5 + r // 2), (0, I32_MAX)]
    b = len(spans)
    seed = 77000 + p * 1000 + d * 10 + int(affine)
    x = _rand((b, h, t_len), seed)
    w = _rand((h, 1, p), seed + 1)
    bias = _rand((h,), seed + 2)
    gamma, beta = _rand((h,), seed + 3) + 1.5, _rand((h,), seed + 4) + 0.5    # beta != 0: PReLU(beta) is not 0
    slope = torch.tensor([0.25], dtype=torch.float64)
    live = _live(spans, t_len)
    a = F.prelu(x * gamma.view(1, -1, 1) + beta.view(1, -1, 1), slope) if affine else x
    a = a * live.view(b, 1, t_len)                      # a dead frame is a zero AFTER the prologue
    ref = F.conv1d(F.pad(a, ((p - 1) * d, 0)), w, bias, dilation=d, groups=h)
    f32 = lambda t: t.float().to(dev)  # noqa: E731
    g32, b32, s32 = f32(gamma), f32(beta), f32(slope)
    pro = H.make_prologue(PS_NORM_AFFINE, True, None, 0.0, 1e-8, g32, b32, s32) if affine else None
    xin_all = x.clone()
    xin_all[~live.view(b, 1, t_len).expand_as(x)] = NAN  # dead frames carry NaN in the input ...
    ring = torch.zeros(r, h, b, device=dev)
    for slot in range(r):                               # ... and in every ring slot a dead frame owns at the start
        ring[slot, :, ~live[:, slot].to(dev)] = NAN
    ring_plain = torch.zeros(r, h, b, device=dev)
    span = torch.tensor(spans, dtype=torch.int32, device=dev)
    everything = torch.tensor([(0, I32_MAX)] * b, dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    got, t0 = [], 0
    for k in _chunks(t_len):
        ld = H.padded_frames(k * b)
        xin = torch.full((1, h, ld), NAN, device=dev)
        xin[0, :, :k * b] = f32(xin_all[:, :, t0:t0 + k].permute(1, 2, 0).reshape(h, k * b))
        y = torch.zeros(1, h, ld, device=dev)
        H.dwconv_step(xin, ring, counter, f32(w), f32(bias), d, b, k, pro, out=y, span=span)
        assert float(y[0, :, k * b:].abs().sum()) == 0.0             # columns past the chunk are not written
        got.append(y[0, :, :k * b].reshape(h, k, b).permute(2, 0, 1).cpu())
        # a span that makes every frame live: the bits of the entry point without spans
        xfull = torch.full((1, h, ld), NAN, device=dev)
        xfull[0, :, :k * b] = f32(x[:, :, t0:t0 + k].permute(1, 2, 0).reshape(h, k * b))
        ring_a, ring_b = ring_plain.clone(), ring_plain.clone()
        ya = H.dwconv_step(xfull, ring_a, counter, f32(w), f32(bias), d, b, k, pro, out=torch.zeros(1, h, ld, device=dev))
        yb = H.dwconv_step(xfull, ring_b, counter, f32(w), f32(bias), d, b, k, pro, out=torch.zeros(1, h, ld, device=dev),
                           span=everything)
        assert torch.equal(ya, yb) and torch.equal(ring_a, ring_b)
        ring_plain = ring_a
        counter += k
        t0 += k
    got = torch.cat(got, dim=2)
    # the output of a dead frame too: its own tap is 0 like every dead tap, so no NaN of the input reaches any output
    assert bool(torch.isfinite(got).all())
    assert rel_max(got.numpy(), ref.numpy()) <= 1e-5


@pytest.mark.parametrize("out_mode", ["linear", "sigmoid", "none"])
@pytest.mark.parametrize("mask_act", ["linear", "relu", "sigmoid"])
@pytest.mark.parametrize("win,hop,b", [(16, 16, 3), (16, 8, 70), (32, 8, 5)])
def test_free_decode_step_slots_kernel(dev, H, win, hop, b, mask_act, out_mode):
    c, t_len = 24, 45
    seed = 88000 + win * 100 + hop + b
    feats = _rand((b, c, t_len), seed) * 0.6
    mask = _rand((b, c, t_len), seed + 1) * 2.0
    w = _rand((c, 1, win), seed + 2)
    base = [(0, 0), (4, I32_MAX), (0, 30), (7, 9), (0, I32_MAX)]
    spans = [base[i % len(base)] for i in range(b)]
    live = _live(spans, t_len)
    act = {"linear": lambda m: m, "relu": torch.relu, "sigmoid": torch.sigmoid}[mask_act]
    constrain = {"linear": lambda v: v.clamp(-1, 1), "sigmoid": torch.sigmoid, "none": lambda v: v}[out_mode]
    ref = constrain(F.conv_transpose1d(feats * act(mask) * live.view(b, 1, t_len), w, stride=hop)[:, 0])
    ref_all = constrain(F.conv_transpose1d(feats * act(mask), w, stride=hop)[:, 0])
    dead = ~live.view(b, 1, t_len).expand_as(feats)
    feats_n, mask_n = feats.clone(), mask.clone()
    feats_n[dead] = NAN
    mask_n[dead] = float("inf")
    f32 = lambda t: t.float().to(dev)  # noqa: E731
    w32 = f32(w)
    span = torch.tensor(spans, dtype=torch.int32, device=dev)
    everything = torch.tensor([(0, I32_MAX)] * b, dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    tails = [torch.zeros(b, win - hop, device=dev) for _ in range(3)]           # spans, no spans, the all-live span
    got, got_plain, got_all, t0 = [], [], [], 0

    def cols(t, k):
        ld = H.padded_frames(k * b)
        buf = torch.full((1, c, ld), NAN, device=dev)
        buf[0, :, :k * b] = f32(t[:, :, t0:t0 + k].permute(1, 2, 0).reshape(c, k * b))
        return buf

    for k in _chunks(t_len):
        outs = [torch.full((b, k * hop), NAN, device=dev) for _ in range(3)]
        H.free_decode_step(cols(feats_n, k), cols(mask_n, k), w32, tails[0], outs[0], hop, k, mask_act, out_mode, span=span,
                           counter=counter)
        H.free_decode_step(cols(feats, k), cols(mask, k), w32, tails[1], outs[1], hop, k, mask_act, out_mode)
        H.free_decode_step(cols(feats, k), cols(mask, k), w32, tails[2], outs[2], hop, k, mask_act, out_mode, span=everything,
                           counter=counter)
        got.append(outs[0].cpu())
        got_plain.append(outs[1].cpu())
        got_all.append(outs[2].cpu())
        counter += k
        t0 += k
    assert torch.equal(tails[1], tails[2])
    lasts = [torch.empty(b, win - hop, device=dev) for _ in range(3)]
    for tail, last in zip(tails, lasts):
        H.free_decode_step(None, None, w32, tail, last, hop, out_mode=out_mode, flush=True)
    # one row's tail through a B = 1 flush on that row: what close() launches
    row = torch.empty(1, win - hop, device=dev)
    H.free_decode_step(None, None, w32, tails[0][b - 1:b], row, hop, out_mode=out_mode, flush=True)
    assert torch.equal(row[0], lasts[0][b - 1])
    got = torch.cat(got + [lasts[0].cpu()], dim=1)
    got_plain = torch.cat(got_plain + [lasts[1].cpu()], dim=1)
    got_all = torch.cat(got_all + [lasts[2].cpu()], dim=1)
    assert got.shape == ref.shape
    assert bool(torch.isfinite(got).all())
    assert rel_max(got.numpy(), ref.numpy()) <= 1e-5
    assert torch.equal(got[0], constrain(torch.zeros(got.shape[1])).float())    # the empty span: constrain(0) exactly
    assert torch.equal(got_all, got_plain)
    assert rel_max(got_plain.numpy(), ref_all.numpy()) <= 1e-5
