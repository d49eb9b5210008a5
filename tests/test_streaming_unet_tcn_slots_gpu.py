"""Slot sessions of StreamingUnetTcn on the MI355X: the three *_slots_f32 kernels on poisoned inputs (NaN in every dead frame)
against their siblings on the same data with the dead frames zeroed and against the fp64 span rule
(tests/unet_tcn_slots_ref.py), and sessions whose streams join, end, drain and leave on their own against a block session of
each stream, the offline model and the reference golden."""
import copy
import os

import numpy as np
import pytest
import torch

import gated_tcn_step_ref as G
import unet_tcn_slots_ref as R
from conftest import rel_max
from detweights import det_wave
from test_streaming_spectral_gpu import CONV_CASES
from test_streaming_unet_tcn_gpu import PRESET, TOL, _model, _offline, _pro, _stream

pytestmark = pytest.mark.gpu
MAX = R.INT32_MAX
NAN = float("nan")


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


def _rand(shape, seed):
    g = np.random.Generator(np.random.Philox(key=seed))
    return torch.tensor(g.uniform(-1.0, 1.0, shape), dtype=torch.float32)


def _spans(patterns, b, turn):
    """[b, 2] int64: column i takes pattern (i + turn) % len, so every pattern meets every position as the turns go by."""
    return torch.tensor([patterns[(i + turn) % len(patterns)] for i in range(b)], dtype=torch.int64)


def _i32(span, dev):
    return span.to(torch.int32).to(dev).contiguous()


def _misaligned(span, dev):
    flat = torch.zeros(span.numel() + 1, dtype=torch.int32, device=dev)
    flat[1:] = span.to(torch.int32).reshape(-1).to(dev)
    view = flat[1:].view(-1, 2)
    assert view.data_ptr() % 8 == 4 and view.is_contiguous()
    return view


# ---- ps_conv2d_step_slots_f32 -------------------------------------------------------------------------------------------
def _conv_patterns(t, shift):
    """live throughout; born at t, t - 1, t + 1; dead from t - shift on; idle; born inside the history; a finite stream that
    death = INT32_MAX never ends."""
    return [(0, MAX), (t, MAX), (t - 1, MAX), (t + 1, MAX), (0, t - shift), (0, 0), (t - shift - 1, MAX), (t - shift - 2, t - shift)]


@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("b", [1, 5, 130])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv2d_step_slots_kernel(dev, H, case, b, shift):
    transposed, kf, kt, sf, df, dt, two, m = case
    c1, c2, f_in, t = 6, (4 if two else 0), 16, 9
    ci, pf, hist = c1 + c2, kf // 2, (kt - 1) * dt
    seed = hash(case) % 1000 + b + 7 * shift
    w = _rand((ci, m, kf, kt) if transposed else (m, ci, kf, kt), seed + 1).double() * 0.3
    w2 = (w.permute(1, 0, 2, 3) if transposed else w).reshape(m, -1)
    bias, slope = _rand((m,), seed + 2).double(), torch.tensor([0.25], dtype=torch.float64)
    wt, bias_d, slope_d = H.pack_wt(w2.float().to(dev)), bias.float().to(dev), slope.float().to(dev)
    ldb = H.padded_frames(b)
    srcs = [(c1, 0), (c2, c1)] if two else [(c1, 0)]
    counter = torch.full((1,), t, dtype=torch.int32, device=dev)
    patterns = _conv_patterns(t, shift)
    turns = len(patterns) if b < len(patterns) else 2
    f_out = None
    for turn in range(turns + 1):
        full = turn == turns                                             # the last turn: every span (0, INT32_MAX), no poison
        span = torch.tensor([(0, MAX)] * b) if full else _spans(patterns, b, turn)
        x = _rand((b, ci, f_in, hist + 1), seed + 10 + turn).double()    # [..., hist - d] = frame t - shift - d
        dead = torch.stack([~R.live(span, t - shift - d) for d in range(hist, -1, -1)], dim=-1)      # [b, hist + 1]
        poisoned = torch.where(dead[:, None, None, :], torch.full_like(x, NAN), x)
        clean = torch.where(dead[:, None, None, :], torch.zeros_like(x), x)
        want = R.conv2d_last_frame(clean, w, bias, slope, transposed, kf, sf, df, dt)                # [b, m, f_out]
        ring64 = poisoned[..., :hist].permute(3, 0, 1, 2)
        by_rule = R.conv2d_last_frame(R.conv2d_taps(poisoned[..., hist], ring64, span, t, shift), w, bias, slope, transposed, kf,
                                      sf, df, dt)
        assert torch.equal(by_rule, want)                                # the helper's select is the zeroing
        f_out = want.shape[2]
        outs = []
        for data in (poisoned, clean):
            cur = [torch.full((1, c, f_in, ldb), NAN, device=dev) for c, _ in srcs]
            rings = [torch.full((max(hist, 1), c, f_in, ldb), NAN, device=dev) for c, _ in srcs]
            for buf, ring, (c, off) in zip(cur, rings, srcs):
                buf[0, :, :, :b] = data[:, off:off + c, :, hist].permute(1, 2, 0).float().to(dev)
                for d in range(1, hist + 1):
                    ring[ring.shape[0] - d, :, :, :b] = data[:, off:off + c, :, hist - d].permute(1, 2, 0).float().to(dev)
            y = torch.full((1, m, f_out, ldb), 7.0, device=dev)
            slots = dict(counter=counter, span=_i32(span, dev), shift=shift) if data is poisoned else {}
            H.conv2d_step(cur[0], rings[0] if hist else None, cur[1] if two else None, rings[1] if (two and hist) else None, wt,
                          bias_d, m, b, f_out, kf, kt, sf, df, dt, pf, transposed, "prelu", slope_d, out=y, **slots)
            assert bool((y[0, :, :, b:] == 7.0).all())                   # pad frames are not written
            outs.append(y[0, :, :, :b].permute(2, 0, 1).cpu())
        assert torch.equal(outs[0], outs[1]), ("slot entry on poisoned data != sibling on zeroed data", turn, full)
        assert rel_max(outs[0].numpy(), want.numpy()) < 2e-6, turn


# ---- ps_gated_tcn_step_slots_f32 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 5, 130])
@pytest.mark.parametrize("dilation", [1, 16])
@pytest.mark.parametrize("e", [0, 6])
@pytest.mark.parametrize("h", [8, 40, 256])
def test_gated_tcn_step_slots_kernel(dev, H, h, e, dilation, b):
    """The shapes of the sibling's test.  A session of T frames fed as chunks of k = 1, 3 and 16 with NaN in every dead frame
    of y: identical bits for the three k; every live frame equal to the sibling's result on the streams moved to frame 0
    (dead frames zeroed, and with them the embedding constants of dead taps); against the fp64 rule at most twice the error
    of the offline kernels on data of the same shape, floor 2e-6.  Full spans: the sibling's bits, ring included."""
    from puresound_amd.nnet.conv_tasnet import GatedTCN
    p = 3
    r = (p - 1) * dilation + 16
    t = 2 * r + 7
    blk = G.make_block(h, e, p, dilation, seed=h + 7 * e + dilation)
    blk = {k: (v.float().double() if torch.is_tensor(v) else v) for k, v in blk.items()}
    gen = torch.Generator().manual_seed(b + dilation)
    y = (torch.rand(t, h, b, generator=gen, dtype=torch.float64) * 2 - 1).float().double()
    emb = (torch.rand(b, e, generator=gen, dtype=torch.float64) * 2 - 1).float().double() if e else None
    wl = H.pack_wt(GatedTCN._unfolded(blk["wl"].float()).to(dev))
    wr = H.pack_wt(GatedTCN._unfolded(blk["wr"][:, :h, :].float().contiguous()).to(dev))
    pl, keep_l = _pro(H, blk, "l", dev)
    pr, keep_r = _pro(H, blk, "r", dev)
    taps = G.emb_taps(blk, emb).float().to(dev).contiguous() if e else None
    # born at a chunk start of k = 16, one frame before and after it, dead from a chunk start on, idle, finite, never ending
    patterns = [(0, MAX), (16, MAX), (15, MAX), (17, MAX), (0, 32), (0, 0), (r + 3, t - 4), (t // 2, MAX)]

    def run(data, k, span):
        ring = torch.full((r, h, b), NAN, device=dev)                    # nothing clears a ring when a stream begins
        if span is None:
            ring.zero_()
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        got = []
        for t0 in range(0, t, k):
            kk = min(k, t - t0)
            ld = H.padded_frames(k * b)
            ybuf = torch.full((1, h, ld), NAN, device=dev)
            ybuf[0, :, :kk * b] = data[t0:t0 + kk].permute(1, 0, 2).reshape(h, kk * b).float().to(dev)
            out = torch.full((1, h, ld), NAN, device=dev)
            H.gated_tcn_step(ybuf, ring, counter, wl, wr, p, dilation, b, kk, pl, pr, taps, out=out, span=span)
            assert bool(torch.isnan(out[0, :, kk * b:]).all())
            got.append(out[0, :, :kk * b].reshape(h, kk, b).permute(1, 0, 2))
            counter += kk
        return torch.cat(got).cpu(), ring.cpu()

    # the error of the offline pieces on the unpoisoned data (the sibling's yardstick)
    want_all = G.block_step(y, 0, blk, torch.zeros(t + 2 * dilation, h, b, dtype=torch.float64), emb)
    yo = H.pad_rows(y.permute(2, 1, 0).float().contiguous().to(dev))
    left = (p - 1) * dilation
    col_l = H.unfold_taps(yo, t, p, dilation, left)
    col_r = col_l if not e else H.unfold_taps(yo, t, p, dilation, left, None, None, emb.float().to(dev).contiguous())
    lo, _ = H.conv1x1(col_l, t, wl, h)
    ro, _ = H.conv1x1(col_r, t, H.pack_wt(GatedTCN._unfolded(blk["wr"].float()).to(dev)), h)
    off = H.unpad_rows(H.gated_product(lo, ro, t, pl, pr), t).permute(2, 1, 0).cpu()
    err_off = rel_max(off.numpy(), want_all.numpy())

    for turn in range({1: 4, 5: 2}.get(b, 1)):
        span = _spans(patterns, b, 2 * turn)
        dead = torch.stack([~R.live(span, g) for g in range(t)])         # [t, b]
        poisoned = torch.where(dead[:, None, :], torch.full_like(y, NAN), y)
        runs = {k: run(poisoned, k, _i32(span, dev)) for k in (1, 3, 16)}
        for k in (3, 16):
            assert torch.equal(runs[k][0], runs[1][0]), f"g differs between k = 1 and k = {k}"
            assert torch.equal(runs[k][1].nan_to_num(7.0), runs[1][1].nan_to_num(7.0)), f"the ring differs at k = {k}"
        got = runs[1][0]
        assert not bool(torch.isnan(got).any())                          # a dead frame's output is finite: it read zeros
        alone, _ = run(R.align(y, span), 16, None)                       # the sibling: every stream from frame 0, zeros after
        want = R.block_step_slots(poisoned, 0, blk, torch.full((t + 2 * dilation, h, b), NAN, dtype=torch.float64), span, emb)
        checked = 0
        for i in range(b):
            lo_i, hi_i = int(span[i, 0]), min(int(span[i, 1]), t)
            if hi_i > lo_i:
                assert torch.equal(got[lo_i:hi_i, :, i], alone[:hi_i - lo_i, :, i]), (turn, i)
                checked += 1
        assert checked or b == 1
        err = rel_max(got.numpy(), want.numpy())
        assert err <= max(2 * err_off, 2e-6), (err, err_off)

    full = _i32(torch.tensor([(0, MAX)] * b), dev)
    for k in (1, 16):
        a, b_ = run(y, k, full), run(y, k, None)
        assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1]), k


# ---- ps_istft_step_slots_f32 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_mode", ["linear", "none"])
@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("n_fft,hop", [(64, 16), (512, 128)])
def test_istft_step_slots_kernel(dev, H, n_fft, hop, shift, out_mode):
    hops, keep = 16, n_fft - hop
    # live throughout; born at frame 3; finite; idle; a single frame; ends with the session; a stream whose frames are over
    span = torch.tensor([(0, MAX), (3, MAX), (2, 7), (0, 0), (5, 6), (4, hops + 9), (1, 4), (hops + 3, MAX)], dtype=torch.int64)
    b = span.shape[0]
    ldb = H.padded_frames(b)
    window = torch.hann_window(n_fft)
    frames = (_rand((hops, b, n_fft), n_fft + shift) * 40.0).double()    # hop t holds frame t - shift of every stream
    dead = torch.stack([~R.live(span, t - shift) for t in range(hops)])  # [hops, b]
    poisoned = torch.where(dead[:, :, None], torch.full_like(frames, NAN), frames)
    want, tails64 = R.istft_slots(poisoned, window.double(), span, shift, hop, out_mode)

    def run(span_d, shift_, b_, data):
        """-> (out [b_, hops * hop], per hop the flush of every row taken before that hop's step [hops + 1, b_, keep])"""
        tail = torch.zeros(b_, keep, device=dev)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        out = torch.full((b_, hops * hop), NAN, device=dev)
        syn = torch.full((1, n_fft, H.padded_frames(b_)), NAN, device=dev)
        flushes = []
        for t in range(hops + 1):
            last = torch.full((b_, keep), NAN, device=dev)
            if span_d is None:
                H.istft_step(None, window.to(dev), tail, last, counter, hop, out_mode, flush=True)
            else:
                for i in range(b_):                                      # as close() does: B = 1 on the slot's rows
                    H.istft_step(None, window.to(dev), tail[i:i + 1], last[i:i + 1], counter, hop, out_mode, flush=True,
                                 span=span_d[i:i + 1], shift=shift_)
            flushes.append(last.cpu())
            if t == hops:
                break
            syn[0, :, :b_] = data[t].t().float().to(dev)
            kw = {} if span_d is None else dict(span=span_d, shift=shift_)
            H.istft_step(syn, window.to(dev), tail, out[:, t * hop:(t + 1) * hop], counter, hop, out_mode, **kw)
            counter += 1
        return out.cpu(), torch.stack(flushes)

    got, flushed = run(_i32(span, dev), shift, b, poisoned)
    assert rel_max(got.numpy(), want.numpy()) <= 1e-6
    for i in range(b):
        lo, hi = int(span[i, 0]), min(int(span[i, 1]), hops - shift)
        first = (lo + shift) * hop
        assert bool((got[i, :min(first, hops * hop)] == 0).all()), i     # before the stream, and idle: constrain(0)
        if hi <= lo:
            continue
        # the sibling on this stream alone, from frame 0: its steps, then its flush
        own = torch.full((hops, 1, n_fft), NAN, dtype=torch.float64)
        own[:hi - lo, 0] = frames[lo + shift:hi + shift, i]
        alone, alone_flushed = run(None, 0, 1, own)
        n = hi - lo
        assert torch.equal(got[i, first:first + n * hop], alone[0, :n * hop]), i
        if int(span[i, 1]) <= hops - shift:                              # the stream ended inside the session
            t_end = int(span[i, 1]) + shift
            tail_alone = alone_flushed[n, 0]
            for late in range(0, min(keep // hop + 1, hops - t_end) + 1):
                rest = torch.cat([tail_alone[late * hop:], torch.zeros(min(late * hop, keep))])
                assert torch.equal(flushed[t_end + late, i], rest), (i, late)          # close() now, or `late` hops later
                want64 = R.istft_flush_slots(tails64[t_end + late, i], window.double(), span[i], t_end + late, shift, hop, out_mode)
                assert rel_max(flushed[t_end + late, i].numpy(), want64.numpy()) <= 1e-6 or float(want64.abs().max()) == 0.0
            drained = got[i, t_end * hop:t_end * hop + keep]             # later steps drain the tail with the flush's window sum
            assert torch.equal(drained, tail_alone[:drained.shape[0]]), i
            assert bool((got[i, t_end * hop + keep:] == 0).all())
    if shift == 0:                                                       # full spans: the sibling's bits, step and flush
        every = _i32(torch.tensor([(0, MAX)] * b), dev)
        a, fa = run(every, 0, b, frames)
        c, fc = run(None, 0, b, frames)
        assert torch.equal(a, c) and torch.equal(fa, fc)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_slot_entries_refuse_a_bad_span_or_shift_and_write_nothing(dev, H):
    b, h = 3, 8
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    span = torch.tensor([(0, MAX)] * b)
    good, bad = _i32(span, dev), _misaligned(span, dev)
    from puresound_amd import _abi
    sp, st = _abi.ptr, _abi.stream_ptr(dev)

    # ps_conv2d_step_slots_f32
    x, ring, wt, bias = z(1, 2, 4, 128), z(1, 2, 4, 128), H.pack_wt(z(5, 2 * 3 * 2)), z(5)
    y = torch.full((1, 5, 4, 128), 7.0, device=dev)
    conv = lambda **kw: H.conv2d_step(x, ring, None, None, wt, bias, 5, b, 4, 3, 2, 1, 1, 1, 1, False, out=y, counter=counter, **kw)  # noqa: E731
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        conv(span=bad, shift=0)
    with pytest.raises(RuntimeError, match="shift >= 0"):
        conv(span=good, shift=-1)
    rc = H.lib().ps_conv2d_step_slots_f32(sp(x), sp(ring), 2, 1, None, None, 0, 0, sp(wt), sp(bias), sp(y), 5, 4, b, 128, 3, 2, 1, 1,
                                          1, 1, 4, 0, 0, None, sp(counter), None, 0, st)
    assert rc != 0 and "span" in H.lib().ps_last_error().decode()
    rc = H.lib().ps_conv2d_step_slots_f32(sp(x), sp(ring), 2, 1, None, None, 0, 0, sp(wt), sp(bias), sp(y), 5, 4, b, 128, 3, 2, 1, 1,
                                          1, 1, 4, 0, 0, None, None, sp(good), 0, st)
    assert rc != 0 and "counter" in H.lib().ps_last_error().decode()
    conv(span=good, shift=0)                                             # (and the same call with a good span runs)
    assert bool((y[0, :, :, :b] == 0).all()) and bool((y[0, :, :, b:] == 7.0).all())
    y.fill_(7.0)

    # ps_gated_tcn_step_slots_f32
    yy, gring, w = z(1, h, 128), z(3, h, b), H.pack_wt(z(h, 3 * h))
    g = torch.full((1, h, 128), 7.0, device=dev)
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        H.gated_tcn_step(yy, gring, counter, w, w, 3, 1, b, 1, out=g, span=bad)
    rc = H.lib().ps_gated_tcn_step_slots_f32(sp(yy), sp(gring), 3, sp(counter), None, sp(w), sp(w), None, None, None, sp(g), h, b, 1,
                                             128, 3, 1, st)
    assert rc != 0 and "span" in H.lib().ps_last_error().decode()

    # ps_istft_step_slots_f32
    n_fft, hop = 64, 16
    syn, window, tail = z(1, n_fft, 128), torch.hann_window(n_fft).to(dev), torch.full((b, n_fft - hop), 3.0, device=dev)
    out = torch.full((b, hop), 7.0, device=dev)
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        H.istft_step(syn, window, tail, out, counter, hop, "none", span=bad)
    with pytest.raises(RuntimeError, match="shift >= 0"):
        H.istft_step(syn, window, tail, out, counter, hop, "none", span=good, shift=-1)
    rc = H.lib().ps_istft_step_slots_f32(sp(syn), 128, sp(window), sp(tail), sp(out), hop, sp(counter), None, 0, b, n_fft, hop, 2, 0,
                                         st)
    assert rc != 0 and "span" in H.lib().ps_last_error().decode()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((g == 7.0).all()) and bool((out == 7.0).all())
    assert bool((tail == 3.0).all()) and bool((gring == 0).all())


# ---- sessions -----------------------------------------------------------------------------------------------------------
HOP, WIN = 128, 512
_REFS = {}


def _wave(seed, frames):
    """A stream of `frames` frames: (frames + 3) hops of input."""
    return det_wave(seed, 1, (frames + WIN // HOP - 1) * HOP)[0]


def _block_reference(key, model, x, enroll, dev):
    """init_streams(1, enroll=...) streamed plus flush() for one stream, computed once per (model, stream)."""
    if key not in _REFS:
        from puresound_amd.streaming import StreamingUnetTcn
        _REFS[key] = _stream(StreamingUnetTcn(model), x[None].to(dev), 5, enroll=enroll[None].to(dev))[0]
    return _REFS[key]


def _run_slots(s, capacity, streams, split, dev, use_graph=True, use_step=False, how="enroll", model=None, before_first=None):
    """streams: dicts(slot, at, x [L], enroll [L']).  The session runs hop by hop in calls of `split` hops, cut where a stream
    opens or closes; every slot that is idle, ended or draining is fed NaN.  A stream is ended ahead (end(slot, hops) before
    the call that holds its last input hop), drained for D hops and closed.  -> per stream its outputs from open() on ‖ close()."""
    D = s.delay_frames
    s.init_slots(capacity, use_graph=use_graph)
    plan = []
    for i, st in enumerate(streams):
        hops = st["x"].shape[0] // HOP
        plan.append(dict(i=i, slot=st["slot"], at=st["at"], hops=hops, close_at=st["at"] + hops + D, ended=False))
    total = max(p["close_at"] for p in plan)
    ys = [[] for _ in streams]
    t = 0
    while True:
        for p in plan:
            if p["close_at"] == t:
                ys[p["i"]].append(s.close(p["slot"]))
        for p in plan:
            if p["at"] == t:
                st = streams[p["i"]]
                if how == "embed":
                    s.open(p["slot"], embed=model.inference_tse_embedding(st["enroll"][None].to(dev)))
                else:
                    s.open(p["slot"], enroll=st["enroll"].to(dev))
        if t == 0 and before_first is not None:
            before_first()
        if t == total:
            break
        events = [e for p in plan for e in (p["at"], p["close_at"]) if e > t]
        k = min([split] + [e - t for e in events])
        chunk = torch.full((capacity, k * HOP), NAN, device=dev)
        live = [p for p in plan if p["at"] <= t < p["close_at"]]
        for p in live:
            fed = t - p["at"]
            n = max(min(k, p["hops"] - fed), 0)
            if n:
                chunk[p["slot"], :n * HOP] = streams[p["i"]]["x"][fed * HOP:(fed + n) * HOP].to(dev)
            if not p["ended"] and p["hops"] - fed <= k and D:            # the stream's last input hop is in this call
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
    """Streams of 40, 1, 7 and 2 frames at different session frames; slot 1 is closed and reopened with another enrolment;
    capacity 5 adds a fifth stream and leaves slot 3 idle throughout."""
    e = lambda seed: det_wave(seed, 1, 3000)[0]  # noqa: E731
    streams = [dict(slot=0, at=0, x=_wave(101, 40), enroll=e(201)),
               dict(slot=1, at=3, x=_wave(102, 1), enroll=e(202)),
               dict(slot=1, at=12, x=_wave(103, 7), enroll=e(203)),
               dict(slot=2, at=5, x=_wave(104, 2), enroll=e(204))]
    if capacity == 5:
        streams.append(dict(slot=4, at=17, x=_wave(105, 7), enroll=e(205)))
    return streams


@pytest.mark.parametrize("capacity", [3, 5])
def test_each_slot_is_a_block_session_of_its_stream_and_the_offline_model(dev, capacity):
    from puresound_amd.streaming import StreamingUnetTcn
    model = _model("small", dev)
    s = StreamingUnetTcn(model)
    assert s.delay_frames == 3
    streams = _scenario(capacity)
    ys = _run_slots(s, capacity, streams, 5, dev)
    for i, (st, y) in enumerate(zip(streams, ys)):
        samples = st["x"].shape[0]
        r = s.slot_output_range(samples, WIN, HOP, s.delay_frames)
        assert y.shape[0] == r.stop == s.latency_samples + samples, i    # closed right after the drain: nothing more
        mine = y[r.start:r.stop]
        assert torch.equal(mine, _block_reference(("small", i), model, st["x"], st["enroll"], dev)), i
        assert bool((y[:r.start] == 0).all()), i                        # the window fills, the delay passes: constrain(0)
        ref = _offline(model, st["x"][None].to(dev), st["enroll"][None].to(dev))[0]
        sl = slice(16, ref.shape[0] - 16)                                # (the block session's own comparison)
        assert rel_max(mine[sl].cpu().numpy(), ref[sl].cpu().numpy()) <= TOL, i


def test_graph_eager_step_and_chunk_splits_give_the_same_bits(dev):
    from puresound_amd.streaming import StreamingUnetTcn
    model = _model("small", dev)
    s = StreamingUnetTcn(model)
    streams = _scenario(3)
    base = _run_slots(s, 3, streams, 5, dev)
    for split, graph, step in ((1, True, True), (1, False, True), (7, True, False), (7, False, False), (16, True, False)):
        ys = _run_slots(s, 3, streams, split, dev, use_graph=graph, use_step=step)
        for i, (a, c) in enumerate(zip(ys, base)):
            assert torch.equal(a, c), (split, graph, step, i)


def test_full_session_opened_at_frame_0_is_the_block_session(dev):
    from puresound_amd.streaming import StreamingUnetTcn
    model = _model("small", dev)
    s = StreamingUnetTcn(model)
    x = det_wave(71, 3, HOP * 23)
    enroll = det_wave(72, 3, 3000)
    block = _stream(s, x.to(dev), 5, enroll=enroll.to(dev))
    ys = _run_slots(s, 3, [dict(slot=i, at=0, x=x[i], enroll=enroll[i]) for i in range(3)], 5, dev)
    r = s.slot_output_range(x.shape[1], WIN, HOP, s.delay_frames)
    for i in range(3):
        assert torch.equal(ys[i][r.start:r.stop], block[i]), i


def test_golden_stream_in_a_slot_opened_at_frame_5(dev, golden_dir):
    from puresound_amd.streaming import StreamingUnetTcn
    g = dict(np.load(os.path.join(golden_dir, PRESET + ".npz")))
    model = _model("preset", dev)
    x = det_wave(1234, 2, 4000)[:, :3968].contiguous()
    enroll = det_wave(1235, 2, 3000)
    s = StreamingUnetTcn(model)
    assert s.delay_frames == 6
    (y,) = _run_slots(s, 2, [dict(slot=1, at=5, x=x[0], enroll=enroll[0])], 8, dev)
    r = s.slot_output_range(x.shape[1], WIN, HOP, 6)
    assert (r.start, y.shape[0]) == (1152, r.stop)
    mine = y[r.start:r.stop].cpu().numpy()
    sl = slice(16, g["wav"].shape[1] - 16)
    assert mine.shape == g["wav"][0].shape
    assert rel_max(mine[sl], g["wav"][0, sl]) <= 1e-4


def test_embed_equals_enroll(dev):
    from puresound_amd.streaming import StreamingUnetTcn
    model = _model("small", dev)
    s = StreamingUnetTcn(model)
    streams = _scenario(3)[:2]
    a = _run_slots(s, 3, streams, 5, dev)
    c = _run_slots(s, 3, streams, 5, dev, how="embed", model=model)
    for u, v in zip(a, c):
        assert torch.equal(u, v)


def test_parameter_change_rebuilds_the_slots_constants(dev):
    """The weights change after open() computed the slot's tap constants with the old ones and before the first hop: the
    session is that of the new weights, so the constants were rebuilt from the slot's kept embedding."""
    from puresound_amd.streaming import StreamingUnetTcn
    model = copy.deepcopy(_model("small", dev))
    s = StreamingUnetTcn(model)
    streams = [dict(slot=1, at=0, x=_wave(111, 9), enroll=det_wave(211, 1, 3000)[0])]
    (y0,) = _run_slots(s, 2, streams, 4, dev)

    def change():
        with torch.no_grad():
            model.masker.tcn_list[1][0].right_conv[0].weight.mul_(0.5)   # a block that takes the embedding
            model.masker.cnn_up[1][0].weight.mul_(1.25)

    (y1,) = _run_slots(s, 2, streams, 4, dev, before_first=change)
    r = s.slot_output_range(streams[0]["x"].shape[0], WIN, HOP, s.delay_frames)
    want = _stream(StreamingUnetTcn(model), streams[0]["x"][None].to(dev), 5, enroll=streams[0]["enroll"][None].to(dev))[0]
    assert torch.equal(y1[r.start:r.stop], want)
    assert not torch.equal(y0, y1)


def test_the_rules_of_a_slot_session(dev):
    from puresound_amd.streaming import StreamingUnetTcn
    model = _model("small", dev)
    s = StreamingUnetTcn(model)
    e = det_wave(301, 1, 3000)[0].to(dev)
    x = _wave(302, 4).to(dev)
    hop_in = lambda i: torch.stack([x[i * HOP:(i + 1) * HOP], torch.full((HOP,), NAN, device=dev)])  # noqa: E731
    s.init_slots(2)
    with pytest.raises(ValueError, match="exactly one of enroll"):
        s.open(0)
    with pytest.raises(ValueError, match="exactly one of enroll"):
        s.open(0, enroll=e, embed=model.inference_tse_embedding(e[None]))
    assert s.active == []
    s.open(0, enroll=e)
    with pytest.raises(RuntimeError, match="close"):
        s.flush()
    for i in range(7):
        assert s.step(hop_in(i)).shape == (2, HOP)                       # from the first hop on
    with pytest.raises(RuntimeError, match=r"end\(0, 0\), step 3 more hops"):
        s.close(0)                                                       # without end(): raises, and changes nothing
    assert s.active == [0]
    s.end(0, 0)
    s.step(hop_in(0) * NAN)
    with pytest.raises(RuntimeError, match="step 2 more hops"):
        s.close(0)
    s.step_chunk(torch.full((2, 2 * HOP), NAN, device=dev))
    assert s.close(0).shape == (WIN - HOP,) and s.active == []
    # a block session answers the slot calls with the core's RuntimeError
    s.init_streams(2, enroll=torch.stack([e, e]))
    for call in (lambda: s.open(0, enroll=e), lambda: s.end(0, 0), lambda: s.close(0)):
        with pytest.raises(RuntimeError, match="not a slot session"):
            call()


def test_without_transpose_delay_a_slot_closes_as_a_conv_tasnet_slot_does(dev):
    """D = 0: no drain hops, and close() without an earlier end() ends the stream there."""
    from puresound_amd.streaming import StreamingUnetTcn
    model = _model("small_nodelay", dev, transpose_delay=False)
    s = StreamingUnetTcn(model)
    assert s.delay_frames == 0
    x, e = _wave(401, 7), det_wave(402, 1, 3000)[0]
    (y,) = _run_slots(s, 2, [dict(slot=0, at=2, x=x, enroll=e)], 4, dev)  # (D = 0: _run_slots calls no end())
    r = s.slot_output_range(x.shape[0], WIN, HOP)
    assert y.shape[0] == r.stop
    assert torch.equal(y[r.start:r.stop], _stream(StreamingUnetTcn(model), x[None].to(dev), 5, enroll=e[None].to(dev))[0])
