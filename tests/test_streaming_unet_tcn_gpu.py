"""Hop-by-hop streaming of the causal U-Net + gated-TCN speaker extractor (puresound_amd/streaming/unet_tcn.py) on the
MI355X: ps_gated_tcn_step_f32 against its fp64 frame loop (tests/gated_tcn_step_ref.py) at the tile boundaries, the streamed
output against the reference golden and the offline HIP path, and the session against itself (graph / eager, step / chunk,
B = 1 / B, enrolment / cached embedding, short streams, a model without the delay)."""
import copy
import os

import numpy as np
import pytest
import torch

import cases
import gated_tcn_step_ref as G
from conftest import rel_max
from detweights import det_state_dict, det_wave

pytestmark = pytest.mark.gpu
TOL = 1e-4
PRESET = "tse_unet_tcn_causal_short"
SMALL = dict(channels=(1, 8, 8, 8), kernel_t=(2,) * 3, kernel_f=(5,) * 3, stride_t=(1,) * 3, stride_f=(2,) * 3,
             dilation_t=(1,) * 3, dilation_f=(1,) * 3, delay=(0,) * 3, tcn_dim=16, per_tcn_stack=3, repeat_tcn=2,
             tcn_with_embed=[1, 0, 0])


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
    junk = [torch.full((1 << 22,), float("nan"), device=dev) for _ in range(8)]
    junk += [torch.full((n,), float("nan"), device=dev) for n in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20)]
    del junk
    yield


_MODELS = {}


def _model(key, dev, **masker_kw):
    """The preset (key "preset") or the reduced model with `masker_kw` on top of SMALL, deterministic weights, on the GPU."""
    if key not in _MODELS:
        import puresound_amd.nnet as PA
        c = copy.deepcopy(cases.CASES[PRESET])
        if key != "preset":
            c["masker"]["kw"].update({**SMALL, **masker_kw})
        saved = cases.CASES[PRESET]
        cases.CASES[PRESET] = c
        try:
            m = cases.build(PA.NS, PRESET).eval()
        finally:
            cases.CASES[PRESET] = saved
        m.load_state_dict(det_state_dict(m))
        _MODELS[key] = m.to(dev)
    return _MODELS[key]


def _offline(model, x, enroll):
    model.set_gemm_precision("fp32")
    try:
        return model.inference(x, enroll)
    finally:
        model.set_gemm_precision("fp16x2")


def _stream(s, x, chunk=None, use_graph=True, **init):
    """Stream x [B, L] (L a multiple of the hop) -> emitted samples ‖ flush(), [B, L_out]; chunk: hops per step_chunk call
    (None: step(), which returns None for exactly the first prime_hops hops)."""
    hop = s.hop_length
    s.init_streams(x.shape[0], use_graph=use_graph, **init)
    outs, hops = [], x.shape[1] // hop
    if chunk is None:
        for i in range(hops):
            y = s.step(x[:, i * hop:(i + 1) * hop])
            assert (y is None) == (i < s.prime_hops), i
            if y is not None:
                outs.append(y)
    else:
        for i in range(0, hops, chunk):
            outs.append(s.step_chunk(x[:, i * hop:min(hops, i + chunk) * hop]))
    outs.append(s.flush())
    return torch.cat(outs, dim=1)


# ---- ps_gated_tcn_step_f32 --------------------------------------------------------------------------------------------
def _pro(H, blk, side, dev):
    from puresound_amd._abi import PS_NORM_AFFINE
    t = [blk[k + side].float().to(dev).contiguous() for k in ("sc_", "sh_", "slope_")]
    return H.make_prologue(PS_NORM_AFFINE, True, None, 0.0, 1e-8, *t), t


@pytest.mark.parametrize("b", [1, 5, 130])
@pytest.mark.parametrize("dilation", [1, 2, 16])
@pytest.mark.parametrize("e", [0, 6])
@pytest.mark.parametrize("h", [8, 40, 256])
def test_gated_tcn_step_matches_fp64_frame_loop(dev, H, h, e, dilation, b):
    """H below one 16-row tile, 40 = two and a half, 256 = the preset; B = 1, 5 and 130 (N = k B crosses the 64-column tile
    and, at k = 16, the 1024 columns where the 32-row tile takes over); the stream starts at counter 0 (zero-padded taps and
    their missing embedding terms) and runs until the ring of (P-1) d + 16 slots has wrapped more than twice, fed as chunks of
    k = 1, 3 and 16 frames: identical bits in g and in the ring, and an error against fp64 of at most twice that of the
    offline kernels on the same inputs (ps_unfold_taps_f32 + ps_conv1x1_f32 + ps_gated_product_f32: another order of the
    K = P H sums), floor 2e-6."""
    from puresound_amd.nnet.conv_tasnet import GatedTCN
    p = 3
    r = (p - 1) * dilation + 16
    t = 2 * r + 7
    blk = G.make_block(h, e, p, dilation, seed=h + 7 * e + dilation)
    gen = torch.Generator().manual_seed(b + dilation)
    y = (torch.rand(t, h, b, generator=gen, dtype=torch.float64) * 2 - 1).float().double()      # fp32-representable
    emb = (torch.rand(b, e, generator=gen, dtype=torch.float64) * 2 - 1).float().double() if e else None
    blk32 = {k: (v.float().double() if torch.is_tensor(v) else v) for k, v in blk.items()}
    want = G.block_step(y, 0, blk32, torch.zeros(t + 2 * dilation, h, b, dtype=torch.float64), emb)   # [T, H, B]

    wl = H.pack_wt(GatedTCN._unfolded(blk32["wl"].float()).to(dev))
    wr = H.pack_wt(GatedTCN._unfolded(blk32["wr"][:, :h, :].float().contiguous()).to(dev))
    pl, keep_l = _pro(H, blk32, "l", dev)
    pr, keep_r = _pro(H, blk32, "r", dev)
    taps = G.emb_taps(blk32, emb).float().to(dev).contiguous() if e else None   # (fp64 products rounded once: the session's
    runs = {}                                                                   #  come from ps_conv1x1_f32)
    for k in (1, 3, 16):
        ld = H.padded_frames(k * b)
        ring = torch.zeros(r, h, b, device=dev)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        got = []
        for t0 in range(0, t, k):
            kk = min(k, t - t0)
            ybuf = torch.full((1, h, ld), float("nan"), device=dev)                 # NaN in the columns past k B
            ybuf[0, :, :kk * b] = y[t0:t0 + kk].permute(1, 0, 2).reshape(h, kk * b).float().to(dev)
            out = torch.full((1, h, ld), float("nan"), device=dev)
            H.gated_tcn_step(ybuf, ring, counter, wl, wr, p, dilation, b, kk, pl, pr, taps, out=out)
            assert bool(torch.isnan(out[0, :, kk * b:]).all())                       # nothing written past the chunk
            got.append(out[0, :, :kk * b].reshape(h, kk, b).permute(1, 0, 2))
            counter += kk
        runs[k] = (torch.cat(got).cpu(), ring.cpu())
    for k in (3, 16):
        assert torch.equal(runs[k][0], runs[1][0]), f"g differs between k = 1 and k = {k}"
        assert torch.equal(runs[k][1], runs[1][1]), f"the ring differs between k = 1 and k = {k}"
    for g_slot in range(t - r, t):                                                   # the ring holds the last R frames
        assert torch.equal(runs[1][1][g_slot % r], y[g_slot].float())
    err = rel_max(runs[1][0].numpy(), want.numpy())

    # the offline pieces on the same inputs: [B, H, ldt] rows of T frames
    yo = H.pad_rows(y.permute(2, 1, 0).float().contiguous().to(dev))
    left = (p - 1) * dilation
    col_l = H.unfold_taps(yo, t, p, dilation, left)
    col_r = col_l if not e else H.unfold_taps(yo, t, p, dilation, left, None, None, emb.float().to(dev).contiguous())
    lo, _ = H.conv1x1(col_l, t, wl, h)
    ro, _ = H.conv1x1(col_r, t, H.pack_wt(GatedTCN._unfolded(blk32["wr"].float()).to(dev)), h)
    off = H.unpad_rows(H.gated_product(lo, ro, t, pl, pr), t).permute(2, 1, 0).cpu()
    err_off = rel_max(off.numpy(), want.numpy())
    print(f"gated_tcn_step H={h} E={e} d={dilation} B={b}: error vs fp64 {err:.3e}, offline pieces {err_off:.3e}")
    assert err <= max(2 * err_off, 2e-6), (err, err_off)


def test_gated_tcn_step_refuses_what_it_does_not_take(dev, H):
    from puresound_amd._abi import PS_NORM_GLOBAL
    h, b = 8, 2
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    y, ring, counter = z(1, h, 128), z(3, h, b), torch.zeros(1, dtype=torch.int32, device=dev)
    w = H.pack_wt(z(h, 3 * h))
    out = torch.full((1, h, 128), 7.0, device=dev)
    glob = H.make_prologue(PS_NORM_GLOBAL, True, None, 1.0, 1e-8, z(h), z(h), z(1))
    with pytest.raises(RuntimeError, match="global norm does not stream"):
        H.gated_tcn_step(y, ring, counter, w, w, 3, 1, b, 1, glob, None, out=out)
    with pytest.raises(RuntimeError, match=r"\(P-1\)\*dilation \+ k"):
        H.gated_tcn_step(y, ring, counter, w, w, 3, 1, b, 2, out=out)           # R = 3 < 2 + 2
    assert bool((out == 7.0).all()) and bool((ring == 0).all())                 # nothing was written


# ---- the streamed output ----------------------------------------------------------------------------------------------
def test_streamed_matches_reference_golden(dev, golden_dir):
    from puresound_amd.streaming import StreamingUnetTcn
    g = dict(np.load(os.path.join(golden_dir, PRESET + ".npz")))
    model = _model("preset", dev)
    x = det_wave(1234, 2, 4000)[:, :3968].contiguous().to(dev)       # 31 hops -> 28 frames, as offline
    enroll = det_wave(1235, 2, 3000).to(dev)
    s = StreamingUnetTcn(model)
    assert (s.hop_length, s.delay_frames, s.prime_hops, s.latency_samples) == (128, 6, 9, 1152)
    sl = slice(16, g["wav"].shape[1] - 16)
    for chunk in (None, 5):                                          # step() checks None for exactly 9 hops in _stream
        y = _stream(s, x, chunk, enroll=enroll).cpu().numpy()
        assert y.shape == g["wav"].shape
        assert rel_max(y[:, sl], g["wav"][:, sl]) <= TOL, chunk


def _against_offline(model, s, x, enroll, chunk):
    y = _stream(s, x, chunk, enroll=enroll)
    ref = _offline(model, x, enroll)
    assert y.shape == ref.shape
    sl = slice(16, ref.shape[1] - 16)
    for b in range(x.shape[0]):
        assert rel_max(y[b, sl].cpu().numpy(), ref[b, sl].cpu().numpy()) <= TOL, b
    return y


def test_long_stream_of_the_reduced_model_matches_offline(dev):
    """300 frames, B = 5: past the receptive field of the 2 x 3 gated blocks and many turns of every ring."""
    from puresound_amd.streaming import StreamingUnetTcn
    model = _model("small", dev)
    x = det_wave(31, 5, 128 * 303).to(dev)
    enroll = det_wave(32, 5, 3000).to(dev)
    _against_offline(model, StreamingUnetTcn(model), x, enroll, 16)


def test_two_seconds_of_the_preset_match_offline(dev):
    """250 frames: longer than the TCN's receptive field of 3 x 62 = 186 frames, which the golden's 28 frames never leave."""
    from puresound_amd.streaming import StreamingUnetTcn
    model = _model("preset", dev)
    x = det_wave(41, 2, 32000 - 32000 % 128).to(dev)
    enroll = det_wave(42, 2, 3000).to(dev)
    _against_offline(model, StreamingUnetTcn(model), x, enroll, 8)


# ---- the session ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [1, 2, 6])
def test_streams_shorter_than_the_delay_flush_correctly(dev, frames):
    """1, 2 and 6 frames against delays of 3 (reduced model) and 6 (preset) frames: fewer than the delay, exactly the delay,
    more.  Up to the delay every step() returns None (checked in _stream) and flush() returns the whole offline output."""
    from puresound_amd.streaming import StreamingUnetTcn
    for key in ("small", "preset"):
        model = _model(key, dev)
        s = StreamingUnetTcn(model)
        x = det_wave(50 + frames, 2, (frames + 3) * 128).to(dev)
        enroll = det_wave(60, 2, 3000).to(dev)
        y = _against_offline(model, s, x, enroll, None)
        assert y.shape[1] == (frames - 1) * 128 + 512


def test_graph_eager_step_chunk_give_the_same_bits(dev):
    from puresound_amd.streaming import StreamingUnetTcn
    model = _model("small", dev)
    s = StreamingUnetTcn(model)
    x = det_wave(71, 3, 128 * 40).to(dev)
    enroll = det_wave(72, 3, 3000).to(dev)
    base = _stream(s, x, None, enroll=enroll)
    for chunk, graph in ((None, False), (7, True), (7, False), (16, True)):
        assert torch.equal(_stream(s, x, chunk, use_graph=graph, enroll=enroll), base), (chunk, graph)


def test_streams_are_independent(dev):
    from puresound_amd.streaming import StreamingUnetTcn
    model = _model("small", dev)
    s = StreamingUnetTcn(model)
    x = det_wave(77, 5, 128 * 60).to(dev)
    enroll = det_wave(78, 5, 3000).to(dev)
    y = _stream(s, x, 7, enroll=enroll)
    sl = slice(16, y.shape[1] - 16)
    for b in range(5):
        alone = _stream(s, x[b:b + 1].contiguous(), 7, enroll=enroll[b:b + 1].contiguous())
        assert rel_max(alone[:, sl].cpu().numpy(), y[b:b + 1, sl].cpu().numpy()) < 1e-5, b


def test_without_transpose_delay_the_latency_is_the_window(dev):
    from puresound_amd.streaming import StreamingUnetTcn
    model = _model("small_nodelay", dev, transpose_delay=False)
    s = StreamingUnetTcn(model)
    assert (s.delay_frames, s.prime_hops, s.latency_samples) == (0, 3, 384)
    x = det_wave(81, 2, 128 * 50).to(dev)
    enroll = det_wave(82, 2, 3000).to(dev)
    _against_offline(model, s, x, enroll, None)
    _against_offline(model, s, x, enroll, 6)


def test_model_is_left_intact_and_embed_equals_enroll(dev):
    from puresound_amd.streaming import StreamingUnetTcn
    model = _model("small", dev)
    x = det_wave(91, 2, 128 * 30).to(dev)
    enroll = det_wave(92, 2, 3000).to(dev)
    before = model.inference(x, enroll)
    s = StreamingUnetTcn(model)
    y = _stream(s, x, 5, enroll=enroll)
    assert torch.equal(model.inference(x, enroll), before)
    assert torch.equal(_stream(s, x, 5, embed=model.inference_tse_embedding(enroll)), y)
    with pytest.raises(ValueError, match="exactly one of enroll"):
        s.init_streams(2)
    with pytest.raises(ValueError, match="exactly one of enroll"):
        s.init_streams(2, enroll=enroll, embed=model.inference_tse_embedding(enroll))


def test_parameter_change_rebuilds_the_packs(dev):
    from puresound_amd.streaming import StreamingUnetTcn
    model = copy.deepcopy(_model("small", dev))
    x = det_wave(95, 2, 128 * 24).to(dev)
    enroll = det_wave(96, 2, 3000).to(dev)
    s = StreamingUnetTcn(model)
    y0 = _stream(s, x, 4, enroll=enroll)
    with torch.no_grad():
        model.masker.tcn_list[1][0].right_conv[0].weight.mul_(0.5)   # a block that takes the embedding
        model.masker.cnn_up[1][0].weight.mul_(1.25)
    y1 = _against_offline(model, s, x, enroll, 4)
    assert not torch.equal(y0, y1)
