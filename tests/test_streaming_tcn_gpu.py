"""Hop-by-hop streaming of the causal time-domain Conv-TasNet (puresound_amd/streaming/tcn.py) on the MI355X: against the
reference goldens, the offline HIP path, the CPU oracle, itself (graph / eager, step / chunk, B = 1 / B, one stream's input
against another's output), and unit checks of its kernels (ps_dwconv_step_f32, ps_free_decode_step_f32)."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
from conftest import rel_max
from detweights import det_state_dict, det_wave
from oracle import separator_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4
SCHEDULE = (1, 3, 8, 16, 37)


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


def _stream(s, x, enroll=None, schedule=None, use_graph=True):
    """Stream x [B, L] (L a multiple of the hop) -> emitted samples ‖ flush(), [B, L_out]; schedule: hops per step_chunk
    call, cycled (None: step())."""
    hop = s.hop_length
    s.init_streams(streams=x.shape[0], enroll=enroll, use_graph=use_graph)
    outs, hops, i, j = [], x.shape[1] // hop, 0, 0
    while i < hops:
        if schedule is None:
            y = s.step(x[:, i * hop:(i + 1) * hop])
            assert (y is None) == (i < s.prime_hops)
            i += 1
        else:
            k = min(schedule[j % len(schedule)], hops - i)
            y = s.step_chunk(x[:, i * hop:(i + k) * hop])
            i, j = i + k, j + 1
        if y is not None:
            outs.append(y)
    outs.append(s.flush())
    return torch.cat(outs, dim=1)


def _inputs(name, dev):
    c = cases.CASES[name]
    hop = c["enc"]["hop"]
    x = det_wave(c["seed"], c["B"], c["L"])
    x = x[:, :x.shape[1] // hop * hop].contiguous().to(dev)
    e = det_wave(c["seed"] + 1, c["B"], c["L_enroll"]).to(dev) if "L_enroll" in c else None
    return x, e


@pytest.mark.parametrize("name", ["cfg3_causal_short", "tiny_free_relu_causal"])
def test_streamed_matches_reference_golden(dev, golden_dir, name):
    from puresound_amd.streaming import StreamingConvTasNet
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    model, _ = _model(name, dev)
    x, e = _inputs(name, dev)
    s = StreamingConvTasNet(model)
    win, hop = cases.CASES[name]["enc"]["win"], cases.CASES[name]["enc"]["hop"]
    assert (s.hop_length, s.latency_samples) == (hop, win - hop)
    for schedule in (None, SCHEDULE):
        y = _stream(s, x, e, schedule).cpu().numpy()
        assert y.shape == g["wav"].shape
        assert rel_max(y, g["wav"]) < TOL, schedule


def test_long_streams_match_offline_fp32(dev):
    """The preset at B = 4 x 10 s: ~10 000 frames, every ring (at most 272 + 16 slots) wraps many times."""
    from puresound_amd.streaming import StreamingConvTasNet
    model, _ = _model("cfg3_causal_short", dev)
    model.set_gemm_precision("fp32")
    try:
        x = det_wave(31, 4, 160000).to(dev)
        e = det_wave(32, 4, 32000).to(dev)
        y = _stream(StreamingConvTasNet(model), x, e, (16,))
        ref = model.inference(x, e)
    finally:
        model.set_gemm_precision("fp16x2")
    assert y.shape == ref.shape
    for b in range(4):
        assert rel_max(y[b].cpu().numpy(), ref[b].cpu().numpy()) <= 1e-5, b


def test_model_left_intact(dev):
    from puresound_amd.streaming import StreamingConvTasNet
    model, _ = _model("cfg3_causal_short", dev)
    x, e = _inputs("cfg3_causal_short", dev)
    before = model.inference(x, e)
    s = StreamingConvTasNet(model)
    _stream(s, x, e, (4,))
    _stream(s, x, e, None, use_graph=False)
    assert all(m.gemm_precision == "fp16x2" for stack in model.masker.tcn_list for m in stack)
    assert torch.equal(model.inference(x, e), before)


def test_cln_variant_matches_offline_and_oracle(dev):
    from puresound_amd.streaming import StreamingConvTasNet
    name = "tiny_free_relu_causal"
    model, sd = _model(name, dev, **CLN)
    x = det_wave(41, 3, 8 * 300).to(dev)
    y = _stream(StreamingConvTasNet(model), x, None, SCHEDULE)
    ref = model.inference(x)
    assert y.shape == ref.shape
    assert rel_max(y.cpu().numpy(), ref.cpu().numpy()) <= 1e-5
    saved = cases.CASES[name]
    cases.CASES[name] = _case(name, CLN)
    try:
        cfg = cases.oracle_cfg(name)
    finally:
        cases.CASES[name] = saved
    oracle = O.inference(x.cpu(), sd, cfg)
    assert rel_max(y.cpu().numpy(), oracle.numpy()) <= TOL


def test_graph_eager_step_chunk(dev):
    """Graph replay and eager run the same launches: the same bits.  step() and step_chunk tile their GEMMs by another
    column count, so they agree to fp32 roundings."""
    from puresound_amd.streaming import StreamingConvTasNet
    model, _ = _model("cfg3_causal_short", dev)
    x, e = _inputs("cfg3_causal_short", dev)
    s = StreamingConvTasNet(model)
    a = _stream(s, x, e, SCHEDULE, use_graph=True)
    b = _stream(s, x, e, SCHEDULE, use_graph=False)
    assert torch.equal(a, b)
    c = _stream(s, x, e, None)
    assert rel_max(c.cpu().numpy(), a.cpu().numpy()) <= 1e-6


def test_streams_are_independent(dev):
    from puresound_amd.streaming import StreamingConvTasNet
    model, _ = _model("cfg3_causal_short", dev)
    s = StreamingConvTasNet(model)
    x = det_wave(77, 64, 16 * 200).to(dev)
    e = det_wave(78, 64, 4000).to(dev)
    y = _stream(s, x, e, (8,))
    x2, e2 = x.clone(), e.clone()
    x2[5] = det_wave(79, 1, 16 * 200)[0].to(dev)
    e2[5] = det_wave(80, 1, 4000)[0].to(dev)
    y2 = _stream(s, x2, e2, (8,))
    keep = [b for b in range(64) if b != 5]
    assert torch.equal(y[keep], y2[keep])
    assert not torch.equal(y[5], y2[5])
    for b in (0, 5, 63):
        alone = _stream(s, x[b:b + 1].contiguous(), e[b:b + 1].contiguous(), (8,))
        assert rel_max(alone.cpu().numpy(), y[b:b + 1].cpu().numpy()) <= 1e-5, b


def test_training_mode_refused(dev):
    from puresound_amd.streaming import StreamingConvTasNet
    model, _ = _model("tiny_free_relu_causal", dev)
    model.train()
    try:
        with pytest.raises(RuntimeError):
            StreamingConvTasNet(model)
    finally:
        model.eval()


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


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("d", [1, 3, 128])
@pytest.mark.parametrize("p", [2, 3, 5])
def test_dwconv_step_kernel(dev, H, p, d, affine):
    from puresound_amd._abi import PS_NORM_AFFINE
    h, b = 6, 3
    r = (p - 1) * d + 16
    t_len = r + 200                                     # the ring wraps
    seed = p * 1000 + d * 10 + int(affine)
    x = _rand((b, h, t_len), seed)
    w = _rand((h, 1, p), seed + 1)
    bias = _rand((h,), seed + 2)
    gamma, beta = _rand((h,), seed + 3) + 1.5, _rand((h,), seed + 4) + 0.5    # beta != 0: PReLU(beta) is not 0
    slope = torch.tensor([0.25], dtype=torch.float64)
    a = F.prelu(x * gamma.view(1, -1, 1) + beta.view(1, -1, 1), slope) if affine else x
    ref = F.conv1d(F.pad(a, ((p - 1) * d, 0)), w, bias, dilation=d, groups=h)
    f32 = lambda t: t.float().to(dev)  # noqa: E731
    g32, b32, s32 = f32(gamma), f32(beta), f32(slope)
    pro = H.make_prologue(PS_NORM_AFFINE, True, None, 0.0, 1e-8, g32, b32, s32) if affine else None
    ring = torch.zeros(r, h, b, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    got, t0 = [], 0
    for k in _chunks(t_len):
        ld = H.padded_frames(k * b)
        xin = torch.full((1, h, ld), float("nan"), device=dev)
        xin[0, :, :k * b] = f32(x[:, :, t0:t0 + k].permute(1, 2, 0).reshape(h, k * b))
        y = torch.zeros(1, h, ld, device=dev)
        H.dwconv_step(xin, ring, counter, f32(w), f32(bias), d, b, k, pro, out=y)
        assert float(y[0, :, k * b:].abs().max()) == 0.0             # columns past the chunk are not written
        got.append(y[0, :, :k * b].reshape(h, k, b).permute(2, 0, 1).cpu())
        counter += k
        t0 += k
    got = torch.cat(got, dim=2)
    assert rel_max(got.numpy(), ref.numpy()) < 2e-6


@pytest.mark.parametrize("out_mode", ["linear", "sigmoid", "none"])
@pytest.mark.parametrize("mask_act", ["linear", "relu", "sigmoid"])
@pytest.mark.parametrize("win,hop,b", [(16, 16, 3), (16, 8, 70), (32, 8, 5)])
def test_free_decode_step_kernel(dev, H, win, hop, b, mask_act, out_mode):
    c, t_len = 24, 45
    seed = win * 100 + hop + b
    feats = _rand((b, c, t_len), seed) * 0.6
    mask = _rand((b, c, t_len), seed + 1) * 2.0
    w = _rand((c, 1, win), seed + 2)
    act = {"linear": lambda m: m, "relu": torch.relu, "sigmoid": torch.sigmoid}[mask_act]
    ref = F.conv_transpose1d(feats * act(mask), w, stride=hop)[:, 0]
    ref = {"linear": lambda v: v.clamp(-1, 1), "sigmoid": torch.sigmoid, "none": lambda v: v}[out_mode](ref)
    f32 = lambda t: t.float().to(dev)  # noqa: E731
    w32 = f32(w)
    tail = torch.zeros(b, win - hop, device=dev)
    got, t0 = [], 0
    for k in _chunks(t_len):
        ld = H.padded_frames(k * b)
        fin = torch.full((1, c, ld), float("nan"), device=dev)
        min_ = torch.full((1, c, ld), float("nan"), device=dev)
        fin[0, :, :k * b] = f32(feats[:, :, t0:t0 + k].permute(1, 2, 0).reshape(c, k * b))
        min_[0, :, :k * b] = f32(mask[:, :, t0:t0 + k].permute(1, 2, 0).reshape(c, k * b))
        out = torch.full((b, k * hop), float("nan"), device=dev)
        H.free_decode_step(fin, min_, w32, tail, out, hop, k, mask_act, out_mode)
        got.append(out.cpu())
        t0 += k
    last = torch.empty(b, win - hop, device=dev)
    H.free_decode_step(None, None, w32, tail, last, hop, out_mode=out_mode, flush=True)
    got = torch.cat(got + [last.cpu()], dim=1)
    assert got.shape == ref.shape
    assert rel_max(got.numpy(), ref.numpy()) <= 1e-5
