"""Hop-by-hop streaming of the causal conv-STFT noise suppressors (puresound_amd/streaming/spectral.py) on the MI355X:
against the reference goldens, the offline HIP path, the CPU oracle, itself (graph / eager, step / chunk, B = 1 / B), and
unit checks of its kernels (ps_conv2d_step_f32, ps_stream_commit_f32, ps_istft_step_f32)."""
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
NS = ["ns_dpcrn_short", "ns_dparn_short"]


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


def _model(name, dev):
    if name not in _MODELS:
        import puresound_amd.nnet as PA
        m = cases.build(PA.NS, name).eval()
        sd = det_state_dict(m)
        m.load_state_dict(sd)
        _MODELS[name] = (m.to(dev), sd)
    return _MODELS[name]


def _stream(sep, x, chunk=None, use_graph=True):
    """Stream x [B, L] (L a multiple of the hop) -> emitted samples ‖ flush(), [B, L_out]; chunk: hops per step_chunk call
    (None: step())."""
    hop = sep.hop_length
    sep.init_streams(streams=x.shape[0], use_graph=use_graph)
    outs, hops = [], x.shape[1] // hop
    if chunk is None:
        for i in range(hops):
            y = sep.step(x[:, i * hop:(i + 1) * hop])
            assert (y is None) == (i < sep.prime_hops)
            if y is not None:
                outs.append(y)
    else:
        for i in range(0, hops, chunk):
            outs.append(sep.step_chunk(x[:, i * hop:min(hops, i + chunk) * hop]))
    outs.append(sep.flush())
    return torch.cat(outs, dim=1)


@pytest.mark.parametrize("name", NS)
def test_streamed_matches_reference_golden(dev, golden_dir, name):
    from puresound_amd.streaming import StreamingSeparator
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    model, _ = _model(name, dev)
    x = det_wave(1234, 2, 4000)[:, :3968].contiguous().to(dev)     # 31 hops -> 28 frames, as offline
    sep = StreamingSeparator(model)
    assert (sep.hop_length, sep.latency_samples) == (128, 384)
    sl = slice(16, g["wav"].shape[1] - 16)
    for chunk in (None, 5):                                          # 5-hop chunks: the last one is a short one
        y = _stream(sep, x, chunk).cpu().numpy()
        assert y.shape == g["wav"].shape
        assert rel_max(y[:, sl], g["wav"][:, sl]) <= TOL, chunk


@pytest.mark.parametrize("name", NS)
def test_long_streams_match_offline_and_oracle(dev, name):
    from puresound_amd.streaming import StreamingSeparator
    model, sd = _model(name, dev)
    sep = StreamingSeparator(model)
    x = det_wave(31, 8, 160000).to(dev)                              # 10 s at 16 kHz, 8 streams
    y = _stream(sep, x, 16)
    model.set_gemm_precision("fp32")
    try:
        ref = model.inference(x)
    finally:
        model.set_gemm_precision("fp16x2")
    assert y.shape == ref.shape
    sl = slice(16, ref.shape[1] - 16)
    assert rel_max(y[:, sl].cpu().numpy(), ref[:, sl].cpu().numpy()) <= TOL
    x3 = det_wave(32, 2, 48000)                                      # 3 s against the CPU oracle
    ref3 = O.inference(x3, sd, cases.oracle_cfg(name))
    y3 = _stream(sep, x3.to(dev), 4).cpu()
    sl = slice(16, ref3.shape[1] - 16)
    assert y3.shape == ref3.shape
    assert rel_max(y3[:, sl].numpy(), ref3[:, sl].numpy()) <= TOL


@pytest.mark.parametrize("name", NS)
def test_streams_are_independent(dev, name):
    from puresound_amd.streaming import StreamingSeparator
    model, _ = _model(name, dev)
    sep = StreamingSeparator(model)
    x = det_wave(77, 5, 128 * 60).to(dev)                            # 5 different signals, B not a multiple of anything
    y = _stream(sep, x, 7)
    model.set_gemm_precision("fp32")
    try:
        ref = model.inference(x)
    finally:
        model.set_gemm_precision("fp16x2")
    sl = slice(16, ref.shape[1] - 16)
    assert rel_max(y[:, sl].cpu().numpy(), ref[:, sl].cpu().numpy()) <= TOL
    # the reused GEMM / recurrence kernels pick their tiling from the column count, so a stream's sums run in another order
    # at B = 1 than at B = 5: equal to a few fp32 roundings (measured 1.5e-6 / 1.9e-6), not bit for bit
    for b in range(5):
        alone = _stream(sep, x[b:b + 1].contiguous(), 7)
        assert rel_max(y[b:b + 1].cpu().numpy(), alone.cpu().numpy()) <= 1e-5, b


@pytest.mark.parametrize("name", NS)
def test_graph_eager_step_chunk_identical(dev, name):
    """Every kernel of the hop body is deterministic (fixed reduction order), so the four ways give the same bits."""
    from puresound_amd.streaming import StreamingSeparator
    model, _ = _model(name, dev)
    sep = StreamingSeparator(model)
    x = det_wave(5, 3, 128 * 40).to(dev)
    ys = [_stream(sep, x, chunk, graph) for graph in (True, False) for chunk in (None, 4, 16)]
    for y in ys[1:]:
        assert torch.equal(y, ys[0])


@pytest.mark.parametrize("name", NS)
def test_model_left_intact(dev, name):
    from puresound_amd.streaming import StreamingSeparator
    model, _ = _model(name, dev)
    x = det_wave(9, 2, 128 * 50).to(dev)
    before = model.inference(x)
    sep = StreamingSeparator(model)
    _stream(sep, x, 4)
    _stream(sep, x, None, use_graph=False)
    assert all(m.gemm_precision == "fp16x2" for m in model.masker.modules() if hasattr(m, "_plan_get"))
    assert torch.equal(model.inference(x), before)


def test_parameter_change_rebuilds(dev):
    from puresound_amd.streaming import StreamingSeparator
    import puresound_amd.nnet as PA
    name = "ns_dpcrn_short"
    model = cases.build(PA.NS, name).eval()
    model.load_state_dict(det_state_dict(model))
    model.to(dev)
    sep = StreamingSeparator(model)
    x = det_wave(11, 2, 128 * 30).to(dev)
    _stream(sep, x, 4)
    with torch.no_grad():
        for p in model.masker.parameters():
            p.mul_(0.9)
    y = _stream(sep, x, 4)
    model.set_gemm_precision("fp32")
    ref = model.inference(x)
    sl = slice(16, ref.shape[1] - 16)
    assert rel_max(y[:, sl].cpu().numpy(), ref[:, sl].cpu().numpy()) <= TOL


# -------------------------------------------------------------------------------------------------------------------------
# kernel units
# -------------------------------------------------------------------------------------------------------------------------
def _rand(shape, seed):
    g = np.random.Generator(np.random.Philox(key=seed))
    return torch.tensor(g.uniform(-1.0, 1.0, shape), dtype=torch.float32)


CONV_CASES = [  # transposed, kf, kt, sf, df, dt, two sources, M
    (False, 5, 2, 2, 1, 1, False, 40),
    (False, 3, 3, 1, 1, 2, False, 7),
    (False, 3, 1, 1, 2, 1, True, 20),
    (False, 3, 2, 1, 1, 1, True, 70),
    (True, 3, 2, 2, 1, 1, True, 33),
    (True, 3, 3, 1, 1, 2, True, 12),
    (True, 5, 1, 2, 1, 1, False, 2),
    (True, 3, 2, 2, 1, 2, False, 64),
]


@pytest.mark.parametrize("b", [1, 5, 130])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv2d_step_kernel(dev, H, case, b):
    transposed, kf, kt, sf, df, dt, two, m = case
    c1, c2, f_in, t_len = 6, (4 if two else 0), 16, 7
    ci = c1 + c2
    seed = hash(case) % 1000 + b
    x = _rand((b, ci, f_in, t_len), seed).double()
    pf = kf // 2
    w = _rand((ci, m, kf, kt) if transposed else (m, ci, kf, kt), seed + 1).double() * 0.3
    bias = _rand((m,), seed + 2).double()
    slope = torch.tensor([0.25], dtype=torch.float64)
    hist = (kt - 1) * dt
    if transposed:
        op = sf - kf + 2 * pf
        ref = F.conv_transpose2d(x, w, stride=(sf, 1), padding=(pf, 0), output_padding=(op, 0), dilation=(df, dt))[..., :t_len]
        w2 = w.permute(1, 0, 2, 3).reshape(m, -1)
    else:
        ref = F.conv2d(F.pad(x, (hist, 0, pf, pf)), w, stride=(sf, 1), dilation=(df, dt))
        w2 = w.reshape(m, -1)
    ref = F.prelu(ref + bias.view(1, -1, 1, 1), slope)
    f_out = ref.shape[2]
    ldb = H.padded_frames(b)
    wt = H.pack_wt(w2.float().to(dev))
    srcs = [(c1, 0), (c2, c1)] if two else [(c1, 0)]
    rings = [torch.zeros(max(hist, 1), c, f_in, ldb, device=dev) for c, _ in srcs]
    cur = [torch.full((1, c, f_in, ldb), float("nan"), device=dev) for c, _ in srcs]
    y = torch.zeros(1, m, f_out, ldb, device=dev)
    table = H.commit_table(list(zip(cur, rings)))
    got = []
    for t in range(t_len):
        for buf, (c, off) in zip(cur, srcs):
            buf[0, :, :, :b] = x[:, off:off + c, :, t].permute(1, 2, 0).float().to(dev)
        H.conv2d_step(cur[0], rings[0] if hist else None, cur[1] if two else None, rings[1] if (two and hist) else None, wt,
                      bias.float().to(dev), m, b, f_out, kf, kt, sf, df, dt, pf, transposed, "prelu", slope.float().to(dev),
                      out=y)
        got.append(y[0, :, :, :b].permute(2, 0, 1).cpu().clone())
        H.stream_commit(table, None, dev)
    assert float(y[0, :, :, b:].abs().max()) == 0.0 if b < ldb else True   # pad frames are not written
    got = torch.stack(got, dim=-1)
    assert rel_max(got.numpy(), ref.numpy()) < 2e-6


@pytest.mark.parametrize("out_mode", ["linear", "sigmoid", "none"])
@pytest.mark.parametrize("n_fft,hop,t_len,b", [(64, 16, 7, 3), (64, 16, 2, 1), (512, 128, 9, 130), (48, 48, 3, 2)])
def test_istft_step_kernel(dev, H, n_fft, hop, t_len, b, out_mode):
    frames = _rand((b, n_fft, t_len), n_fft + t_len).to(dev) * 40.0
    window = torch.hann_window(n_fft).to(dev)
    ref = H.istft_ola(H.pad_rows(frames), t_len, window, hop, out_mode)
    ldb = H.padded_frames(b)
    tail = torch.zeros(b, n_fft - hop, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty(b, t_len * hop, device=dev)
    syn = torch.full((1, n_fft, ldb), float("nan"), device=dev)
    for t in range(t_len):
        syn[0, :, :b] = frames[:, :, t].t()
        H.istft_step(syn, window, tail, out[:, t * hop:(t + 1) * hop], counter, hop, out_mode)
        counter += 1
    last = torch.empty(b, n_fft - hop, device=dev)
    H.istft_step(None, window, tail, last, counter, hop, out_mode, flush=True)
    got = torch.cat([out, last], dim=1)
    assert got.shape == ref.shape
    assert rel_max(got.cpu().numpy(), ref.cpu().numpy()) <= 1e-6   # same frames, same summation order
