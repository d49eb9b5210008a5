"""ps_conv2d_ragged_f32 and ps_istft_ola_ragged_f32 on the MI355X, through their wrappers: row n of a launch with per-row frame
limits is, bit for bit, what the plain entry computes for that row alone with T = T_in = T_n (nothing in either summation order
depends on T), exact 0.0 behind it, and the same bits whatever stands behind a row's end -- NaN included, in both sources of
the convolution and in the frames the overlap-add must not load.  Both routes of the convolution (the implicit GEMM at
MB = 1 / 2 / 4, the row-block kernel at MM = 2 / 4) with limits at their tile edges, and two cases against the float64
oracle at the FP32 bound of test_abi_kernels_gpu.py."""
import pytest
import torch

from abi_refs import rand as _rand
from conftest import rel_max
from oracle import unet_oracle as UO
from puresound_amd import _abi

pytestmark = pytest.mark.gpu
FP32 = 2e-5          # test_abi_kernels_gpu.FP32
NAN = float("nan")

# the implicit GEMM's frame tile is 128, the row-block kernel's workgroup 512 frames (a thread owns t and t + 256)
GEMM_T, GEMM_LD, GEMM_ROWS = 300, 384, (300, 1, 127, 128, 129, 256, 257, 0, 305)     # (the last two are clamped)
ROWS_T, ROWS_LD, ROWS_ROWS = 600, 640, (600, 1, 255, 256, 257, 511, 512, 513)

# name: (transposed, C1, C2, Fin, kf, kt, sf, pad_t, M, Fout)
CONV = {
    "conv_m8": (False, 3, 0, 9, 3, 2, 1, 1, 8, 9),
    "conv_ahead_m40": (False, 2, 0, 11, 5, 2, 2, 0, 40, 6),          # pad_t = 0: the second time tap is one frame ahead
    "up_m70_fout8": (True, 3, 2, 4, 3, 2, 2, 0, 70, 8),              # Fout % 8 == 0: the XCD-aware block order
    "up_m70_fout10": (True, 3, 2, 5, 3, 2, 2, 0, 70, 10),
    "up_delay_m2": (True, 3, 2, 5, 3, 2, 2, 1, 2, 10),               # transpose_delay: one frame ahead, both sources
    "conv_m4": (False, 3, 0, 9, 3, 2, 1, 1, 4, 9),
}


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
    """NaN-filled blocks in torch's caching allocator: `torch.empty` outputs start as NaN, not as zeros."""
    junk = [torch.full((1 << 22,), NAN, device=dev) for _ in range(8)]
    del junk
    yield


def _problem(name):
    transposed, c1, c2, f_in, kf, kt, sf, pt, m, f_out = CONV[name]
    t, ld, rows = (ROWS_T, ROWS_LD, ROWS_ROWS) if m <= 4 else (GEMM_T, GEMM_LD, GEMM_ROWS)
    n = len(rows)
    x1 = _rand((n, c1, f_in, ld), 61)
    x2 = _rand((n, c2, f_in, ld), 62) if c2 else None
    w2, b = _rand((m, (c1 + c2) * kf * kt), 63, -0.3, 0.3), _rand((m,), 64)
    geom = (f_out, kf, kt, sf, 1, 1, kf // 2, pt, transposed)
    return x1, x2, w2, b, t, ld, rows, geom


def _nan_behind(x, rows, t):
    x = x.clone()
    for n, tn in enumerate(rows):
        x[n, ..., max(0, min(tn, t)):] = NAN
    return x


@pytest.mark.parametrize("act", ["prelu", "none"])
@pytest.mark.parametrize("name", list(CONV))
def test_conv2d_ragged_is_each_row_alone_bit_for_bit(H, dev, name, act):
    x1, x2, w2, b, t, ld, rows, geom = _problem(name)
    m = w2.shape[0]
    wt, bd = H.pack_wt(w2.to(dev)), b.to(dev)
    slope = torch.tensor([0.2], device=dev) if act == "prelu" else None
    lim = torch.tensor(rows, dtype=torch.int32, device=dev)
    d1, d2 = x1.to(dev), (None if x2 is None else x2.to(dev))
    y = H.conv2d_ragged(d1, d2, wt, bd, m, t, lim, *geom, act, slope)
    n1, n2 = _nan_behind(x1, rows, t).to(dev), (None if x2 is None else _nan_behind(x2, rows, t).to(dev))
    y_nan = H.conv2d_ragged(n1, n2, wt, bd, m, t, lim, *geom, act, slope)
    torch.cuda.synchronize()
    assert y.shape == (len(rows), m, geom[0], ld)
    assert torch.equal(y, y_nan), "what stands behind a row's end reached the result"
    assert not torch.isnan(y).any()
    for n, tn in enumerate(rows):
        tn = max(0, min(tn, t))
        assert float(y[n, ..., tn:].abs().max()) == 0.0, (n, tn)
        if tn == 0:
            continue
        alone = H.conv2d(d1[n:n + 1], None if d2 is None else d2[n:n + 1], wt, bd, m, tn, *geom, act, slope, t_in=tn)
        assert torch.equal(y[n, ..., :tn], alone[0, ..., :tn]), (n, tn)
        assert float(y[n, ..., :tn].abs().max()) > 0.0


@pytest.mark.parametrize("name", ["conv_ahead_m40", "up_m70_fout10", "up_delay_m2"])
def test_conv2d_ragged_against_the_float64_oracle(H, dev, name):
    """nn.ZeroPad2d + nn.Conv2d / nn.ConvTranspose2d + the time trim of each row's valid frames alone, PReLU behind it"""
    transposed, c1, c2, f_in, kf, kt, sf, pt, m, f_out = CONV[name]
    x1, x2, w2, b, t, ld, rows, geom = _problem(name)
    lim = torch.tensor(rows, dtype=torch.int32, device=dev)
    slope = torch.tensor([0.2], device=dev)
    y = H.conv2d_ragged(x1.to(dev), None if x2 is None else x2.to(dev), H.pack_wt(w2.to(dev)), b.to(dev), m, t, lim, *geom,
                        "prelu", slope).cpu()
    x = (torch.cat([x1, x2], 1) if c2 else x1).double()
    pf = kf // 2
    worst = 0.0
    for n, tn in enumerate(rows):
        tn = max(0, min(tn, t))
        if tn == 0:
            continue
        xn = x[n:n + 1, ..., :tn]
        if transposed:
            w4 = w2.double().reshape(m, c1 + c2, kf, kt).permute(1, 0, 2, 3)
            full = UO.conv_transpose2d(xn, w4, b.double(), (sf, 1), (1, 1), (pf, 0), (sf - kf + 2 * pf, 0))
            pre = full[..., pt:pt + tn]           # the trim: frames [shift, shift + T) of the T + kt - 1
        else:
            pre = UO.conv2d(xn, w2.double().reshape(m, c1, kf, kt), b.double(), (sf, 1), (1, 1), (pf, pf), (pt, kt - 1 - pt))
        ref = torch.where(pre >= 0, pre, 0.2 * pre)
        assert ref.shape == (1, m, f_out, tn)
        worst = max(worst, rel_max(y[n:n + 1, ..., :tn].numpy(), ref.numpy()))
    print(f"conv2d_ragged {name}: rel_max against float64 {worst:.3e}")
    assert worst < FP32


def test_conv2d_ragged_refuses_on_the_host(H, dev):
    x = torch.zeros(2, 2, 4, 128, device=dev)
    wt, b = H.pack_wt(torch.zeros(3, 12, device=dev)), torch.zeros(3, device=dev)
    lim = torch.tensor([100, 50], dtype=torch.int32, device=dev)
    y = torch.empty(2, 3, 4, 128, device=dev)
    ptr, L = _abi.ptr, H.lib()
    args = lambda t_rows: (ptr(x), 2, None, 0, ptr(wt), ptr(b), ptr(y), 2, 3, 4, t_rows, 100, 128, 3, 2, 1, 1, 1, 1, 1, 4, 0, 1,  # noqa: E731
                           None, _abi.stream_ptr(dev))
    assert L.ps_conv2d_ragged_f32(*args(None)) == -1                       # PS_E_INVALID
    assert b"t_rows is NULL" in L.ps_last_error()
    assert L.ps_conv2d_ragged_f32(*args(ptr(lim))) == 0
    ok = (4, 3, 2, 1, 1, 1, 1, 1, False)
    with pytest.raises(RuntimeError, match="ps_conv2d_ragged_f32"):       # PReLU without a slope: conv2d_args' rule
        H.conv2d_ragged(x, None, wt, b, 3, 100, lim, *ok, "prelu", None)
    with pytest.raises(RuntimeError):                                       # more frames than the row holds
        H.conv2d_ragged(x, None, wt, b, 3, 129, lim, *ok, "relu", None)
    with pytest.raises(ValueError, match="int32 tensor"):                   # limits of another batch size
        H.conv2d_ragged(x, None, wt, b, 3, 100, lim[:1].contiguous(), *ok, "relu", None)
    with pytest.raises(RuntimeError, match="limits"):                       # limits on the host
        H.conv2d_ragged(x, None, wt, b, 3, 100, lim.cpu(), *ok, "relu", None)
    torch.cuda.synchronize()


# ---- the overlap-add ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_mode", ["linear", "sigmoid", "none"])
@pytest.mark.parametrize("n_fft,hop,t", [(32, 8, 37), (512, 128, 9)])
def test_istft_ola_ragged_is_each_row_alone_bit_for_bit(H, dev, n_fft, hop, t, out_mode):
    rows = (1, 3, 4, 5, t, 0, t - 1, t + 7)
    n, ld = len(rows), 128
    frames = (_rand((n, n_fft, ld), 71) * 3.0).to(dev)
    window = torch.hann_window(n_fft).to(dev)
    lim = torch.tensor(rows, dtype=torch.int32, device=dev)
    y = H.istft_ola_ragged(frames, t, lim, window, hop, out_mode)
    poisoned = frames.clone()
    for i, tn in enumerate(rows):
        poisoned[i, :, max(0, min(tn, t)):] = NAN
    y_nan = H.istft_ola_ragged(poisoned, t, lim, window, hop, out_mode)
    torch.cuda.synchronize()
    assert y.shape == (n, (t - 1) * hop + n_fft) and torch.equal(y, y_nan) and not torch.isnan(y).any()
    for i, tn in enumerate(rows):
        tn = max(0, min(tn, t))
        valid = (tn - 1) * hop + n_fft if tn else 0
        assert float(y[i, valid:].abs().max() if valid < y.shape[1] else 0.0) == 0.0, (i, tn)
        if tn == 0:
            continue
        alone = H.istft_ola(frames[i:i + 1], tn, window, hop, out_mode)
        assert alone.shape == (1, valid) and torch.equal(y[i, :valid], alone[0]), (i, tn)
        assert float(y[i, :valid].abs().max()) > 0.0
    with pytest.raises(ValueError, match="int32 tensor"):
        H.istft_ola_ragged(frames, t, lim[:2].contiguous(), window, hop, out_mode)
    assert H.lib().ps_istft_ola_ragged_f32(_abi.ptr(frames), _abi.ptr(window), _abi.ptr(y), None, n, n_fft, hop, t, ld, 2,
                                           _abi.stream_ptr(dev)) == -1
