"""Every branch of the depthwise-conv, encoder / decoder and conv2d kernel choice, run once through its wrapper at the
smallest shape that reaches it and compared with a float64 reference (the oracle's operators on float64 tensors,
tests/abi_refs.py for conv2d).  NaN in the caching allocator, so that output a kernel leaves unwritten shows.  Which kernel
a case reaches is recorded, from a trace of tools/conv_dispatch_cases.py, in profiles/conv_dispatch_ledger.txt.

No tolerance is new: each assertion names the test of the same kernel it takes its bound from."""
import functools

import numpy as np
import pytest
import torch

import abi_refs as R
from abi_refs import rand as _rand
from conftest import rel_max
from oracle import separator_oracle as O
from puresound_amd import _abi

pytestmark = pytest.mark.gpu
NAN = float("nan")
WG = _abi.PS_DBG_DWCONV_WG


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
    """NaN-filled blocks in torch's caching allocator: `torch.empty` scratch and outputs start as NaN, not as zeros."""
    junk = [torch.full((1 << 22,), NAN, device=dev) for _ in range(16)]
    junk += [torch.full((n,), NAN, device=dev) for n in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20)]
    del junk
    yield


def _err(got, ref):
    return rel_max(got.detach().cpu().double().numpy(), ref.detach().double().numpy())


# ------------------------------------------------------------------------------------------------
# dwconv: N = 2, H = 17 (one row past DW_ROWS), T = 1025 (one frame past DW_FRAMES)
# ------------------------------------------------------------------------------------------------
DW_N, DW_H, DW_T = 2, 17, 1025


@functools.lru_cache(maxsize=None)
def _dw_problem(p, dil):
    """gLN + PReLU prologue, centred taps (left = (P-1)/2 dilations); x holds bf16 values, so the bf16 rows read the same."""
    x = (_rand((DW_N, DW_H, DW_T), 15) + 0.1).bfloat16().float()
    w, b = _rand((DW_H, 1, p), 16), _rand((DW_H,), 17)
    gamma, beta, slope = _rand((DW_H,), 18, 0.5, 1.5), _rand((DW_H,), 19, -0.2, 0.2), torch.tensor([0.3])
    a = O.prelu(O.glob_ln(x.double(), gamma.double(), beta.double()), slope.double())
    ref = O.dilated_conv(a, w.double(), b.double(), dil, (p - 1) // 2 * dil)
    assert ref.shape == x.shape
    return x, w, b, gamma, beta, slope, ref


def _dwconv(H, dev, p, dil, flags=0, xb=False, yb=False, **kw):
    """-> (y, second result of hip.dwconv, the float64 reference); the prologue's tensors live until the synchronize"""
    x, w, b, gamma, beta, slope, ref = _dw_problem(p, dil)
    stats = torch.stack([x.double().sum((1, 2)), (x.double() ** 2).sum((1, 2))], -1).reshape(DW_N, 1, 2).to(dev)
    keep = (stats, gamma.to(dev), beta.to(dev), slope.to(dev))
    pro = H.make_prologue(_abi.PS_NORM_GLOBAL, True, keep[0], DW_H * DW_T, 1e-8, *keep[1:])
    xp = H.pad_rows(x.to(dev))
    with _abi.debug(flags):
        y, second = H.dwconv(xp.bfloat16() if xb else xp, DW_T, w.to(dev), b.to(dev), dil, (p - 1) // 2 * dil, pro,
                             out_dtype=torch.bfloat16 if yb else torch.float32, **kw)
        torch.cuda.synchronize()
    return y, second, ref


def _assert_stats(st, ref):   # (test_dwconv)
    s = st.sum(1).cpu().numpy()
    np.testing.assert_allclose(s[:, 0], ref.sum((1, 2)).numpy(), rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(s[:, 1], (ref ** 2).sum((1, 2)).numpy(), rtol=1e-5)


# fp32 rows: the wave-private kernel, the workgroup kernel's small-halo, large-halo and run-time-taps builds
@pytest.mark.parametrize("p,dil,flags", [(3, 4, 0), (3, 1, 0), (3, 4, WG), (3, 1, WG), (3, 256, 0), (3, 150, 0), (5, 9, 0)])
def test_dwconv_fp32_rows(H, dev, p, dil, flags):
    y, st, ref = _dwconv(H, dev, p, dil, flags, want_stats=True)
    assert _err(y[..., :DW_T], ref) < 1e-5                                     # test_dwconv
    _assert_stats(st, ref)


@pytest.mark.parametrize("dil", [4, 1])
@pytest.mark.parametrize("xb,yb,flags", [(True, True, 0), (True, True, WG), (True, False, 0), (False, True, 0)])
def test_dwconv_bf16_rows_at_every_branch(H, dev, dil, xb, yb, flags):
    """Against the fp32 rows of the wave-private kernel (themselves against float64 above), as test_dwconv_bf16_rows does."""
    y_ref, st_ref, _ = _dwconv(H, dev, 3, dil, want_stats=True)
    y, st, _ = _dwconv(H, dev, 3, dil, flags, xb, yb, want_stats=True)
    assert y.dtype == (torch.bfloat16 if yb else torch.float32)
    if yb:                                                                     # test_dwconv_bf16_rows
        diff = (y[..., :DW_T].float() - y_ref[..., :DW_T].bfloat16().float()).abs()
        assert float(diff.max()) <= 2.0 ** -7 * float(y_ref[..., :DW_T].abs().max())
        assert float((diff > 0).float().mean()) < 1e-2
    else:
        assert torch.allclose(y[..., :DW_T], y_ref[..., :DW_T], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(st.sum(1).cpu().numpy(), st_ref.sum(1).cpu().numpy(), rtol=1e-6)


@pytest.mark.parametrize("dil", [4, 1])
def test_dwconv_amax(H, dev, dil):
    want, _, ref = _dwconv(H, dev, 3, dil)
    got, amax, _ = _dwconv(H, dev, 3, dil, want_amax=True)
    assert _err(got[..., :DW_T], ref) < 1e-5                                   # test_dwconv
    # test_dwconv_leaves_the_maxima_of_its_output
    assert rel_max(got[..., :DW_T].cpu().numpy(), want[..., :DW_T].cpu().numpy()) < 1e-6
    assert amax.shape == (DW_N, _abi.lib().ps_dwconv_stats_parts(DW_H, DW_T))
    assert torch.equal(amax.max(1).values, got[..., :DW_T].abs().amax((1, 2)))


# ------------------------------------------------------------------------------------------------
# encoder: the matrix pipe (32 / 16, C % 32 == 0, T >= 64), free_encode_kernel<32 / 16 / 0>, and C = 4032 / 4033 at N = 1,
# T = 3: 63 / 64 workgroups of 64 channels, i.e. 4 and 64 channels per workgroup
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,length,c,win,hop", [(2, 1040, 32, 32, 16), (2, 1024, 32, 32, 16), (2, 1040, 33, 32, 16),
                                                (2, 600, 24, 16, 8), (2, 211, 9, 20, 6), (1, 64, 4032, 32, 16),
                                                (1, 64, 4033, 32, 16)])
def test_free_encode_at_every_branch(H, dev, n, length, c, win, hop):
    wav, w = _rand((n, length), 1, -0.5, 0.5), _rand((c, 1, win), 2, -0.2, 0.2)
    ref = O.free_encode(wav.double(), w.double(), hop, True)
    feats, t = H.free_encode(wav.to(dev), w.to(dev), hop, True)
    torch.cuda.synchronize()
    assert t == ref.shape[-1] == (length - win) // hop + 1
    assert _err(feats[..., :t], ref) < 1e-5                                    # test_free_encode


# ------------------------------------------------------------------------------------------------
# decoder: free_decode_kernel<32, 16> (T < 64; C % 16 != 0), <16, 8>, the frame kernel (hop = win), the generic one, the
# matrix pipe (C = 2 * DM_UC = 16; T = 64: two whole tiles and an empty one, 65, 97: a partial one) -- and the same three
# through ps_free_decode_moments_f32, with T = 63 as its unfused fallback
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decode_problem(c, t, win, hop):
    feats, mask, w = _rand((2, c, t), 3), _rand((2, c, t), 4), _rand((c, 1, win), 5, -0.3, 0.3)
    ref = O.output_constrain(O.free_decode(feats.double() * O.get_mask(mask.double(), "relu"), w.double(), hop), "linear")
    return feats, mask, w, ref


DECODE = [(16, 63, 32, 16), (17, 64, 32, 16), (16, 70, 16, 8), (16, 5, 64, 64), (9, 33, 20, 6), (16, 64, 32, 16),
          (16, 65, 32, 16), (16, 97, 32, 16)]


@pytest.mark.parametrize("c,t,win,hop", DECODE)
def test_free_decode_at_every_branch(H, dev, c, t, win, hop):
    feats, mask, w, ref = _decode_problem(c, t, win, hop)
    out = H.free_decode(H.pad_rows(feats.to(dev)), t, w.to(dev), hop, H.pad_rows(mask.to(dev)), "relu", "linear")
    torch.cuda.synchronize()
    assert out.shape == ref.shape
    assert _err(out, ref) < 2e-5                                               # test_free_decode


@pytest.mark.parametrize("t", [64, 65, 97, 63])
def test_free_decode_moments_at_every_branch(H, dev, t):
    feats, mask, w, ref = _decode_problem(16, t, 32, 16)
    fp, mp, wd = H.pad_rows(feats.to(dev)), H.pad_rows(mask.to(dev)), w.to(dev)
    assert (_abi.lib().ps_free_decode_moments_parts(2, 16, t, fp.shape[-1], 32, 16) > 0) == (t >= 64)
    score = _rand((2, ref.shape[-1] + 9), 804).to(dev)[:, 5:-7]               # three samples short, rows of a wider buffer
    want = H.free_decode(fp, t, wd, 16, mp, "relu", "linear")
    out, m = H.free_decode_moments(fp, t, wd, 16, score, mp, "relu", "linear")
    torch.cuda.synchronize()
    assert _err(out, ref) < 2e-5                                               # test_free_decode
    assert torch.equal(out, want)                                              # test_decoder_leaves_the_score_moments_behind
    a = want.cpu().double().numpy()
    b = np.concatenate([np.zeros((2, 3)), score.cpu().double().numpy()], -1)
    ref_m = np.stack([a.sum(-1), b.sum(-1), (a * a).sum(-1), (b * b).sum(-1), (a * b).sum(-1)], -1)
    np.testing.assert_allclose(m.cpu().numpy(), ref_m, rtol=1e-11, atol=1e-9)


# ------------------------------------------------------------------------------------------------
# conv2d: a down and an up layer of the presets and two dilated geometries, N = 1, ld = 128, two sources.
# M = 2, 4: conv2d_rows_kernel<2>, <4>; M = 4 with statistics, 33, 65: conv2d_lds_kernel<1>, <2>, <4>;
# M = 32, 64, 65 in fp16x2: conv2d_f16x2_kernel<1>, <2>, <4>
# ------------------------------------------------------------------------------------------------
C2D_F, C2D_T, C2D_C1, C2D_C2 = 11, 100, 3, 2
# (kf, kt, stride_f, dil_f, dil_t, pad_f, pad_t, transposed): PRESET_DOWN[0], PRESET_UP[1] and the two dilated OFF_PRESET
# geometries of test_abi_kernels_gpu.py
C2D_GEOMETRIES = [(5, 2, 2, 1, 1, 2, 1, False), (5, 2, 2, 1, 1, 2, 1, True), (3, 3, 1, 2, 2, 2, 4, False),
                  (3, 2, 2, 2, 3, 1, 3, True)]


@functools.lru_cache(maxsize=None)
def _conv2d_problem(geom, m):
    kf, kt, sf, df, dt, pf, pt, transposed = geom
    f_out = R.conv2d_out_rows(C2D_F, kf, sf, df, pf, transposed)
    x1, x2 = _rand((1, C2D_C1, C2D_F, C2D_T), 81), _rand((1, C2D_C2, C2D_F, C2D_T), 82)
    w2, b = _rand((m, (C2D_C1 + C2D_C2) * kf * kt), 83, -0.3, 0.3), _rand((m,), 84)
    pre = R.conv2d_taps(torch.cat([x1, x2], 1), w2, b, C2D_T, f_out, kf, kt, sf, df, dt, pf, pt, transposed)
    return x1, x2, w2, b, pre, (C2D_T, f_out, kf, kt, sf, df, dt, pf, pt, transposed)


def _conv2d_operands(H, dev, geom, m):
    x1, x2, w2, b, pre, tail = _conv2d_problem(geom, m)
    pad = lambda v: H.pad_rows(v.reshape(1, -1, C2D_T).to(dev)).view(1, v.shape[1], C2D_F, -1)  # noqa: E731
    d1, d2 = pad(x1), pad(x2)
    assert d1.shape[-1] == 128
    return d1, d2, w2.to(dev), b.to(dev), torch.tensor([0.2], device=dev), pre, tail


def _assert_conv2d_stats(stats, pre):   # (test_conv2d_f16x2_kernel)
    tot = stats.sum(dim=1).cpu()
    assert torch.allclose(tot[:, 0], pre.sum(dim=(1, 2, 3)), rtol=1e-5, atol=1e-3 * float(pre.abs().max()))
    assert torch.allclose(tot[:, 1], (pre ** 2).sum(dim=(1, 2, 3)), rtol=1e-5)


@pytest.mark.parametrize("geom", C2D_GEOMETRIES)
@pytest.mark.parametrize("m,stats", [(2, False), (4, False), (4, True), (33, False), (65, True)])
def test_conv2d_fp32_at_every_branch(H, dev, geom, m, stats):
    d1, d2, w2, b, slope, pre, tail = _conv2d_operands(H, dev, geom, m)
    if stats:
        y, st = H.conv2d_stats(d1, d2, H.pack_wt(w2), b, m, *tail)
        ref = pre
    else:
        y, ref = H.conv2d(d1, d2, H.pack_wt(w2), b, m, *tail, "prelu", slope), R.activation(pre, "prelu", 0.2)
    torch.cuda.synchronize()
    assert _err(y[..., :C2D_T], ref) < 2e-5                                    # test_conv2d_implicit_gemm_kernel
    assert float(y[..., C2D_T:].abs().max()) == 0.0
    if stats:
        _assert_conv2d_stats(st, pre)


@pytest.mark.parametrize("geom", C2D_GEOMETRIES)
@pytest.mark.parametrize("m", [32, 64, 65])
def test_conv2d_f16x2_at_every_branch(H, dev, geom, m):
    d1, d2, w2, b, slope, pre, tail = _conv2d_operands(H, dev, geom, m)
    ref = R.activation(pre, "prelu", 0.2)
    img, w_exp = H.pack_conv2d_f16x2(w2)
    y = H.conv2d_f16x2(d1, d2, img, w_exp, b, m, *tail, "prelu", slope)
    y32 = H.conv2d(d1, d2, H.pack_wt(w2), b, m, *tail, "prelu", slope)
    yr, stats = H.conv2d_f16x2(d1, d2, img, w_exp, b, m, *tail, want_stats=True)
    torch.cuda.synchronize()
    e, e32 = _err(y[..., :C2D_T], ref), _err(y32[..., :C2D_T], ref)
    assert e < 5e-6 and e < 4 * e32 + 1e-6                                     # test_conv2d_f16x2_kernel, as are the next three
    assert float(y[..., C2D_T:].abs().max()) == 0.0
    assert _err(yr[..., :C2D_T], pre) < 5e-6
    _assert_conv2d_stats(stats, pre)
