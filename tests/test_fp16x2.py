"""The "fp16x2" arithmetic of the 1x1-conv GEMMs (ps_conv1x1_f16x2_f32): two fp16 terms per operand, three products,
operands brought into fp16's range by powers of two.  The claims under test: its result is as close to an fp64 product
as the exact-fp32 MFMA kernel's at any input scale once the caller hands over the range (a bound behind a norm, the
producer's maxima for raw rows); it fails loudly (inf / NaN), not silently, beyond its range; the partial maxima it
leaves for the next consumer are exact; through the model it meets the reference's golden vector like the fp32 paths."""
import os

import numpy as np
import pytest
import torch

import cases
from conftest import rel_max
from detweights import det_state_dict, det_wave
from oracle import separator_oracle as O


def _rand(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


# ---- host side (no GPU) -----------------------------------------------------------------------------------------------
def test_weight_packer_two_fp16_planes_reconstruct_the_weight():
    from puresound_amd import hip as H
    for scale in (1.0, 3e-5, 700.0):
        w = _rand((300, 40), 5) * scale
        img, w_exp = H.pack_wt_f16x2(w)
        assert img.dtype == torch.float16 and tuple(img.shape) == (2, 3, 2, 256, 16)
        assert 2.0 ** 13 <= float(w.abs().max()) * 2.0 ** w_exp < 2.0 ** 14
        planes = img.float().permute(2, 0, 3, 1, 4).reshape(2, 512, 48)  # [plane][row][k]
        back = (planes[0] + planes[1])[:300, :40] * 2.0 ** -w_exp
        # two 11-bit terms: 2^-22 relative, or the subnormal step 2^-24 / 2^w_exp for the smallest entries
        err = (back - w).abs()
        assert float((err - w.abs() * 2.0 ** -22).max()) <= 2.0 ** -24 * 2.0 ** -w_exp
        assert float(planes[:, 300:].abs().max()) == 0.0 and float(planes[:, :, 40:].abs().max()) == 0.0
    img, w_exp = H.pack_wt_f16x2(torch.zeros(4, 4))
    assert w_exp == 0 and float(img.abs().max()) == 0.0
    with pytest.raises(ValueError):
        H.pack_wt_f16x2(torch.full((2, 2), float("inf")))


def test_fp16x2_blocks_need_a_range_for_their_normalised_values():
    import puresound_amd.nnet.conv_tasnet as CT
    assert CT.GEMM_PLANES["fp16x2"] == 2
    blk = CT.TCN(16, 8, 3, 1, causal=True, tcn_norm="cLN", dconv_norm="cLN").eval()
    blk.gemm_precision = "fp16x2"
    assert blk.gemm_planes_for_plan() == 3  # per-frame norms, run stage by stage -> the three-plane bf16 split
    blk = CT.TCN(16, 8, 3, 1, causal=True, tcn_norm="bN1d", dconv_norm="bN1d").eval()
    blk.gemm_precision = "fp16x2"
    assert blk.gemm_planes_for_plan() == 2  # folded BatchNorm: the producers' measured maxima through its scale / shift
    blk = CT.TCN(16, 8, 3, 1).eval()
    blk.gemm_precision = "fp16x2"
    assert blk.gemm_planes_for_plan() == 2  # global norms: a bound on the normalised values


# ---- device ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    return torch.device("cuda:0")


def _case(n, k, m, t, mode, scale, dev):
    from puresound_amd import _abi, hip as H
    x = (_rand((n, k, t), 121) + 0.2) * scale
    w, b = _rand((m, k), 122, -0.2, 0.2), _rand((m,), 123)
    gamma, beta, slope = _rand((k,), 124, 0.5, 1.5), _rand((k,), 125, -0.2, 0.2), torch.tensor([0.2])
    a, pro, keep, kw = x.double(), None, None, {}
    xd = H.pad_rows(x.to(dev))
    if mode.startswith("norm"):
        a = O.prelu(O.glob_ln(a, gamma.double(), beta.double()), slope.double())
        stats = torch.stack([x.double().sum((1, 2)), (x.double() ** 2).sum((1, 2))], -1).reshape(n, 1, 2).to(dev)
        keep = (stats, gamma.to(dev), beta.to(dev), slope.to(dev))
        pro = H.make_prologue(_abi.PS_NORM_GLOBAL, True, keep[0], k * t, 1e-8, keep[1], keep[2], keep[3])
        kw = dict(x_bound=float(gamma.abs().max()) * (k * t) ** 0.5 + float(beta.abs().max()))
    else:
        kw = dict(x_amax=H.absmax(xd, t))
    ref = torch.matmul(w.double(), a) + b.double().reshape(1, -1, 1)
    res = _rand((n, m, t), 126) if mode == "norm_res" else None
    if res is not None:
        ref = ref + res.double()
    return xd, w, b, pro, keep, kw, res, ref


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 1e-4, 3e3])
@pytest.mark.parametrize("n,k,m,t,mode", [(2, 24, 12, 77, "plain"), (2, 256, 256, 500, "norm_stats"),
                                          (1, 256, 512, 300, "norm_res"), (2, 512, 256, 129, "stats"),
                                          (9, 64, 256, 3800, "norm_stats"), (5, 48, 512, 3700, "norm_res"),
                                          (9, 40, 200, 3800, "plain"),
                                          (8, 512, 256, 3999, "stats"), (8, 256, 512, 3999, "norm_res"),
                                          (8, 256, 256, 3999, "norm_stats")])
def test_fp16x2_gemm_is_as_close_to_fp64_as_the_fp32_kernel(dev, n, k, m, t, mode, scale):
    from puresound_amd import _abi, hip as H
    xd, w, b, pro, keep, kw, res, ref = _case(n, k, m, t, mode, scale, dev)
    want = mode in ("norm_stats", "stats")
    resd = None if res is None else H.pad_rows(res.to(dev))
    y32, _ = H.conv1x1(xd, t, H.pack_wt(w.to(dev)), m, pro, b.to(dev), None, resd, want_stats=want)
    rms = float(ref.pow(2).mean().sqrt())
    e32 = float((y32[..., :t].cpu().double() - ref).pow(2).mean().sqrt()) / rms
    wf, we = H.pack_wt_f16x2(w.to(dev))
    first = None
    # 0 = the persistent interleaved kernel where the launch is large enough, SIMPLE = the one-tile-per-workgroup
    # kernel (256 x 32 tiles for small grids), SIMPLE | WIDE_TILE = its 256 x 128 tile, ANY_SIZE = a persistent kernel
    # at any launch size (where the shape allows one), NO_RB = the interleaved kernel where the default is the
    # register-B kernel (conv1x1_f16x2_rb.inc: K % 32 == 0, M % 256 == 0)
    # NO_PAIR = the persistent grids without their m-tile pairing (workgroups 8 apart, one XCD, share a run of frame tiles).
    # Where the default pairs, on a 256-CU device (conv1x1_bf16.hip, tiles_t = ceil(T / 128), tiles_m = ceil(M / 256),
    # nsuper = ceil(tiles_t / 2) tiles_m N): only (8, 256, 512, 3999) of the shapes above has two m-tiles AND fills the grid --
    #   register-B kernel (flags 0): ntiles = 32 * 2 * 8 = 512 = Gr = 2 x CUs (2 * 256), Gr % (8 tiles_m) = 512 % 16 = 0 -> pair_r = 1
    #     (gp = 256 pairs for 256 frame tiles: one tile per pair, inside PP_MAXU utterances);
    #   interleaved kernel (NO_RB): st_per = 16, nsuper = 16 * 2 * 8 = 256 = G, nsuper % 256 = 0, per = 1 -> pair_r = 16.
    # The other two-m-tile shapes do not pair: (1, 256, 512, 300) has 6 tiles (Gr = 6, G = 4), (5, 48, 512, 3700) has
    # nsuper = 150 = G != 256 and K % 32 != 0 (no register-B kernel).  So no_pair / no_rb | no_pair change the numbering at
    # that one shape and are the defaults again elsewhere; placement only -- the same bits are expected, the bound is the loop's.
    simple, wide, any_size, no_rb, no_pair = (_abi.PS_DBG_GEMM_SIMPLE, _abi.PS_DBG_GEMM_WIDE_TILE, _abi.PS_DBG_GEMM_ANY_SIZE,
                                              _abi.PS_DBG_GEMM_NO_RB, _abi.PS_DBG_GEMM_NO_PAIR)
    for flags in (0, simple, simple | wide, any_size, no_rb, no_rb | any_size, no_pair, no_rb | no_pair):
        with _abi.debug(flags):
            y, st, am = H.conv1x1_f16x2(xd, t, wf, we, m, pro, b.to(dev), None, resd, want_stats=want, want_amax=True,
                                        **kw)
            torch.cuda.synchronize()
        got = y[..., :t].cpu().double()
        assert torch.isfinite(got).all()
        err = float((got - ref).pow(2).mean().sqrt()) / rms
        assert err < 1.5 * e32 + 1e-8, (flags, err, e32)  # rms error: the fp32 kernel's (accumulation rounding) class
        assert rel_max(got.numpy(), ref.numpy()) < 4e-6, flags
        if first is None:
            first = got
        else:
            assert rel_max(got.numpy(), first.numpy()) < 2e-6, flags
        # the maxima handed to the next consumer are exact
        assert torch.equal(am.amax(1).cpu(), y[..., :t].abs().amax((1, 2)).cpu()), flags
        if want:
            s = st.sum(1).cpu().numpy()
            np.testing.assert_allclose(s[:, 0], got.sum((1, 2)).numpy(), rtol=1e-6, atol=1e-3 * max(scale, 1.0))
            np.testing.assert_allclose(s[:, 1], (got * got).sum((1, 2)).numpy(), rtol=1e-5)


def _small_case(mode, m, dev, rows16=False):
    """N = 2, K = 64 (four K-steps: the persistent kernels' minimum; a multiple of 32 for the register-B kernel), T = 129
    (two frame tiles, the second one partial); mode: "plain" / "stats" / "res", "affine" in front for a scale / shift +
    PReLU prologue.  -> operands, the range to hand over, the fp64 result and sum_k |w| |f(x)| per output"""
    from puresound_amd import _abi, hip as H
    n, k, t = 2, 64, 129
    x = _rand((n, k, t), 141) + 0.2
    res = _rand((n, m, t), 146) if mode.endswith("res") else None
    if rows16:
        x, res = x.bfloat16().float(), None if res is None else res.bfloat16().float()
    w, b = _rand((m, k), 142, -0.2, 0.2), _rand((m,), 143)
    gamma, beta, slope = _rand((k,), 144, 0.5, 1.5), _rand((k,), 145, -0.2, 0.2), torch.tensor([0.2])
    a, pro, keep = x.double(), None, None
    bound = float(x.abs().max())
    if mode.startswith("affine"):
        a = O.prelu(gamma.double().reshape(1, -1, 1) * a + beta.double().reshape(1, -1, 1), slope.double())
        keep = (gamma.to(dev), beta.to(dev), slope.to(dev))
        pro = H.make_prologue(_abi.PS_NORM_AFFINE, True, None, 0.0, 0.0, keep[0], keep[1], keep[2])
        bound = float(gamma.abs().max()) * bound + float(beta.abs().max())
    ref = torch.matmul(w.double(), a) + b.double().reshape(1, -1, 1)
    if res is not None:
        ref = ref + res.double()
    return x, w, b, pro, keep, res, bound, ref, torch.matmul(w.double().abs(), a.abs()), t


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["res", "affine"])
@pytest.mark.parametrize("kernel", ["narrow", "wide", "il", "rb"])
def test_fp16x2_variants_the_large_shapes_leave_out(dev, kernel, mode):
    """The shapes above reach (prologue, statistics, residual) = (0,0,0), (0,1,0), (1,1,0), (1,0,1) on the one-tile,
    the interleaved and the register-B kernel.  Here the other two -- a residual without a prologue (two m-tiles) and a
    prologue alone -- on each of them and both tiles of the first, forced at a small size: SIMPLE (256 x 32 tiles while
    2 * tiles <= CUs; with WIDE_TILE 256 x 128), ANY_SIZE (register-B: K % 32 == 0, M % 256 == 0), ANY_SIZE | NO_RB
    (interleaved).  Same bounds as there."""
    from puresound_amd import _abi, hip as H
    flags = {"narrow": _abi.PS_DBG_GEMM_SIMPLE, "wide": _abi.PS_DBG_GEMM_SIMPLE | _abi.PS_DBG_GEMM_WIDE_TILE,
             "il": _abi.PS_DBG_GEMM_ANY_SIZE | _abi.PS_DBG_GEMM_NO_RB, "rb": _abi.PS_DBG_GEMM_ANY_SIZE}[kernel]
    m = 512 if mode == "res" else 256
    x, w, b, pro, keep, res, bound, ref, _, t = _small_case(mode, m, dev)
    xd = H.pad_rows(x.to(dev))
    resd = None if res is None else H.pad_rows(res.to(dev))
    y32, _ = H.conv1x1(xd, t, H.pack_wt(w.to(dev)), m, pro, b.to(dev), None, resd)
    rms = float(ref.pow(2).mean().sqrt())
    e32 = float((y32[..., :t].cpu().double() - ref).pow(2).mean().sqrt()) / rms
    wf, we = H.pack_wt_f16x2(w.to(dev))
    with _abi.debug(flags):
        y, _, am = H.conv1x1_f16x2(xd, t, wf, we, m, pro, b.to(dev), None, resd, want_amax=True, x_bound=bound)
        torch.cuda.synchronize()
    got = y[..., :t].cpu().double()
    assert torch.isfinite(got).all()
    err = float((got - ref).pow(2).mean().sqrt()) / rms
    assert err < 1.5 * e32 + 1e-8, (err, e32)
    assert rel_max(got.numpy(), ref.numpy()) < 4e-6
    assert torch.equal(am.amax(1).cpu(), y[..., :t].abs().amax((1, 2)).cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("res_inside", [False, True])
def test_gemm_with_layernorm_epilogue_behind_a_prologue(dev, res_inside):
    """ps_conv1x1_f16x2_ln_f32 with a scale / shift + PReLU prologue (the register-B kernel's TR = 1 LayerNorm variant;
    test_gemm_with_layernorm_epilogue runs the TR = 0 one) against fp64, at that test's bound."""
    import torch.nn.functional as F
    from puresound_amd import _abi, hip as H
    c = 128
    x, w, b, pro, keep, res, bound, p, _, t = _small_case("affine_res", c, dev)
    g, be = _rand((c,), 147, 0.5, 1.5), _rand((c,), 148, -0.3, 0.3)
    p = p - res.double()   # W f(x) + b
    ln = lambda v: F.layer_norm(v.transpose(1, 2), (c,), g.double(), be.double(), 1e-5).transpose(1, 2)
    ref = ln(p + res.double()) if res_inside else res.double() + ln(p)
    w256 = torch.zeros(256, w.shape[1])
    w256[:c] = w
    wf, we = H.pack_wt_f16x2(w256.to(dev))
    with _abi.debug(_abi.PS_DBG_GEMM_ANY_SIZE):
        assert H.conv1x1_f16x2_ln_ok(2, w.shape[1], c, t)
        y = H.conv1x1_f16x2_ln(H.pad_rows(x.to(dev)), t, wf, we, c, b.to(dev), g.to(dev), be.to(dev), 1e-5,
                               H.pad_rows(res.to(dev)), x_bound=bound, pro=pro, res_inside=res_inside)
        torch.cuda.synchronize()
    assert rel_max(y[..., :t].cpu().numpy(), ref.numpy()) < 5e-6


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "stats", "res", "affine", "affine_stats", "affine_res"])
def test_f16_rows_gemm_in_every_variant(dev, mode):
    """ps_conv1x1_f16_rows (bf16 rows, one fp16 term per operand, the register-B kernel) called directly in all six
    (prologue, statistics, residual) variants; the masker reaches three of them (ps_conv_tasnet_bf16_rows).  Against the
    fp64 product of the same bf16 rows at the bounds of test_bf16_gemm_with_bf16_residual_and_output_rows (one bf16
    rounding of the result).  The statistics are those of the fp32 values before that rounding: every output is within
    E = 1.01 * 2^-10 sum_k |w| |f(x)| of the fp64 one (2^-11 per fp16 operand; 1 % for their cross term and the fp32
    accumulation), so the sums are within sum E and sum (2 |y| E + E^2)."""
    import ctypes as C
    from puresound_amd import _abi, hip as H
    m = 512 if mode.endswith("res") else 256
    x, w, b, pro, keep, res, bound, ref, absprod, t = _small_case(mode, m, dev, rows16=True)
    n, k = x.shape[:2]
    xd = H.pad_rows(x.to(dev)).bfloat16()
    rd = None if res is None else H.pad_rows(res.to(dev)).bfloat16()
    wf, we = H.pack_wt_f16x2(w.to(dev))
    y = torch.empty(n, m, xd.shape[-1], dtype=torch.bfloat16, device=dev)
    bd = b.to(dev)
    st = torch.zeros(n, _abi.lib().ps_conv1x1_stats_parts(m, t), 2, dtype=torch.float64, device=dev) if mode.endswith("stats") else None
    rng = _abi.F16x2Range(int(we), bound, None, 0, None)
    with _abi.debug(_abi.PS_DBG_GEMM_ANY_SIZE):
        assert _abi.lib().ps_conv1x1_f16_rows_ok(n, k, m, t)
        _abi.check(_abi.lib().ps_conv1x1_f16_rows(_abi.ptr(xd), _abi.ptr(wf), C.byref(rng), _abi.ptr(y), n, k, m, t, xd.shape[-1],
                                                  C.byref(pro) if pro is not None else None, _abi.ptr(bd), None, _abi.ptr(rd),
                                                  _abi.ptr(st), _abi.stream_ptr(dev)), "ps_conv1x1_f16_rows")
        torch.cuda.synchronize()
    got = y[..., :t].float().cpu().double()
    assert torch.isfinite(got).all()
    assert float(np.linalg.norm(got.numpy() - ref.numpy()) / np.linalg.norm(ref.numpy())) < 6e-3
    assert rel_max(got.numpy(), ref.numpy()) < 2e-2
    if st is not None:
        s, e = st.sum(1).cpu().numpy(), absprod * (1.01 * 2.0 ** -10)
        assert (np.abs(s[:, 0] - ref.sum((1, 2)).numpy()) <= e.sum((1, 2)).numpy()).all()
        assert (np.abs(s[:, 1] - (ref ** 2).sum((1, 2)).numpy()) <= (2 * ref.abs() * e + e * e).sum((1, 2)).numpy()).all()


@pytest.mark.gpu
def test_fp16x2_default_range_and_its_loud_failure(dev):
    """Without a range from the caller the kernel scales raw rows by 2^-4: fine around unit scale, coarser for tiny
    inputs (absolute resolution 2^-21), and inf / NaN -- never a silently wrong number -- beyond 1e6."""
    from puresound_amd import hip as H
    n, k, m, t = 2, 64, 32, 300
    w, b = _rand((m, k), 1, -0.2, 0.2).to(dev), _rand((m,), 2).to(dev)
    wf, we = H.pack_wt_f16x2(w)
    for scale, tol in ((1.0, 2e-6), (1e-3, 2e-3)):
        x = _rand((n, k, t), 3) * scale
        ref = torch.matmul(w.cpu().double(), x.double())
        y, _, _ = H.conv1x1_f16x2(H.pad_rows(x.to(dev)), t, wf, we, m, None, None)
        assert rel_max(y[..., :t].cpu().double().numpy(), ref.numpy()) < tol
        ya, _, _ = H.conv1x1_f16x2(H.pad_rows(x.to(dev)), t, wf, we, m, None, None, x_amax=H.absmax(H.pad_rows(x.to(dev)), t))
        assert rel_max(ya[..., :t].cpu().double().numpy(), ref.numpy()) < 2e-6
    x = _rand((n, k, t), 4) * 1e7
    y, _, _ = H.conv1x1_f16x2(H.pad_rows(x.to(dev)), t, wf, we, m, None, b)
    assert not torch.isfinite(y[..., :t]).all()
    ya, _, _ = H.conv1x1_f16x2(H.pad_rows(x.to(dev)), t, wf, we, m, None, b, x_amax=H.absmax(H.pad_rows(x.to(dev)), t))
    ref = torch.matmul(w.cpu().double(), x.double()) + b.cpu().double().reshape(1, -1, 1)
    assert rel_max(ya[..., :t].cpu().double().numpy(), ref.numpy()) < 2e-6
    # an all-zero utterance next to a loud one: per-utterance ranges
    x = _rand((n, k, t), 5)
    x[0] = 0.0
    xd = H.pad_rows(x.to(dev))
    ya, _, am = H.conv1x1_f16x2(xd, t, wf, we, m, None, b, x_amax=H.absmax(xd, t), want_amax=True)
    assert torch.equal(ya[0, :, :t].cpu(), b.cpu().reshape(-1, 1).expand(m, t))
    assert float(H.absmax(xd, t)[0].max()) == 0.0


@pytest.mark.gpu
def test_fp16x2_meets_the_reference_like_the_fp32_paths(dev, golden_dir):
    import puresound_amd.nnet as PA
    name = "cfg2_full"
    c = cases.CASES[name]
    g = dict(np.load(os.path.join(golden_dir, f"{name}.npz")))
    model = cases.build(PA.NS, name).eval()
    model.load_state_dict(det_state_dict(model))
    model.to(dev)
    x = det_wave(c["seed"], c["B"], c["L"]).to(dev)
    errs = {}
    for prec in ("fp32", "fp16x2"):
        model.masker.set_gemm_precision(prec)
        feats, t = model.encoder.encode_padded(x)
        mask = model.masker.forward_padded(feats, t)
        pre = model.encoder.decode_padded(feats, t, mask, "relu", "none").cpu().numpy()
        errs[prec] = rel_max(pre, g["wav_preclamp"])
        assert rel_max(model.inference(x).cpu().numpy(), g["wav"]) < 1e-4
    assert errs["fp16x2"] < 1e-5 and errs["fp16x2"] < 2 * errs["fp32"], errs
    # the benchmark's batch (the persistent kernels, the range chain across 24 blocks): against the exact-fp32 run
    xb = det_wave(7, 32, 64000).to(dev)
    model.masker.set_gemm_precision("fp32")
    ref = model.inference(xb)
    model.masker.set_gemm_precision("fp16x2")
    y = model.inference(xb)
    assert torch.isfinite(y).all()
    assert float((y - ref).abs().max()) < 5e-5 and float((y - ref).norm() / ref.norm()) < 1e-5
    # a row does not depend on its neighbours: every range is per utterance
    y1 = model.inference(xb[5:6])
    assert float((y1 - y[5:6]).abs().max()) < 2e-5
    # an utterance 1e3 times quieter goes through the same arithmetic at its own range
    yq = model.inference(xb[:2] * 1e-3)
    model.masker.set_gemm_precision("fp32")
    rq = model.inference(xb[:2] * 1e-3)
    assert float((yq - rq).norm() / rq.norm()) < 1e-5


@pytest.mark.gpu
def test_fp16x2_inside_a_captured_graph(dev):
    import puresound_amd.nnet as PA
    from puresound_amd.graphs import GraphedInference
    model = cases.build(PA.NS, "cfg2_full").eval()
    model.load_state_dict(det_state_dict(model))
    model.to(dev)
    model.masker.set_gemm_precision("fp16x2")
    x = det_wave(3, 1, 16000).to(dev)
    eager = model.inference(x)
    graphed = GraphedInference(model)
    assert torch.equal(graphed(x), eager)
    x2 = det_wave(4, 1, 16000).to(dev) * 0.01  # another range through the same graph
    assert torch.equal(graphed(x2), model.inference(x2))


@pytest.mark.gpu
def test_input_range_may_be_a_loose_bound(dev):
    """ps_conv_tasnet_ranged_f32: the range of the first block's input may be any upper bound (the wrapper passes
    max |wav| x the largest row sum of the encoder's |w|); a bound 16 x too loose costs four bits of headroom, not
    accuracy, and the measured maxima (no range given: one ps_absmax_f32 pass) give the same result to rounding."""
    import puresound_amd.nnet as PA
    from puresound_amd import hip as H
    model = cases.build(PA.NS, "cfg2_full").eval()
    model.load_state_dict(det_state_dict(model))
    model.to(dev)
    x = det_wave(9, 3, 16000).to(dev)
    x[1] *= 1e-3
    feats, t = model.encoder.encode_padded(x)
    bound = model.encoder.feature_bound(x)
    true_max = feats[..., :t].abs().amax((1, 2))
    assert bound.shape[0] == 3 and bound.dim() == 2   # [N, parts] partial bounds
    assert (bound.amax(1) >= true_max).all() and (bound.amax(1) < 64 * true_max).all()
    model.masker.set_gemm_precision("fp32")
    ref = model.masker.forward_padded(feats, t)[..., :t]
    model.masker.set_gemm_precision("fp16x2")
    outs = [model.masker.forward_padded(feats, t, x_amax=r)[..., :t] for r in (None, bound, bound * 16.0, H.absmax(feats, t))]
    for o in outs:
        assert float((o - ref).norm() / ref.norm()) < 5e-6
    with pytest.raises(ValueError):
        model.masker.forward_padded(feats, t, x_amax=bound[:2])


@pytest.mark.gpu
def test_fp16x2_on_degenerate_inputs(dev):
    """Silence, near-silence, an impulse, a full-scale square wave and a batch mixing them: the ranges are per utterance
    and an all-zero utterance must not turn into 0 * inf; against the exact-fp32 path."""
    import puresound_amd.nnet as PA
    model = cases.build(PA.NS, "cfg2_full").eval()
    model.load_state_dict(det_state_dict(model))
    model.to(dev)
    n, length = 5, 8000
    x = torch.zeros(n, length)
    x[1] = det_wave(21, 1, length)[0] * 1e-7
    x[2, 4000] = 0.9
    x[3] = torch.sign(torch.sin(torch.arange(length) * 0.05)) * 0.99
    x[4] = det_wave(22, 1, length)[0]
    x = x.to(dev)
    model.masker.set_gemm_precision("fp32")
    ref = model.inference(x)
    model.masker.set_gemm_precision("fp16x2")
    y = model.inference(x)
    assert torch.isfinite(y).all()
    for i in range(n):
        scale = float(ref[i].abs().max())
        err = float((y[i] - ref[i]).abs().max())
        assert err <= 2e-5 * max(scale, 1e-30) + 1e-12, (i, err, scale)
