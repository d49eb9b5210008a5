"""One NaN or infinity in a live input sample, on the HIP path, against the masks of the reference
(tests/golden/nonfinite_masks.json) and the values of the fp64 oracle, which tests/test_nonfinite.py pins to those masks.

The contract ("Non-finite input"):
  a. a row the bad sample does not reach is bit-identical to the same row of the clean batch, in every arithmetic;
  b. exact fp32: the isnan and isinf masks are the reference's, the finite elements within the case's parity tolerance;
  c. an arithmetic that scales by a range (fp16x2, the default): the NaN mask is a superset of the reference's and no
     element is a finite number where the reference has none or a wrong one; the mask is strictly wider exactly for the
     (case, scenario) pairs of WIDENED below;
  d. probe_lookahead_receptive_field() gives the reference's two numbers for every preset (tests/golden/lookahead.json);
  e. the range-carrying entries called directly: one bad row next to a clean one.
Tolerances are those of the cases' own parity tests (1e-4, nonfinite_cases.TOL) and of tests/test_fp16x2.py (4e-6)."""
import numpy as np
import pytest
import torch

import abi_refs as R
import cases
import nonfinite_cases as NF
from conftest import rel_max
from oracle import separator_oracle as O
from puresound_amd import _abi

pytestmark = pytest.mark.gpu

PAIRS = [(n, s) for n in NF.CASES for s in NF.scenarios(n)]
TRIPLES = [(n, s, p) for n in NF.CASES for p in NF.precisions(n) for s in NF.scenarios(n)]
_ID = lambda v: "default" if v is None else str(v)  # noqa: E731


def _partial(name, sc):
    """the reference leaves part of the bad row(s) finite: there is something a whole-utterance NaN can widen"""
    nan, _ = NF.golden_masks(name, sc)
    which, row, _, _ = NF.scenarios(name)[sc]
    return not nan[row].all()


# (c) The pairs whose default-arithmetic NaN mask is strictly wider than the reference's, from the range rules:
#  1. A Conv-TasNet masker behind a FreeEncDec takes the features' range from the encoder without a pass over them:
#     max |wav[n]| x the largest row sum of |w| (FreeEncDec.feature_bound, SoTaskWrapModule._masker_padded).  Any NaN or
#     infinity in the noisy row -- also one in the tail samples that no frame covers -- makes that bound non-finite, and
#     f16_scales returns the utterance NaN as a whole.  That is wider than the reference wherever the reference leaves
#     part of the row finite: the causal presets (the non-causal ones lose the whole row in the reference too, through
#     the global norms).  Every Conv-TasNet GEMM of these cases is an fp16x2 launch, the 24- / 12-channel ones of the
#     tiny cases included (ps_conv1x1_f16x2_f32 takes any K and M).
#  2. Every other range of a preset is measured from values (ps_absmax_f32, the y_amax epilogues, the conv2d kernel's
#     own chunk maxima) with fmaxf, which skips a NaN: the finite values keep their range and a NaN carries itself, so a
#     NaN sample widens nothing.  An INFINITY in such a range blanks the utterance (conv1x1) or the wave's 32 frames
#     (conv2d), so it matters whether an infinite value -- not a NaN -- reaches a ranged launch:
#     a. DPRNN (cfg4): the first launch is the intra-LSTM's input projection on the raw encoder features (an infinite
#        sample gives infinite features, w * inf), its range ps_absmax_f32 of them: the utterance is lost.  The same for
#        the enrolment features of the embedding-free preset, whose pass seeds every block's inter-LSTM state.
#     b. SkiM: the first launch on the features is a FiLM with an input LayerNorm (exact fp32), which makes a frame that
#        holds an infinity NaN (inf - inf) before any range is taken: nothing is widened.
#     c. The 2-D presets (Unet, UnetTcn, DPCRN, DPARN behind the conv-STFT): the spectrum of the frames that cover the
#        sample is +-inf, the first convolution (K = 10: the fp32 kernel), the folded BatchNorm and the PReLU keep an
#        infinity wherever the infinities under a window weigh in with one sign, and from the second layer on the
#        convolutions are fp16x2 launches that measure their range per wave: 32 frames, which is every frame of these
#        fixtures (L = 4000, hop 128).  The utterance is lost.
#     d. STFT + Conv-TasNet (cfg1, tiny_stft*): non-causal gLN, the reference loses the whole row as well.
#  3. The enrolment's +inf reaches the other maskers as an embedding that is NaN in the reference too: the whole row is
#     lost there as well.
def _covered(name, sc):
    """the bad sample lies under a frame of the FreeEncDec (the tail that no frame reaches does not count in its bound)"""
    c = cases.CASES[name]
    _, _, at, _ = NF.scenarios(name)[sc]
    return at < (c["L"] - c["enc"]["win"]) // c["enc"]["hop"] * c["enc"]["hop"] + c["enc"]["win"]


def _widened():
    out = set()
    for name in NF.CASES:
        c = cases.CASES[name]
        cls = c["masker"].get("cls", "ConvTasNet")
        for sc, (which, _, _, v) in NF.scenarios(name).items():
            inf = v in (float("inf"), float("-inf"))
            if cls == "ConvTasNet" and c["enc"]["kind"] == "free":
                hit = which == "noisy" and _covered(name, sc)                                         # rule 1
            elif cls == "DPRNN":
                hit = inf and (which == "noisy" or c["masker"]["kw"].get("embedding_free_tse", False))  # rule 2a
            elif cls in ("Unet", "UnetTcn", "DPCRN", "DPARN"):
                hit = inf and which == "noisy"                                                          # rule 2c
            else:
                hit = False                                                                             # rules 2b, 2d
            if hit and _partial(name, sc):
                out.add((name, sc))
    return out


WIDENED = _widened()


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
    junk = [torch.full((1 << 22,), float("nan"), device=dev) for _ in range(8)]
    del junk
    yield


class _Runs:
    """HIP outputs per (case, arithmetic, scenario), computed once; one model on the device at a time."""

    def __init__(self, dev):
        self.dev, self.key, self.model, self.out = dev, None, None, {}

    def __call__(self, name, prec, sc):
        k = (name, prec, sc)
        if k not in self.out:
            if self.key != (name, prec):
                self.model = None
                self.model = NF.hip_model(name, self.dev)
                if prec is not None:
                    self.model.set_gemm_precision(prec)
                self.key = (name, prec)
            self.out[k] = NF.hip_out(self.model, name, sc, self.dev)
        return self.out[k]


@pytest.fixture(scope="module")
def run(dev):
    return _Runs(dev)


def _bad_rows(name, sc):
    nan, inf = NF.golden_masks(name, sc)
    return (nan | inf).any(axis=1)


@pytest.mark.parametrize("name,sc,prec", TRIPLES, ids=_ID)
def test_rows_the_bad_sample_does_not_reach_are_bit_identical(run, name, sc, prec):
    """(a) same shapes, launches and dispatch as the clean batch, and every statistic and range is per utterance."""
    clean = ~_bad_rows(name, sc)
    got, ref = run(name, prec, sc), run(name, prec, None)
    assert np.array_equal(got[clean], ref[clean])
    assert np.isfinite(ref).all()


@pytest.mark.parametrize("name,sc", PAIRS)
def test_exact_fp32_has_the_reference_masks_and_values(run, name, sc):
    """(b) set_gemm_precision("fp32"): no range to blame."""
    nan, inf = NF.golden_masks(name, sc)
    got, want = run(name, "fp32", sc), NF.oracle_out(name, sc)
    err, den = NF.finite_error(name, got, want)
    print(f"{name} {sc} fp32: NaN {int(np.isnan(got).sum())} (reference {int(nan.sum())}), inf {int(np.isinf(got).sum())}, "
          f"finite error {err / den:.3e}")
    assert NF.runs(np.isnan(got)) == NF.runs(nan)
    assert NF.runs(np.isinf(got)) == NF.runs(inf)
    assert err / den < NF.TOL


def _ranged_check(name, got, want, nan):
    """the shared check of (c): `got` fp32 HIP output, `want` the oracle's, `nan` the reference's NaN mask"""
    fin = np.isfinite(got)
    assert np.isfinite(want[fin]).all()          # no finite number where the reference has none
    err, den = NF.finite_error(name, got, want)
    assert err / den < NF.TOL                    # and no wrong one
    assert np.isnan(got[nan]).all()              # a NaN stays a NaN
    assert np.isnan(got[np.isnan(want)]).all()
    return err / den


@pytest.mark.parametrize("name,sc,prec", [t for t in TRIPLES if t[2] != "fp32"], ids=_ID)
def test_ranged_arithmetic_never_returns_a_wrong_finite_number(run, name, sc, prec):
    """(c) the default arithmetic (fp16x2 wherever a module has the choice), and the three-term bf16 split, which has no
    range but turns an infinity into NaN in its second term."""
    nan, _ = NF.golden_masks(name, sc)
    got = run(name, prec, sc)
    e = _ranged_check(name, got, NF.oracle_out(name, sc), nan)
    print(f"{name} {sc} {prec or 'default'}: NaN {int(np.isnan(got).sum())} (reference {int(nan.sum())}), finite error {e:.3e}")


@pytest.mark.parametrize("prec", [None, "bf16x3"], ids=_ID)
def test_the_widened_masks_are_the_ones_the_range_rules_give(run, prec):
    wider = set()
    for name, sc in PAIRS:
        if prec not in NF.precisions(name):
            continue
        nan, _ = NF.golden_masks(name, sc)
        got = np.isnan(run(name, prec, sc))
        assert got[nan].all(), (name, sc)
        if (got & ~nan).any():
            wider.add((name, sc))
    # bf16x3 scales by nothing: it may not widen anything
    assert wider == (WIDENED if prec is None else set())


@pytest.mark.parametrize("name", NF.PRESETS)
def test_probe_gives_the_reference_numbers(dev, name):
    """(d) at the default arithmetic and after set_gemm_precision("fp32"); the probe runs in exact fp32 either way and
    leaves every module's setting as it found it."""
    want = tuple(NF.golden()[1][name])
    model = NF.hip_model(name, dev)
    before = {id(m): m.__dict__.get("gemm_precision") for m in model.modules()}
    assert model.probe_lookahead_receptive_field() == want
    assert {id(m): m.__dict__.get("gemm_precision") for m in model.modules()} == before
    model.set_gemm_precision("fp32")
    assert model.probe_lookahead_receptive_field() == want
    assert all(m.gemm_precision == "fp32" for m in model.modules() if hasattr(m, "gemm_precision"))


# ------------------------------------------------------------------------------------------------------------------------
# (e) the range-carrying entries on their own: N = 2, row 1 holds one +inf or one NaN, row 0 is clean
# ------------------------------------------------------------------------------------------------------------------------
BAD = [float("inf"), float("nan")]
GEMM_FLAGS = {"default": 0, "simple": _abi.PS_DBG_GEMM_SIMPLE, "simple_wide": _abi.PS_DBG_GEMM_SIMPLE | _abi.PS_DBG_GEMM_WIDE_TILE,
              "any_size": _abi.PS_DBG_GEMM_ANY_SIZE, "any_size_no_rb": _abi.PS_DBG_GEMM_ANY_SIZE | _abi.PS_DBG_GEMM_NO_RB}


def _bad_row_check(got, ref, tol, exact_masks=False):
    """Every element of the bad row is within `tol` of the fp64 one (relative to its largest finite element), or non-finite
    where fp64 is non-finite, or NaN; a NaN of fp64 is a NaN.  exact_masks (an exact-fp32 entry): the masks are fp64's."""
    got, ref = got.double(), ref.double()
    den = float(ref[torch.isfinite(ref)].abs().max()) if torch.isfinite(ref).any() else 1.0
    both = torch.isfinite(got) & torch.isfinite(ref)
    close = torch.zeros_like(both)
    close[both] = (got[both] - ref[both]).abs() <= tol * den
    ok = torch.isnan(got) | (~torch.isfinite(got) & ~torch.isfinite(ref)) | close
    assert bool(ok.all()), f"{int((~ok).sum())} finite elements are wrong or stand where fp64 has no number"
    assert bool(torch.isnan(got[torch.isnan(ref)]).all())
    if exact_masks:
        assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(torch.isinf(got), torch.isinf(ref))


def _amax_hides_nothing(am_row, y_row):
    """The maxima a launch hands to the next fp16x2 GEMM: an infinity in y makes them infinite (the consumer then returns
    the utterance NaN), and they cover every finite |y| (a NaN in y needs no range: it carries itself)."""
    am = float(am_row.max()) if not bool(torch.isnan(am_row).any()) else float("nan")
    if bool(torch.isinf(y_row).any()):
        assert not am < float("inf")
    fin = torch.isfinite(y_row)
    if bool(fin.any()):
        assert not am < float(y_row[fin].abs().max())


def _small(mode, m, dev):
    from test_fp16x2 import _small_case
    return _small_case(mode, m, dev)


@pytest.mark.parametrize("flags", list(GEMM_FLAGS), ids=str)
@pytest.mark.parametrize("bad", BAD, ids=str)
def test_conv1x1_f16x2_with_measured_maxima(H, dev, bad, flags):
    """x_amax = ps_absmax_f32 of the rows: an infinity makes the range infinite and the row NaN as a whole; a NaN is skipped
    by the maxima, the finite values keep their range and the NaN takes its own frame."""
    m = 256
    x, w, b, _, _, _, _, ref, _, t = _small("plain", m, dev)
    xb = x.clone()
    xb[1, 17, 70] = bad
    refb = torch.matmul(w.double(), xb.double()) + b.double().reshape(1, -1, 1)
    wf, we = H.pack_wt_f16x2(w.to(dev))
    with _abi.debug(GEMM_FLAGS[flags]):
        xd, xbd = H.pad_rows(x.to(dev)), H.pad_rows(xb.to(dev))
        y, _, _ = H.conv1x1_f16x2(xd, t, wf, we, m, None, b.to(dev), want_amax=True, x_amax=H.absmax(xd, t))
        yb, _, am = H.conv1x1_f16x2(xbd, t, wf, we, m, None, b.to(dev), want_amax=True, x_amax=H.absmax(xbd, t))
        torch.cuda.synchronize()
    assert rel_max(y[..., :t].cpu().double().numpy(), ref.numpy()) < 4e-6
    assert torch.equal(yb[0, :, :t], y[0, :, :t])
    got = yb[1, :, :t].cpu()
    _bad_row_check(got, refb[1], 4e-6)
    _amax_hides_nothing(am[1].cpu(), got)
    if bad != bad:  # the NaN: one frame is lost, not the row
        assert bool(torch.isfinite(got[:, :70]).all()) and bool(torch.isfinite(got[:, 71:]).all())
    else:
        assert bool(torch.isnan(got).all())


@pytest.mark.parametrize("flags", list(GEMM_FLAGS), ids=str)
def test_conv1x1_f16x2_with_an_infinite_bound(H, dev, flags):
    """x_bound = inf.  A bound is one number per launch (it comes from weights: max |gamma| sqrt(count) + max |beta|), so an
    infinite one says nothing about any row: the launch comes back NaN, every row of it, for clean rows as for bad ones --
    not scaled by a power of two picked from the bits of an infinity."""
    m = 256
    x, w, b, _, _, _, _, _, _, t = _small("plain", m, dev)
    xb = x.clone()
    xb[1, 17, 70] = float("inf")
    wf, we = H.pack_wt_f16x2(w.to(dev))
    with _abi.debug(GEMM_FLAGS[flags]):
        for v in (x, xb):
            y, _, am = H.conv1x1_f16x2(H.pad_rows(v.to(dev)), t, wf, we, m, None, b.to(dev), want_amax=True,
                                       x_bound=float("inf"))
            torch.cuda.synchronize()
            assert bool(torch.isnan(y[..., :t]).all())


@pytest.mark.parametrize("kernel", ["fp32", "f16x2_default", "f16x2_any_size", "f16x2_any_size_no_rb", "bf16x3"])
def test_global_norm_prologue_of_an_utterance_that_holds_an_infinity(H, dev, kernel):
    """PS_NORM_GLOBAL with the statistics of a row that holds +inf: sum = sum of squares = inf, the variance is inf - inf.
    O.glob_ln in fp64 (and torch) give NaN for the whole row.  Channel 0's weights are all positive, so that a kernel that
    normalised with mean = inf and a finite rstd would give -inf there, not a NaN by cancellation."""
    n, k, m, t = 2, 64, 256, 129
    x = R.rand((n, k, t), 901) + 0.2
    w, b = R.rand((m, k), 902, -0.2, 0.2), R.rand((m,), 903)
    w[0] = w[0].abs() + 0.01
    gamma, beta, slope = R.rand((k,), 904, 0.5, 1.5), R.rand((k,), 905, -0.2, 0.2), torch.tensor([0.2])
    xb = x.clone()
    xb[1, 17, 70] = float("inf")

    def call(v):
        stats = torch.stack([v.double().sum((1, 2)), (v.double() ** 2).sum((1, 2))], -1).reshape(n, 1, 2).to(dev)
        keep = (stats, gamma.to(dev), beta.to(dev), slope.to(dev))
        pro = H.make_prologue(_abi.PS_NORM_GLOBAL, True, stats, k * t, 1e-8, keep[1], keep[2], keep[3])
        vd = H.pad_rows(v.to(dev))
        if kernel == "fp32":
            y, _ = H.conv1x1(vd, t, H.pack_wt(w.to(dev)), m, pro, b.to(dev))
        elif kernel == "bf16x3":
            y, _ = H.conv1x1_bf16(vd, t, H.pack_wt_bf16(w.to(dev), 3), m, pro, b.to(dev))
        else:
            wf, we = H.pack_wt_f16x2(w.to(dev))
            with _abi.debug(GEMM_FLAGS[kernel[len("f16x2_"):]]):
                y, _, _ = H.conv1x1_f16x2(vd, t, wf, we, m, pro, b.to(dev),
                                          x_bound=float(gamma.abs().max()) * (k * t) ** 0.5 + float(beta.abs().max()))
        torch.cuda.synchronize()
        return y[..., :t].cpu(), keep

    def ref(v):
        a = O.prelu(O.glob_ln(v.double(), gamma.double(), beta.double()), slope.double())
        return torch.matmul(w.double(), a) + b.double().reshape(1, -1, 1)

    (y, _), (yb, _) = call(x), call(xb)
    assert bool(torch.isnan(ref(xb)[1]).all())
    assert rel_max(y.double().numpy(), ref(x).numpy()) < (4e-6 if kernel != "fp32" else 2e-5)
    assert torch.equal(yb[0], y[0])
    assert bool(torch.isnan(yb[1]).all())


@pytest.mark.parametrize("bad", BAD, ids=str)
@pytest.mark.parametrize("res_inside", [False, True])
def test_conv1x1_f16x2_ln_one_bad_row(H, dev, bad, res_inside):
    """ps_conv1x1_f16x2_ln_f32 (the shapes of test_gemm_with_layernorm_epilogue_behind_a_prologue, its 5e-6) with the
    measured maxima as the range, and the maxima it leaves for the next GEMM."""
    import torch.nn.functional as F
    c = 128
    x, w, b, _, _, res, _, _, _, t = _small("res", c, dev)
    g, be = R.rand((c,), 147, 0.5, 1.5), R.rand((c,), 148, -0.3, 0.3)
    xb = x.clone()
    xb[1, 17, 70] = bad
    ln = lambda v: F.layer_norm(v.transpose(1, 2), (c,), g.double(), be.double(), 1e-5).transpose(1, 2)  # noqa: E731

    def ref(v):
        p = torch.matmul(w.double(), v.double()) + b.double().reshape(1, -1, 1)
        return ln(p + res.double()) if res_inside else res.double() + ln(p)
    w256 = torch.zeros(256, w.shape[1])
    w256[:c] = w
    wf, we = H.pack_wt_f16x2(w256.to(dev))
    with _abi.debug(_abi.PS_DBG_GEMM_ANY_SIZE):
        assert H.conv1x1_f16x2_ln_ok(2, w.shape[1], c, t)
        outs = []
        for v in (x, xb):
            vd = H.pad_rows(v.to(dev))
            outs.append(H.conv1x1_f16x2_ln(vd, t, wf, we, c, b.to(dev), g.to(dev), be.to(dev), 1e-5, H.pad_rows(res.to(dev)),
                                           x_amax=H.absmax(vd, t), res_inside=res_inside, want_amax=True))
        torch.cuda.synchronize()
    (y, _), (yb, am) = outs
    assert rel_max(y[..., :t].cpu().numpy(), ref(x).numpy()) < 5e-6
    assert torch.equal(yb[0, :, :t], y[0, :, :t])
    got = yb[1, :, :t].cpu()
    _bad_row_check(got, ref(xb)[1], 5e-6)
    _amax_hides_nothing(am[1].cpu(), got)


@pytest.mark.parametrize("bad", BAD, ids=str)
def test_conv1x1_f16_rows_one_bad_row(H, dev, bad):
    """ps_conv1x1_f16_rows (bf16 rows, one fp16 term) with the measured maxima of the rows as its range, at the 2e-2 of
    test_f16_rows_gemm_in_every_variant."""
    import ctypes as C
    from test_fp16x2 import _small_case
    m = 256
    x, w, b, _, _, _, _, _, _, t = _small_case("plain", m, dev, rows16=True)
    n, k = x.shape[:2]
    xb = x.clone()
    xb[1, 17, 70] = bad
    wf, we = H.pack_wt_f16x2(w.to(dev))
    bd = b.to(dev)
    outs = []
    with _abi.debug(_abi.PS_DBG_GEMM_ANY_SIZE):
        assert _abi.lib().ps_conv1x1_f16_rows_ok(n, k, m, t)
        for v in (x, xb):
            v32 = H.pad_rows(v.to(dev))
            vd = v32.bfloat16()
            amax = H.absmax(v32, t)
            y = torch.empty(n, m, vd.shape[-1], dtype=torch.bfloat16, device=dev)
            rng = _abi.F16x2Range(int(we), 0.0, _abi.ptr(amax), amax.shape[1], None)
            _abi.check(_abi.lib().ps_conv1x1_f16_rows(_abi.ptr(vd), _abi.ptr(wf), C.byref(rng), _abi.ptr(y), n, k, m, t,
                                                      vd.shape[-1], None, _abi.ptr(bd), None, None, None,
                                                      _abi.stream_ptr(dev)), "ps_conv1x1_f16_rows")
            torch.cuda.synchronize()
            outs.append(y[..., :t].float().cpu())
    y, yb = outs
    ref = lambda v: torch.matmul(w.double(), v.double()) + b.double().reshape(1, -1, 1)  # noqa: E731
    assert rel_max(y.double().numpy(), ref(x).numpy()) < 2e-2
    assert torch.equal(yb[0], y[0])
    _bad_row_check(yb[1], ref(xb)[1], 2e-2)


@pytest.mark.parametrize("bad", BAD, ids=str)
def test_conv2d_f16x2_one_bad_row(H, dev, bad):
    """ps_conv2d_f16x2_f32 (the smallest shape of test_conv2d_f16x2_kernel: transposed, 32 channels from 16 + 16, its
    5e-6): the kernel measures its range per wave and K chunk; an infinity there costs the wave's 32 frames, a NaN only
    the outputs whose taps hold it."""
    import torch.nn.functional as F
    n, f, t, m, c1, c2 = 2, 11, 150, 32, 16, 16
    x1, x2 = R.rand((n, c1, f, t), 651), R.rand((n, c2, f, t), 652)
    kf, kt, sf = 3, 2, 1
    b = R.rand((m,), 653)
    w = R.rand((c1 + c2, m, kf, kt), 654, -0.3, 0.3)
    w2, shift = w.permute(1, 0, 2, 3).reshape(m, -1), kt - 1
    img, w_exp = H.pack_conv2d_f16x2(w2.contiguous().to(dev))
    pad = lambda v: H.pad_rows(v.reshape(n, -1, t).to(dev)).view(n, v.shape[1], f, -1)  # noqa: E731
    x1b = x1.clone()
    x1b[1, 5, 4, 70] = bad

    def ref(a):
        op = sf - kf + 2 * (kf // 2)
        return F.conv_transpose2d(torch.cat([a, x2], 1).double(), w.double(), b.double(), stride=(sf, 1), padding=(kf // 2, 0),
                                  output_padding=(op, 0))[..., (kt - 1):]
    args = (m, t, f, kf, kt, sf, 1, 1, kf // 2, shift, True)
    y = H.conv2d_f16x2(pad(x1), pad(x2), img, w_exp, b.to(dev), *args)
    yb = H.conv2d_f16x2(pad(x1b), pad(x2), img, w_exp, b.to(dev), *args)
    torch.cuda.synchronize()
    assert rel_max(y[..., :t].cpu().numpy(), ref(x1).numpy()) < 5e-6
    assert torch.equal(yb[0], y[0])
    _bad_row_check(yb[1, ..., :t].cpu(), ref(x1b)[1], 5e-6)


@pytest.mark.parametrize("bad", BAD, ids=str)
@pytest.mark.parametrize("k,m", [(64, 128), (20, 100)])
def test_proj_layernorm_amax_one_bad_row(H, dev, bad, k, m):
    """ps_proj_layernorm_amax_f32 (exact fp32; T = 129, the pipelined and the rows<4> kernel, the 2e-5 of their direct
    tests): the bad sample costs its own frame, as in fp64, and the maxima still cover the finite rest."""
    n, t = 2, 129
    x, res = R.rand((n, k, t), 671), R.rand((n, m, t), 672)
    w, b = R.rand((m, k), 673, -0.3, 0.3), R.rand((m,), 674)
    g, be = R.rand((m,), 675, 0.5, 1.5), R.rand((m,), 676)
    xb = x.clone()
    xb[1, 7, 70] = bad
    outs = []
    for v in (x, xb):
        outs.append(H.proj_layernorm(H.pad_rows(v.to(dev)), t, H.pack_wt(w.to(dev)), b.to(dev), m, g.to(dev), be.to(dev), 1e-5,
                                     H.pad_rows(res.to(dev)), want_amax=True))
    torch.cuda.synchronize()
    (y, _, _), (yb, _, am) = outs
    assert rel_max(y[..., :t].cpu().double().numpy(), R.proj_layernorm_ref(x, w, b, g, be, 1e-5, res)[0].numpy()) < 2e-5
    assert torch.equal(yb[0, :, :t], y[0, :, :t])
    got = yb[1, :, :t].cpu()
    _bad_row_check(got, R.proj_layernorm_ref(xb, w, b, g, be, 1e-5, res)[0][1], 2e-5, exact_masks=True)
    _amax_hides_nothing(am[1].cpu(), got)


@pytest.mark.parametrize("bad", BAD + [float("-inf")], ids=str)
def test_lstm_fmajor_h256_one_bad_sequence(H, dev, bad):
    """ps_lstm_fmajor_h256_f16x2_f32 (the smallest case of its direct test: one direction, N = 2 rows of S = 3 sequences of
    K = 10 steps, the 2e-5 of that test against the fp64 LSTM): one gate pre-activation of sequence 4 at step 5 is bad.
    The accumulator scale comes from the weights, so nothing but the recurrence carries it: the sequence is non-finite
    where the fp64 recurrence is (a saturated gate of +-inf is 0 / 1 / +-1 there, not NaN), the others bit-identical."""
    import torch.nn as nn
    from oracle import dualpath_oracle as DP
    from puresound_amd.nnet._plans import lstm_plan
    n, s, k, c, hid = 2, 3, 10, 12, 256
    mod = nn.LSTM(c, hid, num_layers=1, batch_first=True)
    sd = {kk: R.rand(tuple(v.shape), 430 + i, -0.25, 0.25) for i, (kk, v) in enumerate(mod.state_dict().items())}
    mod.load_state_dict(sd)
    x = R.rand((n, c, s * k), 431)
    p = lstm_plan(mod.to(dev), torch.device(dev))
    t = s * k
    gx, _ = H.conv1x1(H.pad_rows(x.to(dev)), t, p["wih"], p["rows"], None, p["bias"])
    img, scale = H.pack_whh_h256(p["whh_t"])
    gxb = gx.clone()
    row = 2 * hid + 9      # a cell-candidate (g) row in nn.LSTM's gate order: tanh
    gxb[1, row, 1 * k + 5] = bad
    outs = [H.lstm_fmajor_h256(v.transpose(1, 2).contiguous(), img, scale, 1, s, k, k, 1)[0][..., :t].cpu() for v in (gx, gxb)]
    torch.cuda.synchronize()
    y, yb = outs

    def ref(g):   # the fp64 recurrence on the kernel's own pre-activations [N, 4H, T] -> [N, H, T]
        g = g[..., :t].cpu().double()
        whh = sd["weight_hh_l0"].double()
        out = torch.zeros(n, hid, t, dtype=torch.float64)
        for q in range(s):
            h = torch.zeros(n, hid, dtype=torch.float64)
            cc = torch.zeros(n, hid, dtype=torch.float64)
            for j in range(k):
                a = g[:, :, q * k + j] + h @ whh.t()
                i_, f_, g_, o_ = a[:, :hid], a[:, hid:2 * hid], a[:, 2 * hid:3 * hid], a[:, 3 * hid:]
                cc = torch.sigmoid(f_) * cc + torch.sigmoid(i_) * torch.tanh(g_)
                h = torch.sigmoid(o_) * torch.tanh(cc)
                out[:, :, q * k + j] = h
        return out
    assert rel_max(y.double().numpy(), ref(gx).numpy()) < 2e-5
    assert torch.equal(yb[0], y[0])
    keep = torch.ones(t, dtype=torch.bool)
    keep[k:2 * k] = False
    assert torch.equal(yb[1][:, keep], y[1][:, keep])
    _bad_row_check(yb[1], ref(gxb)[1], 2e-5)
