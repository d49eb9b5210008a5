"""Batches of utterances of unequal length on the MI355X: the kernels of csrc/ragged.hip through their wrappers against the
float64 references of ragged_ref.py, the ragged driver on two blocks, and SoTaskWrapModule.inference(..., lengths=...) on
cfg2_short, cfg3_short and cfg3_causal_short against the float64 oracle of every utterance alone.

Bounds, none of them new: FP32 (2e-5 on rel_max) is the FP32 class of test_abi_kernels_gpu.py and edge_length_cases.FP32_TOL the
project's bound for the exact-fp32 arithmetic on these presets; the ragged path forms the same products and fp64 sums.  The
statistics are checked as the mean and rstd a consumer derives from the partials, to 1e-6: the partials are fp64 sums of the
fp32 values (the reference reads the same fp32 values), and the inputs carry a mean of the order of their deviation, so
neither quantity is a difference of nearly equal numbers.  The junk behind an utterance is 20 x the signal's amplitude, or NaN
(the same bits are asserted); test_ragged_batch.py shows that zero-padding moves the oracle's answer by >= 1e-2 on every short
row of this batch."""
import pytest
import torch

import cases
import edge_length_cases as E
import ragged_ref as R
from abi_refs import rand
from conftest import rel_max
from oracle import separator_oracle as O
from puresound_amd._abi import TcnBlock

pytestmark = pytest.mark.gpu
FP32 = 2e-5
STATS_TOL = 1e-6
NAN = float("nan")
T_ROWS = (301, 1, 2, 3, 127, 128, 129, 257)   # T = 301: one, two, three frames; around the 128-frame granule; 257
TILE = 1024                                   # frames of a ps_dwconv_ragged_f32 workgroup (include/puresound_hip.h)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def hip():
    from puresound_amd import hip
    hip.lib()
    return hip


@pytest.fixture(scope="module")
def PA():
    import puresound_amd.nnet as PA
    return PA


@pytest.fixture(autouse=True)
def _nan_in_the_allocator_cache(dev):
    """NaN-filled blocks in torch's caching allocator: `torch.empty` scratch and outputs start as NaN, not as zeros."""
    junk = [torch.full((1 << 22,), NAN, device=dev) for _ in range(16)]
    junk += [torch.full((n,), NAN, device=dev) for n in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20)]
    del junk
    yield


def _rand(seed, *shape):
    """seeded Philox values in [-1, 1)"""
    return rand(shape, seed)


def _err(got, ref):
    return rel_max(got.detach().cpu().double().numpy(), ref.detach().double().numpy())


def _ragged_rows(hip, dev, x, t_rows, junk):
    """compact [N, R, T] -> padded device rows with `junk` behind each row's end and in the pad columns"""
    p = hip.pad_rows(x.float().to(dev))
    for n, tn in enumerate(t_rows):
        p[n, :, tn:] = junk
    return p


def _limits(dev, values):
    return torch.tensor(values, dtype=torch.int32, device=dev)


def _data(seed, n, rows, t):
    """values with a mean of the order of their deviation: [N, rows, T] float32"""
    return (_rand(seed, n, rows, t) + 0.5).float()


# ---- ps_ragged_stats_f32 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [16, 256])
@pytest.mark.parametrize("junk", [20.0, NAN])
def test_ragged_stats(hip, dev, h, junk):
    t = 301
    y = _data(11 + h, len(T_ROWS), h, t)
    mean_ref, rstd_ref = R.stats_ref(y, T_ROWS)
    yp = _ragged_rows(hip, dev, y, T_ROWS, junk)
    for parts in (None, 1, 7, 600):       # the driver's slot count, one slot, rows that wrap, more slots than rows
        stats = hip.ragged_stats(yp, t, _limits(dev, T_ROWS), parts)
        torch.cuda.synchronize(dev)
        assert stats.shape[1] == (hip.lib().ps_stats_parts(h, t) if parts is None else parts)
        assert bool(torch.isfinite(stats).all())
        if parts == 600:
            assert float(stats[:, h:].abs().max()) == 0.0   # slots without rows are written, as 0
        mean, rstd = R.consumer_scalars(stats.cpu(), float(h * t))
        em, er = _err(mean, mean_ref), _err(rstd, rstd_ref)
        print(f"ragged_stats H={h} parts={parts} junk={junk}: mean {em:.2e} rstd {er:.2e}")
        assert ((mean - mean_ref).abs() <= STATS_TOL * mean_ref.abs()).all(), (parts, mean, mean_ref)
        assert ((rstd - rstd_ref).abs() <= STATS_TOL * rstd_ref).all(), (parts, rstd, rstd_ref)


# ---- ps_dwconv_ragged_f32 ------------------------------------------------------------------------------------------------------------
def _dwconv_case(hip, dev, h, t, t_rows, dilation, causal, kind, junk, p=3, seed=0):
    n = len(t_rows)
    x = _data(100 + seed + h + dilation, n, h, t)
    w, b = _rand(200 + seed, h, 1, p).float(), _rand(201 + seed, h).float()
    gamma, beta = (_rand(202 + seed, h) * 0.5 + 1.0).float(), (_rand(203 + seed, h) * 0.3).float()
    slope = torch.tensor([0.25])
    left = (p - 1) * dilation if causal else ((p - 1) // 2) * dilation
    y_ref = R.dwconv_ragged_ref(x, t_rows, w, b, dilation, left, kind, gamma, beta, slope)
    xp = _ragged_rows(hip, dev, x, t_rows, junk)
    lim = _limits(dev, t_rows)
    g, be, sl = gamma.to(dev), beta.to(dev), slope.to(dev)
    stats_in = hip.ragged_stats(xp, t, lim) if kind == R.GLOBAL else None
    pro = hip.make_prologue(kind, True, stats_in, float(h * t), 1e-8, g if kind else None, be if kind else None, sl)
    y, stats = hip.dwconv_ragged(xp, t, lim, w.to(dev), b.to(dev), dilation, left, pro, want_stats=True)
    torch.cuda.synchronize(dev)
    y = y.cpu()
    assert bool(torch.isfinite(y[..., :t]).all())
    for row, tn in enumerate(t_rows):
        assert float(y[row, :, tn:t].abs().max() if tn < t else 0.0) == 0.0, (row, tn)   # exact zeros on [T_n, T)
    err = _err(y[..., :t], y_ref)
    mean, rstd = R.consumer_scalars(stats.cpu(), float(h * t))
    mean_ref, rstd_ref = R.stats_ref(y[..., :t], t_rows)          # the statistics of the values the kernel wrote
    print(f"dwconv_ragged H={h} T={t} P={p} d={dilation} causal={causal} kind={kind} junk={junk}: y {err:.2e} "
          f"mean {_err(mean, mean_ref):.2e} rstd {_err(rstd, rstd_ref):.2e}")
    assert err < FP32
    assert stats.shape[1] == hip.lib().ps_dwconv_stats_parts(h, t) and bool(torch.isfinite(stats).all())
    assert ((mean - mean_ref).abs() <= STATS_TOL * mean_ref.abs()).all(), (mean, mean_ref)
    assert ((rstd - rstd_ref).abs() <= STATS_TOL * rstd_ref).all(), (rstd, rstd_ref)


@pytest.mark.parametrize("h", [16, 256])
@pytest.mark.parametrize("dilation", [1, 128])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("kind", [R.GLOBAL, R.AFFINE, R.NONE])
def test_dwconv_ragged(hip, dev, h, dilation, causal, kind):
    _dwconv_case(hip, dev, h, 301, T_ROWS, dilation, causal, kind, NAN if (h == 16) == causal else 20.0)


def test_dwconv_ragged_across_the_workgroup_tile(hip, dev):
    """T one 128-frame tile past the kernel's frames per workgroup; rows that end one frame below, at and one above that
    boundary (the second tile of the first two stores zeros without loading), and a full row"""
    t = TILE + 128
    for dilation, causal in ((1, False), (128, False), (128, True)):
        _dwconv_case(hip, dev, 16, t, (TILE - 1, TILE, TILE + 1, t), dilation, causal, R.GLOBAL, NAN)


def test_dwconv_ragged_other_tap_counts(hip, dev):
    """the run-time tap loop (P != 3) and the wide halo (P = 3, dilation 256)"""
    _dwconv_case(hip, dev, 20, 301, T_ROWS, 2, False, R.AFFINE, NAN, p=5, seed=5)
    _dwconv_case(hip, dev, 16, 301, T_ROWS, 3, True, R.GLOBAL, 20.0, p=2, seed=6)
    _dwconv_case(hip, dev, 16, 701, (701, 1, 300, 513), 256, False, R.GLOBAL, NAN, seed=7)


def test_ragged_kernels_refuse_bad_arguments(hip, dev):
    x = torch.zeros(2, 16, 128, device=dev)
    lim = _limits(dev, (5, 3))
    w, b = torch.zeros(16, 1, 3, device=dev), torch.zeros(16, device=dev)
    with pytest.raises(RuntimeError, match="left=3 exceeds the receptive field"):
        hip.dwconv_ragged(x, 100, lim, w, b, 1, 3)
    with pytest.raises(RuntimeError, match="halo"):
        hip.dwconv_ragged(x, 100, lim, w, b, 600, 600)
    with pytest.raises(ValueError, match="int32 tensor"):
        hip.dwconv_ragged(x, 100, _limits(dev, (5, 3, 1)), w, b, 1, 1)
    with pytest.raises(RuntimeError, match="int32"):
        hip.ragged_stats(x, 100, lim.long())
    with pytest.raises(RuntimeError, match="int32"):
        hip.zero_tail(x, lim.cpu())
    with pytest.raises(RuntimeError, match="parts > 0"):
        hip.ragged_stats(x, 100, lim, 0)


# ---- ps_zero_tail_f32 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", [128, 384])
def test_zero_tail(hip, dev, ld):
    limits = (0, 1, ld - 1, ld, 2, 3, 4, 5, 130 % ld)
    x = _data(31, len(limits), 5, ld)
    got = hip.zero_tail(x.to(dev), _limits(dev, limits))
    torch.cuda.synchronize(dev)
    assert torch.equal(got.cpu(), R.zero_tail_ref(x, limits))
    # a waveform batch [N, ld'] whose rows are no multiple of 4 floats (the scalar stores), NaN behind the limit
    wav = _data(32, len(limits), 1, ld - 3)[:, 0].contiguous()
    lim2 = tuple(min(v, ld - 3) for v in limits)
    dirty = wav.clone()
    for n, v in enumerate(lim2):
        dirty[n, v:] = NAN
    got = hip.zero_tail(dirty.to(dev), _limits(dev, lim2))
    torch.cuda.synchronize(dev)
    assert torch.equal(got.cpu(), R.zero_tail_ref(wav[:, None], lim2)[:, 0])


# ---- ps_conv_tasnet_ragged_f32 on two blocks of cfg2_short's stack ------------------------------------------------------------------
def test_conv_tasnet_ragged_on_two_blocks(hip, dev, PA):
    name, t = "cfg2_short", 301
    t_rows = (301, 1, 2, 127, 129, 257)
    model = cases.build(PA.NS, name).eval()
    model.load_state_dict(E.weights(name)[0])
    masker = model.masker.to(dev)
    blocks = [masker.tcn_list[0][6], masker.tcn_list[0][7]]          # dilations 64 and 128
    plans = [m.plan(dev) for m in blocks]
    array = (TcnBlock * 2)(*[p["block"] for p in plans])
    c, h = masker.input_dim, masker.tcn_dim
    x = (_rand(41, len(t_rows), c, t) * 0.3).float()
    sd = E.weights(name)[1]
    xp = _ragged_rows(hip, dev, x, t_rows, NAN)
    out = hip.conv_tasnet_ragged(array, 2, xp, t, c, h, _limits(dev, t_rows), None, False)
    torch.cuda.synchronize(dev)
    out = out.cpu()
    for n, tn in enumerate(t_rows):
        ref = x[n:n + 1, :, :tn].double()
        with torch.no_grad():
            for i, d in ((6, 64), (7, 128)):
                ref = O.tcn_block(ref, sd, f"masker.tcn_list.0.{i}.", 3, d, False, "gLN", "gGN")
        err = _err(out[n:n + 1, :, :tn], ref)
        print(f"conv_tasnet_ragged row {n} (T_n = {tn}): {err:.2e}")
        assert err < FP32, (n, tn, err)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(PA, dev, name):
    if name not in _MODELS:
        model = cases.build(PA.NS, name).eval()
        model.load_state_dict(E.weights(name)[0])
        _MODELS[name] = model.to(dev)
    return _MODELS[name]


def _run(model, dev, noisy, enroll, lens, e_lens):
    out = model.inference(noisy.to(dev), None if enroll is None else enroll.to(dev), lengths=lens, enroll_lengths=e_lens)
    torch.cuda.synchronize(dev)
    return out.cpu()


def _check_rows(name, out, refs, frames, what):
    win, hop = E.win_hop(name)
    assert out.dtype == torch.float32 and out.shape == (len(refs), (max(frames) - 1) * hop + win)
    missed = []
    for n, ref in enumerate(refs):
        valid = ref.shape[-1]
        assert valid == E.out_length(name, frames[n])
        assert E.clamped_share(name, ref) <= E.CLAMP_CAP
        assert bool(torch.isfinite(out[n]).all()), n
        err = E.errors(name, out[n:n + 1, :valid].numpy(), ref.numpy())["rel_max"]
        print(f"{what} {name} row {n} (T_n = {frames[n]}): rel_max {err:.3e}")
        if not err < E.FP32_TOL:
            missed.append((n, frames[n], err))
        assert float(out[n, valid:].abs().max() if valid < out.shape[1] else 0.0) == 0.0, n
    assert not missed, missed


def test_cfg2_ragged_batch_against_the_oracle_of_each_utterance(PA, dev):
    name = "cfg2_short"
    model = _model(PA, dev, name)
    noisy, lens, _, _, refs = R.batch(name, R.CFG2_T)
    model.set_gemm_precision("fp32")
    out = _run(model, dev, noisy, None, lens, None)
    _check_rows(name, out, refs, R.CFG2_T, "ragged")
    assert model.output_lengths(lens) == [r.shape[-1] for r in refs]
    # NaN in the place of the junk: the same bits
    nan_batch = R.batch(name, R.CFG2_T, junk="nan")[0]
    assert torch.equal(nan_batch[0], noisy[0]) and bool(torch.isnan(nan_batch[1, lens[1]:]).all())
    assert torch.equal(_run(model, dev, nan_batch, None, lens, None), out)
    # the model's gemm_precision does not reach the ragged path: the same bits
    model.set_gemm_precision("fp16x2")
    assert torch.equal(_run(model, dev, noisy, None, lens, None), out)
    assert torch.equal(_run(model, dev, noisy, None, torch.tensor(lens), None), out)
    model.set_gemm_precision("fp32")


@pytest.mark.parametrize("name", ["cfg3_short", "cfg3_causal_short"])
def test_cfg3_ragged_batch_with_ragged_enrolments(PA, dev, name):
    model = _model(PA, dev, name)
    noisy, lens, enroll, e_lens, refs = R.batch(name, R.CFG3_T, R.CFG3_ENROL_T)
    model.set_gemm_precision("fp16x2")     # (the default; the ragged path computes exact fp32 products all the same)
    out = _run(model, dev, noisy, enroll, lens, e_lens)
    _check_rows(name, out, refs, R.CFG3_T, "ragged + enrolment")
    noisy_nan, _, enroll_nan, _, _ = R.batch(name, R.CFG3_T, R.CFG3_ENROL_T, junk="nan")
    assert torch.equal(_run(model, dev, noisy_nan, enroll_nan, lens, e_lens), out)
    model.set_gemm_precision("fp32")


def test_equal_lengths_and_no_leak_into_plain_inference(PA, dev):
    name = "cfg2_short"
    model = _model(PA, dev, name)
    model.set_gemm_precision("fp32")
    t = 129
    noisy, _, ref = E.problem(name, E.length_of(name, t), 2)
    plain_before = model.inference(noisy.to(dev)).cpu()
    out = _run(model, dev, noisy, None, [noisy.shape[1]] * 2, None)
    err = E.errors(name, out.numpy(), ref.numpy())["rel_max"]
    print(f"equal lengths {name} T = {t}: rel_max {err:.3e}")
    assert out.shape == ref.shape and err < E.FP32_TOL
    # a short batch through the same kept scratch, then the plain call again: the same bits as before
    short = R.batch(name, R.CFG2_T)
    _run(model, dev, short[0], None, short[1], None)
    assert torch.equal(model.inference(noisy.to(dev)).cpu(), plain_before)


def test_refusals_on_device_tensors_launch_nothing(PA, dev, monkeypatch):
    from puresound_amd import hip as H
    model = _model(PA, dev, "cfg2_short")
    noisy = torch.zeros(2, 400, device=dev)

    def lib():
        raise AssertionError("the HIP library was called")
    monkeypatch.setattr(H, "lib", lib)
    with pytest.raises(ValueError, match="exceeds the row length"):
        model.inference(noisy, lengths=[400, 401])
    with pytest.raises(RuntimeError, match="shorter than the window"):
        model.inference(noisy, lengths=[400, 31])
    with pytest.raises(ValueError, match="without enroll"):
        model.inference(noisy, lengths=[400, 400], enroll_lengths=[100, 100])
    with pytest.raises(NotImplementedError, match="inference with lengths"):
        cases.build(PA.NS, "cfg4_short").eval().to(dev).inference(noisy, lengths=[400, 400])
