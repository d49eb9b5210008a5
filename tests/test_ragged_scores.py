"""Scores of batches of unequal-length utterances, without a GPU: per-row `lengths` through the SDR family (loss/sdr.py) and the
STFT family (loss/stft_loss.py) on CPU tensors -- stock ATen over each row alone, the definition of the semantics -- and
SoTaskWrapModule.inference_scored_ragged on a small model, against the float64 restatements (tests/stft_loss_ref.py,
oracle/loss_oracle.py) applied to every utterance alone; every refusal before a library call; and the condition that keeps the
tests honest: on this batch, scoring the zero-padded rows moves the spectral scores by far more than any bound in use.

Bounds, none of them new: stft_loss_ref.FP32_TOL for the sums (test_stft_loss.py's bound for the same quantities), 2e-3 dB for
the SDR modes (test_inference_scored_equals_inference_then_the_oracle_score), 1e-2 relative for "zero-padding is wrong"
(test_ragged_batch.py's threshold for the waveform)."""
import numpy as np
import pytest
import torch

import cases
import ragged_scores_ref as RS
import stft_loss_ref as R
from detweights import det_wave
from oracle import loss_oracle as LO

LENS = list(RS.LENGTHS)


@pytest.fixture(scope="module")
def PA():
    import puresound_amd.nnet as PA
    return PA


@pytest.fixture(scope="module")
def S():
    from puresound_amd.nnet.loss import stft_loss
    return stft_loss


@pytest.fixture
def no_library(monkeypatch):
    """any call into the HIP library fails the test"""
    from puresound_amd import _abi, hip

    def lib():
        raise AssertionError("the HIP library was called")
    monkeypatch.setattr(_abi, "lib", lib)
    monkeypatch.setattr(hip, "lib", lib)


def _small(PA, **masker_kw):
    """FreeEncDec(win 16, hop 8, 24) + a two-block ConvTasNet -> a wrapper the refusal tests vary"""
    kw = dict(tcn_kernel=3, tcn_dim=12, repeat_tcn=1, tcn_dilated_basic=2, per_tcn_stack=2, tcn_with_embed=[0, 0])
    kw.update(masker_kw)
    wrap = {k: kw.pop(k) for k in ("speaker_net", "embedding_free_tse") if k in kw}
    enc = PA.FreeEncDec(win_length=16, hop_length=8, laten_length=24)
    return PA.SoTaskWrapModule(encoder=enc, masker=PA.ConvTasNet(24, kw.pop("embed_dim", 0), False, **kw), verbose=False,
                               **wrap).eval()


# ---- the STFT family ---------------------------------------------------------------------------------------------------------------
def test_stft_sums_per_row_are_those_of_each_utterance_alone(S):
    enh, ref = RS.batch()
    mr = S.MultiResolutionSTFTLoss()
    sc_want, mag_want = [], []
    for f, res in zip(mr.stft_losses, R.RESOLUTIONS):
        want = RS.row_sums(res)
        m = f.moments(enh, ref, lengths=LENS)
        assert m.dtype == torch.float64 and tuple(m.shape) == (RS.N, 4)
        assert f.frame_counts(LENS) == RS.frame_counts(res)
        err = R.rel_each(m.numpy(), want)
        print(f"{res}: S0..S3 per row against each utterance alone, largest relative error {err:.3e}")
        assert err < R.FP32_TOL
        # the batch values are the reference's formulas over the elements that exist, on those sums
        sc, mag = f(enh, ref, lengths=LENS)
        count = (res[0] // 2 + 1) * sum(RS.frame_counts(res))
        assert torch.equal(sc, (torch.sqrt(m[:, 0].sum()) / torch.sqrt(m[:, 1].sum())).float())
        assert torch.equal(mag, (m[:, 2].sum() / count).float())
        sc64, mag64, _ = RS.batch_values(want, res)
        assert R.rel(float(sc), sc64) < R.FP32_TOL and R.rel(float(mag), mag64) < R.FP32_TOL
        sc_want.append(sc64)
        mag_want.append(mag64)
    total = mr(enh, ref, lengths=LENS)
    want_total = R.FACTOR_SC * float(np.mean(sc_want)) + R.FACTOR_MAG * float(np.mean(mag_want))
    print(f"multi-resolution with lengths: {float(total):.8g} (ref {want_total:.8g})")
    assert total.dtype == torch.float32 and total.dim() == 0 and R.rel(float(total), want_total) < R.FP32_TOL
    assert torch.equal(mr(enh, ref, lengths=torch.tensor(LENS)), total)


@pytest.mark.parametrize("p", R.OV_POWERS)
def test_over_suppression_sums_per_row(S, p):
    enh, ref = RS.batch()
    want = RS.row_sums(R.OV_RESOLUTION, p)
    m = S.STFTLoss(*R.OV_RESOLUTION).moments(enh, ref, p=p, lengths=LENS)
    err = R.rel_each(m.numpy(), want)
    ov = S.over_suppression_loss_ragged(enh, ref, p=p, lengths=LENS)
    ov64 = RS.batch_values(want, R.OV_RESOLUTION)[2]
    print(f"ov p={p}: S0..S3 per row {err:.3e}; value {float(ov):.8g} (ref {ov64:.8g})")
    assert err < R.FP32_TOL and R.rel(float(ov), ov64) < R.FP32_TOL
    count = (R.OV_RESOLUTION[0] // 2 + 1) * sum(RS.frame_counts(R.OV_RESOLUTION))
    assert torch.equal(ov, (m[:, 3].sum() / count).float())


# ---- the SDR family ------------------------------------------------------------------------------------------------------------------
def _oracle_rows(enh, ref, lens, mode, labels):
    """LO.sdr_loss of each row alone, in the order SDRLoss returns them: the active rows, then the inactive ones"""
    order = [n for n in range(len(lens)) if not labels[n]] + [n for n in range(len(lens)) if labels[n]]
    return torch.cat([LO.sdr_loss(enh[n:n + 1, :lens[n]].double(), ref[n:n + 1, :lens[n]].double(), reduction=False,
                                  inactive_labels=labels[n:n + 1], **LO.mode_flags(mode)) for n in order])


@pytest.mark.parametrize("mode", ["sisnr", "sdsdr", "tsdr"])
def test_sdr_modes_per_row_against_the_oracle_of_each_row_alone(PA, mode):
    enh, ref = RS.batch()
    labels = torch.tensor([False, False, True, False])
    loss = PA.SDRLoss.init_mode(mode, reduction=False)
    got = loss(enh, ref, labels, lengths=LENS)
    want = _oracle_rows(enh, ref, LENS, mode, labels)
    print(f"{mode}: {got.view(-1).tolist()} (oracle {want.view(-1).tolist()})")
    assert got.dtype == torch.float32 and tuple(got.shape) == (RS.N, 1)
    np.testing.assert_allclose(got.numpy(), want.numpy(), atol=2e-3, rtol=0)
    # reduction and threshold act on the rows as they do without lengths
    mean = PA.SDRLoss.init_mode(mode, reduction=True)(enh, ref, labels, lengths=LENS)
    assert torch.equal(mean, torch.mean(got))


# ---- junk, equal lengths, zero padding -----------------------------------------------------------------------------------------------
def test_nan_behind_the_rows_changes_no_bit(PA, S):
    enh, ref = RS.batch()
    enh_nan, ref_nan = RS.batch("nan")
    assert torch.equal(enh_nan[0], enh[0]) and bool(torch.isnan(enh_nan[1, LENS[1]:]).all()) and bool(torch.isnan(ref_nan[2, LENS[2]:]).all())
    mr = S.MultiResolutionSTFTLoss()
    assert torch.equal(mr(enh_nan, ref_nan, lengths=LENS), mr(enh, ref, lengths=LENS))
    for f in mr.stft_losses:
        assert torch.equal(f.moments(enh_nan, ref_nan, lengths=LENS), f.moments(enh, ref, lengths=LENS))
    assert torch.equal(S.over_suppression_loss_ragged(enh_nan, ref_nan, lengths=LENS), S.over_suppression_loss_ragged(enh, ref, lengths=LENS))
    labels = torch.tensor([False, False, True, False])
    for mode in ("sisnr", "sdsdr", "tsdr"):
        loss = PA.SDRLoss.init_mode(mode, reduction=False)
        assert torch.equal(loss(enh_nan, ref_nan, labels, lengths=LENS), loss(enh, ref, labels, lengths=LENS))


def test_equal_lengths_are_the_call_without_lengths(PA, S):
    enh, ref = RS.batch()        # (whole rows: the junk is part of the signal here)
    full = [RS.L] * RS.N
    mr = S.MultiResolutionSTFTLoss()
    assert torch.equal(mr(enh, ref, lengths=full), mr(enh, ref))
    for f in mr.stft_losses:
        assert all(torch.equal(a, b) for a, b in zip(f(enh, ref, lengths=full), f(enh, ref)))
        assert torch.equal(f.moments(enh, ref, lengths=full), f.moments(enh, ref))
    for p in R.OV_POWERS:
        assert torch.equal(S.over_suppression_loss_ragged(enh, ref, p=p, lengths=full), S.over_suppression_loss(enh, ref, p=p))
    labels = torch.tensor([False, True, False, False])
    for mode in ("sisnr", "sdsdr", "tsdr"):
        for reduction in (False, True):
            loss = PA.SDRLoss.init_mode(mode, reduction=reduction)
            assert torch.equal(loss(enh, ref, labels, lengths=full), loss(enh, ref, labels))
            assert torch.equal(loss(enh, ref, lengths=torch.tensor(full)), loss(enh, ref))


def test_scoring_the_zero_padded_batch_is_wrong(S):
    """Zeros behind each row, scored without lengths, against the values with lengths: >= 1e-2 relative (the means divide by
    frames that do not exist and the reflect padding at an utterance's end reads the padding)."""
    enh, ref = RS.batch("zero")
    mr = S.MultiResolutionSTFTLoss()
    for what, padded, ragged in (("multi-resolution", mr(enh, ref), mr(enh, ref, lengths=LENS)),
                                 ("over-suppression", S.over_suppression_loss(enh, ref),
                                  S.over_suppression_loss_ragged(enh, ref, lengths=LENS))):
        moved = R.rel(float(padded), float(ragged))
        print(f"{what}: zero-padded {float(padded):.6g} against per-row {float(ragged):.6g}: relative {moved:.3e}")
        assert moved >= 1e-2, (what, moved)


# ---- the wrapper on a small model ----------------------------------------------------------------------------------------------------
def test_inference_scored_ragged_is_inference_then_the_rows_one_by_one(PA, S):
    torch.manual_seed(11)
    model = _small(PA)
    lens = [400, 215, 120, 57]
    out = model.output_lengths(lens)
    assert out == [400, 208, 120, 56]
    r_lens = [370, 208, 140, 56]                       # shorter, equal, longer, equal
    noisy = det_wave(7310, 4, 400) * 0.2
    clean = det_wave(7311, 4, 420) * 0.2
    for n in range(4):                                 # junk behind every row of both
        noisy[n, lens[n]:] = float("nan")
        clean[n, r_lens[n]:] = float("nan")
    want = model.inference(noisy, lengths=lens)
    rows = [(want[n:n + 1, :out[n]], RS.aligned_row(clean[n:n + 1, :r_lens[n]], out[n])) for n in range(4)]
    aligned = torch.zeros_like(want)
    for n in range(4):
        aligned[n, :out[n]] = rows[n][1][0]
    # an SDRLoss: the value of every row alone, the inactive row last
    labels = torch.tensor([False, True, False, False])
    for mode in ("sisnr", "sdsdr", "tsdr"):
        loss = PA.SDRLoss.init_mode(mode, reduction=False)
        enh, score = model.inference_scored_ragged(noisy, clean, loss_func=loss, inactive_labels=labels, lengths=lens,
                                                   ref_lengths=r_lens)
        assert torch.equal(enh, want)
        alone = torch.cat([loss(*rows[n], labels[n:n + 1]) for n in (0, 2, 3, 1)])
        assert torch.equal(score, alone), (mode, score, alone)
        np.testing.assert_allclose(score.numpy(), _oracle_rows_of(rows, mode, labels).numpy(), atol=2e-3, rtol=0)
    # the default: loss_func_wav, else SI-SNR with the mean reduction; ref_lengths defaults to lengths
    ref_same = det_wave(7312, 4, 400) * 0.2
    for n in range(4):
        ref_same[n, lens[n]:] = float("nan")
    _, score = model.inference_scored_ragged(noisy, ref_same, lengths=lens)
    rows_same = [(want[n:n + 1, :out[n]], RS.aligned_row(ref_same[n:n + 1, :lens[n]], out[n])) for n in range(4)]
    sisnr = PA.SDRLoss.init_mode("sisnr", reduction=False)
    assert torch.equal(score, torch.mean(torch.cat([sisnr(*r) for r in rows_same])))
    # an STFTLoss of a small resolution: the formulas over the sums of every row alone
    one = S.STFTLoss(32, 8, 32)
    enh, (sc, mag) = model.inference_scored_ragged(noisy, clean, loss_func=one, lengths=lens, ref_lengths=r_lens)
    m = torch.cat([one.moments(*r) for r in rows])
    assert torch.equal(enh, want)
    assert torch.equal(sc, (torch.sqrt(m[:, 0].sum()) / torch.sqrt(m[:, 1].sum())).float())
    assert torch.equal(mag, (m[:, 2].sum() / (17 * sum(one.frame_counts(out)))).float())
    # a closure that takes lengths
    mr = S.MultiResolutionSTFTLoss([32, 64], [8, 16], [32, 48])

    def closure(est, ref, unused, lengths=None):
        return mr(est, ref, lengths=lengths) + S.over_suppression_loss_ragged(est, ref, fft_size=32, hop_size=8, win_length=32,
                                                                       lengths=lengths)
    enh, score = model.inference_scored_ragged(noisy, clean, loss_func=closure, lengths=lens, ref_lengths=r_lens)
    assert torch.equal(enh, want) and torch.equal(score, closure(want, aligned, None, lengths=out)) and float(score) > 0
    assert torch.equal(model.inference_scored_ragged(noisy, clean, loss_func=mr, lengths=lens, ref_lengths=r_lens)[1],
                       mr(want, aligned, lengths=out))


def _oracle_rows_of(rows, mode, labels):
    order = [n for n in range(len(rows)) if not labels[n]] + [n for n in range(len(rows)) if labels[n]]
    return torch.cat([LO.sdr_loss(rows[n][0].double(), rows[n][1].double(), reduction=False, inactive_labels=labels[n:n + 1],
                                  **LO.mode_flags(mode)) for n in order])


# ---- refusals: each before any library call --------------------------------------------------------------------------------------
def test_bad_length_values_are_refused(PA, S, no_library):
    from puresound_amd.nnet.loss import sdr as sdr_module
    model = _small(PA)
    noisy, clean = torch.zeros(3, 200), torch.zeros(3, 180)
    ok = [200, 100, 50]
    for bad, exc, text in (([200, 100], ValueError, "2 values for a batch of 3"),
                           ([200, 201, 100], ValueError, "exceeds the row length 200"),
                           ([200, 100.0, 50], ValueError, "Python ints"),
                           (torch.tensor([200.0, 100.0, 50.0]), ValueError, "integer tensor"),
                           ([200, 15, 100], RuntimeError, "input length 15 is shorter than the window 16")):
        with pytest.raises(exc, match=text):
            model.inference_scored_ragged(noisy, clean, lengths=bad, ref_lengths=[180, 100, 50])
    for bad, exc, text in (([180, 100], ValueError, "ref_lengths holds 2 values for a batch of 3"),
                           ([180, 181, 50], ValueError, r"ref_lengths\[1\] = 181 exceeds the row length 180"),
                           ([180, 0, 50], ValueError, r"ref_lengths\[1\] = 0 must be at least 1"),
                           (torch.tensor([180, 100, 50], dtype=torch.float32), ValueError, "integer tensor")):
        with pytest.raises(exc, match=text):
            model.inference_scored_ragged(noisy, clean, lengths=ok, ref_lengths=bad)
    with pytest.raises(ValueError, match=r"ref_lengths\[0\] = 200 exceeds the row length 180"):
        model.inference_scored_ragged(noisy, clean, lengths=ok)           # ref_lengths defaults to lengths
    with pytest.raises(ValueError, match="lengths is needed"):
        model.inference_scored_ragged(noisy, clean)
    with pytest.raises(RuntimeError, match="ref_clean must be"):
        model.inference_scored_ragged(noisy, clean[:2], lengths=ok)
    # the losses on their own
    x = torch.zeros(3, 200)
    sdr = PA.SDRLoss.init_mode("sisnr")
    with pytest.raises(ValueError, match=r"SDRLoss: lengths\[1\] = 0 must be at least 1"):
        sdr(x, x, lengths=[200, 0, 50])
    with pytest.raises(ValueError, match=r"SDRLoss: lengths\[2\] = 201 exceeds the row length 200"):
        sdr(x, x, lengths=[200, 1, 201])
    with pytest.raises(ValueError, match="si_snr: lengths holds 2 values"):
        sdr_module.si_snr(x, x, lengths=[200, 100])
    with pytest.raises(ValueError, match=r"inactive_sdr_loss: lengths\[0\] = 0 must be at least 1"):
        sdr_module.inactive_sdr_loss(x, x, lengths=[0, 100, 100])
    with pytest.raises(ValueError, match="integer tensor"):
        S.STFTLoss(64, 16, 64)(x, x, lengths=torch.tensor([200.0, 100.0, 50.0]))


def test_a_row_at_or_below_half_the_fft_size_is_refused_by_name(PA, S, no_library):
    x = torch.zeros(3, 4000)
    with pytest.raises(RuntimeError, match=r"STFTLoss: .*lengths\[1\] = 512 with fft_size 1024"):
        S.STFTLoss()(x, x, lengths=[4000, 512, 3000])
    with pytest.raises(RuntimeError, match=r"STFTLoss: .*lengths\[2\] = 500 with fft_size 1024"):
        S.STFTLoss().moments(x, x, lengths=[4000, 513, 500])
    # the multi-resolution loss raises before the first launch of any resolution: 1024 passes the first, not the second
    with pytest.raises(RuntimeError, match=r"MultiResolutionSTFTLoss: .*lengths\[0\] = 1024 with fft_size 2048"):
        S.MultiResolutionSTFTLoss()(x, x, lengths=[1024, 4000, 4000])
    with pytest.raises(RuntimeError, match=r"over_suppression_loss_ragged: .*lengths\[2\] = 256 with fft_size 512"):
        S.over_suppression_loss_ragged(x, x, [4000, 257, 256])
    model = _small(PA)
    noisy, clean = torch.zeros(2, 200), torch.zeros(2, 200)
    with pytest.raises(RuntimeError, match=r"inference_scored_ragged: .*lengths\[1\] = 32 with fft_size 64"):
        model.inference_scored_ragged(noisy, clean, loss_func=S.STFTLoss(64, 16, 64), lengths=[200, 39])   # out_n = 32
    with pytest.raises(RuntimeError, match=r"inference_scored_ragged: .*lengths\[1\] = 32 with fft_size 64"):
        model.inference_scored_ragged(noisy, clean, loss_func=S.MultiResolutionSTFTLoss([32, 64], [8, 16], [32, 64]),
                                      lengths=[200, 39])


def test_row_entries_refuse_bad_arguments_on_the_host():
    """the C entries refuse on the host, before any launch (the library loads without a GPU)"""
    import ctypes as C
    from puresound_amd import _abi
    lib = _abi.lib()
    buf = C.create_string_buffer(1 << 14)
    base = (C.addressof(buf) + 255) // 256 * 256     # aligned host memory that nothing dereferences: every call is refused
    x, y, lim = base, base + 4096, base + 8192

    def refused(rc, text):
        assert rc != 0 and text in lib.ps_last_error().decode(), (rc, lib.ps_last_error())
    refused(lib.ps_align_rows_f32(x, y, None, lim, 2, 64, 64, 64, None), "ps_align_rows_f32: null pointer")
    refused(lib.ps_align_rows_f32(x, y, lim, lim, 2, 64, 64, 63, None), "ldr=63")
    refused(lib.ps_align_rows_f32(x, x, lim, lim, 2, 64, 64, 64, None), "must not alias")
    refused(lib.ps_wave_moments_rows_f64(x, y, None, y, 2, 64, 64, 64, None), "len_rows is NULL")
    refused(lib.ps_wave_moments_rows_f64(x, y, lim, y, 2, 64, 63, 64, None), "ps_wave_moments_rows_f64: null pointer or bad size")
    refused(lib.ps_frame_reflect_rows_f32(x, None, None, y, 2, 64, 64, 0, 32, 32, 8, 9, 128, None), "len_rows is NULL")
    refused(lib.ps_frame_reflect_rows_f32(x, None, lim, y, 2, 64, 64, 0, 32, 32, 8, 8, 128, None),
            "ps_frame_reflect_rows_f32: bad argument")            # T = 9 is the launch's frame count
    refused(lib.ps_frame_reflect_rows_f32(x, None, lim, y, 2, 16, 64, 0, 32, 32, 8, 3, 128, None), "reflect padding needs L > n_fft/2")
    refused(lib.ps_spec_pair_moments_rows_f64(x, None, y, 1, 9, 5, 128, 0.5, None), "t_rows is NULL")
    refused(lib.ps_spec_pair_moments_rows_f64(x, lim, y, 1, 9, 129, 128, 0.5, None), "ps_spec_pair_moments_rows_f64: bad argument")


def test_uncovered_losses_and_models_are_refused(PA, S, no_library):
    model = _small(PA)
    noisy, clean, lens = torch.zeros(2, 200), torch.zeros(2, 200), [200, 100]
    with pytest.raises(NotImplementedError, match="source-aggregated"):
        model.inference_scored_ragged(noisy, clean, loss_func=PA.SDRLoss.init_mode("sasdr"), lengths=lens)
    with pytest.raises(NotImplementedError, match="source-aggregated"):
        PA.SDRLoss.init_mode("sasisnr")(torch.zeros(2, 2, 200), torch.zeros(2, 2, 200), lengths=lens)
    with pytest.raises(NotImplementedError, match="cannot know where the rows end"):
        model.inference_scored_ragged(noisy, clean, loss_func=R.stft_ov_closure(S), lengths=lens)
    with pytest.raises(NotImplementedError, match="must take `lengths`"):
        model.inference_scored_ragged(noisy, clean, loss_func=lambda enh, ref, dummy: enh.sum(), lengths=lens)
    # a model outside ragged.check_model: its refusal, unchanged
    with pytest.raises(NotImplementedError, match='tcn_layer="gated"'):
        _small(PA, tcn_layer="gated").inference_scored_ragged(noisy, clean, lengths=lens)
    with pytest.raises(NotImplementedError, match="inference with lengths"):
        cases.build(PA.NS, "cfg4_short").eval().inference_scored_ragged(torch.zeros(2, 4000), torch.zeros(2, 4000),
                                                                        lengths=[4000, 2000])
    simo = cases.build(PA.NS, "simo_free").eval()
    assert not hasattr(simo, "inference_scored_ragged")
    with pytest.raises(AttributeError):
        simo.inference_scored_ragged(noisy, clean, lengths=lens)
    # inference_scored keeps refusing lengths, and says where to go
    with pytest.raises(NotImplementedError, match="inference_scored_ragged"):
        model.inference_scored(noisy, clean, lengths=lens)
