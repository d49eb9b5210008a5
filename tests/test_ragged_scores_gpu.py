"""Scores of batches of unequal-length utterances on the MI355X: the four row-limited entries through their hip.py wrappers
against float64 numpy / torch at the shapes where they can go wrong, the losses of nnet/loss/ with `lengths` on the batch of
test_ragged_scores.py, and SoTaskWrapModule.inference_scored_ragged on cfg2_short and cfg3_short.

House rules of test_abi_kernels_gpu.py: seeded Philox inputs, NaN in the caching allocator, junk (20.0 or NaN) wherever an
entry promises not to read, exact zeros asserted where it promises them.  Bounds, none of them new: rtol 1e-11 / atol 1e-9 for
the waveform moments (test_decoder_leaves_the_score_moments_behind), stft_loss_ref.FP32_TOL = 2e-5 for the spectral sums
(test_stft_loss_gpu.py), 2e-3 dB for the SDR modes (test_inference_scored_equals_inference_then_the_oracle_score).  The row
kernels keep the summation order of the whole-row kernels, so equal lengths are asserted with torch.equal."""
import numpy as np
import pytest
import torch

import cases
import edge_length_cases as E
import ragged_ref as RB
import ragged_scores_ref as RS
import stft_loss_ref as R
from abi_refs import rand as _rand
from detweights import det_wave
from oracle import loss_oracle as LO

pytestmark = pytest.mark.gpu
NAN = float("nan")
JUNK = [20.0, NAN]
LENS = list(RS.LENGTHS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def H():
    from puresound_amd import hip
    hip.lib()
    return hip


@pytest.fixture(scope="module")
def S():
    from puresound_amd.nnet.loss import stft_loss
    return stft_loss


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


def _limits(dev, values):
    return torch.tensor(values, dtype=torch.int32, device=dev)


def _rows_of_a_wider_buffer(x, junk, limits, base=5, extra=9):
    """x [N, L] -> (a view [N, L] at column `base` of a buffer [N, L + extra] of `junk`, with `junk` behind limits[n] too)"""
    wide = torch.full((x.shape[0], x.shape[1] + extra), junk)
    wide[:, base:base + x.shape[1]] = x
    for n, v in enumerate(limits):
        wide[n, base + v:] = junk
    return wide


# ---- ps_wave_moments_rows_f64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("junk", JUNK)
def test_wave_moments_rows(H, dev, junk):
    chunk = 8192                                           # WM_CHUNK of csrc/loss.hip
    length = 2 * chunk + 5
    len_rows = (1, 3, 4, 5, chunk - 1, chunk, chunk + 1, length)
    a, b = _rand((len(len_rows), length), 901), _rand((len(len_rows), length), 902) + 0.25
    wa = _rows_of_a_wider_buffer(a, junk, len_rows).to(dev)
    wb = _rows_of_a_wider_buffer(b, junk, len_rows, extra=14).to(dev)
    va, vb = wa[:, 5:5 + length], wb[:, 5:5 + length]      # lda, ldb > L, base offset 5 floats
    assert va.stride(0) == length + 9 and vb.stride(0) == length + 14
    lim = _limits(dev, len_rows)
    got = H.wave_moments_rows(va, vb, lim)
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(len_rows), 5)
    want = np.zeros((len(len_rows), 5))
    for n, v in enumerate(len_rows):
        x, y = a[n, :v].double().numpy(), b[n, :v].double().numpy()
        want[n] = [x.sum(), y.sum(), (x * x).sum(), (y * y).sum(), (x * y).sum()]
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-11, atol=1e-9)
    assert torch.equal(H.wave_moments_rows(va, vb, lim), got), "one writer per slot: the same call gives the same bits"
    # limits beyond the rows are clamped to them; whole rows give the bits of the whole-row entry
    full = H.wave_moments_rows(va[-1:], vb[-1:], _limits(dev, [length + 1000]))
    assert torch.equal(full, got[-1:]) and torch.equal(full, H.wave_moments(va[-1:], vb[-1:]))


# ---- ps_align_rows_f32 -------------------------------------------------------------------------------------------------------------
# (a_len, b_len): b < a with d = a - b in {1, 2, 3, 4, 5, a - 1}, b = a, b > a, and a_len = 1 (equal, longer)
ALIGN_PAIRS = [(1031, 1030), (1000, 998), (1031, 1028), (900, 896), (777, 772), (500, 1), (1031, 1031), (640, 1040), (1, 1),
               (1, 7), (1024, 1040)]


@pytest.mark.parametrize("l_out", [1031, 1032])            # dword stores; 16-byte stores
@pytest.mark.parametrize("junk", JUNK)
def test_align_rows(H, dev, l_out, junk):
    l_ref = 1040
    pairs = [(min(a, l_out), b) for a, b in ALIGN_PAIRS]
    b_len = [b for _, b in pairs]
    ref = _rand((len(pairs), l_ref), 911)
    wide = _rows_of_a_wider_buffer(ref, junk, b_len, base=3, extra=6).to(dev)
    view = wide[:, 3:3 + l_ref]                            # rows of a wider buffer, at a base that is not 16-byte aligned
    got = H.align_rows(view, _limits(dev, [a for a, _ in pairs]), _limits(dev, b_len), l_out).cpu()
    want = torch.zeros(len(pairs), l_out)
    for n, (a, b) in enumerate(pairs):
        want[n, :a] = RS.aligned_row(ref[n:n + 1, :b], a)[0]
    assert torch.equal(got, want)
    for n, (a, _) in enumerate(pairs):
        assert float(got[n, a:].abs().max() if a < l_out else 0.0) == 0.0, n


# ---- ps_frame_reflect_rows_f32 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,win", [(16, 4, 16), (16, 4, 10), (15, 5, 9)])
@pytest.mark.parametrize("junk", JUNK)
def test_frame_reflect_rows(H, dev, n_fft, hop, win, junk):
    length = 1040
    len_rows = (n_fft // 2 + 1, n_fft, 4 * 127, 4 * 128, 4 * 129 + 1, length)
    n = len(len_rows)
    a, b = _rand((n, length), 921), _rand((n, length), 922)
    da = _rows_of_a_wider_buffer(a, junk, len_rows, base=0, extra=0).to(dev)
    db = _rows_of_a_wider_buffer(b, junk, len_rows, base=0, extra=0).to(dev)
    frames, t = H.frame_reflect_rows(da, db, _limits(dev, len_rows), n_fft, win, hop)
    assert t == R.frames(length, n_fft, hop) and tuple(frames.shape) == (2 * n, win, H.padded_frames(t))
    frames = frames.cpu()
    off = (n_fft - win) // 2
    t_rows = [H.stft_frames(v, n_fft, hop) for v in len_rows]
    assert t_rows == [R.frames(v, n_fft, hop) for v in len_rows]
    for r, src in enumerate([a, b]):
        for i, v in enumerate(len_rows):
            padded = torch.nn.functional.pad(src[i:i + 1, :v][None], (n_fft // 2, n_fft // 2), mode="reflect")[0, 0]
            idx = (torch.arange(t_rows[i]) * hop)[None, :] + torch.arange(win)[:, None] + off
            row = frames[r * n + i]
            assert torch.equal(row[:, :t_rows[i]], padded[idx]), (r, i, v)
            assert not bool(row[:, t_rows[i]:].any()), (r, i, "zeros on [T_n, ldt)")
    # one waveform batch alone: N rows, the same bits; whole rows: the bits of the whole-row entry
    alone, _ = H.frame_reflect_rows(da, None, _limits(dev, len_rows), n_fft, win, hop)
    assert torch.equal(alone.cpu(), frames[:n])
    clean = a.to(dev)
    whole, _ = H.frame_reflect_rows(clean, None, _limits(dev, [length] * n), n_fft, win, hop)
    assert torch.equal(whole, H.frame_reflect(clean, None, n_fft, win, hop)[0])


# ---- ps_spec_pair_moments_rows_f64 -------------------------------------------------------------------------------------------------
T_ROWS = (1, 127, 128, 129, 255, 256, 257, 300)


@pytest.mark.parametrize("bins", [9, 33])
@pytest.mark.parametrize("junk", JUNK)
def test_spec_pair_moments_rows(H, dev, bins, junk):
    t, n = 300, len(T_ROWS)
    ldt = H.padded_frames(t)
    spec = torch.full((2 * n, 2 * bins, ldt), junk)
    body = _rand((2 * n, 2 * bins, t), 931)
    scale = torch.where(torch.arange(bins) % 4 == 1, 1e-5, 1.0)      # a quarter of the bins far below the clamp
    body *= torch.cat([scale, scale])[None, :, None]
    spec[..., :t] = body
    for i, tn in enumerate(T_ROWS):
        spec[i, :, tn:] = junk
        spec[n + i, :, tn:] = junk
    on_dev, lim = spec.to(dev), _limits(dev, T_ROWS)
    tchunks = (t + 255) // 256
    for p in (0.5, 1.0):
        got = H.spec_pair_moments_rows(on_dev, bins, t, lim, p)
        assert got.dtype == torch.float64 and tuple(got.shape) == (n, 4)
        for i, tn in enumerate(T_ROWS):
            s = body[[i, n + i], :, :tn].double().numpy()
            mags = np.sqrt(np.maximum(s[:, :bins] ** 2 + s[:, bins:] ** 2, R.CLAMP))
            err = R.rel_each(got[i:i + 1].cpu().numpy(), R.sums_of(mags[:1], mags[1:], p))
            print(f"bins={bins} p={p} T_n={tn} junk={junk}: S0..S3 largest relative error {err:.3e}")
            assert err < R.FP32_TOL, (i, tn, err)
        slots = H.spec_pair_moments_rows(on_dev, bins, t, lim, p, slots=True)
        assert tuple(slots.shape) == (n, H.lib().ps_spec_pair_moments_parts(bins, t), 4) and torch.equal(slots.sum(1), got)
        for i, tn in enumerate(T_ROWS):       # slot = bin group * tchunks + frame chunk: chunks at or behind T_n hold 0.0
            for c in range(tchunks):
                if c * 256 >= tn:
                    assert float(slots[i, c::tchunks].abs().max()) == 0.0, (i, tn, c)
        assert torch.equal(H.spec_pair_moments_rows(on_dev, bins, t, lim, p), got)
    # whole rows: the bits of the whole-row entry
    whole = torch.cat([body, torch.zeros(2 * n, 2 * bins, ldt - t)], -1).to(dev)
    assert torch.equal(H.spec_pair_moments_rows(whole, bins, t, _limits(dev, [t] * n)), H.spec_pair_moments(whole, bins, t))


def test_row_entries_refuse_bad_arguments(H, dev):
    x = torch.zeros(2, 64, device=dev)
    lim = _limits(dev, (64, 40))
    with pytest.raises(ValueError, match="int32 tensor"):
        H.wave_moments_rows(x, x, _limits(dev, (64, 40, 1)))
    with pytest.raises(RuntimeError, match="int32"):
        H.wave_moments_rows(x, x, lim.long())
    with pytest.raises(RuntimeError, match="int32"):
        H.align_rows(x, lim.cpu(), lim, 64)
    with pytest.raises(RuntimeError, match="length 32"):
        H.frame_reflect_rows(x[:, :32].contiguous(), None, lim, 64, 64, 16)
    with pytest.raises(RuntimeError, match="2N, 2\\*bins, ldt"):
        H.spec_pair_moments_rows(torch.zeros(2, 18, 128, device=dev), 8, 5, lim[:1])
    with pytest.raises(RuntimeError, match="bad argument"):
        H.spec_pair_moments_rows(torch.zeros(2, 18, 128, device=dev), 9, 129, lim[:1])


# ---- the losses with lengths ---------------------------------------------------------------------------------------------------------
def test_losses_with_lengths_on_the_device(S, PA, dev):
    enh, ref = (t.to(dev) for t in RS.batch())
    enh_nan, ref_nan = (t.to(dev) for t in RS.batch("nan"))
    mr = S.MultiResolutionSTFTLoss()
    sums = []
    for f, res in zip(mr.stft_losses, R.RESOLUTIONS):
        m = f.moments(enh, ref, lengths=LENS)
        err = R.rel_each(m.cpu().numpy(), RS.row_sums(res))
        print(f"{res}: S0..S3 per row against each utterance alone, largest relative error {err:.3e}")
        assert m.dtype == torch.float64 and m.device == enh.device and err < R.FP32_TOL
        assert torch.equal(f.moments(enh_nan, ref_nan, lengths=LENS), m), "NaN behind the rows: the same bits"
        sums.append(m)
    for p in R.OV_POWERS:
        m = S.STFTLoss(*R.OV_RESOLUTION).moments(enh, ref, p=p, lengths=LENS)
        assert R.rel_each(m.cpu().numpy(), RS.row_sums(R.OV_RESOLUTION, p)) < R.FP32_TOL
    total, ov = mr(enh, ref, lengths=LENS), S.over_suppression_loss_ragged(enh, ref, lengths=LENS)
    sc = [RS.batch_values(RS.row_sums(res), res) for res in R.RESOLUTIONS]
    want = R.FACTOR_SC * float(np.mean([v[0] for v in sc])) + R.FACTOR_MAG * float(np.mean([v[1] for v in sc]))
    want_ov = RS.batch_values(RS.row_sums(R.OV_RESOLUTION), R.OV_RESOLUTION)[2]
    print(f"multi-resolution {float(total):.8g} (ref {want:.8g}); over-suppression {float(ov):.8g} (ref {want_ov:.8g})")
    assert R.rel(float(total), want) < R.FP32_TOL and R.rel(float(ov), want_ov) < R.FP32_TOL
    assert torch.equal(mr(enh_nan, ref_nan, lengths=LENS), total)
    assert torch.equal(S.over_suppression_loss_ragged(enh_nan, ref_nan, lengths=LENS), ov)
    # what the kept scratch held changes no bit
    for buf in S._WORK.values():
        buf.fill_(NAN)
    assert torch.equal(mr(enh, ref, lengths=LENS), total) and torch.equal(S.over_suppression_loss_ragged(enh, ref, lengths=LENS), ov)
    for f, m in zip(mr.stft_losses, sums):
        assert torch.equal(f.moments(enh, ref, lengths=LENS), m)
    # whole rows: the row kernels keep the summation order of the whole-row kernels, so the same bits
    full = [RS.L] * RS.N
    for f in mr.stft_losses:
        assert torch.equal(f.moments(enh, ref, lengths=full), f.moments(enh, ref))
    assert torch.equal(mr(enh, ref, lengths=full), mr(enh, ref))
    assert torch.equal(S.over_suppression_loss_ragged(enh, ref, lengths=full), S.over_suppression_loss(enh, ref))
    # the SDR family
    labels = torch.tensor([False, False, True, False])
    order = [0, 1, 3, 2]
    e_cpu, r_cpu = RS.batch()
    for mode in ("sisnr", "sdsdr", "tsdr"):
        loss = PA.SDRLoss.init_mode(mode, reduction=False)
        got = loss(enh, ref, labels.to(dev), lengths=LENS)
        want = torch.cat([LO.sdr_loss(e_cpu[n:n + 1, :LENS[n]].double(), r_cpu[n:n + 1, :LENS[n]].double(), reduction=False,
                                      inactive_labels=labels[n:n + 1], **LO.mode_flags(mode)) for n in order])
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), atol=2e-3, rtol=0)
        assert torch.equal(loss(enh_nan, ref_nan, labels.to(dev), lengths=LENS), got)
    from puresound_amd.nnet.loss import sdr
    np.testing.assert_allclose(sdr.si_snr(enh, ref, reduction=False, lengths=LENS).cpu().numpy(),
                               torch.cat([LO.si_snr(e_cpu[n:n + 1, :v].double(), r_cpu[n:n + 1, :v].double(), reduction=False)
                                          for n, v in enumerate(LENS)]).numpy(), atol=2e-3, rtol=0)
    assert torch.equal(sdr.inactive_sdr_loss(enh_nan, ref_nan, reduction=False, lengths=LENS),
                       sdr.inactive_sdr_loss(enh, ref, reduction=False, lengths=LENS))


# ---- inference_scored_ragged -----------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(PA, dev, name):
    if name not in _MODELS:
        model = cases.build(PA.NS, name).eval()
        model.load_state_dict(E.weights(name)[0])
        _MODELS[name] = model.to(dev)
    return _MODELS[name]


def _problem(PA, dev, name, frames, enrol_frames, deltas, keep=None):
    """-> the ragged batch of ragged_ref (its rows `keep`) on the device, inference(..., lengths=...)'s result, a clean
    reference with ref_lengths[n] = out_n + deltas[n] samples per row and NaN behind them, and per row (estimate, aligned
    reference) on the CPU: the device's own waveform rows and the reference aligned by _align_waveform's rule"""
    model = _model(PA, dev, name)
    model.set_gemm_precision("fp32")
    noisy, lens, enroll, e_lens, _ = RB.batch(name, frames, enrol_frames)
    if keep is not None:
        noisy, lens, deltas = noisy[keep], [lens[n] for n in keep], [deltas[n] for n in keep]
    noisy, enroll = noisy.to(dev), None if enroll is None else enroll.to(dev)
    want = model.inference(noisy, enroll, lengths=lens, enroll_lengths=e_lens)
    out = model.output_lengths(lens)
    r_lens = [o + d for o, d in zip(out, deltas)]
    assert min(r_lens) >= 1
    clean = torch.full((len(lens), max(r_lens) + 3), NAN)
    for n, v in enumerate(r_lens):
        body = 0.7 * torch.nn.functional.pad(want[n, :out[n]].cpu(), (0, 64)) + 0.05 * det_wave(7400 + n, 1, out[n] + 64)[0]
        clean[n, :v] = body[:v]
    rows = [(want[n:n + 1, :out[n]].cpu(), RS.aligned_row(clean[n:n + 1, :r_lens[n]], out[n])) for n in range(len(lens))]
    return model, noisy, enroll, lens, e_lens, want, out, clean.to(dev), r_lens, rows


# ref_lengths shorter by 100, equal and longer by 64 than out_n across the rows; on the 32- and 48-sample rows a shortening
# smaller than the row
CFG2_DELTAS = (-100, -10, -10, 0, 64, -100)     # out_n = 4832, 32, 48, 2048, 2080, 4128
CFG3_DELTAS = (-100, 64, 0)                     # out_n = 4832, 48, 2080


@pytest.mark.parametrize("name,frames,enrol,deltas", [("cfg2_short", RB.CFG2_T, None, CFG2_DELTAS),
                                                      ("cfg3_short", RB.CFG3_T, RB.CFG3_ENROL_T, CFG3_DELTAS)])
def test_inference_scored_ragged_sdr_modes(PA, H, dev, name, frames, enrol, deltas):
    model, noisy, enroll, lens, e_lens, want, out, clean, r_lens, rows = _problem(PA, dev, name, frames, enrol, deltas)
    assert 48 in out and (32 in out) == (name == "cfg2_short")      # two frames; cfg2's batch also holds the one-frame row
    plain = noisy[:2, :E.length_of(name, 129)].contiguous()
    plain_enroll = None if enroll is None else enroll[:2].contiguous()
    plain_ref = clean[:2, :30].nan_to_num(0.0)
    before = model.inference_scored(plain, plain_ref, plain_enroll)
    n = len(lens)
    labels = torch.zeros(n, dtype=torch.bool)
    labels[-1] = True
    order = list(range(n - 1)) + [n - 1]
    for mode in ("sisnr", "sdsdr", "tsdr"):
        loss = PA.SDRLoss.init_mode(mode, reduction=False)
        enh, score = model.inference_scored_ragged(noisy, clean, enroll, loss, labels.to(dev), lengths=lens, ref_lengths=r_lens,
                                                   enroll_lengths=e_lens)
        assert torch.equal(enh, want)
        ref_score = torch.cat([LO.sdr_loss(rows[i][0].double(), rows[i][1].double(), reduction=False,
                                           inactive_labels=labels[i:i + 1], **LO.mode_flags(mode)) for i in order])
        print(f"{name} {mode}: {score.view(-1).tolist()}")
        np.testing.assert_allclose(score.cpu().numpy(), ref_score.numpy(), atol=2e-3, rtol=0)
        again = model.inference_scored_ragged(noisy, clean, enroll, loss, labels.to(dev), lengths=lens, ref_lengths=r_lens,
                                              enroll_lengths=e_lens)
        assert torch.equal(again[0], enh) and torch.equal(again[1], score), "two ragged scored calls: the same bits"
    # the aligned reference the scores read, as a tensor: the rows aligned on the CPU, exact zeros behind them
    aligned = H.align_rows(clean, _limits(dev, out), _limits(dev, r_lens), want.shape[1]).cpu()
    for i, (_, ref_row) in enumerate(rows):
        assert torch.equal(aligned[i, :out[i]], ref_row[0]) and not bool(aligned[i, out[i]:].any()), i
    # plain inference_scored on the same model: the same bits before and after
    after = model.inference_scored(plain, plain_ref, plain_enroll)
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])


def test_inference_scored_ragged_spectral_scores(PA, S, H, dev):
    """the rows with out_n > 32 (fft_size 64 needs more than 32 samples): an STFTLoss, a MultiResolutionSTFTLoss and a closure
    that takes lengths"""
    name = "cfg2_short"
    keep = [n for n, t in enumerate(RB.CFG2_T) if t >= 2]
    model, noisy, _, lens, _, want, out, clean, r_lens, rows = _problem(PA, dev, name, RB.CFG2_T, None, CFG2_DELTAS, keep)
    assert min(out) == 48
    aligned = H.align_rows(clean, _limits(dev, out), _limits(dev, r_lens), want.shape[1])
    one = S.STFTLoss(64, 16, 48)
    mr = S.MultiResolutionSTFTLoss([64, 32], [16, 8], [48, 32])
    for f, res in [(one, (64, 16, 48))] + list(zip(mr.stft_losses, [(64, 16, 48), (32, 8, 32)])):
        m = f.moments(want, aligned, lengths=out).cpu().numpy()
        for i, (e, r) in enumerate(rows):
            err = R.rel_each(m[i:i + 1], R.sums(e.numpy(), r.numpy(), *res))
            print(f"{res} row {i} (out_n = {out[i]}): S0..S3 largest relative error {err:.3e}")
            assert err < R.FP32_TOL, (res, i, err)
    enh, (sc, mag) = model.inference_scored_ragged(noisy, clean, loss_func=one, lengths=lens, ref_lengths=r_lens)
    s = np.concatenate([R.sums(e.numpy(), r.numpy(), 64, 16, 48) for e, r in rows])
    count = 33 * sum(R.frames(v, 64, 16) for v in out)
    assert torch.equal(enh, want)
    assert R.rel(float(sc), float(np.sqrt(s[:, 0].sum()) / np.sqrt(s[:, 1].sum()))) < R.FP32_TOL
    assert R.rel(float(mag), float(s[:, 2].sum() / count)) < R.FP32_TOL
    assert all(torch.equal(a, b) for a, b in zip((sc, mag), one(want, aligned, lengths=out)))
    enh, total = model.inference_scored_ragged(noisy, clean, loss_func=mr, lengths=lens, ref_lengths=r_lens)
    assert torch.equal(enh, want) and torch.equal(total, mr(want, aligned, lengths=out))
    vals = []
    for res in ((64, 16, 48), (32, 8, 32)):
        s = np.concatenate([R.sums(e.numpy(), r.numpy(), *res) for e, r in rows])
        count = (res[0] // 2 + 1) * sum(R.frames(v, res[0], res[1]) for v in out)
        vals.append((np.sqrt(s[:, 0].sum()) / np.sqrt(s[:, 1].sum()), s[:, 2].sum() / count))
    want_total = 0.1 * float(np.mean([v[0] for v in vals])) + 0.1 * float(np.mean([v[1] for v in vals]))
    print(f"multi-resolution through the wrapper: {float(total):.8g} (ref {want_total:.8g})")
    assert R.rel(float(total), want_total) < R.FP32_TOL

    def closure(est, ref, unused, lengths=None):
        return mr(est, ref, lengths=lengths) + S.over_suppression_loss_ragged(est, ref, fft_size=64, hop_size=16, win_length=64,
                                                                       lengths=lengths)
    enh, score = model.inference_scored_ragged(noisy, clean, loss_func=closure, lengths=lens, ref_lengths=r_lens)
    assert torch.equal(enh, want) and torch.equal(score, closure(want, aligned, None, lengths=out))
    # the same closure on CPU tensors (stock ATen, the rows one by one): the device path within the fp32 class
    assert R.rel(float(score), float(closure(want.cpu(), aligned.cpu(), None, lengths=out))) < R.FP32_TOL


def test_refusals_on_device_tensors_launch_nothing(PA, S, dev, monkeypatch):
    from puresound_amd import hip as hip_module
    model = _model(PA, dev, "cfg2_short")
    noisy, clean = torch.zeros(2, 400, device=dev), torch.zeros(2, 400, device=dev)

    def lib():
        raise AssertionError("the HIP library was called")
    monkeypatch.setattr(hip_module, "lib", lib)
    with pytest.raises(ValueError, match="exceeds the row length"):
        model.inference_scored_ragged(noisy, clean, lengths=[400, 401])
    with pytest.raises(ValueError, match=r"ref_lengths\[1\] = 0 must be at least 1"):
        model.inference_scored_ragged(noisy, clean, lengths=[400, 400], ref_lengths=[400, 0])
    with pytest.raises(RuntimeError, match=r"lengths\[1\] = 32 with fft_size 64"):
        model.inference_scored_ragged(noisy, clean, loss_func=S.STFTLoss(64, 16, 48), lengths=[400, 40])
    with pytest.raises(NotImplementedError, match="must take `lengths`"):
        model.inference_scored_ragged(noisy, clean, loss_func=R.stft_ov_closure(S), lengths=[400, 400])
    with pytest.raises(RuntimeError, match=r"lengths\[0\] = 32 with fft_size 64"):
        S.MultiResolutionSTFTLoss([32, 64], [8, 16], [32, 48])(noisy, clean, lengths=[32, 400])   # passes 32, not 64
    with pytest.raises(ValueError, match="must be at least 1"):
        PA.SDRLoss.init_mode("sisnr")(noisy, clean, lengths=[400, 0])
