"""Float64 restatement of the reference's loss/stft_loss.py, with the inputs and cases shared by test_stft_loss.py (CPU),
test_stft_loss_gpu.py and tests/golden/make_stft_loss_golden.py.

The transform is written out: explicit reflect indexing, the window zero-padded to fft_size and centred, frames t * hop,
numpy's rfft -- torch.stft(center=True, pad_mode="reflect") without calling it.  With x / y the clamped magnitudes of
estimate / reference the four sums per utterance are S0 = sum (y-x)^2, S1 = sum y^2, S2 = sum |log y - log x|,
S3 = sum relu(y^p - x^p)^2, and the scores are algebra on them over the whole batch.

Inputs: x = det_wave rows at 0.3 amplitude, y = 0.7 x + 0.2 other, so that no sum is a small difference of large terms.
Case "quiet" adds what a clamp and a zero denominator can get wrong: an all-zero reference row and a pair that is silent in
its second half."""
import functools

import numpy as np
import torch

from detweights import det_wave

CLAMP = 1e-7
RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))   # MultiResolutionSTFTLoss's defaults
OV_RESOLUTION = (512, 128, 512)                                       # over_suppression_loss's defaults
OV_POWERS = (0.5, 1.0)
MAG_RESOLUTION = (64, 16, 40)                                         # the magnitudes the fixture records (case "short")
FACTOR_SC = FACTOR_MAG = 0.1
CASES = {"plain": (3, 4000), "quiet": (3, 4000), "short": (1, 1025)}  # name: (N, L); 1025 = 2048 // 2 + 1, the shortest legal
LONG = (2, 7999)                                                      # not in the fixture: restatement only


@functools.lru_cache(maxsize=None)
def pair(name):
    """-> (estimate, reference) fp32 [N, L]; never written to."""
    n, length = CASES[name] if name in CASES else LONG
    seed = 7100 + 10 * (sorted(CASES).index(name) if name in CASES else len(CASES))
    x = det_wave(seed, n, length, amp=0.3)
    y = 0.7 * x + 0.2 * det_wave(seed + 1, n, length, amp=0.3)
    if name == "quiet":
        y[1] = 0.0
        x[2, length // 2:] = 0.0
        y[2, length // 2:] = 0.0
    return x, y


def hann(win):
    """The module's window buffer (fp32 torch.hann_window) as float64."""
    return torch.hann_window(win).double().numpy()


def frames(length, n_fft, hop):
    """Whole frames of n_fft samples, hop apart, in the length + 2 (n_fft // 2) samples of the reflect-padded signal: for an odd
    n_fft one fewer than 1 + length // hop when hop divides the length."""
    return 1 + (length + 2 * (n_fft // 2) - n_fft) // hop


def magnitudes(x, n_fft, hop, win, window=None):
    """x [N, L] -> float64 clamped magnitudes [N, frames(L, n_fft, hop), n_fft // 2 + 1]"""
    x = np.asarray(x, dtype=np.float64)
    length, pad = x.shape[1], n_fft // 2
    assert length > pad and win <= n_fft
    idx = np.abs(np.arange(-pad, length + pad))
    idx = np.where(idx >= length, 2 * (length - 1) - idx, idx)
    w = np.zeros(n_fft)
    off = (n_fft - win) // 2
    w[off:off + win] = hann(win) if window is None else np.asarray(window, dtype=np.float64)
    t = frames(length, n_fft, hop)
    frames_ = x[:, idx][:, (np.arange(t) * hop)[:, None] + np.arange(n_fft)[None, :]] * w
    spec = np.fft.rfft(frames_, axis=-1)
    return np.sqrt(np.maximum(spec.real ** 2 + spec.imag ** 2, CLAMP))


def sums_of(x_mag, y_mag, p=0.5):
    """-> float64 [N, 4] = (S0, S1, S2, S3)"""
    x_mag, y_mag = np.asarray(x_mag, dtype=np.float64), np.asarray(y_mag, dtype=np.float64)
    over = np.maximum(y_mag ** p - x_mag ** p, 0.0)
    return np.stack([((y_mag - x_mag) ** 2).sum((1, 2)), (y_mag ** 2).sum((1, 2)),
                     np.abs(np.log(y_mag) - np.log(x_mag)).sum((1, 2)), (over ** 2).sum((1, 2))], axis=-1)


def sums(x, y, n_fft, hop, win, p=0.5):
    return sums_of(magnitudes(x, n_fft, hop, win), magnitudes(y, n_fft, hop, win), p)


def count(length, n_fft, hop):
    """elements of one utterance's spectrogram"""
    return frames(length, n_fft, hop) * (n_fft // 2 + 1)


def sc_mag(s, per_row):
    """(spectral convergence, log-magnitude distance) of a batch from its sums [N, 4]"""
    return float(np.sqrt(s[:, 0].sum()) / np.sqrt(s[:, 1].sum())), float(s[:, 2].sum() / (s.shape[0] * per_row))


@functools.lru_cache(maxsize=None)
def scores(name):
    """-> {"sums": {resolution: [N, 4] at p = 0.5}, "sc": [3], "mag": [3], "mr": float, "ov": {p: float},
           "ov_sums": {p: [N, 4]}} of a case's pair, in float64"""
    x, y = pair(name)
    length = x.shape[1]
    out = {"sums": {}, "sc": [], "mag": [], "ov": {}, "ov_sums": {}}
    for res in RESOLUTIONS:
        s = out["sums"][res] = sums(x.numpy(), y.numpy(), *res)
        sc, mag = sc_mag(s, count(length, res[0], res[1]))
        out["sc"].append(sc)
        out["mag"].append(mag)
    out["mr"] = FACTOR_SC * float(np.mean(out["sc"])) + FACTOR_MAG * float(np.mean(out["mag"]))
    for p in OV_POWERS:
        s = out["ov_sums"][p] = sums(x.numpy(), y.numpy(), *OV_RESOLUTION, p=p)
        out["ov"][p] = float(s[:, 3].sum() / (s.shape[0] * count(length, OV_RESOLUTION[0], OV_RESOLUTION[1])))
    return out


def rel(got, want):
    """max |got - want| / max |want| over an array, or the relative error of a scalar"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def rel_each(got, want):
    """element by element |got - want| / |want|, the largest (for sums of very different sizes per row)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max())


# Bounds, none of them new: GOLDEN_TOL is test_hip_parity.TOL (against recorded fp32 values of the reference), FP32_TOL the
# fp32 class of edge_length_cases (against the float64 restatement).
GOLDEN_TOL = 1e-4
FP32_TOL = 2e-5


def check_scores(S, name, golden, move=lambda t: t):
    """Every score of the module S (puresound_amd.nnet.loss.stft_loss) on a case's pair, moved by `move`, against the
    restatement (FP32_TOL) and, for the fixture's cases, the recorded values (GOLDEN_TOL): sc_r, mag_r, the total, ov at both
    powers, S0..S3 per row.  Each figure is printed before it is asserted."""
    x, y = (move(t) for t in pair(name))
    want = scores(name)
    recorded = name in CASES
    mr = S.MultiResolutionSTFTLoss()
    assert [(f.fft_size, f.shift_size, f.win_length) for f in mr.stft_losses] == list(RESOLUTIONS)
    for i, (f, res) in enumerate(zip(mr.stft_losses, RESOLUTIONS)):
        sc, mag = f(x, y)
        assert sc.dtype == torch.float32 and mag.dtype == torch.float32 and sc.dim() == 0 and sc.device == x.device
        print(f"{name} {res}: sc {float(sc):.8g} (ref {want['sc'][i]:.8g}) mag {float(mag):.8g} (ref {want['mag'][i]:.8g})")
        assert rel(float(sc), want["sc"][i]) < FP32_TOL and rel(float(mag), want["mag"][i]) < FP32_TOL
        if recorded:
            assert rel(float(sc), golden[f"{name}.sc"][i]) < GOLDEN_TOL
            assert rel(float(mag), golden[f"{name}.mag"][i]) < GOLDEN_TOL
        m = f.moments(x, y)
        assert m.dtype == torch.float64 and tuple(m.shape) == (x.shape[0], 4) and m.device == x.device
        err = rel_each(m.cpu().numpy(), want["sums"][res])
        print(f"    S0..S3 per row, largest relative error {err:.3e}")
        assert err < FP32_TOL
    total = mr(x, y)
    assert total.dtype == torch.float32 and total.dim() == 0
    print(f"{name} multi-resolution: {float(total):.8g} (ref {want['mr']:.8g})")
    assert rel(float(total), want["mr"]) < FP32_TOL
    if recorded:
        assert rel(float(total), golden[f"{name}.mr"]) < GOLDEN_TOL
    ov_loss = S.STFTLoss(*OV_RESOLUTION)
    for i, p in enumerate(OV_POWERS):
        ov = S.over_suppression_loss(x, y, p=p)
        err = rel_each(ov_loss.moments(x, y, p=p).cpu().numpy(), want["ov_sums"][p])
        print(f"{name} ov p={p}: {float(ov):.8g} (ref {want['ov'][p]:.8g}); S0..S3 per row {err:.3e}")
        assert rel(float(ov), want["ov"][p]) < FP32_TOL
        if recorded:
            assert rel(float(ov), golden[f"{name}.ov"][i]) < GOLDEN_TOL
        assert err < FP32_TOL


def stft_ov_closure(S):
    """What the recipes' `sig_loss: stft_ov` stands for: the multi-resolution value plus over_suppression_loss, as a callable of
    (estimate, reference, labels), the three arguments of the wrapper's forward."""
    mr = S.MultiResolutionSTFTLoss()

    def score(est, clean, labels):
        return mr(est, clean) + S.over_suppression_loss(est, clean)
    return score
