"""The shared batch and float64 references of the ragged-score tests (test_ragged_scores.py, test_ragged_scores_gpu.py).

Batch: N = 4 rows of L = 4000 samples holding utterances of 4000 / 1025 / 2000 / 3001 samples (1025 = 2048 // 2 + 1 is the
shortest legal length of the 2048 resolution), inputs of stft_loss_ref's kind -- the reference det_wave rows at 0.3 amplitude,
the estimate 0.7 ref + 0.2 other -- and behind each utterance junk at 20 x that amplitude, NaN, or zeros.  Per row the sums
S0..S3 are those of stft_loss_ref (the float64 restatement of the reference) on the utterance alone: computed once, shared,
never written to."""
import functools

import numpy as np
import torch

import stft_loss_ref as R
from detweights import det_wave

N, L = 4, 4000
LENGTHS = (4000, 1025, 2000, 3001)
AMP = 0.3
JUNK_GAIN = 20.0


@functools.lru_cache(maxsize=None)
def batch(junk="noise"):
    """-> (estimate, reference) fp32 [N, L]; junk: "noise" (20 x the amplitude), "nan" or "zero" behind each utterance"""
    ref = det_wave(7300, N, L, amp=AMP)
    enh = 0.7 * ref + 0.2 * det_wave(7301, N, L, amp=AMP)
    fill = {"noise": lambda seed: det_wave(seed, N, L, amp=AMP * JUNK_GAIN),
            "nan": lambda seed: torch.full((N, L), float("nan")),
            "zero": lambda seed: torch.zeros(N, L)}[junk]
    behind = torch.arange(L)[None, :] >= torch.tensor(LENGTHS)[:, None]
    return torch.where(behind, fill(7302), enh), torch.where(behind, fill(7303), ref)


def rows():
    """-> [(estimate, reference) float64 numpy [1, lengths[n]]]: every utterance alone"""
    enh, ref = batch()
    return [(enh[n:n + 1, :v].numpy(), ref[n:n + 1, :v].numpy()) for n, v in enumerate(LENGTHS)]


@functools.lru_cache(maxsize=None)
def row_sums(res, p=0.5):
    """float64 [N, 4]: S0..S3 of each utterance alone at the resolution (fft_size, hop, win)"""
    return np.concatenate([R.sums(x, y, *res, p=p) for x, y in rows()])


def frame_counts(res):
    return [R.frames(v, res[0], res[1]) for v in LENGTHS]


def batch_values(s, res):
    """(sc, mag, ov) of the batch from the per-row sums [N, 4], over the elements that exist"""
    count = (res[0] // 2 + 1) * sum(frame_counts(res))
    return (float(np.sqrt(s[:, 0].sum()) / np.sqrt(s[:, 1].sum())), float(s[:, 2].sum() / count),
            float(s[:, 3].sum() / count))


def aligned_row(ref_row, out_n):
    """_align_waveform's rule on one row [1, b] -> [1, out_n]: shorter left-padded with zeros, longer cut"""
    b = ref_row.shape[-1]
    return torch.nn.functional.pad(ref_row, (out_n - b, 0)) if b < out_n else ref_row[..., :out_n]
