"""One preset per kernel family at the utterance lengths where a length turns into other kernel arguments: the cases,
inputs, float64 oracle results and metrics shared by test_edge_lengths.py (CPU) and test_edge_lengths_gpu.py.

Frames, not samples, name a case: T frames of the preset's encoder are L = win + hop * (T - 1) + r samples, r = hop // 2 + 1
for an odd T (a ragged tail the model must ignore) and 0 for an even one; the output has (T - 1) * hop + win samples.
FREE_T brackets one frame, the DPRNN segment (20), the 128-frame row and tile, the SkiM segment (150) and two SkiM segments
plus one; STFT_T brackets one frame, the transposed convolutions' trim, the 4-frame overlap of the 512 / 128 window and the
128-frame row.

The mixture is det_wave(901) * 0.05: at full scale the output clamp hides most of the waveform (it flattens 12-28 % of
cfg2_short's samples and up to 61 % of cfg1_short's), at 0.05 it touches no free-encoder case and at most 2.8 % of an STFT
case (cfg1_short at T = 2).  CLAMP_CAP is asserted on the oracle's output wherever it is the reference.

Metrics: rel_max (conftest.py) after the project's 16-sample cut for STFT encoders, and for those also weighted_rel_max.
The iSTFT divides by the overlap-added squared window, which is tiny near both ends, so a few samples just past the cut carry
max|ref| (0.7-1.0 against a median |ref| of 0.002-0.04) and rel_max passes body errors of several per cent.  The weighted
metric multiplies error and reference by min(1, wss / 1.5), the window sum over its steady-state value, and cuts nothing.

Bounds, none of them new: FP32_TOL is the FP32 class of test_abi_kernels_gpu.py (the float32 restatement of the oracle is
within 1.0e-6 of the float64 one on this ladder, so 2e-5 leaves about 20 x for another summation order and tanhf / expf over
~100 chained layers), FP16X2_TOL and PROJECT_TOL are test_hip_parity.TOL."""
import functools

import numpy as np
import torch

import cases
from conftest import rel_max
from detweights import det_state_dict, det_wave
from oracle import separator_oracle as O

PRESETS = ("cfg2_short",                  # gLN TCN
           "cfg3_causal_short",           # causal bN1d TCN + speaker net + ASP; fp16x2 through measured maxima
           "cfg4_tse_short",              # DPRNN, embedding-free TSE
           "tse_skim_causal_short",       # SkiM, H = 256 recurrences
           "cfg1_short",                  # STFT + complex mask
           "ns_dpcrn_short",              # conv2d + frame-major H = 128 LSTM
           "ns_dparn_short",              # self-attention
           "tse_unet_tcn_causal_short")   # U-Net + gated TCN + magnitude speaker net
FREE_T = (1, 2, 3, 19, 20, 21, 41, 127, 128, 129, 149, 150, 151, 301)
STFT_T = (1, 2, 3, 4, 5, 33, 127, 128, 129)
ENROL_T = (1, 2, 128, 129)
ODD_BATCHES = (1, 3, 17)
CPU_T = (1, 3, 129)

AMP = 0.05
L_ENROLL = 3000
EDGE = 16            # samples the project cuts at both ends of an iSTFT output before rel_max
CLAMP_CAP = 0.03
FP32_TOL = 2e-5
FP16X2_TOL = 1e-4
PROJECT_TOL = 1e-4
PRECISIONS = ("fp32", "fp16x2")


def is_stft(name):
    return cases.CASES[name]["enc"]["kind"] == "stft"


def has_enrolment(name):
    return "L_enroll" in cases.CASES[name]


ENROL_PRESETS = tuple(n for n in PRESETS if has_enrolment(n))


def ladder(name):
    return STFT_T if is_stft(name) else FREE_T


def mid_frames(name):
    """The mixture of the enrolment and batch cases: one frame past a DPRNN segment / past the window's overlap."""
    return 5 if is_stft(name) else 21


def win_hop(name):
    enc = cases.CASES[name]["enc"]
    return (enc["n_fft"] if is_stft(name) else enc["win"]), enc["hop"]


def length_of(name, t):
    win, hop = win_hop(name)
    return win + hop * (t - 1) + (hop // 2 + 1 if t % 2 else 0)


def out_length(name, t):
    win, hop = win_hop(name)
    return (t - 1) * hop + win


def walk_order(name):
    """The ladder from both ends: longest, shortest, second longest, second shortest, ..."""
    rest = sorted(ladder(name))
    order = []
    while rest:
        order.append(rest.pop(-1))
        if rest:
            order.append(rest.pop(0))
    return tuple(order)


def all_cases():
    return [(n, t) for n in PRESETS for t in ladder(n)]


@functools.lru_cache(maxsize=None)
def weights(name):
    """-> (float32 state dict, float64 state dict) of the preset, by det_state_dict"""
    import puresound_amd.nnet as PA
    sd = det_state_dict(cases.build(PA.NS, name))
    return sd, {k: v.double() for k, v in sd.items()}


def inputs(name, length, batch, enrol_length=L_ENROLL, row=None):
    """-> (mixture [B, L], enrolment [B, Le] or None).  `row`: that one utterance of a batch of row + 1, on its own."""
    def wave(seed, n_samples):
        if row is None:
            return det_wave(seed, batch, n_samples) * AMP
        assert batch == 1
        return (det_wave(seed, row + 1, n_samples) * AMP)[row:row + 1].clone()
    return wave(901, length), (wave(902, enrol_length) if has_enrolment(name) else None)


@functools.lru_cache(maxsize=None)
def problem(name, length, batch, enrol_length=L_ENROLL, row=None):
    """-> (mixture, enrolment or None, the float64 oracle's output): computed once, handed out to every test that asks, and
    never written to."""
    noisy, enroll = inputs(name, length, batch, enrol_length, row)
    with torch.no_grad():
        ref = O.inference(noisy.double(), weights(name)[1], cases.oracle_cfg(name),
                          None if enroll is None else enroll.double())
    assert ref.dtype == torch.float64 and ref.shape[0] == batch
    return noisy, enroll, ref


def frames_of(name, n_samples_out):
    win, hop = win_hop(name)
    assert (n_samples_out - win) % hop == 0
    return (n_samples_out - win) // hop + 1


def window_weight(t, n_fft=512, hop=128):
    """s[g] = min(1, wss[g] / 1.5): wss the overlap-added squared Hann window of t frames, 1.5 its steady-state value at a
    hop of a quarter window."""
    wss = O.window_sumsquare(torch.hann_window(n_fft, dtype=torch.float64), t, hop)
    return torch.clamp(wss / 1.5, max=1.0).numpy()


def weighted_rel_max(got, ref, t):
    s = window_weight(t)
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and ref.shape[-1] == s.shape[0]
    return float((np.abs(got - ref) * s).max() / max((np.abs(ref) * s).max(), 1e-30))


def inner(name, x):
    """What the project's metric looks at: everything, or an iSTFT output without its 16 samples at either end."""
    return x[..., EDGE:x.shape[-1] - EDGE] if is_stft(name) else x


def clamped_share(name, ref):
    return float((np.abs(inner(name, np.asarray(ref))) >= 1.0).mean())


def errors(name, got, ref):
    """-> {metric: value} of a result against a reference of the same shape"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    out = {"rel_max": rel_max(inner(name, got), inner(name, ref))}
    if is_stft(name):
        out["weighted"] = weighted_rel_max(got, ref, frames_of(name, ref.shape[-1]))
    return out


def bounds(name, precision):
    """-> {metric: bound} for the arithmetic "fp32" or "fp16x2" """
    tight = {"fp32": FP32_TOL, "fp16x2": FP16X2_TOL}[precision]
    return {"rel_max": PROJECT_TOL, "weighted": tight} if is_stft(name) else {"rel_max": tight}
