"""Every model family with checkpoint-like weights (detweights mode "trained") against the float64 oracle: the presets, inputs,
cached oracle results, metrics and bounds shared by test_trained_weights.py (CPU) and test_trained_weights_gpu.py.

The law: norm gains 2^-2 .. 2^2, biases in +-1, PReLU slopes 0.05 .. 1.5, four rows of every weight matrix of 16 rows or more
scaled by 2^4, 2^-4, 2^3, 2^-3 (detweights._trained).  Formula weights put every range of the fp16x2 arithmetic at its easiest
point -- gains near 1, all rows of a matrix alike -- and "wild" (cfg2_wild_short, cfg3_wild_short) overflows or loses the
conditioning of every family but the Conv-TasNet TCN; this one keeps the float32 restatement of the oracle within 3.6e-6 of
the float64 one on eleven of the twelve presets and within 1.4e-5 on cfg3_causal_short (SELF_NOISE), so the project's 1e-4
keeps its meaning.  cfg3_causal_short's noise is its masker's: a float32 masker fed the float64 features and embedding shows
all of it (3e-5 on the mask), the embedding 6e-7, and the same weights in the gLN preset cfg3_short 5e-7.  Its bN1d norms are
fixed affine maps in eval mode, so nothing rescales the residual stream between the 24 blocks: under gains up to 4 the mask
reaches 6.5e4 at a median of 37, and every rounding is relative to the largest values.  Hence that preset's "fp32" bound is the
capped 1e-4, not 2e-5.

What is compared is the waveform BEFORE the output clamp (at amplitude 0.05 it reaches 3.5e6 in DPCRN / DPARN: the clamp would
flatten nearly all of it), with the preset's own mask constraint, and the speaker embedding where a preset has a speaker net.
The mixture is det_wave(901, B, 4000) at amplitude amp, the enrolment det_wave(902, B, 3000) likewise, amp in AMPS.

Metrics are edge_length_cases.errors: rel_max after the 16-sample cut for STFT presets, and for those also the window-weighted
one.  Bounds: PROJECT_TOL for "bf16x3" and "fp16x2"; for "fp32" max(FP32_TOL, 20 x SELF_NOISE[preset]), never above
PROJECT_TOL -- 20 x is the room edge_length_cases.py argues for between the float32 oracle and a float32 kernel chain (another
summation order, tanhf / expf over ~100 layers)."""
import functools

import numpy as np
import torch

import cases
import edge_length_cases as E
from conftest import rel_max
from detweights import det_state_dict, det_wave
from oracle import separator_oracle as O

PRESETS = ("cfg1_short", "cfg2_short", "cfg3_causal_short", "cfg4_short", "cfg4_tse_short", "tse_skim_v0_short",
           "tse_skim_v1_short", "tse_skim_causal_short", "ns_dpcrn_short", "ns_dparn_short", "tse_unet_tcn_short",
           "tse_unet_tcn_causal_short")
AMPS = (1e-3, 0.05)
SENS_AMP = 0.1          # the amplitude of the sensitivity check
BATCH = 2
LENGTH = 4000
L_ENROLL = 3000
PRECISIONS = ("fp32", "bf16x3", "fp16x2")
FP32_TOL = E.FP32_TOL
PROJECT_TOL = E.PROJECT_TOL

# The float32 oracle against the float64 one, worst of both amplitudes and of the preset's metrics, as recorded in
# profiles/trained_weights.txt (test_trained_weights.py re-measures it and holds it against this table).
SELF_NOISE = {"cfg1_short": 5.5e-7, "cfg2_short": 6.3e-7, "cfg3_causal_short": 1.4e-5, "cfg4_short": 7.4e-7,
              "cfg4_tse_short": 7.9e-7, "tse_skim_v0_short": 1.6e-6, "tse_skim_v1_short": 1.2e-6,
              "tse_skim_causal_short": 1.3e-6, "ns_dpcrn_short": 8.4e-7, "ns_dparn_short": 8.9e-7,
              "tse_unet_tcn_short": 1.4e-6, "tse_unet_tcn_causal_short": 3.6e-6}


# Per-utterance ranges: one family each of TCN, DPRNN, SkiM (the non-causal one: the causal preset hands the last segment state
# of utterance n - 1 to utterance n, as the reference does, so only its first row has a run on its own), DPCRN, U-Net + TCN.
RANGE_PRESETS = ("cfg2_short", "cfg4_tse_short", "tse_skim_v0_short", "ns_dpcrn_short", "tse_unet_tcn_causal_short")
RANGE_AMP = 0.05
QUIET = 1e-3            # the middle row of the batch of 3 against its neighbours
# A row inside a batch against the same row on its own: test_scratch_state_gpu.py allows 1e-5 on a waveform whose full scale is
# the clamp's 1; in front of the clamp the row's own largest sample is the scale.
ROW_TOL = 1e-5

# The streamers emit the clamped waveform only, and rel_max on a clamped waveform is max|pre-clamp| times the one in front of
# the clamp (its largest sample is 1).  So each class streams at the largest power of ten (0.05 for the two quiet presets) at
# which the float64 oracle's waveform, inside the project's 16-sample cut, stays inside the clamp: there both are the same
# number (test_trained_weights.py holds the table against the oracle).  class -> (preset, amplitude)
STREAMED = {"tcn": ("cfg3_causal_short", 1e-5), "dprnn": ("cfg4_tse_short", 0.05), "skim": ("tse_skim_causal_short", 0.05),
            "spectral": ("ns_dpcrn_short", 1e-6), "unet_tcn": ("tse_unet_tcn_causal_short", 1e-4)}
STREAM_TOL = 1e-4       # test_streamed_matches_reference_golden of every class


def stream_problem(kind):
    """-> (preset, mixture, enrolment or None, the float64 oracle's results on every utterance alone, as the streamers run them)"""
    name, amp = STREAMED[kind]
    noisy, enroll, ref = problem(name, amp, BATCH, None, True)
    top = float(E.inner(name, ref["pre"]).abs().max())
    assert 0.05 <= top <= 1.0, (kind, top)   # inside the clamp, and of ordinary size
    return name, noisy, enroll, ref


def is_stft(name):
    return E.is_stft(name)


def has_enrolment(name):
    return E.has_enrolment(name)


def has_speaker_net(name):
    return "speaker_net" in cases.CASES[name]


def all_cases():
    return [(n, a) for n in PRESETS for a in AMPS]


@functools.lru_cache(maxsize=None)
def weights(name):
    """-> (float32 state dict, float64 state dict) of the preset under the trained law"""
    import puresound_amd.nnet as PA
    sd = det_state_dict(cases.build(PA.NS, name), mode="trained")
    return sd, {k: v.double() for k, v in sd.items()}


def inputs(name, amp, batch=BATCH, quiet_row=None):
    """-> (mixture [B, L], enrolment [B, Le] or None); quiet_row: that utterance, mixture and enrolment, QUIET times as loud"""
    noisy = det_wave(901, batch, LENGTH, amp)
    enroll = det_wave(902, batch, L_ENROLL, amp) if has_enrolment(name) else None
    if quiet_row is not None:
        noisy[quiet_row] *= QUIET
        if enroll is not None:
            enroll[quiet_row] *= QUIET
    return noisy, enroll


def oracle_cfg(name):
    """The preset as the oracle reads it; the clamp of the "linear" output constraint is bypassed by reading the oracle's
    pre-clamp tap."""
    cfg = cases.oracle_cfg(name)
    cfg["output_constraint"] = "linear"
    return cfg


def run_oracle(name, noisy, enroll, sd):
    """-> {"pre": waveform before the output clamp, "mask": the mask, "dvec": speaker embedding or None} in sd's dtype"""
    dtype = next(iter(sd.values())).dtype
    taps = {}
    with torch.no_grad():
        O.inference(noisy.to(dtype), sd, oracle_cfg(name), None if enroll is None else enroll.to(dtype), taps)
    assert taps["wav_preclamp"].dtype == dtype
    return {"pre": taps["wav_preclamp"], "mask": taps["mask"], "dvec": taps["dvec"] if has_speaker_net(name) else None}


@functools.lru_cache(maxsize=None)
def problem(name, amp, batch=BATCH, quiet_row=None, rows_alone=False):
    """-> (mixture, enrolment or None, the float64 oracle's results): computed once, handed out to every test that asks, and
    never written to.  rows_alone: the oracle on every utterance as a batch of one (what the streamers compute: no state
    passes from one stream to the next)."""
    noisy, enroll = inputs(name, amp, batch, quiet_row)
    if rows_alone:
        parts = [run_oracle(name, noisy[b:b + 1], None if enroll is None else enroll[b:b + 1], weights(name)[1])
                 for b in range(batch)]
        ref = {k: None if parts[0][k] is None else torch.cat([p[k] for p in parts]) for k in parts[0]}
    else:
        ref = run_oracle(name, noisy, enroll, weights(name)[1])
    assert ref["pre"].dtype == torch.float64 and ref["pre"].shape[0] == batch
    assert bool(torch.isfinite(ref["pre"]).all()) and bool(torch.isfinite(ref["mask"]).all())
    return noisy, enroll, ref


def errors(name, got, ref):
    """-> {metric: value} of a pre-clamp waveform against the reference's (edge_length_cases.errors)"""
    return E.errors(name, got, ref)


def embedding_error(got, ref):
    return rel_max(np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64))


def bound(name, precision):
    """The bound on every metric of the preset, and on its speaker embedding, in the arithmetic `precision`."""
    if precision == "fp32":
        return min(PROJECT_TOL, max(FP32_TOL, 20.0 * SELF_NOISE[name]))
    assert precision in ("bf16x3", "fp16x2")
    return PROJECT_TOL


def fp16_rounded(sd):
    """What a dropped second fp16 term costs: every weight of two or more dimensions under masker. / speaker_net. rounded
    to fp16."""
    return {k: (v.to(torch.float16).to(v.dtype) if v.dim() >= 2 and k.startswith(("masker.", "speaker_net.")) else v)
            for k, v in sd.items()}
