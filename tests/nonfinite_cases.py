"""Non-finite input scenarios shared by tests/golden/make_nonfinite_golden.py (reference side) and the tests that read its
fixtures (oracle, CPU path, HIP path): which wrapper cases, which inputs, where the bad sample goes, and how a mask is
written down.  Masks are runs `[row, start, stop)` of a [B, L] boolean array."""
import functools
import json
import os

import numpy as np
import torch

import cases
from detweights import det_state_dict, det_wave

# every end-to-end wrapper case short enough to run six times on the CPU (the "trained"-law copies of the presets are models
# already in the list with other parameter values: where a NaN goes does not depend on them, and "wild" covers the ranges)
CASES = [n for n, c in cases.CASES.items() if c["kind"] == "wrap" and c["L"] <= 20000 and c.get("weights") != "trained"]
# the egs presets (tools/preset_sweep.py: PRESETS), the cases of lookahead.json
PRESETS = ["cfg1_short", "cfg2_short", "cfg3_short", "cfg3_causal_short", "cfg4_short", "cfg4_tse_short", "ns_dpcrn_short",
           "ns_dparn_short", "tse_unet_tcn_short", "tse_unet_tcn_causal_short", "tse_unet_tcn_v1_short", "tse_skim_v0_short",
           "tse_skim_v1_short", "tse_skim_v2_short", "tse_skim_causal_short", "tse_skim_fbank_short", "tse_skim_vad_short"]
TOL = 1e-4  # the parity tolerance of every one of these cases (test_hip_parity.py / test_round3_gpu.py / test_cpu_path.py)


def clean_inputs(name):
    """(noisy, enroll or None) exactly as make_golden.run_wrap draws them; the one single-utterance case gets a second row,
    so that every batch has a row the bad sample is not in."""
    c = cases.CASES[name]
    noisy = det_wave(c["seed"], c["B"], c["L"], c.get("amp", 0.5))
    if c["B"] == 1:
        noisy = torch.cat([noisy, det_wave(c["seed"] + 7, 1, c["L"], c.get("amp", 0.5))])
    enroll = det_wave(c["seed"] + 1, c["B"], c["L_enroll"]) if "L_enroll" in c else None
    if enroll is not None and enroll.shape[0] != noisy.shape[0]:
        raise ValueError(name)
    return noisy, enroll


def scenarios(name):
    """name -> (tensor, row, sample, value): tensor is "noisy" or "enroll"."""
    c = cases.CASES[name]
    last = max(c["B"], 2) - 1
    s = {"mid_last_nan": ("noisy", last, c["L"] // 2, float("nan")),
         "mid_last_pinf": ("noisy", last, c["L"] // 2, float("inf")),
         "mid_last_ninf": ("noisy", last, c["L"] // 2, float("-inf")),
         "first_row0_nan": ("noisy", 0, 0, float("nan")),
         "last_row0_nan": ("noisy", 0, c["L"] - 1, float("nan"))}
    if "L_enroll" in c:
        s["enroll_row0_pinf"] = ("enroll", 0, c["L_enroll"] // 2, float("inf"))
    return s


def bad_inputs(name, scenario):
    noisy, enroll = clean_inputs(name)
    which, row, at, v = scenarios(name)[scenario]
    (noisy if which == "noisy" else enroll)[row, at] = v
    return noisy, enroll


@functools.lru_cache(maxsize=None)
def golden():
    """(nonfinite_masks.json, lookahead.json) as the reference gave them (tests/golden/make_nonfinite_golden.py)."""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "nonfinite_masks.json")) as f:
        masks = json.load(f)
    with open(os.path.join(here, "lookahead.json")) as f:
        look = json.load(f)
    return masks, look


def golden_masks(name, scenario):
    """(isnan, isinf) of the reference's output, [B, L] boolean arrays"""
    g = golden()[0][name][scenario]
    return from_runs(g["nan"], g["shape"]), from_runs(g["inf"], g["shape"])


@functools.lru_cache(maxsize=None)
def state_dict(name):
    import puresound_amd.nnet as PA
    return det_state_dict(cases.build(PA.NS, name), mode=cases.CASES[name].get("weights", "plain"))


@functools.lru_cache(maxsize=None)
def oracle_out(name, scenario):
    """The fp64 oracle's output for one scenario (None: the clean batch), computed once per process and never written to."""
    from oracle import separator_oracle as O
    noisy, enroll = clean_inputs(name) if scenario is None else bad_inputs(name, scenario)
    sd = state_dict(name)  # (building the model draws from the global generator: before the seed)
    torch.manual_seed(cases.CASES[name]["seed"])  # (tse_skim_v2_short: SpecAugment draws from the global generator)
    return O.inference(noisy, sd, cases.oracle_cfg(name), enroll).double().numpy()


def precisions(name):
    """The arithmetics a case is run in on the GPU: exact fp32, the model's default (None: fp16x2 where a module has the
    choice), and for the Conv-TasNet family the three-term bf16 split."""
    return ["fp32", None] + ([] if "cls" in cases.CASES[name]["masker"] else ["bf16x3"])


def hip_model(name, dev):
    import puresound_amd.nnet as PA
    model = cases.build(PA.NS, name).eval()
    model.load_state_dict(state_dict(name))
    return model.to(dev)


def hip_out(model, name, scenario, dev):
    """model.inference on the device for one scenario (None: the clean batch) -> fp32 CPU array"""
    noisy, enroll = clean_inputs(name) if scenario is None else bad_inputs(name, scenario)
    torch.manual_seed(cases.CASES[name]["seed"])
    return model.inference(noisy.to(dev), None if enroll is None else enroll.to(dev)).cpu().numpy()


def edge_slice(name, length):
    """the 16-sample iSTFT edge rule of the parity tests: those samples are divided by a window sum as small as 1.4e-9"""
    return slice(16, length - 16) if cases.CASES[name]["enc"]["kind"] == "stft" else slice(None)


def finite_error(name, got, want):
    """(largest |got - want| over the elements where `got` is finite, max |want| over the finite elements of `want`), both
    inside the iSTFT edge rule; `want` must be finite wherever `got` is (the caller asserts it)."""
    sl = edge_slice(name, got.shape[-1])
    got, want = np.asarray(got, dtype=np.float64)[..., sl], np.asarray(want, dtype=np.float64)[..., sl]
    fin = np.isfinite(got) & np.isfinite(want)
    den = float(np.abs(want[np.isfinite(want)]).max()) if np.isfinite(want).any() else 0.0
    err = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    return err, max(den, 1e-30)


def runs(mask):
    """[B, L] boolean array -> [[row, start, stop), ...]"""
    mask = np.asarray(mask, dtype=bool)
    out = []
    for r in range(mask.shape[0]):
        d = np.diff(np.concatenate([[0], mask[r].astype(np.int8), [0]]))
        out += [[r, int(a), int(b)] for a, b in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1))]
    return out


def from_runs(rr, shape):
    mask = np.zeros(tuple(shape), dtype=bool)
    for r, a, b in rr:
        mask[r, a:b] = True
    return mask
