"""The models, the batch and the float64 references of the ragged noise-suppression tests (test_ragged_ns.py,
test_ragged_ns_gpu.py): the two egs/ns presets of golden/cases.py (ns_dpcrn_v0_causal, ns_dparn_v0_causal) and a deep copy of
each with transpose_delay=True (ns_dpcrn_v0, ns_dparn_v0: every up layer reads one frame ahead), det_state_dict weights.

The batch: utterances of FRAMES frames built as edge_length_cases builds them (det_wave(901) * 0.05, an odd frame count with a
ragged tail), row n followed by junk at ragged_ref.JUNK_GAIN x the amplitude or by NaN; per row the float64 oracle of the
utterance alone.  Everything is computed once, handed out to every test that asks, and never written to."""
import copy
import functools

import numpy as np
import torch

import cases
import edge_length_cases as E
import ragged_ref as R
from detweights import det_state_dict, det_wave
from oracle import separator_oracle as O

BASE = {"ns_dpcrn_short": "ns_dpcrn_short", "ns_dparn_short": "ns_dparn_short",
        "ns_dpcrn_lookahead": "ns_dpcrn_short", "ns_dparn_lookahead": "ns_dparn_short"}
NAMES = tuple(BASE)
LOOKAHEAD = tuple(n for n in NAMES if n.endswith("_lookahead"))
FRAMES = (129, 1, 2, 5, 6, 33, 128)      # one and two frames, the 4-frame overlap of the window, the 128-frame tile
WIN, HOP = 512, 128
ZONE_HOPS = 5                            # the up layers' lookahead reaches this many hops in front of the last window


def spec(name):
    c = copy.deepcopy(cases.CASES[BASE[name]])
    if name in LOOKAHEAD:
        c["masker"]["kw"]["transpose_delay"] = True
    return c


def build(ns, name):
    c = spec(name)
    return ns.SoTaskWrapModule(encoder=cases.build_encoder(ns, c["enc"]), masker=cases.build_masker(ns, c["masker"]),
                               verbose=False, **c["wrap"])


def oracle_cfg(name):
    c = spec(name)
    cfg = dict(encoder=dict(c["enc"]), masker=cases.unet_args(c["masker"]), masker_kind=c["masker"]["oracle"])
    cfg.update({k: v for k, v in c["wrap"].items() if k != "drop_first_bin"})
    return cfg


@functools.lru_cache(maxsize=None)
def weights(name):
    """-> (float32 state dict, float64 state dict); transpose_delay adds no parameter: a copy has its preset's weights"""
    if name in cases.CASES:
        return E.weights(name)
    import puresound_amd.nnet as PA
    sd = det_state_dict(build(PA.NS, name))
    return sd, {k: v.double() for k, v in sd.items()}


def oracle(name, noisy):
    with torch.no_grad():
        return O.inference(noisy.double(), weights(name)[1], oracle_cfg(name))


def lengths():
    return [E.length_of(BASE[NAMES[0]], t) for t in FRAMES]


def out_lengths():
    return [(t - 1) * HOP + WIN for t in FRAMES]


@functools.lru_cache(maxsize=None)
def alone(name, row):
    """-> (utterance [1, L_n] float32, the float64 oracle's output [1, out_n]) of row `row` on its own"""
    length = lengths()[row]
    if name in cases.CASES:
        noisy, _, ref = E.problem(name, length, 1, row=row)
        return noisy, ref
    noisy, _ = E.inputs(BASE[name], length, 1, row=row)
    return noisy, oracle(name, noisy)


@functools.lru_cache(maxsize=None)
def batch(junk="noise"):
    """-> noisy [N, L]: row n is utterance n followed by junk ("noise": uniform noise at JUNK_GAIN x the amplitude; "nan";
    "zero": the zero-padded batch).  The utterances are the same for every model."""
    lens = lengths()
    if junk == "noise":
        noisy = det_wave(7001, len(lens), max(lens)) * (E.AMP * R.JUNK_GAIN)
    else:
        noisy = torch.full((len(lens), max(lens)), float("nan") if junk == "nan" else 0.0)
    for n, length in enumerate(lens):
        noisy[n, :length] = E.inputs(BASE[NAMES[0]], length, 1, row=n)[0][0]
    return noisy


def zone(t):
    """[lo, hi): the ZONE_HOPS hops in front of the last window of an utterance of t frames"""
    out = (t - 1) * HOP + WIN
    return max(0, out - WIN - ZONE_HOPS * HOP), out - WIN


def weighted_parts(got, ref, t):
    """edge_length_cases.weighted_rel_max split over the samples -> (before the zone, in the zone, behind it), each the
    largest weighted error there over the row's largest weighted |ref| (0.0 for an empty part)"""
    s = E.window_weight(t)
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    assert got.shape == ref.shape == s.shape
    err, den = np.abs(got - ref) * s, max(float((np.abs(ref) * s).max()), 1e-30)
    lo, hi = zone(t)
    return tuple(float(part.max()) / den if part.size else 0.0 for part in (err[:lo], err[lo:hi], err[hi:]))
