"""The reference side of the trained-weight sweep (trained_weight_cases.py), on the CPU: the law itself (detweights mode
"trained"), the oracle's own float32 noise under it, and that the comparison can see what it is there to see -- a dropped
second fp16 term of the weights moves the float64 result by more than the project's bound.  (The oracle is pinned to the
reference under the law by the *_trained_short fixtures of test_oracle_golden.py.)

With PS_TRAINED_WEIGHTS_TABLE=<path> in the environment the module writes what it measured to that file when its last test
has run (profiles/trained_weights.txt keeps a copy)."""
import os
import zlib

import numpy as np
import pytest
import torch

import cases
import trained_weight_cases as W
from detweights import _KEEP, det_state_dict, det_tensor

_ROWS = []


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    path = os.environ.get("PS_TRAINED_WEIGHTS_TABLE")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(_ROWS) + "\n")


def _crc(t):
    return zlib.crc32(t.numpy().tobytes())


def test_plain_and_wild_draws_are_what_they_were():
    """Values recorded before the law was added (the committed fixtures pin both modes end to end; this is the quick form)."""
    ref = torch.zeros(32, 8)
    assert _crc(det_tensor("masker.a.weight", ref)) == 2644775745
    assert _crc(det_tensor("masker.a.weight", ref, "wild")) == 1777679765
    assert _crc(det_tensor("masker.a.gamma", torch.zeros(24), "wild")) == 883009707
    assert _crc(det_tensor("masker.a.bias", torch.zeros(24))) == 1489969857
    # a key outside the maskers / speaker nets is the plain one in every mode
    for mode in ("wild", "trained"):
        assert torch.equal(det_tensor("encoder.a.weight", ref, mode), det_tensor("encoder.a.weight", ref))


@pytest.mark.parametrize("name", ["cfg3_causal_short", "tse_skim_v1_short", "ns_dparn_short", "tse_unet_tcn_causal_short"])
def test_the_law_touches_what_it_should(name):
    import puresound_amd.nnet as PA
    model = cases.build(PA.NS, name)
    plain, trained = det_state_dict(model), det_state_dict(model, mode="trained")
    assert list(plain) == list(trained)
    again = det_state_dict(cases.build(PA.NS, name), mode="trained")
    seen = {"gain": 0, "bias": 0, "slope": 0, "rows": 0, "kept": 0}
    for k, p in plain.items():
        t = trained[k]
        assert t.dtype == p.dtype and t.shape == p.shape and torch.equal(t, again[k]), k
        leaf, shape = k.rsplit(".", 1)[-1], tuple(p.shape)
        under = k.startswith(("masker.", "speaker_net.")) and leaf not in (
            "num_batches_tracked", "running_mean", "running_var") + _KEEP
        if under and (leaf == "gamma" or (leaf == "weight" and len(shape) == 1 and shape[0] > 1)):
            assert float(t.min()) >= 0.25 and float(t.max()) <= 4.0 and not torch.equal(t, p), k
            seen["gain"] += 1
        elif under and (leaf == "beta" or (leaf == "bias" and len(shape) == 1)):
            assert float(t.abs().max()) <= 1.0 and not torch.equal(t, p), k
            if t.numel() >= 64:
                assert float(t.abs().max()) > 0.5, k
            seen["bias"] += 1
        elif under and leaf == "weight" and shape == (1,):
            assert 0.05 <= float(t) <= 1.5, k
            seen["slope"] += 1
        elif under and len(shape) > 1 and shape[0] >= 16:
            rows_p, rows_t = p.reshape(shape[0], -1).double(), t.reshape(shape[0], -1).double()
            changed = [r for r in range(shape[0]) if not torch.equal(rows_p[r], rows_t[r])]
            assert len(changed) == 4, (k, changed)
            ratios = sorted(float((rows_t[r].abs().sum() / rows_p[r].abs().sum())) for r in changed)
            np.testing.assert_allclose(ratios, [2.0 ** -4, 2.0 ** -3, 2.0 ** 3, 2.0 ** 4], rtol=1e-6, err_msg=k)
            seen["rows"] += 1
        else:
            assert torch.equal(t, p), k
            seen["kept"] += 1
    assert all(seen.values()), seen
    # the draw is its own: a gain's position in 2^-2 .. 2^2 says nothing about the plain gain's position in 0.5 .. 1.5
    gains = [k for k in plain if k.startswith("masker.") and plain[k].dim() == 1 and plain[k].numel() >= 64
             and k.rsplit(".", 1)[-1] in ("gamma", "weight")]
    a = np.concatenate([plain[k].numpy() for k in gains])
    b = np.concatenate([np.log2(trained[k].numpy()) for k in gains])
    assert abs(float(np.corrcoef(a, b)[0, 1])) < 0.1


def _self_noise(name, amp):
    noisy, enroll, ref = W.problem(name, amp)
    got = W.run_oracle(name, noisy, enroll, W.weights(name)[0])
    assert got["pre"].dtype == torch.float32 and bool(torch.isfinite(got["pre"]).all())
    err = W.errors(name, got["pre"].numpy(), ref["pre"].numpy())
    if ref["dvec"] is not None:
        err["dvec"] = W.embedding_error(got["dvec"].numpy(), ref["dvec"].numpy())
    return err, float(ref["pre"].abs().max()), float(ref["mask"].abs().max())


@pytest.mark.parametrize("name", W.PRESETS)
def test_float32_oracle_self_noise_is_the_recorded_one(name):
    worst = 0.0
    for amp in W.AMPS:
        err, top, top_mask = _self_noise(name, amp)
        row = (f"self-noise  {name:<26} amp {amp:<6g} " + " ".join(f"{m} {v:.3e}" for m, v in err.items())
               + f"  max|pre-clamp| {top:.3g} max|mask| {top_mask:.3g}")
        print(row)
        _ROWS.append(row)
        worst = max(worst, *err.values())
    assert worst < W.PROJECT_TOL / 2, (name, worst)
    # the table the "fp32" bound is made from: not understated (summation order differs a little from machine to machine)
    assert worst <= 2.0 * W.SELF_NOISE[name], (name, worst, W.SELF_NOISE[name])
    assert W.FP32_TOL <= W.bound(name, "fp32") <= W.PROJECT_TOL


@pytest.mark.parametrize("name", W.PRESETS)
def test_a_dropped_fp16_term_is_visible(name):
    """Every weight matrix rounded to fp16 moves the float64 oracle's pre-clamp waveform by at least the project's bound: a
    kernel that lost the second term of its fp16 pair would miss it."""
    noisy, enroll = W.inputs(name, W.SENS_AMP)
    sd = W.weights(name)[1]
    whole = W.run_oracle(name, noisy, enroll, sd)["pre"].numpy()
    rounded = W.run_oracle(name, noisy, enroll, W.fp16_rounded(sd))["pre"].numpy()
    err = W.errors(name, rounded, whole)
    row = f"sensitivity {name:<26} amp {W.SENS_AMP:<6g} " + " ".join(f"{m} {v:.3e}" for m, v in err.items())
    print(row)
    _ROWS.append(row)
    assert err["rel_max"] >= W.PROJECT_TOL, (name, err)


@pytest.mark.parametrize("kind", list(W.STREAMED))
def test_streamed_amplitudes_keep_the_oracle_inside_the_clamp(kind):
    name, noisy, enroll, ref = W.stream_problem(kind)
    assert noisy.shape == (W.BATCH, W.LENGTH) and (enroll is not None) == W.has_enrolment(name)
    clamped = ref["pre"].clamp(min=-1.0, max=1.0)
    assert W.errors(name, clamped.numpy(), ref["pre"].numpy())["rel_max"] == 0.0


def test_cases_and_bounds():
    assert len(W.PRESETS) == 12 and len(W.all_cases()) == 24 and set(W.SELF_NOISE) == set(W.PRESETS)
    assert W.bound("cfg2_short", "fp32") == W.FP32_TOL == 2e-5
    assert W.bound("cfg3_causal_short", "fp32") == W.PROJECT_TOL          # 20 x 1.4e-5, capped
    assert W.bound("tse_unet_tcn_causal_short", "fp32") == pytest.approx(7.2e-5)
    assert W.bound("cfg2_short", "fp16x2") == W.bound("cfg2_short", "bf16x3") == W.PROJECT_TOL == 1e-4
    assert [n.replace("_trained", "") for n, c in cases.CASES.items() if c.get("weights") == "trained"] == list(
        cases.TRAINED_BASES)
