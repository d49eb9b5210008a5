"""The reference side of the edge-length sweep (edge_length_cases.py), on the CPU: the oracle itself is well conditioned on
the ladder (its float32 form stays inside the bounds the HIP result is held to), the output clamp leaves the waveform
visible, a too short utterance is refused, and the window-weighted metric sees a body error the project metric passes."""
import numpy as np
import pytest
import torch

import cases
import edge_length_cases as E
from detweights import det_wave
from oracle import separator_oracle as O


@pytest.mark.parametrize("name,t", [(n, t) for n in E.PRESETS for t in E.CPU_T])
def test_float32_oracle_is_inside_the_bounds(name, t):
    noisy, enroll, ref = E.problem(name, E.length_of(name, t), 2)
    assert ref.shape == (2, E.out_length(name, t)) and bool(torch.isfinite(ref).all())
    share = E.clamped_share(name, ref)
    with torch.no_grad():
        got = O.inference(noisy, E.weights(name)[0], cases.oracle_cfg(name), enroll)
    assert got.dtype == torch.float32 and got.shape == ref.shape
    err = E.errors(name, got.numpy(), ref.numpy())
    print(f"{name} T={t}: fp32 oracle vs fp64 {err}, clamped {share:.4f}")
    assert share <= E.CLAMP_CAP
    for metric, bound in E.bounds(name, "fp32").items():
        assert err[metric] < bound, (metric, err)


@pytest.mark.parametrize("name", E.PRESETS)
def test_oracle_refuses_less_than_one_window(name):
    win, _ = E.win_hop(name)
    noisy, enroll = E.inputs(name, win - 1, 2)
    with pytest.raises((RuntimeError, ValueError)):
        O.inference(noisy.double(), E.weights(name)[1], cases.oracle_cfg(name),
                    None if enroll is None else enroll.double())


def test_weighted_metric_sees_a_body_error_the_project_metric_passes():
    """0.1 % on every sample that lies a whole window inside: under 1e-4 of the edge-dominated max|ref|, but ten times the
    weighted metric's widest bound."""
    name, t = "ns_dpcrn_short", 33
    _, _, ref = E.problem(name, E.length_of(name, t), 2)
    ref = ref.numpy()
    n_fft, lout = E.win_hop(name)[0], ref.shape[-1]
    assert lout == E.out_length(name, t) and lout > 4 * n_fft
    bent = ref.copy()
    bent[:, n_fft:lout - n_fft] *= 1.0 + 1e-3
    err = E.errors(name, bent, ref)
    print(err)
    assert err["rel_max"] < 1e-4
    assert err["weighted"] > max(E.FP32_TOL, E.FP16X2_TOL)
    assert E.errors(name, ref, ref) == {"rel_max": 0.0, "weighted": 0.0}


def test_window_weight_is_the_normalised_window_sum():
    for t in E.STFT_T:
        s = E.window_weight(t)
        assert s.shape == (E.out_length("cfg1_short", t),) and s[0] == 0.0 and 0.0 < s.max() <= 1.0
        if t >= 4:   # four overlapping frames reach the steady state
            assert s.max() == 1.0
            np.testing.assert_allclose(s[384:s.shape[0] - 384], 1.0, rtol=1e-12)
    # what the ladder's geometry promises
    for name, t in E.all_cases():
        win, hop = E.win_hop(name)
        length = E.length_of(name, t)
        assert (length - win) // hop + 1 == t and (length - win) % hop == (hop // 2 + 1 if t % 2 else 0)
    assert len(E.all_cases()) == 92
    assert E.walk_order("cfg1_short") == (129, 1, 128, 2, 127, 3, 33, 4, 5)
    assert sorted(E.walk_order("cfg2_short")) == sorted(E.FREE_T) and E.walk_order("cfg2_short")[:4] == (301, 1, 151, 2)


def test_a_batch_of_one_is_the_first_row_of_a_larger_batch():
    """test_odd_batches compares an utterance on its own with the same utterance inside 17."""
    big = det_wave(901, 17, 352)
    assert torch.equal(det_wave(901, 1, 352), big[:1]) and torch.equal(det_wave(901, 3, 352), big[:3])
    one, _ = E.inputs("cfg2_short", 352, 1, row=16)
    assert torch.equal(one, big[16:17] * E.AMP)
