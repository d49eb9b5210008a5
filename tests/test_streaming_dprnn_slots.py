"""Slot sessions of StreamingDPRNN (puresound_amd/streaming/dprnn.py) without a GPU: the ABI of the slot kernel, the slot
reference of tests/dprnn_slots_ref.py against the block reference, and the host-only length bookkeeping."""
import os
import re

import pytest
import torch

import dprnn_slots_ref as RS
import dprnn_step_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MAX = 2 ** 31 - 1


def _header():
    with open(os.path.join(ROOT, "include", "puresound_hip.h")) as f:
        return f.read()


def test_slot_entry_point_is_bound_and_declared():
    from puresound_amd import _abi
    name = "ps_dprnn_block_step_slots_f32"
    assert name in _abi.SIGNATURES
    assert re.search(r"^int %s\(" % name, _header(), re.M), f"{name} is not declared in the header"
    n = lambda key: len(_abi.SIGNATURES[key][1])  # noqa: E731
    assert n(name) == n("ps_dprnn_block_step_f32") + 1               # the span


def test_the_addition_keeps_the_abi_number():
    from puresound_amd import _abi
    assert _abi.ABI_VERSION == 24
    assert re.search(r"^#define PS_ABI_VERSION 24$", _header(), re.M)


def test_slot_kernel_is_in_the_source_as_a_compile_time_variant():
    with open(os.path.join(ROOT, "puresound_amd", "csrc", "dprnn_step.hip")) as f:
        src = f.read()
    assert re.search(r'extern "C" int ps_dprnn_block_step_slots_f32\(', src)
    assert re.search(r"^template <bool SLOTS", src, re.M)
    assert "if constexpr (SLOTS)" in src


def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1


def _chunks(total, k_max=16):
    """Chunk lengths 1, 2, ..., k_max, 1, 2, ... covering `total` frames."""
    out, k = [], 1
    while sum(out) < total:
        out.append(min(k, total - sum(out)))
        k = k % k_max + 1
    return out


@pytest.mark.parametrize("c,h,k", [(6, 4, 5), (5, 3, 7)])
def test_slot_reference_against_block_reference(c, h, k):
    """A column born at frame s and fed from there is block_step started at t0 = 0 on the same frames and states, whatever
    the session's counter says; a column with an empty span is left alone."""
    births = [0, 1, k - 1, k, 3 * k + 2]
    spans = [(s, I32_MAX) for s in births] + [(0, 0)]
    b, t_len = len(spans), 5 * k + 3
    intra, inter = R.make_pass(c, h, 3), R.make_pass(c, h, 4)
    x = _rand((t_len, b, c), 10)
    state = dict(h_intra=_rand((b, h), 11), c_intra=_rand((b, h), 12), h_bank=_rand((k, b, h), 13), c_bank=_rand((k, b, h), 14))
    before = {key: t.clone() for key, t in state.items()}
    xin = x.clone()
    for col, (birth, _) in enumerate(spans[:-1]):
        xin[:birth, col] = float("nan")                               # dead frames are not read
    xin[:, b - 1] = float("nan")
    outs, seen, t0 = [], [set() for _ in spans], 0
    for n in _chunks(t_len):
        o, vis = RS.block_step_slots(xin[t0:t0 + n], t0, k, intra, inter, state, spans)
        outs.append(o)
        seen = [a | v for a, v in zip(seen, vis)]
        t0 += n
    out = torch.cat(outs)
    for col, s in enumerate(births):
        one = {key: t[..., col:col + 1, :].clone() for key, t in before.items()}
        want, vis = R.block_step(x[s:, col:col + 1], 0, k, intra, inter, one)
        assert bool(torch.isnan(out[:s, col]).all())
        assert torch.equal(out[s:, col:col + 1], want), s
        for key, t in one.items():
            assert torch.equal(state[key][..., col:col + 1, :], t), (s, key)
        assert seen[col] == vis
    assert bool(torch.isnan(out[:, b - 1]).all()) and seen[b - 1] == set()
    for key, t in before.items():
        assert torch.equal(state[key][..., b - 1, :], t[..., b - 1, :]), key


@pytest.mark.parametrize("win,hop", [(32, 16), (16, 8), (16, 16), (64, 16), (256, 4)])
@pytest.mark.parametrize("extra_hops", [0, 1, 7, 500])
def test_slot_output_range_is_the_offline_output_after_the_latency(win, hop, extra_hops):
    from puresound_amd.streaming import StreamingDPRNN as S
    samples = win + extra_hops * hop
    r = S.slot_output_range(samples, win, hop)
    n = S.output_length(samples, win, hop)
    frames = (samples - win) // hop + 1
    assert r.start == win - hop                                   # latency_samples
    assert len(r) == n["emitted"] + n["flushed"] == (frames - 1) * hop + win
    assert r.stop == samples + (win - hop)
    assert n["prime_hops"] * hop == r.start


def test_frame_limit_is_the_session_core_s():
    from puresound_amd.streaming import _session, dprnn, tcn
    assert dprnn.FRAME_LIMIT == tcn.FRAME_LIMIT == _session.FRAME_LIMIT == 2 ** 31 - 1 - 16
    assert dprnn.K_MAX == tcn.K_MAX == 16
