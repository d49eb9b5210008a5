"""StreamingConvTasNet (puresound_amd/streaming/tcn.py) without a GPU: which models it refuses, its length bookkeeping, and
the ABI of its kernels."""
import copy
import os

import pytest
import torch.nn as nn

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(name="tiny_free_relu_causal", enc=None, **masker_kw):
    import puresound_amd.nnet as PA
    c = copy.deepcopy(cases.CASES[name])
    c["masker"].update(masker_kw)
    c["enc"].update(enc or {})
    saved = cases.CASES[name]
    cases.CASES[name] = c
    try:
        return cases.build(PA.NS, name).eval()
    finally:
        cases.CASES[name] = saved


def _refused(model, words):
    from puresound_amd.streaming import StreamingConvTasNet
    with pytest.raises(NotImplementedError) as e:
        StreamingConvTasNet(model)
    assert words.lower() in str(e.value).lower(), str(e.value)


def test_refuses_stft_encoder():
    import puresound_amd.nnet as PA
    _refused(cases.build(PA.NS, "tiny_stft").eval(), "StreamingSeparator")


def test_refuses_window_not_a_multiple_of_hop():
    _refused(_build(enc=dict(hop=6)), "multiple of hop")


def test_refuses_other_maskers():
    import puresound_amd.nnet as PA
    _refused(cases.build(PA.NS, "cfg4_short").eval(), "ConvTasNet only")


def test_refuses_non_causal():
    import puresound_amd.nnet as PA
    _refused(cases.build(PA.NS, "tiny_free").eval(), "not causal")


def test_refuses_gated_blocks():
    _refused(_build(tcn_layer="gated"), "gated")


def test_refuses_global_norms():
    _refused(_build(tcn_norm="gLN"), "tcn_norm")
    _refused(_build(dconv_norm="iLN"), "dconv_norm")


def test_refuses_embedding_free_tse():
    m = _build()
    m.embedding_free_tse = True
    _refused(m, "embedding_free_tse")


def test_refuses_complex_pairing():
    m = _build()
    m.mask_type = m.f_type = "complex"
    _refused(m, "pairing")


def test_refuses_constraints():
    m = _build()
    m.mask_constraint = "tanh"
    _refused(m, "mask_constraint")
    m = _build()
    m.output_constraint = "clamp"
    _refused(m, "output_constraint")


def test_refuses_per_channel_prelu():
    m = _build()
    m.masker.tcn_list[0][1].in_conv[2] = nn.PReLU(12)
    _refused(m, "per-channel")


def test_refuses_cpu_tensors_last():
    _refused(_build(), "ROCm device")
    _refused(_build(tcn_norm="cLN", dconv_norm="cLN"), "ROCm device")
    _refused(_build("cfg3_causal_short"), "ROCm device")


def test_length_bookkeeping():
    from puresound_amd.streaming import StreamingConvTasNet
    assert StreamingConvTasNet.output_length(4000, 32, 16) == dict(prime_hops=1, frames=249, emitted=3984, flushed=16)
    for samples, win, hop in ((776, 16, 8), (160000, 32, 16), (48, 16, 16), (64, 64, 16)):
        n = StreamingConvTasNet.output_length(samples, win, hop)
        t = (samples - win) // hop + 1
        assert n["frames"] == t and n["emitted"] + n["flushed"] == (t - 1) * hop + win
    with pytest.raises(ValueError):
        StreamingConvTasNet.output_length(777, 16, 8)


def test_kernels_declared_with_abi_24():
    from puresound_amd import _abi
    assert _abi.ABI_VERSION == 24
    with open(os.path.join(ROOT, "include", "puresound_hip.h")) as f:
        header = f.read()
    assert "#define PS_ABI_VERSION 24" in header
    for name in ("ps_dwconv_step_f32", "ps_free_decode_step_f32", "ps_stream_commit_frames_f32"):
        assert name in _abi.SIGNATURES and f"int {name}(" in header
