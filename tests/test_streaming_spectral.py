"""StreamingSeparator (puresound_amd/streaming/spectral.py) without a GPU: which models it refuses, and its length
bookkeeping."""
import copy

import pytest
import torch.nn as nn

import cases


def _build(name="ns_dpcrn_short", cls=None, **masker_kw):
    import puresound_amd.nnet as PA
    c = copy.deepcopy(cases.CASES[name])
    c["masker"]["kw"].update(masker_kw)
    if cls is not None:
        c["masker"]["cls"] = cls
    saved = cases.CASES[name]
    cases.CASES[name] = c
    try:
        return cases.build(PA.NS, name).eval()
    finally:
        cases.CASES[name] = saved


def _refused(model, words):
    from puresound_amd.streaming import StreamingSeparator
    with pytest.raises(NotImplementedError) as e:
        StreamingSeparator(model)
    assert words.lower() in str(e.value).lower(), str(e.value)


def test_refuses_free_encoder():
    import puresound_amd.nnet as PA
    _refused(cases.build(PA.NS, "tiny_free").eval(), "ConvEncDec")


def test_refuses_lookahead_decoder():
    _refused(_build(transpose_delay=True), "transpose_delay")


def test_refuses_delay():
    _refused(_build(delay=(0, 1, 0, 0, 0)), "delay")


def test_refuses_gln_norm():
    _refused(_build(norm_type="gLN"), "norm_type")


def test_refuses_speaker_net():
    m = _build()
    m.speaker_net = nn.Sequential(nn.Identity())
    _refused(m, "speaker_net")


def test_refuses_dparn_mout():
    m = _build("ns_dparn_short", cls="DPARN_Mout")
    _refused(m, "DPARN_Mout")


def test_refuses_skip_conv():
    _refused(_build(skip_conv=True), "skip_conv")


def test_refuses_future_frames_of_dilated_down_convolution():
    _refused(_build(dilation_t=(1, 2, 1, 1, 1)), "future frames")


def test_refuses_other_maskers():
    import puresound_amd.nnet as PA
    _refused(cases.build(PA.NS, "tse_unet_tcn_causal_short").eval(), "speaker_net")


def test_refuses_cpu_tensors():
    _refused(_build(), "ROCm device")
    _refused(_build("ns_dparn_short"), "ROCm device")


def test_length_bookkeeping():
    from puresound_amd.streaming import StreamingSeparator
    n = StreamingSeparator.output_length(3968, 512, 128)
    assert n == dict(prime_hops=3, frames=28, emitted=28 * 128, flushed=384)
    for samples in (512, 640, 160000):
        n = StreamingSeparator.output_length(samples, 512, 128)
        t = (samples - 512) // 128 + 1
        assert n["frames"] == t and n["emitted"] + n["flushed"] == (t - 1) * 128 + 512
    with pytest.raises(ValueError):
        StreamingSeparator.output_length(3969, 512, 128)
