"""StreamingUnetTcn (puresound_amd/streaming/unet_tcn.py) without a GPU: which models it refuses, the length bookkeeping of a
session with a model delay, the ABI of its kernel, and the two references the GPU tests compare against -- the frame loop of
ps_gated_tcn_step_f32 (tests/gated_tcn_step_ref.py) against F.conv1d on whole sequences, and the up path's hop schedule
with its flush (tests/unet_delay_ref.py) against F.conv_transpose2d with the first frame trimmed."""
import copy
import itertools
import os
import re

import pytest
import torch
import torch.nn as nn

import cases
import gated_tcn_step_ref as G
import unet_delay_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESET = "tse_unet_tcn_causal_short"
#: the reduced model of the GPU tests: three U-Net levels, 2 x 3 gated blocks of 16 channels, the embedding in the first of each
SMALL = dict(channels=(1, 8, 8, 8), kernel_t=(2,) * 3, kernel_f=(5,) * 3, stride_t=(1,) * 3, stride_f=(2,) * 3,
             dilation_t=(1,) * 3, dilation_f=(1,) * 3, delay=(0,) * 3, tcn_dim=16, per_tcn_stack=3, repeat_tcn=2,
             tcn_with_embed=[1, 0, 0])


def _build(name=PRESET, **masker_kw):
    import puresound_amd.nnet as PA
    c = copy.deepcopy(cases.CASES[name])
    c["masker"]["kw"].update(masker_kw)
    saved = cases.CASES[name]
    cases.CASES[name] = c
    try:
        return cases.build(PA.NS, name).eval()
    finally:
        cases.CASES[name] = saved


def _small(**kw):
    return _build(**{**SMALL, **kw})


def _refused(model, words):
    from puresound_amd.streaming import StreamingUnetTcn
    with pytest.raises(NotImplementedError) as e:
        StreamingUnetTcn(model)
    assert words.lower() in str(e.value).lower(), str(e.value)


def test_refuses_other_wrappers_encoders_and_maskers():
    import puresound_amd.nnet as PA
    _refused(nn.Linear(2, 2), "SoTaskWrapModule")
    _refused(cases.build(PA.NS, "tiny_free_relu_causal").eval(), "only the conv-STFT encoder")
    _refused(cases.build(PA.NS, "ns_dpcrn_short").eval(), "UnetTcn only")


def test_refuses_tcn_configurations():
    _refused(_small(causal=False), "not causal")
    _refused(_small(tcn_layer="normal"), "only the gated block streams")
    _refused(_small(tcn_use_film=True), "FiLM")
    _refused(_small(tcn_norm="gLN"), "tcn_norm 'gLN'")
    _refused(_small(tcn_norm="cLN"), "tcn_norm 'cLN'")


def test_refuses_unet_configurations():
    _refused(_small(norm_type="gLN"), "norm_type 'gLN'")
    _refused(_small(skip_conv=True), "skip_conv")
    _refused(_small(delay=(0, 1, 0)), "delay (0, 1, 0)")
    _refused(_small(stride_t=(1, 2, 1)), "stride_t must be 1")
    _refused(_small(dilation_t=(1, 2, 1)), "reads 1 future frames")
    _refused(_small(transpose_t_size=3), "one frame per layer")


def test_refuses_pairing_missing_speaker_net_and_per_channel_slopes():
    m = _small()
    m.mask_type = m.f_type = "complex"
    _refused(m, "mask pairing")
    m = _small()
    m.speaker_net = None
    _refused(m, "without a speaker_net")
    m = _small()
    m.masker.cnn_down[1][3] = nn.PReLU(8)
    _refused(m, "per-channel")
    m = _small()
    m.masker.tcn_list[0][1].right_conv[2] = nn.PReLU(16)
    _refused(m, "per-channel")


def test_refuses_more_ring_pairs_than_a_commit_takes():
    n = 15                                                   # 1 + 15 + 15 tensors with history, the features, the queue
    m = _small(channels=(1,) + (2,) * n, kernel_t=(2,) * n, kernel_f=(1,) * n, stride_t=(1,) * n, stride_f=(1,) * n,
               dilation_t=(1,) * n, dilation_f=(1,) * n, delay=(0,) * n)
    _refused(m, "33 ring pairs")


def test_refuses_training_mode_then_cpu_tensors_last():
    from puresound_amd.streaming import StreamingUnetTcn
    _refused(_small(), "ROCm device")
    _refused(_small(transpose_delay=False), "ROCm device")
    _refused(_build(), "ROCm device")                        # the preset itself: everything but the device is accepted
    m = _small()
    m.train()
    with pytest.raises((RuntimeError, NotImplementedError)):
        StreamingUnetTcn(m)


def test_length_bookkeeping_with_a_model_delay():
    from puresound_amd.streaming import StreamingSeparator, StreamingUnetTcn
    n = StreamingUnetTcn.output_length(3968, 512, 128, 6)
    assert n == dict(prime_hops=9, frames=28, emitted=22 * 128, flushed=1152)
    assert n["emitted"] + n["flushed"] == (28 - 1) * 128 + 512
    # fewer frames than the delay, or exactly the delay: nothing is emitted, flush() returns the whole offline output
    for frames in (1, 2, 6):
        n = StreamingUnetTcn.output_length((frames + 3) * 128, 512, 128, 6)
        assert (n["frames"], n["emitted"], n["flushed"]) == (frames, 0, (frames - 1) * 128 + 512)
    # no delay: the bookkeeping every other streamer has
    assert StreamingUnetTcn.output_length(3968, 512, 128) == StreamingSeparator.output_length(3968, 512, 128) \
        == dict(prime_hops=3, frames=28, emitted=28 * 128, flushed=384)
    with pytest.raises(ValueError):
        StreamingUnetTcn.output_length(3969, 512, 128, 6)


def test_session_defaults_to_no_delay():
    """HopSession's new argument changes nothing for the streamers that do not pass it."""
    from puresound_amd.streaming._session import HopSession
    m = _small()
    s = HopSession(m, 512, 128)
    assert (s.delay_frames, s.prime_hops, s.latency_samples) == (0, 3, 384)
    s = HopSession(m, 512, 128, delay_frames=6)
    assert (s.delay_frames, s.prime_hops, s.latency_samples) == (6, 9, 1152)


def _header_args(name):
    with open(os.path.join(ROOT, "include", "puresound_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    proto = re.search(rf"^int {name}\((.*?)\);", header, flags=re.S | re.M).group(1)
    return [" ".join(a.split()) for a in proto.split(",")]


def test_kernel_declared_with_abi_24():
    import ctypes as C
    from puresound_amd import _abi
    assert _abi.ABI_VERSION == 24
    with open(os.path.join(ROOT, "include", "puresound_hip.h")) as f:
        assert "#define PS_ABI_VERSION 24" in f.read()
    args = _header_args("ps_gated_tcn_step_f32")
    res, sig = _abi.SIGNATURES["ps_gated_tcn_step_f32"]
    assert res is C.c_int and len(sig) == len(args) == 17
    for a, t in zip(args, sig):
        if "ps_prologue*" in a:
            assert t is C.POINTER(_abi.Prologue), a
        elif "*" in a:
            assert t is C.c_void_p, a
        else:
            assert a.startswith("int ") and t is C.c_int, a
    assert [a.split()[-1].lstrip("*") for a in args] == ["y", "ring", "R", "counter", "wl", "wr", "emb_taps", "pro_left",
                                                          "pro_right", "g", "H", "B", "k", "ld", "P", "dilation", "stream"]
    with open(os.path.join(ROOT, "puresound_amd", "csrc", "Makefile")) as f:
        assert "gated_tcn_step.hip" in f.read()


@pytest.mark.parametrize("e", [0, 6])
@pytest.mark.parametrize("dilation", [1, 4])
def test_step_reference_matches_conv1d_on_whole_sequences(e, dilation):
    """H = 8, P = 3, T = 2 (P-1) d + 5 frames through F.conv1d with left padding -- the embedding concatenated to the right
    convolution's input and zero-padded with it -- against the frame loop; every split of T into chunks of 1, 3 and 16 frames
    gives identical values."""
    h, p, b = 8, 3, 3
    t = 2 * (p - 1) * dilation + 5
    blk = G.make_block(h, e, p, dilation, seed=10 * e + dilation)
    g = torch.Generator().manual_seed(5)
    y = torch.rand(b, h, t, generator=g, dtype=torch.float64) * 2 - 1
    emb = torch.rand(b, e, generator=g, dtype=torch.float64) * 2 - 1 if e else None
    want = G.offline(y, blk, emb)
    if e:   # the embedding shows in the first (P-1) d frames only as a missing term: a constant elsewhere
        full = G.offline(torch.zeros_like(y), blk, emb)
        edge, inner = float((full[..., 0] - full[..., -1]).abs().max()), float((full[..., (p - 1) * dilation] - full[..., -1]).abs().max())
        assert edge > 1e-3 and inner < 1e-12, (edge, inner)

    def splits(left):
        """every way to write `left` as an ordered sum of 1s, 3s and 16s"""
        if left == 0:
            yield ()
        for size in (1, 3, 16):
            if size <= left:
                for rest in splits(left - size):
                    yield (size,) + rest

    runs = {}
    for sizes in splits(t):
        ring = torch.full(((p - 1) * dilation + 16, h, b), float("nan"), dtype=torch.float64)
        got, t0 = [], 0
        for size in sizes:
            got.append(G.block_step(y[:, :, t0:t0 + size].permute(2, 1, 0).contiguous(), t0, blk, ring, emb))
            t0 += size
        assert t0 == t
        runs[sizes] = torch.cat(got).permute(2, 1, 0)
    first = runs[(1,) * t]
    assert float((first - want).abs().max()) < 1e-12
    assert all(torch.equal(first, r) for r in runs.values()), "a split changed the values"


@pytest.mark.parametrize("t", [1, 2, 3, 9])
def test_hop_schedule_matches_conv_transpose2d_with_the_first_frame_trimmed(t):
    """n = 3 layers with skips: fewer frames than the delay (T = 1, 2), exactly the delay (3), more (9); the flush hops give
    the last frames."""
    n, ch, f, b = 3, 4, 5, 2
    layers = U.make_decoder(n, ch, seed=t)
    g = torch.Generator().manual_seed(t)
    x = torch.rand(b, ch, f, t, generator=g, dtype=torch.float64) * 2 - 1
    skips = [torch.rand(b, ch, f, t, generator=g, dtype=torch.float64) * 2 - 1 for _ in range(n)]
    want = U.offline(x, skips, layers)
    got = U.stream(x, skips, layers)
    assert got.shape == want.shape == (b, ch, f, t)
    assert float((got - want).abs().max()) < 1e-12
