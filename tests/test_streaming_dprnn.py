"""StreamingDPRNN (puresound_amd/streaming/dprnn.py) without a GPU: which models it refuses, its length bookkeeping, the ABI
of its kernel, and the frame-by-frame reference of one block step (tests/dprnn_step_ref.py) against torch's own modules."""
import copy
import os

import pytest
import torch
import torch.nn as nn

import cases
import dprnn_step_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(name="cfg4_short", enc=None, wrap=None, **masker_kw):
    import puresound_amd.nnet as PA
    c = copy.deepcopy(cases.CASES[name])
    c["masker"]["kw"].update(masker_kw)
    c["enc"].update(enc or {})
    c["wrap"].update(wrap or {})
    saved = cases.CASES[name]
    cases.CASES[name] = c
    try:
        return cases.build(PA.NS, name).eval()
    finally:
        cases.CASES[name] = saved


def _refused(model, words):
    from puresound_amd.streaming import StreamingDPRNN
    with pytest.raises(NotImplementedError) as e:
        StreamingDPRNN(model)
    assert words.lower() in str(e.value).lower(), str(e.value)


def test_refuses_other_wrappers():
    _refused(nn.Linear(2, 2), "SoTaskWrapModule")


def test_refuses_stft_encoder():
    import puresound_amd.nnet as PA
    _refused(cases.build(PA.NS, "tiny_stft").eval(), "StreamingSeparator")


def test_refuses_window_not_a_multiple_of_hop():
    _refused(_build(enc=dict(hop=12)), "multiple of hop")


def test_refuses_other_maskers():
    import puresound_amd.nnet as PA
    _refused(cases.build(PA.NS, "tiny_free_relu_causal").eval(), "DPRNN only")


def test_refuses_non_causal():
    _refused(_build(causal=False), "not causal")


def test_refuses_segment_overlap():
    _refused(_build(seg_overlap=True), "seg_overlap")


def test_refuses_film_blocks_and_speaker_nets():
    _refused(_build(embed_dim=16, block_with_embed=(True,) + (False,) * 5), "FiLM")
    m = _build()
    m.speaker_net = nn.ModuleList([nn.Conv1d(128, 16, 1)])
    _refused(m, "speaker_net")


def test_refuses_embedding_free_tse_on_one_side_only():
    m = _build()
    m.embedding_free_tse = True
    _refused(m, "embedding_free_tse differs")
    m = _build("cfg4_tse_short")
    m.embedding_free_tse = False
    _refused(m, "embedding_free_tse differs")


def test_refuses_per_channel_prelu():
    m = _build()
    m.masker.output_fc[0] = nn.PReLU(128)
    _refused(m, "per-channel")


def test_refuses_complex_pairing_and_constraints():
    m = _build()
    m.mask_type = m.f_type = "complex"
    _refused(m, "pairing")
    m = _build()
    m.mask_constraint = "tanh"
    _refused(m, "mask_constraint")
    m = _build()
    m.output_constraint = "clamp"
    _refused(m, "output_constraint")


def test_refuses_shapes_without_a_kernel():
    from puresound_amd import hip
    assert hip.dprnn_block_step_ok(128, 64, 20) and hip.dprnn_block_step_ok(16, 8, 5)
    assert not hip.dprnn_block_step_ok(512, 128, 20) and not hip.dprnn_block_step_ok(128, 64, 0)
    import puresound_amd.nnet as PA
    m = PA.SoTaskWrapModule(PA.FreeEncDec(32, 128, 16, output_active=True),
                            PA.DPRNN(128, 256, 128, n_blocks=1, seg_size=20, causal=True), verbose=False).eval()
    _refused(m, "(C, H, K) = (128, 256, 20)")
    m = PA.SoTaskWrapModule(PA.FreeEncDec(32, 128, 16, output_active=True),
                            PA.DPRNN(128, 64, 64, n_blocks=1, seg_size=20, causal=True), verbose=False).eval()
    _refused(m, "a mask per encoder channel")


def test_refuses_training_mode_then_cpu_tensors_last():
    m = _build()
    m.train()
    _refused(m, "training mode")
    _refused(_build(), "ROCm device")
    _refused(_build("cfg4_tse_short"), "ROCm device")


def test_length_bookkeeping():
    from puresound_amd.streaming import StreamingDPRNN
    assert StreamingDPRNN.output_length(4000, 32, 16) == dict(prime_hops=1, frames=249, emitted=3984, flushed=16)
    assert StreamingDPRNN.max_hops == 16
    with pytest.raises(ValueError):
        StreamingDPRNN.output_length(4001, 32, 16)


def test_kernel_declared_with_abi_24():
    from puresound_amd import _abi
    assert _abi.ABI_VERSION == 24
    with open(os.path.join(ROOT, "include", "puresound_hip.h")) as f:
        header = f.read()
    assert "#define PS_ABI_VERSION 24" in header
    for name in ("ps_dprnn_block_step_f32", "ps_dprnn_block_step_ok"):
        assert name in _abi.SIGNATURES and f"int {name}(" in header
    with open(os.path.join(ROOT, "puresound_amd", "csrc", "Makefile")) as f:
        assert "dprnn_step.hip" in f.read()


@pytest.mark.parametrize("seeded", [False, True])
def test_step_reference_matches_torch_modules_on_whole_segments(seeded):
    """[N, S, K, C] through nn.LSTM / nn.Linear / nn.LayerNorm with the reference model's reshapes (intra: N*S sequences of K
    frames from zero; inter: N*K sequences of S frames, from zero or from given states) against the frame loop fed in
    chunks of uneven length."""
    n, s, k, c, h = 3, 4, 5, 12, 7
    f64 = torch.float64
    intra, inter = R.make_pass(c, h, 1, f64), R.make_pass(c, h, 2, f64)
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(n, s, k, c, generator=g, dtype=f64) * 2 - 1)
    h0 = torch.rand(1, n * k, h, generator=g, dtype=f64) - 0.5 if seeded else torch.zeros(1, n * k, h, dtype=f64)
    c0 = torch.rand(1, n * k, h, generator=g, dtype=f64) - 0.5 if seeded else torch.zeros(1, n * k, h, dtype=f64)
    with torch.no_grad():
        a, (hi, ci) = intra[0](x.reshape(n * s, k, c))
        y = x + intra[2](intra[1](a)).reshape(n, s, k, c)
        b, (hn, cn) = inter[0](y.transpose(1, 2).reshape(n * k, s, c), (h0, c0))
        want = y + inter[2](inter[1](b)).reshape(n, k, s, c).transpose(1, 2)
    state = dict(h_intra=torch.rand(n, h, generator=g, dtype=f64), c_intra=torch.rand(n, h, generator=g, dtype=f64),
                 h_bank=h0.reshape(n, k, h).transpose(0, 1).clone(), c_bank=c0.reshape(n, k, h).transpose(0, 1).clone())
    frames = x.reshape(n, s * k, c).transpose(0, 1).contiguous()          # [T, N, C]
    got, t0 = [], 0
    for size in (1, 3, 7, 2, 16):
        size = min(size, s * k - t0)
        out, visited = R.block_step(frames[t0:t0 + size], t0, k, intra, inter, state)
        assert visited == {(t0 + f) % k for f in range(size)}
        got.append(out)
        t0 += size
    assert t0 == s * k
    got = torch.cat(got).transpose(0, 1).reshape(n, s, k, c)
    assert float((got - want).abs().max()) < 1e-6
    assert float((state["h_bank"].transpose(0, 1).reshape(1, n * k, h) - hn).abs().max()) < 1e-6
    assert float((state["c_bank"].transpose(0, 1).reshape(1, n * k, h) - cn).abs().max()) < 1e-6
    assert float((state["h_intra"] - hi.reshape(n, s, h)[:, -1]).abs().max()) < 1e-6
    assert float((state["c_intra"] - ci.reshape(n, s, h)[:, -1]).abs().max()) < 1e-6
