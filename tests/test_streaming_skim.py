"""StreamingSkiMExtractor (puresound_amd/streaming/skim.py) without a GPU: the frame-by-frame reference of one block step and
of a block chain (tests/skim_step_ref.py) against the reference project's own outputs and against torch's modules on whole
segments, which models the streamer refuses, its length bookkeeping, the ABI of its kernel, what the kernel's entry refuses
before any launch, and what the kernel test's inputs cost in plain fp32."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import cases
import skim_step_ref as R
from conftest import rel_max
from detweights import det_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = (1, 3, 7, 2, 16, 5, 11, 16)


def _golden_model(name, golden_dir):
    import puresound_amd.nnet as PA
    m = cases.build(PA.NS, name).eval()
    m.load_state_dict(det_state_dict(m))
    return m, dict(np.load(os.path.join(golden_dir, name + ".npz")))


def _chain(m, b, embed=None):
    blocks = [R.block_of(m, i) for i in range(m.n_blocks)]
    terms = [R.embed_terms(m, i, embed) if embed is not None else (None, None) for i in range(m.n_blocks)]
    return R.Chain(blocks, m.seg_size, b, m.hidden_size, R.slots_needed(16, m.seg_size), terms)


def _run(chain, frames):
    """frames [T, B, C] through the chain in chunks of uneven length -> [T, B, C]."""
    outs, t, i = [], 0, 0
    while t < frames.shape[0]:
        size = min(CHUNKS[i % len(CHUNKS)], frames.shape[0] - t)
        outs.append(chain.step(frames[t:t + size]))
        t, i = t + size, i + 1
    return torch.cat(outs)


# -------------------------------------------------------------------------------------------------------------------------
# (a) the reference loop is pinned by the reference project's outputs
# -------------------------------------------------------------------------------------------------------------------------
def test_chain_matches_stream_tiny_golden(golden_dir):
    """One stream, FiLM in all four blocks, 47 frames over segments of 10: the reference's offline output and its own
    frame-by-frame output."""
    m, g = _golden_model("stream_tiny", golden_dir)
    x = torch.tensor(g["x"]).double()
    y = R.output_fc(m, _run(_chain(m, 1, torch.tensor(g["embed"])), x.permute(2, 0, 1).contiguous())).numpy()
    for key in ("y_offline", "y_frame"):
        assert y.shape == g[key].shape
        assert rel_max(y, g[key]) < 1e-5, key


def test_chain_matches_skim_causal_golden_and_the_batch_leak(golden_dir):
    """Two utterances of 30 frames, three blocks, segments of 7.  Utterance 0 is the chain's output as it is.  Utterance 1 is
    NOT a function of its own frames in the reference: MemLSTM.forward shifts its result along the flattened (utterance,
    segment) axis, so utterance 1 starts segment 0 of blocks 1 and 2 from what utterance 0's hand-over made of its last, zero
    padded segment (frames 28 .. 34).  The chain reproduces the golden with that state in slot 0 of utterance 1's banks, and
    is far from it (the streamer's case: a stream on its own) without."""
    m, g = _golden_model("skim_causal", golden_dir)
    x = torch.tensor(g["x"]).double()                                  # [2, C, T]
    t, k = x.shape[2], m.seg_size
    tp = m.padded_frames_needed(t)
    assert (t, tp) == (30, 35)
    first = _chain(m, 1)
    padded = torch.zeros(tp, 1, x.shape[1], dtype=torch.float64)
    padded[:t, 0] = x[0].t()
    y0 = R.output_fc(m, _run(first, padded)[:t]).numpy()
    assert rel_max(y0[0], g["y"][0]) < 1e-5
    alone = _chain(m, 1)
    seeded = _chain(m, 1)
    slot = (tp // k) % R.slots_needed(16, k)                           # where the end of the last segment left its hand-over
    for bank, src in zip(seeded.banks[1:], first.banks[1:]):
        bank[0][0], bank[1][0] = src[0][slot], src[1][slot]
    frames = x[1].t().reshape(t, 1, -1).contiguous()
    assert rel_max(R.output_fc(m, _run(seeded, frames)).numpy()[0], g["y"][1]) < 1e-5
    assert rel_max(R.output_fc(m, _run(alone, frames)).numpy()[0], g["y"][1]) > 1e-2


# -------------------------------------------------------------------------------------------------------------------------
# (b) the same loop against torch's modules on whole segments
# -------------------------------------------------------------------------------------------------------------------------
def test_step_reference_matches_torch_modules_on_whole_segments():
    """[N, S, K, C] through nn.LSTM / nn.Linear / nn.LayerNorm with the reference model's reshapes, every utterance on its
    own: SegLSTM on N*S sequences of K frames (block 0 from zero), MemLSTM on N sequences of S segment states, its result
    shifted by one segment per utterance as block 1's initial states -- against the frame loop fed in chunks of uneven
    length."""
    n, s, k, c, h = 3, 4, 5, 12, 7
    f64 = torch.float64
    b0, b1 = R.make_block(c, h, 1, True, True, f64), R.make_block(c, h, 2, True, False, f64)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(n, s, k, c, generator=g, dtype=f64) * 2 - 1
    terms = [tuple(torch.rand(n, c, generator=g, dtype=f64) - 0.5 for _ in range(2)) for _ in range(2)]

    def film(blk, v, rs, rb):                                          # v [N, S, K, C]
        ws, wb, norm = blk["film"]
        u = norm(v)
        return (u @ ws.t() + rs[:, None, None]) * u + (u @ wb.t() + rb[:, None, None])

    with torch.no_grad():
        v = film(b0, x, *terms[0])
        lstm, proj, norm = b0["seg"]
        a, (hn, cn) = lstm(v.reshape(n * s, k, c))
        y = v + norm(proj(a)).reshape(n, s, k, c)
        init = []
        for key, st in (("h", hn), ("c", cn)):
            net, mproj, mnorm = b0["mem"][key]
            st = st.reshape(n, s, h)
            z, _ = net(st)
            o = st + mnorm(mproj(z))
            shifted = torch.zeros_like(o)
            shifted[:, 1:] = o[:, :-1]
            init.append(shifted.reshape(1, n * s, h))
        v = film(b1, y, *terms[1])
        lstm, proj, norm = b1["seg"]
        a, (h1, c1) = lstm(v.reshape(n * s, k, c), tuple(init))
        want = v + norm(proj(a)).reshape(n, s, k, c)
    chain = R.Chain([b0, b1], k, n, h, R.slots_needed(16, k), terms)
    for st in chain.states:                                            # a missed reset at frame 0 shows
        st["seg_h"].fill_(0.7)
        st["seg_c"].fill_(-0.3)
    got = _run(chain, x.reshape(n, s * k, c).transpose(0, 1).contiguous())
    assert float((got.transpose(0, 1).reshape(n, s, k, c) - want).abs().max()) < 1e-6
    assert float((chain.states[1]["seg_h"] - h1.reshape(n, s, h)[:, -1]).abs().max()) < 1e-6
    assert float((chain.states[1]["seg_c"] - c1.reshape(n, s, h)[:, -1]).abs().max()) < 1e-6
    assert float((chain.states[0]["seg_h"] - hn.reshape(n, s, h)[:, -1]).abs().max()) < 1e-6


# -------------------------------------------------------------------------------------------------------------------------
# (c) refusals
# -------------------------------------------------------------------------------------------------------------------------
def _build(name="tse_skim_vad_short", enc=None, wrap=None, **masker_kw):
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
    from puresound_amd.streaming import StreamingSkiMExtractor
    with pytest.raises(NotImplementedError) as e:
        StreamingSkiMExtractor(model)
    assert words.lower() in str(e.value).lower(), str(e.value)


def test_refuses_other_wrappers_encoders_and_windows():
    import puresound_amd.nnet as PA
    _refused(nn.Linear(2, 2), "SoTaskWrapModule")
    _refused(cases.build(PA.NS, "tiny_stft").eval(), "StreamingSeparator")
    _refused(_build(enc=dict(hop=12)), "multiple of hop")
    _refused(_build(enc=dict(win=30, hop=15)), "multiple of 4")


def test_refuses_other_maskers():
    import puresound_amd.nnet as PA
    _refused(cases.build(PA.NS, "tiny_free_relu_causal").eval(), "SkiM only")
    _refused(cases.build(PA.NS, "cfg4_short").eval(), "SkiM only")


def test_refuses_gate_fusion():
    _refused(_build(embed_fusion="Gate"), "Gate fusion")


def test_refuses_non_causal():
    _refused(_build(causal=False), "not causal")


def test_refuses_segment_overlap():
    _refused(_build(seg_overlap=True), "seg_overlap")


def test_refuses_embedding_free_tse():
    m = _build()
    m.embedding_free_tse = True
    _refused(m, "embedding_free_tse")


def test_refuses_an_embedding_input_nothing_can_feed():
    m = _build()
    m.speaker_net = None
    _refused(m, "no speaker_net")


def test_refuses_film_without_input_norm_and_per_channel_prelu():
    m = _build()
    m.masker.seg_input_fusion[1].inp_norm = False
    _refused(m, "block 1: fusion FiLM")
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
    for shape in R.SHAPES:
        assert hip.skim_block_step_ok(*shape), shape
    assert not hip.skim_block_step_ok(128, 512, 150) and not hip.skim_block_step_ok(128, 64, 0)
    import puresound_amd.nnet as PA
    m = PA.SoTaskWrapModule(PA.FreeEncDec(32, 128, 16, output_active=True),
                            PA.SkiM(128, 512, 128, n_blocks=2, seg_size=150, causal=True), verbose=False).eval()
    _refused(m, "(C, H, K) = (128, 512, 150)")
    m = PA.SoTaskWrapModule(PA.FreeEncDec(32, 128, 16, output_active=True),
                            PA.SkiM(128, 64, 64, n_blocks=2, seg_size=150, causal=True), verbose=False).eval()
    _refused(m, "a mask per encoder channel")


def test_refuses_training_mode_then_cpu_tensors_last():
    m = _build()
    m.train()
    _refused(m, "training mode")
    _refused(_build(), "ROCm device")
    import puresound_amd.nnet as PA
    plain = PA.SoTaskWrapModule(PA.FreeEncDec(32, 16, 16, output_active=True),
                                PA.SkiM(16, 8, 16, n_blocks=2, seg_size=5, causal=True), verbose=False).eval()
    _refused(plain, "ROCm device")                                     # a SkiM without an embedding input is accepted too


# -------------------------------------------------------------------------------------------------------------------------
# (d), (e) bookkeeping and declarations
# -------------------------------------------------------------------------------------------------------------------------
def test_length_bookkeeping():
    from puresound_amd.streaming import StreamingSkiMExtractor
    assert StreamingSkiMExtractor.output_length(4000, 32, 16) == dict(prime_hops=1, frames=249, emitted=3984, flushed=16)
    assert StreamingSkiMExtractor.max_hops == 16
    with pytest.raises(ValueError):
        StreamingSkiMExtractor.output_length(4001, 32, 16)


def test_kernel_declared_with_abi_24():
    from puresound_amd import _abi
    assert _abi.ABI_VERSION == 24
    with open(os.path.join(ROOT, "include", "puresound_hip.h")) as f:
        header = f.read()
    assert "#define PS_ABI_VERSION 24" in header
    for name in ("ps_skim_block_step_f32", "ps_skim_block_step_ok"):
        assert name in _abi.SIGNATURES and f"int {name}(" in header
    with open(os.path.join(ROOT, "puresound_amd", "csrc", "Makefile")) as f:
        assert "skim_step.hip" in f.read()


def test_bank_slots():
    from puresound_amd import hip
    for k, seg in ((16, 150), (16, 5), (16, 1), (1, 1), (7, 7)):
        assert hip.skim_bank_slots(k, seg) == R.slots_needed(k, seg) == (k - 1) // seg + 3


# -------------------------------------------------------------------------------------------------------------------------
# (f) what the entry refuses before any launch
# -------------------------------------------------------------------------------------------------------------------------
_BUF = C.create_string_buffer(4096 + 256)
BUF = (C.addressof(_BUF) + 255) // 256 * 256   # aligned host memory, never dereferenced: the call returns first
_DIMS = dict(C=128, H=64, K=150, NS=3, B=2, k=4, ld=128, ldb=128)
_BAD = "ps_skim_block_step_f32: bad argument (C={C} H={H} K={K} NS={NS} B={B} k={k} ld={ld} ldb={ldb}; 1 <= k <= 16)"
REFUSALS = {
    "null_x": (dict(x=None), -1, _BAD),
    "null_y": (dict(y=None), -1, _BAD),
    "null_counter": (dict(counter=None), -1, _BAD),
    "null_block": (dict(blk=None), -1, _BAD),
    "null_state": (dict(st=None), -1, _BAD),
    "x_is_y": (dict(y="x"), -1, _BAD),
    "k_0": (dict(k=0), -1, _BAD),
    "k_17": (dict(k=17, ld=256), -1, _BAD),
    "B_0": (dict(B=0), -1, _BAD),
    "chunk_past_the_row": (dict(B=40), -1, _BAD),
    "x_misaligned": (dict(x=BUF + 2), -1, "ps_skim_block_step_f32: x, y and counter must be 4-byte aligned"),
    "counter_misaligned": (dict(counter=BUF + 1), -1, "ps_skim_block_step_f32: x, y and counter must be 4-byte aligned"),
    "null_seg_h": (dict(seg_h=None), -1,
                   "ps_skim_block_step_f32: the SegLSTM needs wt, bias, pt, pbias, gamma, beta and the states seg_h, seg_c"),
    "null_seg_weight": (dict(seg_pt=None), -1,
                        "ps_skim_block_step_f32: the SegLSTM needs wt, bias, pt, pbias, gamma, beta and the states seg_h, seg_c"),
    "film_without_terms": (dict(rs=None), -1,
                           "ps_skim_block_step_f32: FiLM needs film_gamma, film_beta and the per-stream terms rs, rb"),
    "one_incoming_bank": (dict(init_c=None), -1, "ps_skim_block_step_f32: init_h and init_c go together"),
    "mem_without_bank": (dict(out_h=None), -1,
                         "ps_skim_block_step_f32: the MemLSTM needs both nets complete, the states mh_h, mc_h, mh_c, mc_c and "
                         "the banks out_h, out_c"),
    "NS_2": (dict(NS=2), -1, "ps_skim_block_step_f32: NS = 2 bank slots; k = 4 frames over segments of K = 150 need "
                             "(k - 1) / K + 3 = 3"),
    "NS_5_at_K_5": (dict(NS=5, K=5, k=16), -1, "ps_skim_block_step_f32: NS = 5 bank slots; k = 16 frames over segments of "
                                               "K = 5 need (k - 1) / K + 3 = 6"),
    "shape_without_a_kernel": (dict(H=512), -3,
                               "ps_skim_block_step_f32: (C, H, K) = (128, 512, 150): the tile of 16 columns needs "
                               "(2 max(C, H) + 2 H + max(4 H, 2 C)) * 64 bytes of LDS, 160 KiB at most"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_entry_refuses_before_any_launch(case):
    from puresound_amd import _abi
    over, rc_want, text = REFUSALS[case]
    a = dict(_DIMS, x=BUF, y=BUF + 1024, counter=BUF + 2048, blk=True, st=True)
    a.update({k: v for k, v in over.items() if k in a})
    if a["y"] == "x":
        a["y"] = a["x"]
    blk, st = _abi.SkimBlock(), _abi.SkimState()
    for p in (blk.seg, blk.mem_h, blk.mem_c):
        for name in ("wt", "bias", "pt", "pbias", "gamma", "beta"):
            setattr(p, name, BUF)
    blk.film_wt = blk.film_gamma = blk.film_beta = BUF
    for name, _ in _abi.SkimState._fields_:
        setattr(st, name, over.get(name, BUF))
    if "seg_pt" in over:
        blk.seg.pt = None
    lib = _abi.lib()
    rc = lib.ps_skim_block_step_f32(a["x"], a["y"], a["counter"], C.byref(blk) if a["blk"] else None,
                                    C.byref(st) if a["st"] else None, a["C"], a["H"], a["K"], a["NS"], a["B"], a["k"], a["ld"],
                                    a["ldb"], None)
    assert rc == rc_want
    assert lib.ps_last_error().decode() == text.format(**a)


# -------------------------------------------------------------------------------------------------------------------------
# the kernel test's inputs in plain fp32
# -------------------------------------------------------------------------------------------------------------------------
def test_kernel_cases_cover_every_axis_at_full_size_and_cost_a_third_of_the_bound_in_fp32():
    """tests/test_streaming_skim_gpu.py holds the kernel to rel_max < 1e-5 against the fp64 loop on these inputs.  The same
    loop in torch fp32 (other summation orders than the kernel's, the same precision) is 2.8e-6 from it at worst, on
    (128, 256, 150) -- under a third of the bound, with make_block's scales: make_pass's, FiLM's matrices at 0.4 / sqrt(C)
    and the LSTM matrices of a fan-in above 192 scaled down by sqrt(192 / fan-in).  With make_pass's +-0.4 everywhere it is
    1.0e-5: the gates of a 384- or 512-wide sum saturate."""
    all_cases = R.kernel_cases()
    full = [c for c in all_cases if c[:3] == (128, 256, 150)]
    assert {c[3] for c in full} == set(R.STREAMS) and {c[4] for c in full} == set(R.HOPS)
    assert {c[5] for c in full} == set(R.STARTS) and {c[6] for c in full} == set(R.VARIANTS)
    assert {c[:3] for c in all_cases} == set(R.SHAPES)
    assert any(c[:3] == (16, 8, 5) and c[4] == 16 for c in all_cases)   # one launch over three segment ends
    worst = 0.0
    for c in all_cases:
        case = R.kernel_case(*c)
        want, got = R.run_case(case), R.run_case(case, torch.float32)
        errs = [rel_max(got["out"].numpy(), want["out"].numpy())]
        errs += [rel_max(got["state"][key].numpy(), want["state"][key].numpy()) for key in want["state"]]
        if want["bank_out"] is not None:
            errs += [rel_max(a.numpy(), b.numpy()) for a, b in zip(got["bank_out"], want["bank_out"])]
        worst = max(worst, max(errs))
    print(f"the kernel test's inputs in torch fp32 against fp64: rel_max {worst:.2e} at worst")
    assert worst < 1e-5 / 3
