"""Batches of utterances of unequal length through the SkiM speaker extractors (FreeEncDec + SkiM), without a GPU: what the
host side accepts for the HIP path and what it refuses, each before any library call; ps_lstm_rows_f32's declaration and its
refusals; and the two conditions that keep the GPU test (test_ragged_skim_gpu.py) honest -- on its batch, zero-padding a
short row changes the float64 oracle's answer by far more than any bound in use, and at equal lengths the reference's causal
Mem-LSTM hands utterance n - 1's last segment to utterance n, so a path that kept the hand-over would fail there too."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

import cases
import edge_length_cases as E
import ragged_skim_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def PA():
    import puresound_amd.nnet as PA
    return PA


@pytest.fixture
def no_library(monkeypatch):
    """any call into the HIP library fails the test"""
    from puresound_amd import _abi, hip

    def lib():
        raise AssertionError("the HIP library was called")
    monkeypatch.setattr(_abi, "lib", lib)
    monkeypatch.setattr(hip, "lib", lib)


# ---- the plan: accepted for the HIP path, without a device -----------------------------------------------------------------------
@pytest.mark.parametrize("name", K.NAMES)
def test_the_host_side_accepts_the_four_presets_for_the_hip_path(PA, no_library, name):
    from puresound_amd.nnet import ragged
    model = cases.build(PA.NS, name).eval()
    lens, e_lens = [E.length_of(name, t) for t in K.SKIM_T], [E.length_of(name, t) for t in K.SKIM_ENROL_T]
    noisy, enroll = torch.zeros(len(lens), max(lens)), torch.zeros(len(lens), max(e_lens))
    ragged.check_model(model, enroll, e_lens, hip_path=True)
    rp = ragged.plan(model, noisy, enroll, lens, e_lens, hip_path=True)
    assert rp.t_rows == list(K.SKIM_T) and rp.out_lengths == [E.out_length(name, t) for t in K.SKIM_T]
    assert rp.seg_rows == [4, 1, 1, 2, 2, 3, 3, 4] == K.SEG_ROWS
    assert rp.enroll_t_rows == list(K.SKIM_ENROL_T) and rp.enroll_frames == max(K.SKIM_ENROL_T)
    assert rp.lengths == lens and rp.enroll_lengths == e_lens
    assert model.output_lengths(lens) == rp.out_lengths
    # no enrolment: the masker runs without an embedding
    assert ragged.plan(model, noisy, None, lens, None, hip_path=True).seg_rows == K.SEG_ROWS
    # the other families have no segment counts
    other = cases.build(PA.NS, "cfg2_short").eval()
    assert ragged.plan(other, torch.zeros(2, 4000), None, [4000, 2000], None, hip_path=True).seg_rows is None
    # the length values are validated as for every other model
    with pytest.raises(RuntimeError, match="input length 31 is shorter than the window 32"):
        ragged.plan(model, noisy, enroll, [31] + lens[1:], e_lens, hip_path=True)
    with pytest.raises(ValueError, match=r"enroll_lengths\[2\] = \d+ exceeds the row length"):
        ragged.plan(model, noisy, enroll, lens, e_lens[:2] + [max(e_lens) + 1] + e_lens[3:], hip_path=True)


@pytest.mark.parametrize("name", K.NAMES)
def test_cpu_tensors_are_refused(PA, no_library, name):
    """cpu_path has no SkiM: refused before any work, and the default of plan() follows the tensor"""
    from puresound_amd.nnet import ragged
    model = cases.build(PA.NS, name).eval()
    noisy, enroll = torch.zeros(2, 4000), torch.zeros(2, 3000)
    with pytest.raises(NotImplementedError, match="inference with lengths.*covered on the HIP path only"):
        model.inference(noisy, enroll, lengths=[4000, 2000], enroll_lengths=[3000, 100])
    with pytest.raises(NotImplementedError, match="HIP path only"):
        ragged.plan(model, noisy, enroll, [4000, 2000], None)
    with pytest.raises(NotImplementedError, match="HIP path only"):
        model.inference_scored_ragged(noisy, torch.zeros(2, 4000), enroll, lengths=[4000, 2000])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _skim(PA, speaker_net=None, encoder_spk=None, **kw):
    """FreeEncDec(win 16, hop 8, 24) + a two-block SkiM -> a wrapper the refusal tests vary"""
    args = dict(n_blocks=2, seg_size=10, seg_overlap=False, causal=True, embed_dim=6, embed_norm=True, block_with_embed=[1, 1],
                embed_fusion="FiLM")
    args.update(kw)
    enc = PA.FreeEncDec(win_length=16, hop_length=8, laten_length=24)
    return PA.SoTaskWrapModule(encoder=enc, masker=PA.SkiM(24, 8, 24, **args), verbose=False, speaker_net=speaker_net,
                               encoder_spk=encoder_spk, mask_constraint="ReLU").eval()


def test_what_the_skim_path_does_not_cover_is_refused_before_any_library_call(PA, no_library):
    from puresound_amd.nnet import ragged
    noisy, enroll, lens, e_lens = torch.zeros(2, 200), torch.zeros(2, 160), [200, 100], [160, 80]
    tcn = lambda c=24: nn.ModuleList([PA.TCN(c, 12, 3, 1), PA.AttentiveStatisticsPooling(c, 8),  # noqa: E731
                                      nn.Conv1d(2 * c, 6, 1, bias=False)])
    rnn = lambda kind: nn.ModuleList([PA.SingleRNN(kind, 24, 8, bidirectional=True), PA.AttentiveStatisticsPooling(24, 8),  # noqa: E731
                                      nn.Conv1d(48, 6, 1, bias=False)])

    def refused(model, text, with_enroll=True):
        e, el = (enroll, e_lens) if with_enroll else (None, None)
        with pytest.raises(NotImplementedError, match=text):
            ragged.plan(model, noisy, e, lens, el, hip_path=True)
        with pytest.raises(NotImplementedError, match="^inference with lengths"):
            ragged.check_model(model, e, el, hip_path=True)

    # the covered shapes pass
    for net in (tcn(), rnn("LSTM")):
        assert ragged.plan(_skim(PA, net), noisy, enroll, lens, e_lens, hip_path=True).seg_rows == [3, 2]
    assert ragged.plan(_skim(PA, embed_dim=0), noisy, None, lens, None, hip_path=True).seg_rows == [3, 2]
    assert ragged.plan(_skim(PA, tcn(), causal=False), noisy, enroll, lens, e_lens, hip_path=True).t_rows == [24, 11]
    refused(_skim(PA, tcn(), seg_overlap=True), "seg_overlap=True.*padding differs per row")
    refused(_skim(PA, tcn(), seg_overlap=True), "seg_overlap=True", with_enroll=False)
    refused(_skim(PA, tcn(), embed_fusion="Gate"), "Gate fusion")
    refused(_skim(PA, rnn("GRU")), "SingleRNN speaker net that is not an LSTM")
    refused(_skim(PA, rnn("RNN")), "not an LSTM")
    refused(_skim(PA), "an enrolment needs a speaker_net")
    fbank = PA.FbankEnc(trainable=False, output_format="Magnitude", n_banks=80)
    refused(_skim(PA, tcn(80), encoder_spk=fbank), "FreeEncDec enrolment encoder only \\(got FbankEnc")
    refused(cases.build(PA.NS, "tse_skim_fbank_short").eval(), "got FbankEnc")
    aug = nn.ModuleList([PA.SpecAugment(10, 0, 0.0)] + list(tcn()))
    refused(_skim(PA, aug), "SpecAugment layer.*no per-row meaning")
    refused(cases.build(PA.NS, "tse_skim_v2_short").eval(), "SpecAugment")
    gated = nn.ModuleList([PA.GatedTCN(24, 12, 3, 1), PA.AttentiveStatisticsPooling(24, 8), nn.Conv1d(48, 6, 1, bias=False)])
    refused(_skim(PA, gated), "plain TCN blocks or SingleRNN\\(LSTM\\)")
    # DPRNN stays refused in every form, on device tensors too
    for name in ("cfg4_short", "cfg4_tse_short"):
        with pytest.raises(NotImplementedError, match="^inference with lengths"):
            ragged.check_model(cases.build(PA.NS, name).eval(), None, None, hip_path=True)
    # in front of a ConvTasNet the RNN speaker net keeps its wording
    small = PA.SoTaskWrapModule(encoder=PA.FreeEncDec(win_length=16, hop_length=8, laten_length=24),
                                masker=PA.ConvTasNet(24, 6, False, tcn_kernel=3, tcn_dim=12, repeat_tcn=1, tcn_dilated_basic=2,
                                                     per_tcn_stack=2, tcn_with_embed=[1, 0]),
                                speaker_net=rnn("LSTM"), verbose=False).eval()
    refused(small, "plain TCN")


# ---- the entry ----------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_and_the_abi_number_stays():
    from puresound_amd import _abi
    header = open(f"{ROOT}/include/puresound_hip.h").read()
    assert _abi.ABI_VERSION == 24 and re.search(r"^#define PS_ABI_VERSION 24$", header, flags=re.M)
    decl = re.search(r"^int ps_lstm_rows_f32\(([^;]*)\);", header, flags=re.M | re.S)
    assert decl and [a.strip() for a in decl.group(1).split(",")] == ["const ps_lstm_args* args", "const int* steps_rows",
                                                                     "void* stream"]
    restype, argtypes = _abi.SIGNATURES["ps_lstm_rows_f32"]
    assert restype is C.c_int and len(argtypes) == 3 and argtypes[0] == C.POINTER(_abi.LstmArgs)
    assert hasattr(C.CDLL(_abi.LIB_PATH), "ps_lstm_rows_f32")
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        assert "ps_lstm_rows_f32" in open(f"{ROOT}/{doc}").read(), doc


_BUF = C.create_string_buffer(4096 + 256)
BUF = (C.addressof(_BUF) + 255) // 256 * 256   # aligned host memory, never dereferenced: the call returns first
VALID = dict(gx=BUF, whh_t=BUF, hout=BUF, h0=None, c0=None, h_last=None, c_last=None, N=2, H=64, D=2, Q=4, q_stride=20,
             steps=20, step_stride=1, ldt=128, ldq=128, state_shift=0)
INVALID, UNSUPPORTED = -1, -3   # PS_E_INVALID, PS_E_UNSUPPORTED
REFUSALS = [
    ("null_args", dict(args=None), "ps_lstm_rows_f32: null args"),
    ("null_steps_rows", dict(steps_rows=None), "ps_lstm_rows_f32: steps_rows is NULL"),
    ("state_shift_1", dict(state_shift=1), "ps_lstm_rows_f32: state_shift must be 0"),
    ("state_shift_negative", dict(state_shift=-1), "ps_lstm_rows_f32: state_shift must be 0"),
    ("ldq_below_Q", dict(h0=BUF, ldq=3), "ps_lstm_rows_f32: ldq=3 < Q=4"),
    ("h_last_ldq_below_Q", dict(h_last=BUF, ldq=2), "ps_lstm_rows_f32: ldq=2 < Q=4"),
    ("last_frame_outside", dict(Q=40), "ps_lstm_rows_f32: the last frame 799 lies outside the row (ldt=128)"),
    ("null_gx", dict(gx=None), "ps_lstm_rows_f32: bad argument (N=2 H=64 D=2 Q=4 steps=20)"),
    ("null_whh_t", dict(whh_t=None), "ps_lstm_rows_f32: bad argument (N=2 H=64 D=2 Q=4 steps=20)"),
    ("D_three", dict(D=3), "ps_lstm_rows_f32: bad argument (N=2 H=64 D=3 Q=4 steps=20)"),
    ("steps_zero", dict(steps=0), "ps_lstm_rows_f32: bad argument (N=2 H=64 D=2 Q=4 steps=0)"),
    ("step_stride_negative", dict(step_stride=-1), "ps_lstm_rows_f32: bad argument (N=2 H=64 D=2 Q=4 steps=20)"),
    ("N_65536", dict(N=65536), "ps_lstm_rows_f32: bad argument (N=65536 H=64 D=2 Q=4 steps=20)"),
    ("H_257", dict(H=257), "ps_lstm_rows_f32: hidden size 257 > 256 is not supported"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_entry_refuses_before_any_launch(case):
    """code and the whole ps_last_error() text, as include/puresound_hip.h states them"""
    from puresound_amd import _abi
    _, over, text = case
    a = dict(VALID, steps_rows=BUF)
    a.update(over)
    args = _abi.LstmArgs()
    for k, _ in _abi.LstmArgs._fields_:
        setattr(args, k, a[k])
    lib = _abi.lib()
    rc = lib.ps_lstm_rows_f32(None if "args" in over else C.byref(args), a["steps_rows"], None)
    assert rc == (UNSUPPORTED if "not supported" in text else INVALID)
    assert lib.ps_last_error().decode() == text


# ---- the float64 oracle: padding, or the hand-over, is wrong on the GPU tests' batches ------------------------------------------------
@pytest.mark.parametrize("name", ["tse_skim_v0_short", "tse_skim_causal_short"])
def test_zero_padding_a_short_row_is_wrong_on_the_gpu_tests_batch(name):
    """The oracle on the zero-padded batch against the oracle on each utterance alone: rel_max >= 1e-2 on every shorter row
    (non-causal: the backward Mem-LSTM starts in the padding; causal: the hand-over from the row above, and the speaker
    net's statistics over the padded enrolment).  Measured: >= 0.12."""
    noisy, lens, enroll, e_lens, refs = K.batch(name)
    out = K.oracle_padded(name, noisy, lens, enroll, e_lens)
    short = [n for n, t in enumerate(K.SKIM_T) if t < max(K.SKIM_T)]
    assert len(short) == len(K.SKIM_T) - 1
    for n in short:
        valid = refs[n].shape[-1]
        err = E.errors(name, out[n:n + 1, :valid].numpy(), refs[n].numpy())["rel_max"]
        print(f"{name} row {n} (T = {K.SKIM_T[n]}, T' = {K.SKIM_ENROL_T[n]}): zero-padded against alone, rel_max {err:.3e}")
        assert err >= 1e-2, (n, err)
    full = K.SKIM_T.index(max(K.SKIM_T))
    assert E.errors(name, out[full:full + 1].numpy(), refs[full].numpy())["rel_max"] < 1e-9


def test_the_causal_hand_over_crosses_utterances_at_equal_lengths():
    """Three rows of one length through the oracle as a batch against each row alone: the reference shifts the Mem-LSTM's
    states over the flattened [N * S] axis, so rows 1 and 2 start from the row above (measured 0.37 and 0.56); the non-causal
    preset has no hand-over (1e-15)."""
    for name, crossing in (("tse_skim_causal_short", True), ("tse_skim_v0_short", False)):
        noisy, lens, enroll, e_lens, refs = K.equal_batch(name)
        out = K.oracle_padded(name, noisy, lens, enroll, e_lens)
        for n in range(len(lens)):
            err = E.errors(name, out[n:n + 1, :refs[n].shape[-1]].numpy(), refs[n].numpy())["rel_max"]
            print(f"{name} row {n}: batched against alone, rel_max {err:.3e}")
            if crossing and n > 0:
                assert err >= 1e-2, (name, n, err)
            else:
                assert err < 1e-9, (name, n, err)
