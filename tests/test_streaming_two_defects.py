"""Which refusal wins when a model has two defects: the three free-encoder streamers share the checks of the wrapper, encoder
and window (streaming/_free.py check_front), of the pairing and constraints (check_back) and of a recurrent masker's head
(check_recurrent), and each keeps the checks of its own masker between them.  Every row below has one defect of a shared
helper and one that is the streamer's own (or, in the rows marked so, of another shared helper), and the whole message that
commit ae04f6f -- the three check_streamable functions written out, before the helpers -- gave for that model on the CPU."""
import pytest
import torch.nn as nn

import test_streaming_dprnn as D
import test_streaming_skim as K
import test_streaming_tcn as T


def _set(**attrs):
    def apply(model):
        for key, value in attrs.items():
            setattr(model, key, value)
    return apply


def _tcn_prelu(m):
    m.masker.tcn_list[0][1].in_conv[2] = nn.PReLU(12)


def _head_prelu(m):
    m.masker.output_fc[0] = nn.PReLU(128)


def _speaker_net(m):
    m.speaker_net = nn.ModuleList([nn.Conv1d(128, 16, 1)])


def _film_without_norm(m):
    m.masker.seg_input_fusion[1].inp_norm = False


COMPLEX = _set(mask_type="complex", f_type="complex")
CLAMP = _set(output_constraint="clamp")
TANH = _set(mask_constraint="tanh")
TRAIN = lambda m: m.train()  # noqa: E731

# (module of the streamer's CPU tests, arguments of its _build, edits of the built model, the message)
ROWS = {
    # Conv-TasNet: its PReLU slopes are looked at after the constraints, and it has no training check of its own
    "tcn per-channel PReLU, output_constraint": (T, {}, (_tcn_prelu, CLAMP),
        "StreamingConvTasNet: output_constraint 'clamp': linear or sigmoid"),
    "tcn hop, gated blocks": (T, dict(enc=dict(hop=6), tcn_layer="gated"), (),
        "StreamingConvTasNet: win = 16 is not a multiple of hop = 6"),
    "tcn pairing, embedding_free_tse": (T, {}, (COMPLEX, _set(embedding_free_tse=True)),
        "StreamingConvTasNet: embedding_free_tse (the enrolment seeds the masker) does not stream"),
    "tcn mask_constraint, global norm": (T, dict(tcn_norm="gLN"), (TANH,),
        "StreamingConvTasNet: tcn_norm 'gLN': bN1d (an affine map in eval mode) or cLN (a norm over one frame's channels) only"),
    "tcn training, per-channel PReLU": (T, {}, (TRAIN, _tcn_prelu),
        "StreamingConvTasNet: PReLU with per-channel slopes is not on the HIP path"),
    "dprnn hop, seg_overlap": (D, dict(enc=dict(hop=12), seg_overlap=True), (),
        "StreamingDPRNN: win = 32 is not a multiple of hop = 12"),
    "dprnn pairing, speaker_net": (D, {}, (COMPLEX, _speaker_net),
        "StreamingDPRNN: a speaker_net (an embedding-conditioned DPRNN) is out of scope; the enrolment enters through "
        "embedding_free_tse only"),
    "dprnn mask_constraint, embedding_free_tse on one side": (D, {}, (TANH, _set(embedding_free_tse=True)),
        "StreamingDPRNN: embedding_free_tse differs between the wrapper (True) and the masker (False)"),
    "dprnn output_constraint, not causal": (D, dict(causal=False), (CLAMP,),
        "StreamingDPRNN: the DPRNN is not causal (causal=False: bidirectional LSTMs read future frames)"),
    "dprnn output_constraint, per-channel PReLU (both shared)": (D, {}, (CLAMP, _head_prelu),
        "StreamingDPRNN: PReLU with per-channel slopes is not on the HIP path"),
    "dprnn training, pairing (both shared)": (D, {}, (TRAIN, COMPLEX),
        "StreamingDPRNN: mask pairing ('complex', 'complex'): the free encoder uses (real, real) only"),
    "skim window, Gate fusion": (K, dict(enc=dict(win=30, hop=15), embed_fusion="Gate"), (),
        "StreamingSkiMExtractor: win = 30: a multiple of 4 up to 256 (the window queue moves in float4 columns, the decoder "
        "keeps a window per stream in LDS)"),
    "skim pairing, no speaker_net": (K, {}, (COMPLEX, _set(speaker_net=None)),
        "StreamingSkiMExtractor: embed_dim = 192 but the model has no speaker_net: model.inference can hand this masker no "
        "embedding, so there is no output to reproduce"),
    "skim output_constraint, FiLM without its norm": (K, {}, (CLAMP, _film_without_norm),
        "StreamingSkiMExtractor: block 1: fusion FiLM: FiLM with its input norm, or none"),
    "skim mask_constraint, seg_overlap": (K, dict(seg_overlap=True), (TANH,),
        "StreamingSkiMExtractor: seg_overlap=True (half-overlapped segments) does not stream here"),
    "skim mask_constraint, per-channel PReLU (both shared)": (K, {}, (TANH, _head_prelu),
        "StreamingSkiMExtractor: PReLU with per-channel slopes is not on the HIP path"),
    "skim training, output_constraint (both shared)": (K, {}, (TRAIN, CLAMP),
        "StreamingSkiMExtractor: output_constraint 'clamp': linear or sigmoid"),
}


def message(row):
    from puresound_amd import streaming as S
    module, build_kw, edits, _ = ROWS[row]
    model = module._build(**build_kw)
    for edit in edits:
        edit(model)
    streamer = {T: S.StreamingConvTasNet, D: S.StreamingDPRNN, K: S.StreamingSkiMExtractor}[module]
    with pytest.raises(NotImplementedError) as e:
        streamer(model)
    return str(e.value)


@pytest.mark.parametrize("row", list(ROWS))
def test_the_first_defect_in_the_order_of_the_checks_is_reported(row):
    assert message(row) == ROWS[row][3]


def test_every_streamer_has_three_rows_with_a_defect_of_its_own():
    for prefix in ("tcn", "dprnn", "skim"):
        assert sum(r.startswith(prefix) and "both shared" not in r for r in ROWS) >= 3, prefix


if __name__ == "__main__":   # the messages of the tree it runs in, row by row
    for name in ROWS:
        got = message(name)
        print(f"{name!r}: {got!r}" + ("" if got == ROWS[name][3] else "   <-- DIFFERS"))
