"""The cases of tests/recurrent_calls.txt: one direct call of _plans.lstm_path or SingleRNN.forward_padded per branch of the
choice "which input-projection GEMM, in which layout, feeding which recurrence entry", and per branch of _proj_norm behind it.
Shared by test_recurrent_calls_gpu.py (which makes the calls and holds them against the ledger) and test_lstm_route.py (which
holds _plans.lstm_route against the same ledger without a GPU).  Data, and the switch setter both tests use: nothing here
needs the library or a device.

A walk is (N, Q, q_stride, steps, step_stride, t); the rows are ldt = padded_frames(t) = 128 frames long in every case."""
import contextlib
import os

from puresound_amd._abi import padded_frames

LEDGER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "recurrent_calls.txt")

SEGMENTS = (2, 6, 20, 20, 1, 120)
ACROSS = (2, 20, 1, 6, 20, 120)
MAP = (2, 5, 1, 4, 32, 128)           # q * steps < t: _h_rows keeps a zeroed buffer for the frames no sequence writes
MAP_OTHER = (2, 4, 1, 3, 32, 128)     # a second geometry in the same rows: the kept buffer is cleared
SEQS_128 = (2, 64, 2, 2, 1, 128)      # N * Q = 128: the count from which the fp32 arithmetic takes ps_lstm_h256_f32
SEQS_127 = (127, 1, 0, 4, 1, 4)
COOP = (2, 3, 30, 30, 1, 90)          # a walk the cooperative kernel takes (tools/lstm_dispatch_cases.py: COOP)
PER_FRAME = (1, 3, 1, 1, 0, 3)        # one step per stream with carried states, as the SkiM streamer launches a hop


def utterances(n, t):
    """SingleRNN's walk: one sequence per utterance over its t frames."""
    return (n, 1, padded_frames(t), t, 1, t)


# recurrence kernel of a route -> the C entries that may run it (fmajor256: the wrapper picks the cooperative kernel by itself)
KERNEL_ENTRIES = {
    "generic": {"ps_lstm_f32"}, "generic_f16x2": {"ps_lstm_f16x2_f32"}, "fmajor128": {"ps_lstm_fmajor_f16x2_f32"},
    "fmajor256": {"ps_lstm_fmajor_h256_f16x2_f32", "ps_lstm_fmajor_coop_f16x2_f32"}, "h256_f32": {"ps_lstm_h256_f32"},
    "rnn": {"ps_rnn_f32"},
}
# (GEMM arithmetic, pre-activation layout) of a route -> the C entry of the input projection
GEMM_ENTRIES = {("fp32", "rows"): "ps_conv1x1_f32", ("bf16", "rows"): "ps_conv1x1_bf16_io",
                ("f16x2", "rows"): "ps_conv1x1_f16x2_f32", ("f16x2", "fmajor"): "ps_conv1x1_f16x2_fmajor_f32"}
# branch of _proj_norm (or SingleRNN's plain projection) -> the C entries behind the recurrence, in order
PROJ_ENTRIES = {
    "fused": ["ps_proj_layernorm_f32"], "fused_amax": ["ps_proj_layernorm_amax_parts", "ps_proj_layernorm_amax_f32"],
    "gemm_ln": ["ps_conv1x1_f16x2_ln_ok", "ps_conv1x1_f16x2_ln_f32"],
    "gemm_ln_amax": ["ps_conv1x1_f16x2_ln_ok", "ps_conv1x1_stats_parts", "ps_conv1x1_f16x2_ln_f32"],
    "f16x2+ln": ["ps_conv1x1_f16x2_f32", "ps_chan_layernorm_f32"], "fp32+ln": ["ps_conv1x1_f32", "ps_chan_layernorm_f32"],
    "plain": ["ps_conv1x1_f32"], "plain_f16x2": ["ps_conv1x1_f16x2_f32"],
}
NO_FUSED = {"_plans.FUSE_PROJ_LN_MAX_FRAMES": 0}


def _case(name, call, gemm, hidden, dirs, walk, route, proj, chans=64, kind="LSTM", states=None, state_shift=0, amax=None,
          any_size=False, switches=None, skip=True, then=()):
    """route = (GEMM arithmetic, bf16 planes, layout, recurrence kernel) the case is meant to take, proj = the branch behind it.
    states: None | "init" (h0, c0, want_state) | "carried" (h0, c0 and state_out the same tensors).  amax: None | "empty"
    ([None]) | "measured" ([hip.absmax(x, t)]).  then: further walks run on the same plan after the first."""
    return dict(name=name, call=call, gemm=gemm, H=hidden, D=dirs, walk=walk, route=route, proj=proj, C=chans, kind=kind,
                states=states, state_shift=state_shift, amax=amax, any_size=any_size, switches=switches or {}, skip=skip,
                then=tuple(then))


FP32 = ("fp32", 0, "rows", "generic")
F16 = ("f16x2", 0, "rows", "generic_f16x2")
FM256 = ("f16x2", 0, "fmajor", "fmajor256")
CASES = [_case(f"path fp32 H=64 D={d} {name}", "lstm_path", "fp32", 64, d, walk, FP32, "fused", then=then)
         for d in (1, 2) for name, walk, then in (("segments", SEGMENTS, ()), ("across", ACROSS, ()),
                                                  ("map", MAP, (MAP_OTHER, MAP)))]
CASES += [
    _case("path fp32 H=256 128 sequences, states shifted", "lstm_path", "fp32", 256, 1, SEQS_128,
          ("fp32", 0, "rows", "h256_f32"), "fused", states="init", state_shift=1),
    _case("path fp32 H=256 127 sequences", "lstm_path", "fp32", 256, 1, SEQS_127, FP32, "fused"),
    _case("path fp32 H=192 D=1 128 sequences", "lstm_path", "fp32", 192, 1, SEQS_128, FP32, "fused"),
    _case("path fp32 H=192 D=2 128 sequences", "lstm_path", "fp32", 192, 2, SEQS_128, ("fp32", 0, "rows", "h256_f32"), "fused"),
    _case("path fp32 H=256 H256_F32_LSTM off", "lstm_path", "fp32", 256, 1, SEQS_128, FP32, "fused",
          switches={"hip.H256_F32_LSTM": False}),
    _case("path bf16x3", "lstm_path", "bf16x3", 64, 1, SEGMENTS, ("bf16", 3, "rows", "generic"), "fused"),
    _case("path bf16", "lstm_path", "bf16", 64, 1, SEGMENTS, ("bf16", 1, "rows", "generic"), "fused"),
    _case("path bf16x3 I=32", "lstm_path", "bf16x3", 64, 1, SEGMENTS, FP32, "fused", chans=32),
    _case("path fp16x2 H=64 no amax", "lstm_path", "fp16x2", 64, 1, SEGMENTS, F16, "fused"),
    _case("path fp16x2 H=64 amax empty", "lstm_path", "fp16x2", 64, 1, SEGMENTS, F16, "fused", amax="empty"),
    _case("path fp16x2 H=64 amax measured", "lstm_path", "fp16x2", 64, 1, SEGMENTS, F16, "fused", amax="measured"),
    _case("path fp16x2 H=64 t=128 amax empty", "lstm_path", "fp16x2", 64, 1, MAP, F16, "fused_amax", amax="empty"),
    _case("path fp16x2 H=64 I=32", "lstm_path", "fp16x2", 64, 1, SEGMENTS, ("fp32", 0, "rows", "generic_f16x2"), "fused",
          chans=32),
    _case("path fp16x2 H=128", "lstm_path", "fp16x2", 128, 1, SEGMENTS, ("f16x2", 0, "fmajor", "fmajor128"), "fused",
          chans=128, any_size=True),
    _case("path fp16x2 H=128 with h0", "lstm_path", "fp16x2", 128, 1, SEGMENTS, F16, "fused", chans=128, any_size=True,
          states="init"),
    _case("path fp16x2 H=128 FMAJOR_LSTM off", "lstm_path", "fp16x2", 128, 1, SEGMENTS, F16, "fused", chans=128,
          any_size=True, switches={"_plans.FMAJOR_LSTM": False}),
    _case("path fp16x2 H=256 D=1 cooperative walk", "lstm_path", "fp16x2", 256, 1, COOP, FM256, "fused", any_size=True),
    _case("path fp16x2 H=192 D=2 cooperative walk", "lstm_path", "fp16x2", 192, 2, COOP, FM256, "fused", any_size=True),
    _case("path fp16x2 H=256 D=1 per frame, carried", "lstm_path", "fp16x2", 256, 1, PER_FRAME, FM256, "fused",
          any_size=True, states="carried"),
    _case("path fp16x2 H=192 D=2 per frame, carried", "lstm_path", "fp16x2", 192, 2, PER_FRAME, FM256, "fused",
          any_size=True, states="carried"),
    _case("proj GEMM + LayerNorm launch, amax", "lstm_path", "fp16x2", 64, 2, SEGMENTS, F16, "gemm_ln_amax", chans=128,
          any_size=True, amax="empty", switches=NO_FUSED),
    _case("proj GEMM + LayerNorm launch", "lstm_path", "fp16x2", 64, 2, SEGMENTS, F16, "gemm_ln", chans=128, any_size=True,
          switches=NO_FUSED),
    _case("proj fp16x2 GEMM, LayerNorm", "lstm_path", "fp16x2", 64, 1, SEGMENTS, F16, "f16x2+ln", switches=NO_FUSED),
    _case("proj fp32 GEMM, LayerNorm", "lstm_path", "fp32", 64, 1, SEGMENTS, FP32, "fp32+ln", switches=NO_FUSED),
    _case("proj fp32 GEMM, LayerNorm, no skip", "lstm_path", "fp32", 64, 1, SEGMENTS, FP32, "fp32+ln", switches=NO_FUSED,
          skip=False),
    _case("single fp16x2 H=192 D=2", "single_rnn", "fp16x2", 192, 2, utterances(2, 90), FM256, "plain_f16x2", any_size=True),
    _case("single fp16x2 H=64", "single_rnn", "fp16x2", 64, 1, utterances(2, 90), ("bf16", 3, "rows", "generic"), "plain"),
    _case("single fp16x2 H=192 FMAJOR_LSTM off", "single_rnn", "fp16x2", 192, 1, utterances(2, 90), FM256, "plain_f16x2",
          any_size=True, switches={"_plans.FMAJOR_LSTM": False}),
    _case("single fp32 H=64", "single_rnn", "fp32", 64, 1, utterances(2, 90), FP32, "plain"),
    _case("single fp32 H=256 128 utterances", "single_rnn", "fp32", 256, 1, utterances(128, 4),
          ("fp32", 0, "rows", "h256_f32"), "plain"),
    _case("single fp32 H=256 127 utterances", "single_rnn", "fp32", 256, 1, utterances(127, 4), FP32, "plain"),
    _case("single bf16", "single_rnn", "bf16", 64, 1, utterances(2, 90), ("bf16", 1, "rows", "generic"), "plain"),
    _case("single GRU H=8", "single_rnn", "fp32", 8, 1, utterances(2, 90), ("fp32", 0, "rows", "rnn"), "plain", chans=16,
          kind="GRU"),
    _case("single RNN H=8", "single_rnn", "fp32", 8, 2, utterances(2, 90), ("fp32", 0, "rows", "rnn"), "plain", chans=16,
          kind="RNN"),
]
assert len({c["name"] for c in CASES}) == len(CASES)
# every branch the ledger is meant to hold: each route of the masker's and of the standalone choice, each branch behind it
WANTED_ROUTES = {FP32, F16, FM256, ("fp32", 0, "rows", "h256_f32"), ("bf16", 3, "rows", "generic"), ("bf16", 1, "rows", "generic"),
                 ("fp32", 0, "rows", "generic_f16x2"), ("f16x2", 0, "fmajor", "fmajor128"), ("fp32", 0, "rows", "rnn")}


@contextlib.contextmanager
def switched(pairs):
    """Module attributes ("hip.lib", "_plans.FMAJOR_LSTM", ...) set for the block and put back after it."""
    from puresound_amd import hip
    from puresound_amd.nnet import _plans
    mods, old = {"hip": hip, "_plans": _plans}, []
    try:
        for key, value in pairs.items():
            mod, name = key.split(".")
            old.append((mods[mod], name, getattr(mods[mod], name)))
            setattr(mods[mod], name, value)
        yield
    finally:
        for mod, name, value in reversed(old):
            setattr(mod, name, value)
