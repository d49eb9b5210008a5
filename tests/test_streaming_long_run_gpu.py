"""A result does not depend on where the frame counter stands: every hop-by-hop streamer on the MI355X at device frame
counters up to the int32 limit.

The kernels read the counter only through g % R (rings), g % K and (g / K) % NS (segments, banks), comparisons with a slot's
span and the iSTFT's window sum.  So a session whose every frame index -- the device counter(s), the host's frames / _hops,
the finite span entries of its open slots -- is shifted by a multiple D of all those periods must return the BITS of its
twin at the small counter, given the same state and the same input: the samples of every call, the samples that end the
streams, and every state tensor.  Per case: a session opened normally steps W frames; twin A goes on for 8 hops (step, step,
step_chunk of 5, step) and ends its streams; twin B starts from the same snapshot shifted by D = X - 4 - W, so that its fifth
hop is frame X.  X: 2^31 / hop (the sample index passes an int), 2^32 / hop (it has wrapped once), FRAME_LIMIT - 4 (twin B ends
exactly at the limit, and one more hop is refused with nothing moved).  W = X - 4 modulo the lcm L of the periods, and at
least the model's look-back.  An idle slot keeps its span (0, 0): a slot idle since the session began, at a large counter.

ps_istft_step_f32, whose sample index used to be an int, is also run on its own from those counters, against the run from a
small counter (bits) and an fp64 overlap-add (tests/test_streaming_long_run.py restates the old index arithmetic on the CPU)."""
import copy
import gc
import math

import numpy as np
import pytest
import torch

from conftest import rel_max
from detweights import det_wave
from test_streaming_dprnn_gpu import _model as _dprnn_model
from test_streaming_skim_gpu import _model as _skim_model
from test_streaming_spectral_gpu import _model as _spectral_model
from test_streaming_tcn_gpu import _model as _tcn_model
from test_streaming_unet_tcn_gpu import _model as _unet_model

pytestmark = pytest.mark.gpu
NAN = float("nan")
I32_MAX = 2 ** 31 - 1
FRAME_LIMIT = I32_MAX - 16
B = 3                          # not a multiple of 4: the pad columns are in play


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def H():
    from puresound_amd import hip
    hip.lib()
    return hip


@pytest.fixture(autouse=True)
def _nan_in_the_allocator_cache(dev):
    """Scratch from torch.empty holds NaN, not a fresh process' zeros: uninitialised memory that reaches a result fails."""
    junk = [torch.full((1 << 22,), NAN, device=dev) for _ in range(16)]
    junk += [torch.full((n,), NAN, device=dev) for n in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20)]
    del junk
    yield


# -------------------------------------------------------------------------------------------------------------------------
# sessions: snapshot, shift, compare
# -------------------------------------------------------------------------------------------------------------------------
def _streamer(kind, dev):
    """The smallest models the streamers' own GPU test files build (through their _model helpers) -> a new streamer.
    cfg3_causal_short at its preset depth has rings of 18 .. 272 frames, lcm 24480: three blocks per stack (18, 20, 24) here."""
    from puresound_amd import streaming as S
    if kind in ("dpcrn", "dparn"):
        return S.StreamingSeparator(_spectral_model(f"ns_{kind}_short", dev)[0])
    if kind == "tcn_tiny":
        return S.StreamingConvTasNet(_tcn_model("tiny_free_relu_causal", dev)[0])
    if kind == "tcn_cfg3":
        return S.StreamingConvTasNet(_tcn_model("cfg3_causal_short", dev, per_tcn_stack=3, tcn_with_embed=(1, 0, 0))[0])
    if kind in ("dprnn_cfg4", "dprnn_cfg4_tse"):
        return S.StreamingDPRNN(_dprnn_model(kind[6:] + "_short", dev)[0])
    if kind == "skim":                                        # K = 150: the 8 hops lie inside one segment
        return S.StreamingSkiMExtractor(_skim_model("tse_skim_causal_short", dev)[0])
    if kind == "skim_tiny_k":                                 # K = 5, NS = 6: they cross a segment end, so a hand-over and its
        from test_streaming_skim_slots_gpu import _model      # bank slot (g / K) % NS are taken at the large counter
        return S.StreamingSkiMExtractor(_model("tiny_k", dev)[0])            # (imported here: that module imports this one)
    if kind == "unet_small":
        return S.StreamingUnetTcn(_unet_model("small", dev))
    assert kind == "unet_small_nodelay", kind
    return S.StreamingUnetTcn(_unet_model("small_nodelay", dev, transpose_delay=False))


def _takes_enrolment(s):
    name, model = type(s).__name__, s.model
    if name == "StreamingSeparator":
        return False
    if name == "StreamingDPRNN":
        return bool(model.embedding_free_tse)
    if name == "StreamingSkiMExtractor":
        return model.masker.embed_dim > 0
    return model.speaker_net is not None


def _periods(s, hip):
    """-> (the periods of the session's counter-addressed state, the frames its model looks back), read off the session."""
    name = type(s).__name__
    back = [s.window // s.hop_length, s.delay_frames, 4]
    if name == "StreamingSeparator":
        periods = []                                                            # shift rings only
        back += [r.shape[0] for r in s._rings.values() if r is not None]
    elif name == "StreamingConvTasNet":
        periods = [r.shape[0] for r in s._rings]
    elif name == "StreamingDPRNN":
        periods = [s.model.masker.seg_size]
        assert all(bank.shape[0] == periods[0] for pair in s._banks for bank in pair)
    elif name == "StreamingSkiMExtractor":
        k = s.model.masker.seg_size
        ns = hip.skim_bank_slots(16, k)
        assert all(bank.shape[0] == ns for pair in s._banks for bank in pair) and s._banks
        periods, back = [k * ns], back + [k]                                    # (one hand-over behind it at least)
    else:
        periods = [r.shape[0] for r in s._tcn_rings]
        back += [r.shape[0] for r in s._rings.values() if r is not None]
    return periods, max(back + periods if name != "StreamingSkiMExtractor" else back)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _snapshot(s):
    return dict(state=[t.clone() for t in s._state()], frames=s.frames, hops=s._hops,
                span=None if s._span is None else s._span.clone(), slots=copy.deepcopy(s._slots))


def _restore(s, snap, delta):
    """The session as it was at the snapshot, every frame index `delta` later."""
    for t, v in zip(s._state(), snap["state"]):
        t.copy_(v)
    s.frames, s._hops, s._finished = snap["frames"] + delta, snap["hops"] + delta, False
    s._counter += delta
    if hasattr(s, "_synth"):
        s._synth += delta
    if snap["span"] is not None:
        s._span.copy_(snap["span"])
        s._slots = copy.deepcopy(snap["slots"])
        for slot in s.active:
            row = s._span[slot].long()
            s._span[slot] = torch.where(row == I32_MAX, row, row + delta).int()


def _counters(s):
    return [t for t in (s._counter, getattr(s, "_synth", None)) if t is not None]


def _record(s, rec, what):
    """Every state tensor but the counters (bits), the counters, the span."""
    counters = _counters(s)
    rec[what] = dict(state=[_bits(t).clone() for t in s._state() if not any(t is c for c in counters)],
                     counters=[int(c) for c in counters], frames=(s.frames, s._hops),
                     span=None if s._span is None else s._span.clone().cpu().long(), idle=[i not in s.active for i in range(B)])


def _refused_at_the_limit(s, hop_in, slots):
    before = (s.frames, s._hops, [int(c) for c in _counters(s)])
    assert s.frames == FRAME_LIMIT == before[2][0]
    state = [_bits(t).clone() for t in s._state()]
    for call, x in ((s.step, hop_in), (s.step_chunk, hop_in.repeat(1, 2))):
        with pytest.raises(RuntimeError) as info:
            call(x)
        msg = str(info.value)
        assert "2**31 - 1" in msg and ("init_slots()" in msg if slots else "flush the streams" in msg and "init_streams()" in msg)
        assert ("init_streams()" in msg) != slots
    assert (s.frames, s._hops, [int(c) for c in _counters(s)]) == before
    assert all(torch.equal(_bits(t), v) for t, v in zip(s._state(), state))


def _twin_block(s, x, at_limit):
    """8 hops and the flush of a block session -> (the samples of every call, records of the state)."""
    hop, rec = s.hop_length, {}
    cut = lambda a, b: x[:, a * hop:b * hop].contiguous()  # noqa: E731
    outs = [s.step(cut(0, 1)), s.step(cut(1, 2)), s.step_chunk(cut(2, 7)), s.step(cut(7, 8))]
    _record(s, rec, "after 8 hops")
    if at_limit:
        _refused_at_the_limit(s, cut(0, 1), slots=False)
    outs.append(s.flush())
    _record(s, rec, "after flush")
    return outs, rec


def _twin_slots(s, x, enrol, at_limit, drain):
    """8 hops of a slot session: slot 0 carries a stream from before, is ended 5 - D hops before the last hop's end and closed
    after it; slot 1 is opened before the third hop, and leaves the session's own way (D = delay_frames more hops when the
    model has a delay; `drain` = False: neither twin takes them, because at the limit they do not exist, and there close()
    says so); slot 2 stays idle.  Idle rows, a row
    after its stream's end and the drain hops are fed NaN."""
    hop, D, rec = s.hop_length, s.delay_frames, {}

    def feed(a, b, upto0, with1):
        chunk = torch.full((B, (b - a) * hop), NAN, device=x.device)
        if upto0 > a:
            chunk[0, :(min(b, upto0) - a) * hop] = x[0, a * hop:min(b, upto0) * hop]
        if with1:
            chunk[1] = x[1, a * hop:b * hop]
        return chunk

    outs = [s.step(feed(0, 1, 8, False)), s.step(feed(1, 2, 8, False))]
    s.open(1, **enrol)                                        # birth = counter + window / hop - 1, added on the device
    s.end(0, 5 - D)                                           # death = counter + 5 - D, likewise
    last0 = 2 + 5 - D
    outs += [s.step_chunk(feed(2, 7, last0, True)), s.step(feed(7, 8, last0, True))]
    _record(s, rec, "after 8 hops")
    if at_limit:
        _refused_at_the_limit(s, feed(0, 1, 8, True), slots=True)
    outs.append(s.close(0))
    if D == 0:
        outs.append(s.close(1))
    elif drain:
        s.end(1, 0)
        outs += [s.step_chunk(torch.full((B, D * hop), NAN, device=x.device)), s.close(1)]
    elif at_limit:
        assert s.frames + D > FRAME_LIMIT
        with pytest.raises(RuntimeError, match=f"step {D} more hops"):
            s.close(1)
    _record(s, rec, "after the closes")
    return outs, rec


SESSIONS = [  # (model, slot session, captured graph): one captured case per streamer, the rest eager
    ("dpcrn", False, True), ("dparn", False, False),
    ("tcn_tiny", False, False), ("tcn_tiny", True, True), ("tcn_cfg3", False, False), ("tcn_cfg3", True, False),
    ("dprnn_cfg4", False, True), ("dprnn_cfg4", True, False), ("dprnn_cfg4_tse", False, False), ("dprnn_cfg4_tse", True, False),
    ("skim", False, False), ("skim", True, False), ("skim_tiny_k", False, False), ("skim_tiny_k", True, True),
    ("unet_small", False, True), ("unet_small", True, False), ("unet_small_nodelay", False, False),
    ("unet_small_nodelay", True, False)]
THRESHOLDS = ["2^31/hop", "2^32/hop", "limit-4"]


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("kind,slots,graph", SESSIONS,
                         ids=[f"{k}-{'slots' if sl else 'block'}-{'graph' if g else 'eager'}" for k, sl, g in SESSIONS])
def test_a_session_shifted_to_a_large_counter_returns_the_bits_of_its_twin(dev, H, kind, slots, graph, threshold):
    s = _streamer(kind, dev)
    hop = s.hop_length
    X = {"2^31/hop": 2 ** 31 // hop, "2^32/hop": 2 ** 32 // hop, "limit-4": FRAME_LIMIT - 4}[threshold]
    assert 2 ** 31 % hop == 0 and X <= FRAME_LIMIT - 4        # (every case's hop is a power of two: X * hop is the edge itself)
    enrol = lambda seed, n: ({"enroll": det_wave(seed, n, 3000).to(dev)} if _takes_enrolment(s) else {})  # noqa: E731
    if slots:
        s.init_slots(B, use_graph=graph)
        s.open(0, **{k: v[0] for k, v in enrol(901, 1).items()})
    else:
        s.init_streams(B, use_graph=graph, **enrol(901, B))
    periods, back = _periods(s, H)
    L = math.lcm(1, *periods)
    assert L <= 500, (periods, L)
    W = back + (X - 4 - back) % L                              # the frames before the snapshot: W = X - 4 (mod L), W >= back
    delta = X - 4 - W
    assert delta % L == 0 and all(delta % p == 0 for p in periods) and delta > 2 ** 20 and W >= back
    print(f"long_run {kind} {'slots' if slots else 'block'} {'graph' if graph else 'eager'} hop={hop} X={threshold}={X}: "
          f"periods={periods} L={L} W={W} delta={delta}")

    lead = W + (0 if slots else s._fill_hops)                  # hops up to the snapshot
    x = det_wave(902, B, lead * hop).to(dev)
    if slots:
        x[1:] = NAN
    for i in range(0, lead, 16):
        s.step_chunk(x[:, i * hop:min(i + 16, lead) * hop].contiguous())
    assert s.frames == W == int(s._counter)
    snap = _snapshot(s)
    x8 = det_wave(903, B, 8 * hop).to(dev)
    one = {k: v[0] for k, v in enrol(904, 1).items()}
    drain = threshold != "limit-4"
    twin = (lambda at_limit: _twin_slots(s, x8, one, at_limit, drain)) if slots else (lambda at_limit: _twin_block(s, x8, at_limit))

    # The state tensors are compared in every bit, the pad columns of a ring included, and those hold whatever the allocator's
    # block held before: the same for both twins as long as the allocator's pool does not change between them.  So sessions
    # of earlier cases that died in a reference cycle (the tracebacks pytest.raises keeps) give their device memory back now,
    # and no cyclic collection runs between the twins.
    gc.collect()
    gc.disable()
    try:
        outs_a, rec_a = twin(False)
        _restore(s, snap, delta)
        assert int(s._counter) == X - 4 == s.frames
        outs_b, rec_b = twin(threshold == "limit-4")
    finally:
        gc.enable()

    assert len(outs_a) == len(outs_b)
    for i, (a, b) in enumerate(zip(outs_a, outs_b)):
        assert a.shape == b.shape and bool(torch.isfinite(a).all()), i
        assert torch.equal(_bits(a), _bits(b)), f"samples of call {i} differ"
    assert float(torch.cat([o.reshape(-1) for o in outs_a]).abs().max()) > 1e-4      # (not a comparison of zeros)
    assert rec_a.keys() == rec_b.keys()
    for what in rec_a:
        a, b = rec_a[what], rec_b[what]
        assert [c + delta for c in a["counters"]] == b["counters"], what
        assert tuple(f + delta for f in a["frames"]) == b["frames"], what
        for i, (u, v) in enumerate(zip(a["state"], b["state"])):
            assert torch.equal(u, v), f"{what}: state tensor {i} of _state() without the counters differs"
        if a["span"] is not None:
            idle = torch.tensor(a["idle"])[:, None]
            assert a["idle"] == b["idle"]
            assert torch.equal(b["span"], torch.where((a["span"] == I32_MAX) | idle, a["span"], a["span"] + delta)), what
            assert bool((a["span"][idle[:, 0]] == 0).all())


# -------------------------------------------------------------------------------------------------------------------------
# the near-limit blocks of the slot rule tests (test_streaming_slots_gpu.py, _dprnn_slots_gpu.py, _skim_slots_gpu.py)
# -------------------------------------------------------------------------------------------------------------------------
def chunk_at_counter(s, counter, slot, chunk, snap=None):
    """Put the session at frame `counter` with the stream in `slot` born there (from `snap`, a _snapshot, when given), run
    step_chunk(chunk) -> its samples.  Two counters that agree modulo the session's periods must give the same bits: the
    stream has no frame before `counter`, so nothing older is read."""
    if snap is not None:
        _restore(s, snap, 0)
    s._counter.fill_(counter)
    s.frames = counter
    s._span[slot, 0] = counter
    return s.step_chunk(chunk)


def same_bits_at_a_small_counter(s, H, near, slot, chunk):
    """What the near-limit blocks add to `isfinite`: the chunk at frame `near` against the same chunk, from the same state,
    at the smallest counter that agrees with `near` modulo every period -> the samples at `near` (the session goes on
    from there)."""
    periods, _ = _periods(s, H)
    L = math.lcm(1, *periods)
    snap = _snapshot(s)
    small = chunk_at_counter(s, near % L + L, slot, chunk)
    y = chunk_at_counter(s, near, slot, chunk, snap)
    assert torch.equal(_bits(y), _bits(small)) and float(y[slot].abs().max()) > 0
    return y


# -------------------------------------------------------------------------------------------------------------------------
# ps_istft_step_f32 on its own
# -------------------------------------------------------------------------------------------------------------------------
def _rand(shape, seed):
    g = np.random.Generator(np.random.Philox(key=seed))
    return torch.tensor(g.uniform(-1.0, 1.0, shape), dtype=torch.float32)


@pytest.mark.parametrize("n_fft,hop,b", [(64, 16, 3), (48, 48, 2)])
def test_istft_step_from_counters_up_to_the_limit(dev, H, n_fft, hop, b):
    """6 steps and the flush from each starting counter: the bits of the run from n_fft / hop (same tail, same frames), which
    is the fp64 overlap-add over the full window-square sum within the bound of test_istft_step_kernel.  (48, 48): no
    overlap, one term per sum, an empty flush."""
    keep, steps = n_fft - hop, 6
    window = torch.hann_window(n_fft)
    frames, tail0 = _rand((steps, b, n_fft), 7 * n_fft + hop), _rand((b, keep), 7 * n_fft + hop + 1)
    ldb = H.padded_frames(b)

    def run(start):
        tail = tail0.clone().to(dev)
        counter = torch.tensor([start], dtype=torch.int32, device=dev)
        out = torch.empty(b, steps * hop, device=dev)
        syn = torch.full((1, n_fft, ldb), NAN, device=dev)
        for i in range(steps):
            syn[0, :, :b] = frames[i].t()
            H.istft_step(syn, window.to(dev), tail, out[:, i * hop:(i + 1) * hop], counter, hop, "none")
            counter += 1
        last = torch.empty(b, keep, device=dev)
        H.istft_step(None, window.to(dev), tail, last, counter, hop, "none", flush=True)
        assert int(counter) == start + steps
        return torch.cat([out, last], dim=1).cpu()

    base = run(n_fft // hop)
    w = window.double().numpy()
    acc = np.zeros((b, steps * hop + keep))
    acc[:, :keep] = tail0.double().numpy()
    for i in range(steps):
        acc[:, i * hop:i * hop + n_fft] += frames[i].double().numpy() * w / n_fft
    wsum = np.array([sum(w[i] ** 2 for i in range(j % hop, n_fft, hop)) for j in range(hop)])      # every covering frame
    wsum = np.tile(wsum, steps + keep // hop)
    for j in range(keep):                                        # after the last frame: only the frames that reach it
        wsum[steps * hop + j] = sum(w[i] ** 2 for i in range(j + hop, n_fft, hop))
    ref = np.where(wsum > 1e-10, acc / np.where(wsum > 1e-10, wsum, 1.0), acc)
    assert base.shape == ref.shape == (b, steps * hop + keep)
    err = rel_max(base.numpy(), ref)
    print(f"istft_step n_fft={n_fft} hop={hop} B={b} from counter {n_fft // hop}: rel_max {err:.2e}")
    assert err <= 1e-6
    for start in (2 ** 31 // hop - 3, 2 ** 32 // hop - 3, FRAME_LIMIT - steps):
        assert start + steps <= FRAME_LIMIT
        assert torch.equal(_bits(run(start)), _bits(base)), start
