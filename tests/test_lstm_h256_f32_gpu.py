"""ps_lstm_h256_f32 through hip.lstm_h256_f32 against a float64 LSTM recurrence written here (gates i, f, g, o; direction 1
walks the steps backwards; initial states in the state layout; state_shift), next to the generic kernel it replaces.

Inputs are deterministic: W_hh = 2 u^3 and pre-activations 30 u^3 with u uniform in [-1, 1) -- most values small, |W| up to 2,
pre-activations out to +-30, so gates saturate in both directions.

Bound, on the same inputs: e_new = rel_max(new, fp64), e_gen = rel_max(hip.lstm(..., f16x2=False), fp64);
e_new <= max(2 e_gen, 4 * 2^-24).  Both kernels form the same H-term fp32 sums in different orders -- a factor of 2 is the spread
two such orders show -- and the floor, 4 ulp at the output's maximum, keeps a case the generic kernel happens to round perfectly
from failing the new one.  Every case prints both errors and, where its header allows the inputs, the fp16x2 sibling's.

Every launch writes into a NaN-filled hout: the frames of the walk must come back finite, every other frame still NaN."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_max
from puresound_amd import hip

pytestmark = pytest.mark.gpu
FLOOR = 4 * 2.0 ** -24
HD = [(256, 1), (256, 2), (192, 1), (192, 2)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _u3(shape, seed, scale):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1
    return (u ** 3 * scale).float()


@functools.lru_cache(maxsize=None)
def _weights(h, d, w_scale=2.0):
    """-> (whh_t [D, H, 4H] on the CPU, the same on the GPU, its fp32 image, the fp16x2 sibling's image and scales)"""
    whh_t = _u3((d, h, 4 * h), 1000 + h + d, w_scale)
    on = whh_t.cuda()
    return whh_t, on, hip.pack_whh_h256_f32(on), hip.pack_whh_h256(on)


def lstm_fp64(gx, whh_t, h, d, q, q_stride, steps, step_stride, h0=None, c0=None, state_shift=0):
    """-> (hout [N, D*H, ldt] with NaN off the walk, h_last, c_last [N, D*H, Q]), all float64"""
    n, _, ldt = gx.shape
    gx, w = gx.double(), whh_t.double()
    hout = torch.full((n, d * h, ldt), float("nan"), dtype=torch.float64)
    h_last, c_last = torch.zeros(n, d * h, q, dtype=torch.float64), torch.zeros(n, d * h, q, dtype=torch.float64)
    b = torch.arange(n * q)
    nn_, qq = b // q, b % q
    for di in range(d):
        rows = slice(di * h, (di + 1) * h)
        hs, cs = torch.zeros(n * q, h, dtype=torch.float64), torch.zeros(n * q, h, dtype=torch.float64)
        src = b - state_shift
        ok = src >= 0
        for given, into in ((h0, hs), (c0, cs)):
            if given is not None:
                into[ok] = given.double()[src[ok] // q, rows, src[ok] % q]
        for s in range(steps):
            f = qq * q_stride + (steps - 1 - s if di == 1 else s) * step_stride
            gates = gx[nn_, di * 4 * h:(di + 1) * 4 * h, f] + hs @ w[di]
            i, fg, g, o = gates.split(h, dim=1)
            cs = torch.sigmoid(fg) * cs + torch.sigmoid(i) * torch.tanh(g)
            hs = torch.sigmoid(o) * torch.tanh(cs)
            hout[nn_, rows, f] = hs
        h_last[nn_, rows, qq], c_last[nn_, rows, qq] = hs, cs
    return hout, h_last, c_last


def run(dev, what, h, d, n, q, q_stride, steps, step_stride, ldt, states="none", state_shift=0, h0_scale=1.0, seed=0,
        sibling=True, w_scale=2.0):
    """One launch of the new entry, the generic kernel and the fp64 recurrence on the same inputs; asserts the bound, the
    overwrite rule and the final states.  -> (hout of the new entry, its final states or None)"""
    whh_cpu, whh, image, (img16, sc16) = _weights(h, d, w_scale)
    gx = _u3((n, d * 4 * h, ldt), 7 * seed + 31 * n + q + steps + h + d, 30.0)
    walk = (q, q_stride, steps, step_stride)
    assert hip.lstm_h256_f32_ok(n, ldt, h, d, *walk, state_shift=state_shift)
    h0 = c0 = None
    if states in ("given", "alias", "shift"):
        h0 = torch.zeros(n, d * h, hip.padded_frames(q))
        c0 = torch.zeros_like(h0)
        h0[..., :q] = _u3((n, d * h, q), seed + 5, h0_scale)
        c0[..., :q] = _u3((n, d * h, q), seed + 6, 3.0)
    want_state = states in ("wanted", "shift", "given")
    ref, ref_h, ref_c = lstm_fp64(gx, whh_cpu, h, d, *walk, h0, c0, state_shift)
    covered = ~torch.isnan(ref)

    def launch(fn, weight):
        out = torch.full((n, d * h, ldt), float("nan"), device=dev)
        kw = dict(h0=None if h0 is None else h0.to(dev), c0=None if c0 is None else c0.to(dev), want_state=want_state,
                  state_shift=state_shift, out=out)
        if states == "alias":   # the final states land on the initial ones
            kw["state_out"] = (kw["h0"], kw["c0"])
        got, st = fn(gx.to(dev), *weight, *walk, **kw)
        assert got is out
        return got.cpu(), None if st is None else tuple(s.cpu()[..., :q] for s in st)

    new, new_st = launch(hip.lstm_h256_f32, (image, d))
    gen, gen_st = launch(lambda g, w, *a, **k: hip.lstm(g, w, h, d, *a, f16x2=False, **k), (whh,))
    assert torch.isfinite(new[covered]).all(), f"{what}: a frame of the walk was not written (or not finite)"
    assert torch.isnan(new[~covered]).all(), f"{what}: a frame outside the walk was written"
    e_new, e_gen = rel_max(new[covered], ref[covered]), rel_max(gen[covered], ref[covered])
    e_16 = float("nan")
    if sibling and h0_scale < 32:   # (the fp16x2 sibling's header: |h0| < 32)
        out16 = torch.full((n, d * h, ldt), float("nan"), device=dev)
        hip.lstm_fmajor_h256(gx.to(dev).transpose(1, 2).contiguous(), img16, sc16, d, *walk,
                             h0=None if h0 is None else h0.to(dev), c0=None if c0 is None else c0.to(dev),
                             state_shift=state_shift, out=out16)
        e_16 = rel_max(out16.cpu()[covered], ref[covered])
    print(f"H256F32 H={h} D={d} {what}: e_new={e_new:.3e} e_gen={e_gen:.3e} e_f16x2={e_16:.3e}")
    assert e_new <= max(2 * e_gen, FLOOR), (what, e_new, e_gen)
    if new_st is not None:
        for got, base, want in zip(new_st, gen_st, (ref_h, ref_c)):
            assert rel_max(got, want) <= max(2 * rel_max(base, want), FLOOR), what
    return new, new_st


@pytest.mark.parametrize("h,d", HD)
@pytest.mark.parametrize("n,q", [(1, 1), (3, 5), (2, 8), (1, 17), (3, 11)])
def test_sequence_counts_around_the_group_of_16(dev, h, d, n, q):
    """1, 15, 16, 17 and 33 sequences: a lone lane, the ragged last group and its replayed lanes, groups that span utterances."""
    assert n * q in (1, 15, 16, 17, 33)
    run(dev, f"seqs={n * q}", h, d, n, q, 3, 3, 1, 3 * q + 2, seed=1)


@pytest.mark.parametrize("h,d", HD)
@pytest.mark.parametrize("steps", [1, 2, 3, 4, 5, 9])
def test_step_counts_around_the_prefetch(dev, h, d, steps):
    run(dev, f"steps={steps}", h, d, 1, 17, steps, steps, 1, 17 * steps + 1, seed=2)


K, S = 7, 5
WALKS = {
    "intra": (4, S, K, K, 1, S * K + 1),            # Q = S segments of K consecutive frames
    "inter": (3, K, 1, S, K, S * K + 3),            # Q = K positions, S steps K frames apart
    "single_t5": (3, 1, 9, 5, 1, 9),                # SingleRNN: one sequence per utterance, q_stride = ldt
    "single_t130": (3, 1, 133, 130, 1, 133),        # ... over 130 frames of a 133-frame row (neither a multiple of 4)
    "single_t130_ldt130": (2, 1, 130, 130, 1, 130), # the last frame is the row's last
}


@pytest.mark.parametrize("h,d", HD)
@pytest.mark.parametrize("walk", sorted(WALKS))
def test_walks_of_the_models(dev, h, d, walk):
    n, q, q_stride, steps, step_stride, ldt = WALKS[walk]
    run(dev, walk, h, d, n, q, q_stride, steps, step_stride, ldt, seed=3)


@pytest.mark.parametrize("h,d", HD)
@pytest.mark.parametrize("states", ["none", "given", "given_1e3", "wanted", "alias"])
def test_initial_and_final_states(dev, h, d, states):
    """h0 / c0 given (|h0| up to 1e3: legal here, outside the fp16x2 sibling's range), final states wanted, and the final states
    written over the initial ones."""
    big = states == "given_1e3"
    new, st = run(dev, f"states={states}", h, d, 1, 17, 6, 6, 1, 17 * 6, states="given" if big else states,
                  h0_scale=1e3 if big else 1.0, seed=4)
    assert (st is None) == (states == "none")


@pytest.mark.parametrize("h", [256, 192])
def test_state_shift_hands_over_across_workgroups(dev, h):
    """MemLSTM's hand-over: flat sequence b starts from the state stored for b - 1, sequence 0 from zeros; 33 sequences, so the
    hand-over crosses workgroup boundaries (b = 16, 32) and utterances."""
    run(dev, "state_shift=1", h, 1, 3, 11, 4, 4, 1, 44, states="shift", state_shift=1, seed=5)


@pytest.mark.parametrize("h,d", HD)
@pytest.mark.parametrize("w_scale", [2.0, 0.125])
@pytest.mark.parametrize("n,q,steps", [(1, 17, 150), (2, 1, 1000)])
def test_drift_over_long_sequences(dev, h, d, n, q, steps, w_scale):
    """A SkiM segment (17 sequences of 150 steps) and 1000 dependent steps: the error against fp64 stays in the generic kernel's
    class however long the chain.  With |W| up to 2 the recurrence is chaotic -- every kernel, the fp64 one's float32 twin
    included, ends up O(1) away after a few dozen steps, so that case shows only that nothing blows up; with |W| up to 1/8 the map
    contracts and the same bound compares rounding errors."""
    run(dev, f"drift={n * q}x{steps} |W|<={w_scale}", h, d, n, q, steps, steps, 1, q * steps, seed=6, w_scale=w_scale)


@pytest.mark.parametrize("h,d", HD)
def test_a_sequence_does_not_depend_on_its_neighbours(dev, h, d):
    """Sequence 0 among 33 (three workgroups) is bit-equal to the same sequence launched alone."""
    steps = 6
    many, _ = run(dev, "independence", h, d, 3, 11, steps, steps, 1, 11 * steps, seed=7, sibling=False)
    _, _, image, _ = _weights(h, d)
    gx = _u3((3, d * 4 * h, 11 * steps), 7 * 7 + 31 * 3 + 11 + steps + h + d, 30.0)   # (run()'s inputs)
    alone, _ = hip.lstm_h256_f32(gx[:1].contiguous().to(dev), image, d, 1, 0, steps, 1)
    assert torch.equal(alone.cpu()[0, :, :steps], many[0, :, :steps])
    assert torch.isfinite(alone[0, :, :steps]).all()


def test_nothing_is_written_outside_the_walk(dev):
    """Strided steps of few sequences in a wide row: run() fills hout with NaN, wants the walk's frames finite and every other
    frame still NaN; here with gaps between the sequences, between the steps and behind the last frame."""
    run(dev, "gaps", 256, 2, 2, 3, 2, 4, 11, 3 * 2 + 3 * 11 + 9, seed=8)
