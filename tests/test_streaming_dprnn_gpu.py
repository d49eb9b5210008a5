"""Hop-by-hop streaming of the causal time-domain DPRNN (puresound_amd/streaming/dprnn.py) on the MI355X: its kernel
(ps_dprnn_block_step_f32) against the frame-by-frame reference of tests/dprnn_step_ref.py, the streamer against the reference
goldens and the offline HIP path, and against itself (graph / eager, step / chunk, B = 1 / 70, one stream's input against
another's output, sessions one after another, changed weights)."""
import os

import numpy as np
import pytest
import torch

import cases
import dprnn_step_ref as R
from conftest import rel_max
from detweights import det_state_dict, det_wave

pytestmark = pytest.mark.gpu
TOL = 1e-4
SCHEDULE = (1, 3, 8, 16, 37)


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
    junk = [torch.full((1 << 22,), float("nan"), device=dev) for _ in range(16)]
    junk += [torch.full((n,), float("nan"), device=dev) for n in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20)]
    del junk
    yield


# -------------------------------------------------------------------------------------------------------------------------
# the kernel
# -------------------------------------------------------------------------------------------------------------------------
_PASSES = {}


def _passes(c, h, dev, H):
    """The two passes of one block at (C, H): torch modules (for the reference) and their device packs, made once."""
    if (c, h) not in _PASSES:
        intra, inter = R.make_pass(c, h, 11 * c + h), R.make_pass(c, h, 13 * c + h)
        _PASSES[(c, h)] = (intra, inter, H.pack_dprnn_pass(*intra, dev), H.pack_dprnn_pass(*inter, dev))
    return _PASSES[(c, h)]


def _rand(shape, seed):
    g = np.random.Generator(np.random.Philox(key=seed))
    return torch.tensor(g.uniform(-1.0, 1.0, shape), dtype=torch.float64)


@pytest.mark.parametrize("start", ["0", "K-1", "3K+2"])
@pytest.mark.parametrize("hops", [1, 7, 16])
@pytest.mark.parametrize("b", [1, 3, 70])
@pytest.mark.parametrize("c,h,k", [(16, 8, 5), (128, 64, 20)])
def test_block_step_kernel(dev, H, c, h, k, b, hops, start):
    t0 = {"0": 0, "K-1": k - 1, "3K+2": 3 * k + 2}[start]
    intra, inter, pk_intra, pk_inter = _passes(c, h, dev, H)
    seed = 100000 * c + 1000 * b + 10 * hops + t0
    x = _rand((hops, b, c), seed)
    state = dict(h_intra=_rand((b, h), seed + 1), c_intra=_rand((b, h), seed + 2),      # random: a missed reset or a wrong
                 h_bank=_rand((k, b, h), seed + 3), c_bank=_rand((k, b, h), seed + 4))  # slot shows
    before = {key: t.clone() for key, t in state.items()}
    want, visited = R.block_step(x, t0, k, intra, inter, state)

    ld, ldb = H.padded_frames(hops * b), H.padded_frames(b)
    nan = float("nan")
    xin = torch.full((1, c, ld), nan, device=dev)
    xin[0, :, :hops * b] = x.permute(2, 0, 1).reshape(c, hops * b).float().to(dev)
    out = torch.full((1, c, ld), 7.0, device=dev)
    st = {}
    for key, t in before.items():                      # columns past B hold NaN: never read, never written
        full = torch.full(t.shape[:-2] + (h, ldb), nan, device=dev)
        full[..., :b] = t.transpose(-1, -2).float().to(dev)
        st[key] = full
    st0 = {key: t.clone() for key, t in st.items()}
    counter = torch.tensor([t0], dtype=torch.int32, device=dev)
    assert H.dprnn_block_step_ok(c, h, k)
    H.dprnn_block_step(xin, counter, pk_intra, pk_inter, st["h_intra"], st["c_intra"], st["h_bank"], st["c_bank"], b, hops,
                       out=out)
    torch.cuda.synchronize()
    assert int(counter[0]) == t0                                                  # read, never written
    assert bool((out[0, :, hops * b:] == 7.0).all())                              # columns past the chunk are not written
    got = out[0, :, :hops * b].reshape(c, hops, b).permute(1, 2, 0).cpu()
    errs = {"out": rel_max(got.numpy(), want.numpy())}
    for key, t in state.items():
        errs[key] = rel_max(st[key][..., :b].transpose(-1, -2).cpu().numpy(), t.numpy())
        assert bool(torch.isnan(st[key][..., b:]).all()), key
    print(f"dprnn_block_step C={c} H={h} K={k} B={b} hops={hops} t0={t0}: rel_max " +
          " ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    assert max(errs.values()) < 1e-5, errs
    for p in set(range(k)) - visited:                                             # slots not visited: the same bits
        for key in ("h_bank", "c_bank"):
            assert torch.equal(st[key][p, :, :b], st0[key][p, :, :b]), (key, p)


def test_block_step_kernel_refuses_unsupported_shapes(dev, H):
    c, h, k, b = 512, 128, 4, 2
    assert not H.dprnn_block_step_ok(c, h, k)
    z = lambda *shape: torch.zeros(*shape, device=dev)  # noqa: E731
    intra, inter = R.make_pass(c, h, 1), R.make_pass(c, h, 2)
    ld, ldb = H.padded_frames(b), H.padded_frames(b)
    out = torch.full((1, c, ld), 7.0, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match=r"rc=-3"):
        H.dprnn_block_step(z(1, c, ld), counter, H.pack_dprnn_pass(*intra, dev), H.pack_dprnn_pass(*inter, dev), z(h, ldb),
                           z(h, ldb), z(k, h, ldb), z(k, h, ldb), b, 1, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# -------------------------------------------------------------------------------------------------------------------------
# the streamer
# -------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(name, dev):
    if name not in _MODELS:
        import puresound_amd.nnet as PA
        m = cases.build(PA.NS, name).eval()
        sd = det_state_dict(m)
        m.load_state_dict(sd)
        _MODELS[name] = (m.to(dev), sd)
    return _MODELS[name]


def _stream(s, x, enroll=None, schedule=None, use_graph=True):
    """Stream x [B, L] (L a multiple of the hop) -> emitted samples ‖ flush(), [B, L_out]; schedule: hops per step_chunk
    call, cycled (None: step())."""
    hop = s.hop_length
    s.init_streams(streams=x.shape[0], enroll=enroll, use_graph=use_graph)
    outs, hops, i, j = [], x.shape[1] // hop, 0, 0
    while i < hops:
        if schedule is None:
            y = s.step(x[:, i * hop:(i + 1) * hop])
            assert (y is None) == (i < s.prime_hops)
            i += 1
        else:
            k = min(schedule[j % len(schedule)], hops - i)
            y = s.step_chunk(x[:, i * hop:(i + k) * hop])
            i, j = i + k, j + 1
        if y is not None:
            outs.append(y)
    outs.append(s.flush())
    return torch.cat(outs, dim=1)


def _inputs(name, dev):
    c = cases.CASES[name]
    hop = c["enc"]["hop"]
    x = det_wave(c["seed"], c["B"], c["L"])
    x = x[:, :x.shape[1] // hop * hop].contiguous().to(dev)
    e = det_wave(c["seed"] + 1, c["B"], c["L_enroll"]).to(dev) if "L_enroll" in c else None
    return x, e


_STREAMED = {}


def _streamed(name, dev, schedule):
    """The golden input of `name` streamed with a graph, once per schedule."""
    from puresound_amd.streaming import StreamingDPRNN
    if (name, schedule) not in _STREAMED:
        model, _ = _model(name, dev)
        _STREAMED[(name, schedule)] = _stream(StreamingDPRNN(model), *_inputs(name, dev), schedule)
    return _STREAMED[(name, schedule)]


@pytest.mark.parametrize("name", ["cfg4_short", "cfg4_tse_short"])
def test_streamed_matches_reference_golden(dev, golden_dir, name):
    from puresound_amd.streaming import StreamingDPRNN
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    model, _ = _model(name, dev)
    s = StreamingDPRNN(model)
    assert (s.hop_length, s.latency_samples, s.max_hops) == (16, 16, 16)
    for schedule in (None, SCHEDULE):
        y = _streamed(name, dev, schedule).cpu().numpy()
        assert y.shape == g["wav"].shape
        err = rel_max(y, g["wav"])
        print(f"StreamingDPRNN {name} schedule {schedule}: rel_max against the golden {err:.3e}")
        assert err < TOL, schedule


def test_long_streams_match_offline_fp32(dev):
    """B = 3 x 2 s: 1999 frames, 100 segments; the enrolment seeds the banks."""
    from puresound_amd.streaming import StreamingDPRNN
    model, _ = _model("cfg4_tse_short", dev)
    before = model.masker.gemm_precision
    model.set_gemm_precision("fp32")
    try:
        x = det_wave(31, 3, 32000).to(dev)
        e = det_wave(32, 3, 3000).to(dev)
        y = _stream(StreamingDPRNN(model), x, e, (16,))
        ref = model.inference(x, e)
    finally:
        model.set_gemm_precision(before)
    assert y.shape == ref.shape
    err = rel_max(y.cpu().numpy(), ref.cpu().numpy())
    print(f"StreamingDPRNN 3 x 2 s against offline fp32: rel_max {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("name", ["cfg4_short", "cfg4_tse_short"])
def test_graph_eager_step_chunk_are_the_same_bits(dev, name):
    """Every sum of a column has one order whatever the chunk length, and a replay runs the launches of the eager run."""
    from puresound_amd.streaming import StreamingDPRNN
    model, _ = _model(name, dev)
    x, e = _inputs(name, dev)
    a = _streamed(name, dev, SCHEDULE)
    assert torch.equal(a, _stream(StreamingDPRNN(model), x, e, SCHEDULE, use_graph=False))
    assert torch.equal(a, _streamed(name, dev, None))


def test_streams_are_independent(dev):
    """Stream 0 of 70 (five tiles of 16 columns, the last ragged): the same bits with other audio beside it, and alone."""
    from puresound_amd.streaming import StreamingDPRNN
    model, _ = _model("cfg4_short", dev)
    s = StreamingDPRNN(model)
    x = det_wave(77, 70, 16 * 60).to(dev)
    y = _stream(s, x, None, (8,))
    x2 = det_wave(79, 70, 16 * 60).to(dev)
    x2[0] = x[0]
    y2 = _stream(s, x2, None, (8,))
    assert torch.equal(y[0], y2[0])
    assert not torch.equal(y[1:], y2[1:])
    alone = _stream(s, x[:1].contiguous(), None, (8,))
    assert torch.equal(alone[0], y[0])


def test_model_left_intact(dev):
    from puresound_amd.streaming import StreamingDPRNN
    model, _ = _model("cfg4_tse_short", dev)
    x, e = _inputs("cfg4_tse_short", dev)
    precision = model.masker.gemm_precision
    before = model.inference(x, e)
    s = StreamingDPRNN(model)
    _stream(s, x, e, (4,))
    _stream(s, x, e, (4,), use_graph=False)
    assert model.masker.gemm_precision == precision
    assert torch.equal(model.inference(x, e), before)


def test_changed_weights_are_used_and_a_second_session_starts_clean(dev):
    from puresound_amd.streaming import StreamingDPRNN
    name = "cfg4_tse_short"
    model, sd = _model(name, dev)
    x, e = _inputs(name, dev)
    x, e = x[:, :16 * 50].contiguous(), e
    s = StreamingDPRNN(model)
    a = _stream(s, x, e, (8,))
    assert torch.equal(a, _stream(s, x, e, (8,)))                      # a second init_streams starts clean
    assert torch.equal(a, _stream(StreamingDPRNN(model), x, e, (8,)))  # ... as a fresh streamer does
    changed = {k: v.clone() for k, v in sd.items()}
    changed["masker.inter_proj.3.weight"] = changed["masker.inter_proj.3.weight"] * 1.5
    try:
        s.init_streams(2, e)
        head = s.step_chunk(x[:, :16 * 9])
        assert torch.equal(head, a[:, :16 * 8])
        model.load_state_dict(changed)                                 # in the middle of a session: the next step uses them
        assert not torch.equal(s.step(x[:, 16 * 9:16 * 10]), a[:, 16 * 8:16 * 9])
        b = _stream(s, x, e, (8,))
        assert not torch.equal(a, b)
        assert torch.equal(b, _stream(StreamingDPRNN(model), x, e, (8,)))
    finally:
        model.load_state_dict(sd)
    assert torch.equal(a, _stream(s, x, e, (8,)))
