"""Hop-by-hop streaming of the causal time-domain SkiM speaker extractors (puresound_amd/streaming/skim.py) on the MI355X: its
kernel (ps_skim_block_step_f32) against the frame-by-frame reference of tests/skim_step_ref.py, the kernel chain and the
streamer against the reference goldens and the offline HIP path, and the streamer against itself (graph / eager, step /
chunk, B = 1 / 70, sessions one after another, enroll= / embed=, changed weights).

A stream is compared with what the model returns for it ALONE.  The reference hands the last segment state of utterance
n - 1 of a batch to the first segment of utterance n (skim.py:102-109; tests/test_streaming_skim.py reproduces it), so only
row 0 of a batched golden or of a batched model.inference is a function of its own input: row 0 is held to the golden, every
row to model.inference of that row as a batch of one (the offline path, which tests/test_hip_parity.py holds to the same
goldens)."""
import os

import numpy as np
import pytest
import torch

import cases
import skim_step_ref as R
from conftest import rel_max
from detweights import det_state_dict, det_wave

pytestmark = pytest.mark.gpu
TOL = 1e-4
SCHEDULE = (1, 3, 8, 16, 37)
GOLDENS = ["tse_skim_causal_short", "tse_skim_vad_short", "tse_skim_v1_short", "tse_skim_fbank_short"]


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
class _Mods:
    """make_block's block with the attributes pack_skim_block reads from a SkiM."""

    def __init__(self, blk, c, h):
        import puresound_amd.nnet as PA
        self.input_size, self.hidden_size = c, h
        self.n_blocks = 2 if blk["mem"] is not None else 1
        self.embed_dim = 1 if blk["film"] is not None else 0
        self.block_with_embed = [blk["film"] is not None]
        lstm, proj, norm = blk["seg"]
        seg = torch.nn.Module()
        seg.lstm, seg.proj, seg.norm = lstm, proj, norm
        self.seg_lstm = [seg]
        if blk["film"] is not None:
            ws, wb, fnorm = blk["film"]
            film = PA.FiLM(c, 1, input_norm=True)
            with torch.no_grad():
                film.cond_scale.weight[:, :c, 0] = ws
                film.cond_bias.weight[:, :c, 0] = wb
            film.norm = fnorm
            self.seg_input_fusion = [film]
        if blk["mem"] is not None:
            mem = torch.nn.Module()
            (mem.h_net, mem.h_proj, mem.h_norm), (mem.c_net, mem.c_proj, mem.c_norm) = blk["mem"]["h"], blk["mem"]["c"]
            self.mem_lstm = [mem]


_PACKS = {}


def _pack(case, c, h, dev, H):
    key = id(case["blk"])
    if key not in _PACKS:
        _PACKS[key] = H.pack_skim_block(_Mods(case["blk"], c, h), 0, dev)
    return _PACKS[key]


def _cols(t, ldb, dev):
    """[.., B, R] float64 -> [.., R, ldb] on the device, NaN past B: never read, never written."""
    full = torch.full(t.shape[:-2] + (t.shape[-1], ldb), float("nan"), device=dev)
    full[..., :t.shape[-2]] = t.transpose(-1, -2).float().to(dev)
    return full


@pytest.mark.parametrize("c,h,k,b,hops,start,variant", R.kernel_cases())
def test_block_step_kernel(dev, H, c, h, k, b, hops, start, variant):
    """rel_max of y, of every state and of the outgoing banks against the fp64 loop under 1e-5, the bound the DPRNN kernel is
    held to.  (The same loop in torch fp32 on these inputs: 2.8e-6 at worst, tests/test_streaming_skim.py.)"""
    case = R.kernel_case(c, h, k, b, hops, start, variant)
    want = R.run_case(case)
    t0, ns = case["t0"], case["ns"]
    pk = _pack(case, c, h, dev, H)
    ld, ldb = H.padded_frames(hops * b), H.padded_frames(b)
    xin = torch.full((1, c, ld), float("nan"), device=dev)
    xin[0, :, :hops * b] = case["x"].permute(2, 0, 1).reshape(c, hops * b).float().to(dev)
    out = torch.full((1, c, ld), 7.0, device=dev)
    st = {name: _cols(t, ldb, dev) for name, t in case["state"].items()}
    terms = None if case["rs"] is None else (_cols(case["rs"], ldb, dev), _cols(case["rb"], ldb, dev))
    bank_in = None if case["bank_in"] is None else tuple(_cols(t, ldb, dev) for t in case["bank_in"])
    bank_out = None if case["bank_out"] is None else tuple(_cols(t, ldb, dev) for t in case["bank_out"])
    kept = [t.clone() for t in (terms or ()) + (bank_in or ())]
    out0 = None if bank_out is None else [t.clone() for t in bank_out]
    counter = torch.tensor([t0], dtype=torch.int32, device=dev)
    assert H.skim_block_step_ok(c, h, k) and ns == H.skim_bank_slots(16, k)
    mem = None if bank_out is None else tuple(st[name] for name in ("mh_h", "mc_h", "mh_c", "mc_c"))
    H.skim_block_step(xin, counter, pk, (st["seg_h"], st["seg_c"]), k, b, hops, out, terms=terms, bank_in=bank_in,
                      mem_state=mem, bank_out=bank_out)
    torch.cuda.synchronize()
    assert int(counter[0]) == t0                                                  # read, never written
    assert bool((out[0, :, hops * b:] == 7.0).all())                              # columns past the chunk are not written
    got = out[0, :, :hops * b].reshape(c, hops, b).permute(1, 2, 0).cpu()
    errs = {"out": rel_max(got.numpy(), want["out"].numpy())}
    for name, t in want["state"].items():
        errs[name] = rel_max(st[name][:, :b].t().cpu().numpy(), t.numpy())
        assert bool(torch.isnan(st[name][:, b:]).all()), name
    for t, t0_ in zip((terms or ()) + (bank_in or ()), kept):                     # inputs: the same bits, NaN included
        assert torch.equal(t.view(torch.int32), t0_.view(torch.int32))
    if bank_out is not None:
        for name, t, ref, before in zip(("out_h", "out_c"), bank_out, want["bank_out"], out0):
            errs[name] = rel_max(t[:, :, :b].transpose(1, 2).cpu().numpy(), ref.numpy())
            assert bool(torch.isnan(t[:, :, b:]).all()), name
            for slot in set(range(ns)) - want["written"]:                         # slots the launch does not visit
                assert torch.equal(t[slot, :, :b], before[slot, :, :b]), (name, slot)
        ends = len([f for f in range(hops) if (t0 + f) % k == k - 1])
        assert len(want["written"]) == ends
    print(f"skim_block_step C={c} H={h} K={k} B={b} hops={hops} t0={t0} {variant}: rel_max " +
          " ".join(f"{name} {v:.2e}" for name, v in errs.items()))
    assert max(errs.values()) < 1e-5, errs


def test_block_step_ok_and_refusal(dev, H):
    for shape in R.SHAPES:
        assert H.skim_block_step_ok(*shape), shape
    c, h, k, b = 128, 512, 150, 2
    assert not H.skim_block_step_ok(c, h, k)
    blk = R.make_block(c, h, 1, film=False, mem=False)
    z = lambda *shape: torch.zeros(*shape, device=dev)  # noqa: E731
    ld = ldb = H.padded_frames(b)
    out = torch.full((1, c, ld), 7.0, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match=r"rc=-3"):
        H.skim_block_step(z(1, c, ld), counter, H.pack_skim_block(_Mods(blk, c, h), 0, dev), (z(h, ldb), z(h, ldb)), k, b, 1,
                          out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# -------------------------------------------------------------------------------------------------------------------------
# the kernel chain and the streamer
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


def test_stream_tiny_through_the_kernel_chain(dev, H, golden_dir):
    """The reference's tiny streaming model (C = 5, H = 20, K = 10, four FiLM blocks): its golden x through four chained
    launches per chunk of uneven length, then output_fc, against its offline output."""
    m, _ = _model("stream_tiny", dev)
    g = dict(np.load(os.path.join(golden_dir, "stream_tiny.npz")))
    x = torch.tensor(g["x"])[0]                                        # [C, T]
    c, t = x.shape
    h, k, ldb = m.hidden_size, m.seg_size, H.padded_frames(1)
    ns = H.skim_bank_slots(16, k)
    z = lambda *shape: torch.zeros(*shape, device=dev)  # noqa: E731
    packs = [H.pack_skim_block(m, i, dev) for i in range(m.n_blocks)]
    embed = torch.nn.functional.normalize(torch.tensor(g["embed"]), dim=1).to(dev)
    terms = []
    for pk in packs:
        both = pk["film"]["embed_wt"] @ embed[0]
        rs, rb = z(c, ldb), z(c, ldb)
        rs[:, 0], rb[:, 0] = both[:c], both[c:]
        terms.append((rs, rb))
    seg = [(z(h, ldb), z(h, ldb)) for _ in packs]
    mem = [tuple(z(h, ldb) for _ in range(4)) for _ in packs[1:]]
    banks = [(z(ns, h, ldb), z(ns, h, ldb)) for _ in packs[1:]]
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    outs, t0, last = [], 0, len(packs) - 1
    for size in (1, 3, 7, 2, 16, 5, 11, 16):
        size = min(size, t - t0)
        if size == 0:
            break
        ld = H.padded_frames(size)
        cur = z(1, c, ld)
        cur[0, :, :size] = x[:, t0:t0 + size].to(dev)
        for i, pk in enumerate(packs):
            nxt = torch.full((1, c, ld), float("nan"), device=dev)
            H.skim_block_step(cur, counter, pk, seg[i], k, 1, size, nxt, terms=terms[i], bank_in=banks[i - 1] if i else None,
                              mem_state=mem[i] if i < last else None, bank_out=banks[i] if i < last else None)
            cur = nxt
        outs.append(cur[0, :, :size].t().reshape(size, 1, c).double().cpu())
        counter += size
        t0 += size
    assert t0 == t
    y = R.output_fc(m.cpu(), torch.cat(outs)).numpy()
    m.to(dev)
    err = rel_max(y, g["y_offline"])
    print(f"stream_tiny through ps_skim_block_step_f32: rel_max against y_offline {err:.3e}")
    assert err < 1e-4


def _stream(s, x, schedule=None, use_graph=True, **how):
    """Stream x [B, L] (L a multiple of the hop) -> emitted samples ‖ flush(), [B, L_out]; schedule: hops per step_chunk
    call, cycled (None: step()); how: enroll= or embed=."""
    hop = s.hop_length
    s.init_streams(streams=x.shape[0], use_graph=use_graph, **how)
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
    return x, det_wave(c["seed"] + 1, c["B"], c["L_enroll"]).to(dev)


_STREAMED = {}


def _streamed(name, dev, schedule):
    """The golden input of `name` streamed with a graph, once per schedule."""
    from puresound_amd.streaming import StreamingSkiMExtractor
    if (name, schedule) not in _STREAMED:
        model, _ = _model(name, dev)
        x, e = _inputs(name, dev)
        _STREAMED[(name, schedule)] = _stream(StreamingSkiMExtractor(model), x, schedule, enroll=e)
    return _STREAMED[(name, schedule)]


def _rows_alone(model, x, e):
    """model.inference of every row as a batch of one."""
    return torch.cat([model.inference(x[b:b + 1].contiguous(), e[b:b + 1].contiguous()) for b in range(x.shape[0])])


@pytest.mark.parametrize("name", GOLDENS)
def test_streamed_matches_reference_golden(dev, golden_dir, name):
    """B = 2, 249 frames, one segment end at frame 150, with step() and with the schedule, then flush().  Row 0 against the
    reference's golden; both rows against the offline path on each row alone (see the module docstring: row 1 of the golden
    starts blocks 1 .. 3 from row 0's last segment, which the second assertion measures)."""
    from puresound_amd.streaming import StreamingSkiMExtractor
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    model, _ = _model(name, dev)
    s = StreamingSkiMExtractor(model)
    assert (s.hop_length, s.latency_samples, s.max_hops) == (16, 16, 16)
    alone = _rows_alone(model, *_inputs(name, dev)).cpu().numpy()
    assert rel_max(alone[0], g["wav"][0]) < TOL
    for schedule in (None, SCHEDULE):
        y = _streamed(name, dev, schedule).cpu().numpy()
        assert y.shape == g["wav"].shape
        err = rel_max(y[0], g["wav"][0])
        err_alone = rel_max(y, alone)
        print(f"StreamingSkiMExtractor {name} schedule {schedule}: rel_max of row 0 against the golden {err:.3e}, of both "
              f"rows against the offline path row by row {err_alone:.3e}; row 1 against the batched golden "
              f"{rel_max(y[1], g['wav'][1]):.3e}")
        assert err < TOL, schedule
        assert err_alone < TOL, schedule


def test_long_streams_match_offline_fp32(dev):
    """B = 3 x 2 s: 1999 frames, 13 segment ends, every stream against the offline path on it alone."""
    from puresound_amd.streaming import StreamingSkiMExtractor
    model, _ = _model("tse_skim_causal_short", dev)
    before = model.masker.gemm_precision
    model.set_gemm_precision("fp32")
    try:
        x = det_wave(31, 3, 32000).to(dev)
        e = det_wave(32, 3, 3000).to(dev)
        y = _stream(StreamingSkiMExtractor(model), x, (16,), enroll=e)
        ref = _rows_alone(model, x, e)
    finally:
        model.set_gemm_precision(before)
    assert y.shape == ref.shape
    err = rel_max(y.cpu().numpy(), ref.cpu().numpy())
    print(f"StreamingSkiMExtractor 3 x 2 s against offline fp32: rel_max {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("name", ["tse_skim_causal_short", "tse_skim_vad_short"])
def test_graph_eager_step_chunk_are_the_same_bits(dev, name):
    """Every sum of a column has one order whatever the chunk length, and a replay runs the launches of the eager run."""
    from puresound_amd.streaming import StreamingSkiMExtractor
    model, _ = _model(name, dev)
    x, e = _inputs(name, dev)
    a = _streamed(name, dev, SCHEDULE)
    assert torch.equal(a, _stream(StreamingSkiMExtractor(model), x, SCHEDULE, use_graph=False, enroll=e))
    assert torch.equal(a, _streamed(name, dev, None))


def test_streams_are_independent(dev):
    """Stream 0 of 70 (five tiles of 16 columns, the last ragged) with its embedding given: the same bits with other audio
    and other embeddings beside it, and alone.  170 frames: past the segment end at 150."""
    from puresound_amd.streaming import StreamingSkiMExtractor
    model, _ = _model("tse_skim_vad_short", dev)
    s = StreamingSkiMExtractor(model)
    x = det_wave(77, 70, 16 * 171).to(dev)
    d = det_wave(78, 70, 192).to(dev)
    y = _stream(s, x, (8,), embed=d)
    x2, d2 = det_wave(79, 70, 16 * 171).to(dev), det_wave(80, 70, 192).to(dev)
    x2[0], d2[0] = x[0], d[0]
    y2 = _stream(s, x2, (8,), embed=d2)
    assert torch.equal(y[0], y2[0])
    assert not torch.equal(y[1:], y2[1:])
    alone = _stream(s, x[:1].contiguous(), (8,), embed=d[:1].contiguous())
    assert torch.equal(alone[0], y[0])


def test_enroll_and_embed(dev):
    from puresound_amd.streaming import StreamingSkiMExtractor
    name = "tse_skim_vad_short"
    model, _ = _model(name, dev)
    x, e = _inputs(name, dev)
    x = x[:, :16 * 170].contiguous()
    s = StreamingSkiMExtractor(model)
    d = model.inference_tse_embedding(e)
    assert tuple(d.shape) == (2, 192, 1)
    a = _stream(s, x, (8,), enroll=e)
    b = _stream(s, x, (8,), embed=d)
    assert torch.equal(b, _stream(s, x, (8,), embed=d[:, :, 0].contiguous()))
    assert rel_max(b.cpu().numpy(), a.cpu().numpy()) < TOL
    with pytest.raises(ValueError, match="exactly one"):
        s.init_streams(2, enroll=e, embed=d)
    with pytest.raises(ValueError, match="exactly one"):
        s.init_streams(2)
    with pytest.raises(ValueError, match=r"embed must be \[2, 192\]"):
        s.init_streams(2, embed=d[:1])
    with pytest.raises(NotImplementedError, match="no slot sessions"):
        s.open(0)


def test_model_left_intact(dev):
    from puresound_amd.streaming import StreamingSkiMExtractor
    name = "tse_skim_vad_short"
    model, _ = _model(name, dev)
    x, e = _inputs(name, dev)
    precision = model.masker.gemm_precision
    before = model.inference(x, e)
    s = StreamingSkiMExtractor(model)
    _stream(s, x, (4,), enroll=e)
    _stream(s, x, (4,), use_graph=False, enroll=e)
    assert model.masker.gemm_precision == precision
    assert torch.equal(model.inference(x, e), before)


def test_changed_weights_are_used_and_a_second_session_starts_clean(dev):
    from puresound_amd.streaming import StreamingSkiMExtractor
    name = "tse_skim_vad_short"
    model, sd = _model(name, dev)
    x, e = _inputs(name, dev)
    x = x[:, :16 * 50].contiguous()
    d = model.inference_tse_embedding(e)
    s = StreamingSkiMExtractor(model)
    a = _stream(s, x, (8,), embed=d)
    assert torch.equal(a, _stream(s, x, (8,), embed=d))                           # a second init_streams starts clean
    assert torch.equal(a, _stream(StreamingSkiMExtractor(model), x, (8,), embed=d))   # ... as a fresh streamer does
    for key in ("masker.seg_lstm.1.proj.weight", "masker.seg_input_fusion.0.cond_bias.weight"):
        changed = {k: v.clone() for k, v in sd.items()}
        changed[key] = changed[key] * 1.5
        try:
            s.init_streams(2, embed=d)
            head = s.step_chunk(x[:, :16 * 9])
            assert torch.equal(head, a[:, :16 * 8])
            model.load_state_dict(changed)                             # in the middle of a session: the next step uses them
            assert not torch.equal(s.step(x[:, 16 * 9:16 * 10]), a[:, 16 * 8:16 * 9]), key
            b = _stream(s, x, (8,), embed=d)
            assert not torch.equal(a, b)
            assert torch.equal(b, _stream(StreamingSkiMExtractor(model), x, (8,), embed=d))
        finally:
            model.load_state_dict(sd)
        assert torch.equal(a, _stream(s, x, (8,), embed=d))
