"""Round-2 GPU tests: the parity-coverage holes the round-1 review named (the benchmark's exact arithmetic at its exact
batch size, BASELINE configs 3 and 4 in the bf16 arithmetic BASELINE.json names for them, the look-ahead /
receptive-field known answers) and regressions for the advisor's findings (a captured graph survives the growth of the
scratch workspace; a model left on the CPU or in half precision raises before any launch; ASP with `lengths`)."""
import numpy as np
import pytest
import torch

import cases
from conftest import rel_max
from detweights import det_state_dict, det_wave
from oracle import separator_oracle as O
from puresound_amd import _abi

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def PA():
    import puresound_amd.nnet as PA
    return PA


def _build(PA, name, dev):
    model = cases.build(PA.NS, name).eval()
    sd = det_state_dict(model)
    model.load_state_dict(sd)
    return model.to(dev), sd


def _l2rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("gemm", ["fp16x2", "bf16x3"])
def test_benchmark_arithmetic_at_benchmark_size(PA, dev, golden_dir, gemm):
    """bench.py's path exactly: config 2, batch 32 x 64000, in the benchmark's default arithmetic (fp16x2: two fp16 terms
    per operand on the persistent kernel, the range chain across 24 blocks) and in the six-product bf16 split.  Row 0 of
    the batch IS the reference's golden utterance (1e-4 against tests/golden/cfg2_full.npz, directly); rows agree with
    their B = 1 runs to fp32 rounding (the split GEMMs pick their kernel by launch size, so not bit for bit); length
    law; |y| <= 1."""
    name = "cfg2_full"
    g = np.load(f"{golden_dir}/{name}.npz")
    model, _ = _build(PA, name, dev)
    model.masker.set_gemm_precision(gemm)
    batch = torch.cat([det_wave(cases.CASES[name]["seed"], 1, 64000), det_wave(99, 31, 64000)]).to(dev)
    for streams in (1, 2):
        model.hip_streams = streams
        out = model.inference(batch)
        assert out.shape == (32, 64000) and torch.isfinite(out).all() and float(out.abs().max()) <= 1.0
        assert rel_max(out[0:1].cpu().numpy(), g["wav"]) < TOL
        for i in (0, 7, 16, 31):
            single = model.inference(batch[i:i + 1])
            assert float((single[0] - out[i]).abs().max()) <= (2e-5 if gemm == "fp16x2" else 1e-5), (streams, i)


def test_config3_in_its_bf16_arithmetic(PA, dev):
    """BASELINE configs[2] ("bf16"): bf16 products on the masker AND on the speaker net, fp32 accumulation, at full
    size (one 4 s mixture + 4 s enrolment against the fp32 oracle): l2-rel <= 3e-2 (the reference's own bf16
    deviation is 1.2e-2 / 2.2e-2)."""
    name = "cfg3_short"
    model, sd = _build(PA, name, dev)
    model.masker.set_gemm_precision("bf16")
    for m in model.speaker_net:
        if hasattr(m, "gemm_precision"):
            m.gemm_precision = "bf16"
    noisy, enroll = det_wave(301, 32, 64000), det_wave(302, 32, 64000)
    out = model.inference(noisy.to(dev), enroll.to(dev))
    assert out.shape == (32, 64000) and torch.isfinite(out).all()
    ref = O.inference(noisy[5:6], sd, cases.oracle_cfg(name), enroll[5:6])
    assert _l2rel(out[5:6].cpu().numpy(), ref.numpy()) < 3e-2
    dvec = model.inference_tse_embedding(enroll[5:6].to(dev))
    taps = {}
    O.inference(noisy[5:6, :4000], sd, cases.oracle_cfg(name), enroll[5:6], taps)
    assert _l2rel(dvec[..., 0].cpu().numpy(), taps["dvec"].numpy()) < 3e-2


@pytest.mark.parametrize("gemm,tol", [("bf16x3", None), ("fp16x2", None), ("bf16", 3e-2)])
def test_config4_input_projections_on_the_bf16_pipe(PA, dev, gemm, tol):
    """BASELINE configs[3]: the DPRNN's LSTM input projections as the fp32-accurate splits (six bf16 products, or three
    fp16 products with the input range handed from recurrence to recurrence by the projection + LayerNorm row kernel:
    1e-4 max-rel) and in the bf16 arithmetic BASELINE.json names (l2-rel <= 3e-2), full size, one utterance against the oracle.  The switch is
    a per-module attribute (PlanCache.set_gemm_precision), not process state: a second model keeps fp32."""
    name = "cfg4_short"
    model, sd = _build(PA, name, dev)
    other, _ = _build(PA, name, dev)
    assert other.masker.gemm_precision == "fp16x2"     # (the default since round 4)
    other.masker.set_gemm_precision("fp32")
    model.masker.set_gemm_precision(gemm)
    assert other.masker.gemm_precision == "fp32"
    noisy = det_wave(301, 32, 64000)
    out = model.inference(noisy.to(dev))
    assert out.shape == (32, 64000) and torch.isfinite(out).all()
    ref = O.inference(noisy[5:6], sd, cases.oracle_cfg(name))
    if tol is None:
        assert rel_max(out[5:6].cpu().numpy(), ref.numpy()) < TOL
    else:
        assert _l2rel(out[5:6].cpu().numpy(), ref.numpy()) < tol
    base = other.inference(noisy[5:6].to(dev))
    assert rel_max(base.cpu().numpy(), ref.numpy()) < TOL


def test_lookahead_and_receptive_field_known_answers(PA, dev):
    """the reference's NaN-propagation probe (base_nn.py:740-777) on td_tse_conv_tasnet_v0_causal gives
    look-ahead 16 samples and receptive field 24 496 samples; the non-causal preset is "infinite" both ways."""
    model, _ = _build(PA, "cfg3_causal_short", dev)
    assert model.probe_lookahead_receptive_field() == (16, 24496)
    model, _ = _build(PA, "cfg3_short", dev)
    assert model.probe_lookahead_receptive_field() == ("infinite", "infinite")


def test_captured_graph_survives_workspace_growth(PA, dev):
    """A graph captured at B = 1 bakes in the scratch workspace's address; a later, larger call makes the module
    allocate a bigger one.  The graph entry keeps the old one alive: replaying the first graph afterwards still equals
    the eager result (and results returned earlier are not overwritten)."""
    from puresound_amd.graphs import GraphedInference
    model, _ = _build(PA, "cfg2_short", dev)
    fast = GraphedInference(model)
    small = det_wave(3, 1, 4000).to(dev)
    a0 = fast(small)
    want_small = model.inference(small)
    assert torch.equal(a0, want_small)
    kept = []
    for b, length in ((4, 4000), (2, 9000), (6, 12000)):  # growing batch, then growing length
        x = det_wave(10 + b, b, length).to(dev)
        y = fast(x)
        assert torch.equal(y, model.inference(x))
        kept.append((x, y.clone(), y))
        torch.empty(64 << 20, dtype=torch.uint8, device=dev).fill_(255)  # churn the allocator
        assert torch.equal(fast(small), want_small)
    for x, y_then, y_now in kept:
        assert torch.equal(y_then, y_now)
    assert torch.equal(a0, want_small)


def test_parameters_off_device_raise_before_any_launch(PA, dev):
    """The kernels take raw pointers: a model left on the CPU or converted to half must raise, not fault."""
    c = cases.CASES["cfg3_short"]
    noisy = det_wave(1, 2, c["L"]).to(dev)
    enroll = det_wave(2, 2, c["L_enroll"]).to(dev)
    cpu_model = cases.build(PA.NS, "cfg3_short").eval()
    with pytest.raises(RuntimeError, match="parameters are on cpu"):
        cpu_model.inference(noisy, enroll)
    half_model = cases.build(PA.NS, "cfg3_short").eval().to(dev).half()
    with pytest.raises(RuntimeError, match="fp32 parameters only"):
        half_model.inference(noisy, enroll)
    enc = PA.FreeEncDec(32, 64, 16)
    with pytest.raises(RuntimeError):
        enc(noisy)
    with pytest.raises(RuntimeError):
        enc.inverse(torch.rand(2, 64, 100, device=dev))


def test_attentive_stats_pooling_with_lengths(PA, dev):
    """lobe/pooling.py:87-126 with `lengths`: frames t with float(t) >= lengths[n] * L are masked out of the softmax."""
    torch.manual_seed(0)
    pool = PA.AttentiveStatisticsPooling(48, 16).eval()
    sd = det_state_dict(pool)
    pool.load_state_dict(sd)
    n, c, length = 5, 48, 333
    x = det_wave(21, n * c, length).reshape(n, c, length)
    lengths = torch.tensor([1.0, 0.5, 0.301, 0.9999, 1.0 / 333])
    # restatement of the reference's masked forward
    a = O.conv1x1(x, sd["tdnn.0.weight"], sd["tdnn.0.bias"])
    a = O.batch_norm_eval(torch.relu(a), sd, "tdnn.2.")
    a = O.conv1x1(torch.tanh(a), sd["conv.weight"], sd["conv.bias"])
    mask = torch.arange(length, dtype=torch.float32).unsqueeze(0) < (lengths * length).unsqueeze(1)
    a = torch.softmax(a.masked_fill(~mask.unsqueeze(1), float("-inf")), dim=2)
    mean = (a * x).sum(2)
    std = torch.sqrt((a * (x - mean.unsqueeze(2)) ** 2).sum(2).clamp(1e-12))
    ref = torch.cat((mean, std), 1).unsqueeze(2)
    got = pool.to(dev)(x.to(dev), lengths.to(dev))
    assert got.shape == ref.shape
    assert rel_max(got.cpu().numpy(), ref.numpy()) < TOL
    assert rel_max(pool(x.to(dev)).cpu().numpy(), O.attentive_stats_pooling(x, sd, "").numpy()) < TOL


def test_chunk_graph_equals_the_hop_loop_across_mem_lstm_updates(dev):
    """BASELINE configs[4]: one hipGraph per 320-sample chunk.  16 chunks = 320 hops cross the 150-frame segment
    boundary twice -- once in the middle of a chunk, once at the start of one -- so all three graph variants replay; the running output equals the eager hop-by-hop loop bit for bit and
    the masker ends in the same state."""
    from puresound_amd.streaming.demo import DemoTseNet
    net = DemoTseNet().eval()
    net.load_state_dict(det_state_dict(net))
    net.to(dev)
    b, n_chunks = 5, 16
    wav = det_wave(501, b, 320 * n_chunks).to(dev)
    emb = torch.rand(b, 192, generator=torch.Generator().manual_seed(502)).to(dev)
    outs, states = [], []
    for use_graph in (False, True):
        net.init_streams(b, use_graph=use_graph)
        pre = None
        for i in range(n_chunks):
            pre = net.streaming_inference_chunk(wav[:, i * 320:(i + 1) * 320], emb, pre)
        outs.append(pre.clone())
        states.append([t.clone() for t in net.masker._seg_h + net.masker._seg_c])
        if use_graph:
            # (the stream's very first hop only fills the window, so the segment counter lags the hop count by one)
            # all three update patterns a 20-hop chunk can meet are captured with the first graphed chunk
            assert set(net._chunk_graphs) == {(20, (10,)), (20, (0,)), (20, ())}
    assert outs[0].shape == (b, 16 * (20 * n_chunks - 1) + 16)
    assert torch.equal(outs[0], outs[1])
    for a, c in zip(*states):
        assert torch.equal(a[..., :b], c[..., :b])  # (columns beyond the b streams are padding)
    # a weight update drops the graphs instead of replaying stale plans
    sd = det_state_dict(net)
    key = next(k for k in sd if k.endswith("weight") and sd[k].dim() > 1)
    sd[key] = sd[key] * 1.25
    net.load_state_dict(sd)
    net.init_streams(b, use_graph=False)
    ref = None
    for i in range(3):
        ref = net.streaming_inference_chunk(wav[:, i * 320:(i + 1) * 320], emb, ref)
    net.init_streams(b, use_graph=True)
    got = None
    for i in range(3):
        got = net.streaming_inference_chunk(wav[:, i * 320:(i + 1) * 320], emb, got)
    assert torch.equal(got, ref) and not torch.equal(got, outs[0][:, :got.shape[1]])


def test_chunk_longer_than_a_segment_wraps_the_counter_more_than_once(dev):
    """A chunk of 170 hops (> seg_size = 150) crosses one or two segment boundaries: every Mem-LSTM update and block-0
    reset inside it happens in the chunk graph as in the hop loop (round 2 handled at most one per chunk)."""
    from puresound_amd.streaming.demo import DemoTseNet
    net = DemoTseNet().eval()
    net.load_state_dict(det_state_dict(net))
    net.to(dev)
    b, hops, n_chunks = 3, 170, 4
    wav = det_wave(511, b, 16 * hops * n_chunks).to(dev)
    emb = torch.rand(b, 192, generator=torch.Generator().manual_seed(512)).to(dev)
    outs = []
    for use_graph in (False, True):
        net.init_streams(b, use_graph=use_graph)
        pre = None
        for i in range(n_chunks):
            pre = net.streaming_inference_chunk(wav[:, i * 16 * hops:(i + 1) * 16 * hops], emb, pre)
        outs.append(pre.clone())
        if use_graph:
            assert any(len(u) == 2 for (_, u) in net._chunk_graphs) and len(net._chunk_graphs) <= net._CHUNK_GRAPH_CAP
    # (170 hops side by side take another GEMM kernel for the output layer than one hop at a time: equal to fp32 rounding,
    #  not bit for bit as at 20 hops; a dropped Mem-LSTM update shows up at 1e-2)
    print("max difference", float((outs[0] - outs[1]).abs().max()))
    assert float((outs[0] - outs[1]).abs().max()) < 2e-6


def test_mask_functions_and_magphase_on_the_device(PA, dev, golden_dir):
    """The reference's mask functions (base_nn.py:41-190) and the "MagPhase" STFT output (lobe/encoder.py:384-389) as
    HIP kernels against the reference's golden values; the pairings the reference itself cannot run fail the same way."""
    c = cases.CASES["mask_functions"]
    g = np.load(f"{golden_dir}/mask_functions.npz")
    tf_rep, mask, wav = cases.func_inputs(c)
    m = PA.SoTaskWrapModule.__mro__[1]()  # EncDecMaskerBaseModel
    x, k = tf_rep.to(dev), mask.to(dev)
    for con in ("linear", "relu", "sigmoid"):
        assert rel_max(m.get_mask(k, con).cpu().numpy(), g["get_mask_" + con]) < TOL
    assert rel_max(m.apply_tf_masks(x, k, "complex", "complex").cpu().numpy(), g["complex_complex"]) < TOL
    assert rel_max(m.apply_tf_masks(x, k, "real", "real").cpu().numpy(), g["real_real"]) < TOL
    re, im = torch.chunk(x, 2, dim=1)
    mre, mim = torch.chunk(k, 2, dim=1)
    got = m._apply_complex_mask_on_polar(torch.stack([re, im], -1), torch.stack([mre, mim], -1))
    assert rel_max(got.cpu().numpy(), g["polar"]) < TOL
    with pytest.raises(RuntimeError):
        m.apply_tf_masks(x, k, "polar", "polar")
    with pytest.raises(UnboundLocalError):
        m.apply_tf_masks(x, k, "real", "complex")
    with pytest.raises(NotImplementedError):
        m.get_mask(k, "softmax")
    for tr in (True, False):
        enc = PA.ConvEncDec(fft_length=c["n_fft"], win_type="hann", win_length=c["n_fft"], hop_length=c["hop"],
                            trainable=tr, output_format="MagPhase").eval()
        enc.load_state_dict(det_state_dict(enc))
        got = enc.to(dev)(wav.to(dev)).cpu().numpy()
        want = g["magphase_trainable" if tr else "magphase_fixed"]
        assert got.shape == want.shape
        assert rel_max(got[..., 0], want[..., 0]) < TOL
        big = want[..., 0] > 1e-3 * want[..., 0].max()
        assert np.abs(np.exp(1j * got[..., 1]) - np.exp(1j * want[..., 1]))[big].max() < 1e-3


# ---- bf16 activation rows (BASELINE "bf16" configurations: bf16 storage, fp32 accumulation) ---------------------------
@pytest.mark.parametrize("flags", [0, _abi.PS_DBG_GEMM_ANY_SIZE, _abi.PS_DBG_GEMM_SIMPLE])
@pytest.mark.parametrize("n,k,m,t,mode,xb,yb", [(8, 512, 256, 3999, "stats", False, True),
                                                (8, 256, 256, 3999, "norm_stats", True, True),
                                                (8, 256, 512, 3999, "norm_res", True, False),
                                                (3, 256, 256, 500, "norm_stats", True, True),
                                                (2, 64, 300, 257, "plain", True, True)])
def test_conv1x1_bf16_rows_equal_the_fp32_row_kernel_on_rounded_data(dev, flags, n, k, m, t, mode, xb, yb):
    """ps_conv1x1_bf16_io with bf16 x / y rows against the same kernel on fp32 rows holding the bf16-rounded values:
    the accumulation is the same instruction stream, so the fp32 result rounded to bf16 is reproduced bit for bit and
    the statistics (taken from the fp32 values) agree."""
    from puresound_amd import hip as H, _abi
    g = torch.Generator().manual_seed(7)
    x = (torch.rand(n, k, t, generator=g) * 2 - 0.8).bfloat16().float()
    w, b = (torch.rand(m, k, generator=g) - 0.5) * 0.4, torch.rand(m, generator=g) - 0.5
    gamma, beta, slope = torch.rand(k, generator=g) + 0.5, (torch.rand(k, generator=g) - 0.5) * 0.4, torch.tensor([0.2])
    pro, keep = None, None
    if mode.startswith("norm"):
        stats = torch.stack([x.double().sum((1, 2)), (x.double() ** 2).sum((1, 2))], -1).reshape(n, 1, 2).to(dev)
        keep = (stats, gamma.to(dev), beta.to(dev), slope.to(dev))
        pro = H.make_prologue(_abi.PS_NORM_GLOBAL, True, keep[0], k * t, 1e-8, keep[1], keep[2], keep[3])
    res = H.pad_rows((torch.rand(n, m, t, generator=g) - 0.5).to(dev)) if mode == "norm_res" else None
    want = mode in ("norm_stats", "stats")
    wb = H.pack_wt_bf16(w.to(dev), 1)
    xp = H.pad_rows(x.to(dev))
    with _abi.debug(flags):
        y_ref, st_ref = H.conv1x1_bf16(xp, t, wb, m, pro, b.to(dev), None, res, want_stats=want)
        y, st = H.conv1x1_bf16(xp.bfloat16() if xb else xp, t, wb, m, pro, b.to(dev), None, res, want_stats=want,
                               out_dtype=torch.bfloat16 if yb else torch.float32)
        torch.cuda.synchronize()
    assert y.dtype == (torch.bfloat16 if yb else torch.float32)
    want_y = y_ref[..., :t].bfloat16() if yb else y_ref[..., :t]
    assert torch.equal(y[..., :t], want_y)
    if want:
        np.testing.assert_allclose(st.sum(1).cpu().numpy(), st_ref.sum(1).cpu().numpy(), rtol=1e-9)


@pytest.mark.parametrize("dil,causal", [(1, False), (2, True), (8, False), (128, False), (128, True)])
def test_dwconv_bf16_rows(dev, dil, causal):
    from puresound_amd import hip as H, _abi
    g = torch.Generator().manual_seed(9)
    n, h, t = 3, 40, 1500
    x = (torch.rand(n, h, t, generator=g) * 2 - 1).bfloat16().float()
    w, b = torch.rand(h, 1, 3, generator=g) - 0.5, torch.rand(h, generator=g) - 0.5
    gamma, beta, slope = torch.rand(h, generator=g) + 0.5, (torch.rand(h, generator=g) - 0.5) * 0.4, torch.tensor([0.3])
    stats = torch.stack([x.double().sum((1, 2)), (x.double() ** 2).sum((1, 2))], -1).reshape(n, 1, 2).to(dev)
    keep = (stats, gamma.to(dev), beta.to(dev), slope.to(dev))
    pro = H.make_prologue(_abi.PS_NORM_GLOBAL, True, keep[0], h * t, 1e-8, keep[1], keep[2], keep[3])
    left = 2 * dil if causal else dil
    xp = H.pad_rows(x.to(dev))
    y_ref, st_ref = H.dwconv(xp, t, w.to(dev), b.to(dev), dil, left, pro, True)
    # (True, True) twice: the wave-private kernel (round 4: bf16 rows there too) and, with PS_DBG_DWCONV_WG, the
    # workgroup-synchronised one
    for xb, yb, flags in ((True, True, 0), (True, True, _abi.PS_DBG_DWCONV_WG), (True, False, 0), (False, True, 0)):
        with _abi.debug(flags):
            y, st = H.dwconv(xp.bfloat16() if xb else xp, t, w.to(dev), b.to(dev), dil, left, pro, True,
                             out_dtype=torch.bfloat16 if yb else torch.float32)
            torch.cuda.synchronize()
        # (the instantiations may contract their multiply-adds differently: equal to one fp32 rounding, i.e. the bf16
        #  results differ in at most the last bit of a few elements)
        if yb:
            diff = (y[..., :t].float() - y_ref[..., :t].bfloat16().float()).abs()
            assert float(diff.max()) <= 2.0 ** -7 * float(y_ref.abs().max()), (xb, yb)
            assert float((diff > 0).float().mean()) < 1e-2, (xb, yb)
        else:
            assert torch.allclose(y[..., :t], y_ref[..., :t], rtol=1e-6, atol=1e-6), (xb, yb)
        np.testing.assert_allclose(st.sum(1).cpu().numpy(), st_ref.sum(1).cpu().numpy(), rtol=1e-6)


def test_bf16_hidden_maps_stay_inside_the_bf16_acceptance(PA, dev):
    """Config 3 in the "bf16" arithmetic with the TCN blocks' hidden maps stored as bf16 rows (the default of that
    mode) against fp32 rows: both inside the 3e-2 l2-rel acceptance against the fp32 oracle, and close to each other."""
    name = "cfg3_short"
    model, sd = _build(PA, name, dev)
    model.masker.set_gemm_precision("bf16")
    c = cases.CASES[name]
    noisy, enroll = det_wave(c["seed"], 4, 16000), det_wave(c["seed"] + 1, 4, 12000)
    ref = O.inference(noisy, sd, cases.oracle_cfg(name), enroll)
    outs = {}
    for hb in (True, False):
        for m in model.masker.modules():
            if hasattr(m, "hidden_bf16"):
                m.hidden_bf16 = hb
        outs[hb] = model.inference(noisy.to(dev), enroll.to(dev)).cpu().numpy()
        assert _l2rel(outs[hb], ref.numpy()) < 3e-2, hb
    assert not np.array_equal(outs[True], outs[False])
    assert _l2rel(outs[True], outs[False]) < 2e-2


def test_step_frame_graph_follows_parameter_updates_and_states_are_assignable(dev):
    """The frame-step graph of StreamingSkiM replays plan pointers: after load_state_dict it has to be captured again
    (not replay the old weights).  The reference's state attributes are assignable lists (skim_inference.py:146-164)."""
    from puresound_amd.streaming.demo import DemoTseNet
    net = DemoTseNet().eval()
    sd = det_state_dict(net)
    net.load_state_dict(sd)
    net.to(dev)
    m = net.masker
    m.init_status(2)
    g = torch.Generator().manual_seed(11)
    frames = [torch.rand(2, m.input_size, 1, generator=g).to(dev) for _ in range(6)]
    emb = torch.rand(2, 192, generator=g).to(dev)
    first = [m.step_frame(f, emb) for f in frames[:3]]
    saved_h, saved_c = m.seg_lstm_h_states, m.seg_lstm_c_states
    assert m._graph is not None
    # new weights: the graph must not replay the old plans
    sd2 = {k: (v * 1.25 if v.dtype.is_floating_point and "weight" in k else v) for k, v in sd.items()}
    net.load_state_dict(sd2)
    after = m.step_frame(frames[3], emb)
    m2 = DemoTseNet().eval()
    m2.load_state_dict(sd2)
    m2.to(dev)
    m2.masker.init_status(2, use_graph=False)
    m2.masker.seg_lstm_h_states, m2.masker.seg_lstm_c_states = saved_h, saved_c  # the setters
    for a, b in zip(m2.masker.seg_lstm_h_states, saved_h):
        assert torch.equal(a, b)
    m2.masker.frames_counter = 3
    ref = m2.masker.step_frame(frames[3], emb)
    assert torch.allclose(after, ref, rtol=0, atol=1e-6), float((after - ref).abs().max())
    assert not torch.allclose(after, first[-1])
    with pytest.raises(ValueError):
        m2.masker.seg_lstm_h_states = [torch.zeros(3, 5)] * len(saved_h)


def test_magnitude_lobe_takes_the_encoders_four_dimensional_output(PA, dev):
    """Magnitude (lobe/trivial.py:21-59) on [N, H, T, 2] and on the channel-halves form [N, 2H, T]."""
    x = det_wave(31, 2 * 9 * 2, 40).reshape(2, 9, 2, 40).permute(0, 1, 3, 2).contiguous()   # [N, H, T, 2]
    for drop, log1p in ((True, False), (False, True)):
        lobe = PA.NS.Magnitude(drop_first=drop, log1p=log1p)
        re, im = x[..., 0], x[..., 1]
        if drop:
            re, im = re[:, 1:], im[:, 1:]
        ref = torch.sqrt(re ** 2 + im ** 2 + 1e-8)
        ref = torch.log1p(ref) if log1p else ref
        y4 = lobe(x.to(dev))
        y3 = lobe(torch.cat([x[..., 0], x[..., 1]], 1).to(dev))
        assert y4.shape == ref.shape and torch.equal(y4, y3)
        assert float((y4.cpu() - ref).abs().max()) < 1e-6
    with pytest.raises(TypeError):
        PA.NS.Magnitude()(x[..., :1].to(dev))
