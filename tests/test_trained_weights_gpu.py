"""Every model family with checkpoint-like weights (detweights mode "trained", trained_weight_cases.py) on the HIP path, against
the float64 oracle.  The parity fixtures carry formula weights -- gains near 1, small biases, all rows of a matrix alike -- where
the ranges of the default fp16x2 arithmetic sit at their easiest point: the amax chain through proj_layernorm, the per-matrix
exponents of the weight packers, conv2d's wave-local ranges, the frame-major LSTM scales, the attention softmax, the one-pass
statistics of the global norms.  Here they run at gains over 2^-2 .. 2^2, biases in +-1 and weight rows 2^8 apart:

(1) every preset in "fp32", "bf16x3" and "fp16x2" at two amplitudes: the waveform in front of the output clamp (what
    inference() returns is the clamp of exactly that waveform: asserted), the speaker embedding, both finite;
(2) the kernels the fixture size does not choose by itself: the persistent and the simple GEMM kernels and the workgroup
    depthwise kernel in the two TCN presets, the general and the narrow attention kernel, the three-pass pooling, and the
    one-launch GEMM + LayerNorm and GEMM + chan_layernorm branches behind the recurrences;
(3) every recurrence kernel: the launches of the recurrence entries are recorded per call (and held against what
    _plans.lstm_route answered: it is pure, wrapped), and "generic", "generic_f16x2", "fmajor128", "fmajor256" (the
    streamed-weight kernel), "h256_f32" and the cooperative kernel must each have been launched;
(4) per-utterance ranges: a batch of 3 whose middle utterance is 1e3 times quieter, each row against its own float64 result
    and against its run on its own;
(5) each streaming class once, against the float64 oracle of the same causal preset.

Bounds are trained_weight_cases.bound: 1e-4 for the split arithmetics, max(2e-5, 20 x the oracle's own float32 noise) for
"fp32".  Measured on the MI355X over the 113 tests (20 s; profiles/trained_weights.txt has every figure): offline at most
3.8e-6 on every preset but cfg3_causal_short, where all three arithmetics land at the oracle's own float32 noise (2.4e-5 at
most against its 1.3e-5); streamed at most 9.1e-6; a row of the batch of 3 equals its lone run bit for bit except in DPCRN
(5.2e-7).  With PS_TRAINED_WEIGHTS_TABLE=<path> in the environment the module writes every measured error to that file when its
last test has run (profiles/trained_weights.txt keeps the table)."""
import contextlib
import os

import pytest
import torch

import cases
import trained_weight_cases as W

pytestmark = pytest.mark.gpu

_MODELS = {}
_RUNS = {}
_ROWS = []
KERNELS = ("generic", "generic_f16x2", "fmajor128", "fmajor256", "h256_f32", "coop")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def PA():
    import puresound_amd.nnet as PA
    from puresound_amd import hip
    hip.lib()  # fail loudly if the extension is missing
    return PA


@pytest.fixture(autouse=True)
def _nan_in_the_allocator_cache(dev):
    """NaN-filled blocks in torch's caching allocator, as in test_hip_parity.py: scratch that a kernel leaves unwritten holds
    NaN, not the zeros of a fresh process."""
    junk = [torch.full((1 << 22,), float("nan"), device=dev) for _ in range(16)]
    junk += [torch.full((n,), float("nan"), device=dev) for n in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20)]
    del junk
    yield
    try:
        torch.cuda.synchronize(dev)
    except RuntimeError as e:   # a fault of the device, not a wrong number: nothing more is launched on it
        pytest.exit(f"the device reports {e}", returncode=3)


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    path = os.environ.get("PS_TRAINED_WEIGHTS_TABLE")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(_ROWS) + "\n")
    _MODELS.clear()
    _RUNS.clear()


def _model(PA, dev, name):
    if name not in _MODELS:
        model = cases.build(PA.NS, name).eval()
        model.load_state_dict(W.weights(name)[0])
        _MODELS[name] = model.to(dev)
    return _MODELS[name]


# recurrence kernel of a route -> what may be launched for it (the wrapper of "fmajor256" picks the cooperative kernel by itself;
# lstm_recurrence falls back to the generic entry when ps_lstm_h256_ok refuses an "h256_f32" pass)
LAUNCHES_OF = {"generic": {"generic"}, "generic_f16x2": {"generic_f16x2"}, "fmajor128": {"fmajor128"},
               "fmajor256": {"fmajor256", "coop"}, "h256_f32": {"h256_f32", "generic"}}


@contextlib.contextmanager
def _recorded_launches(seen):
    """Inside the block every LAUNCH of a recurrence entry adds its kernel to `seen` -- the wrappers of puresound_amd.hip that
    _plans.lstm_recurrence calls are wrapped, and "fmajor256" stands for the streamed-weight kernel alone: a launch that
    hip.lstm_fmajor_h256 gave to the cooperative kernel (it leaves the workspace of each behind) counts as "coop".  What
    _plans.lstm_route answered (it is pure: wrapped too) must allow every launch that was seen."""
    from puresound_amd import hip
    from puresound_amd.nnet import _plans
    from puresound_amd.nnet.lobe import rnn as lobe_rnn
    route = _plans.lstm_route
    assert lobe_rnn.lstm_route is route
    inner = {fn: getattr(hip, fn) for fn in ("lstm", "lstm_fmajor", "lstm_fmajor_h256", "lstm_h256_f32")}
    routed = set()

    def lstm_route(*args, **kw):
        r = route(*args, **kw)
        routed.add(r.kernel)
        return r

    def lstm(*args, **kw):
        seen.add("generic_f16x2" if kw.get("f16x2") else "generic")
        return inner["lstm"](*args, **kw)

    def lstm_fmajor(*args, **kw):
        seen.add("fmajor128")
        return inner["lstm_fmajor"](*args, **kw)

    def lstm_fmajor_h256(*args, **kw):
        before = hip._COOP_LAST[0]
        out = inner["lstm_fmajor_h256"](*args, **kw)
        seen.add("fmajor256" if hip._COOP_LAST[0] is before else "coop")
        return out

    def lstm_h256_f32(*args, **kw):
        seen.add("h256_f32")
        return inner["lstm_h256_f32"](*args, **kw)

    _plans.lstm_route = lobe_rnn.lstm_route = lstm_route
    for fn, wrapped in (("lstm", lstm), ("lstm_fmajor", lstm_fmajor), ("lstm_fmajor_h256", lstm_fmajor_h256),
                        ("lstm_h256_f32", lstm_h256_f32)):
        setattr(hip, fn, wrapped)
    try:
        yield
    finally:
        _plans.lstm_route = lobe_rnn.lstm_route = route
        for fn, f in inner.items():
            setattr(hip, fn, f)
    # ("generic" needs no route: the LSTM inside DPARN's attention layers launches ps_lstm_f32 itself)
    assert seen <= set().union({"generic"}, *[LAUNCHES_OF[k] for k in routed]), (seen, routed)


def _preclamp(PA, model, noisy, enroll):
    """SoTaskWrapModule._inference step by step, with the decoder's output constraint "none" in place of the model's."""
    from puresound_amd import hip
    mask_act = model.check_mask_constraint(model.mask_constraint)
    pairing = model.check_mask_pairing(model.mask_type, model.f_type)
    if isinstance(model.encoder, PA.NS.ConvEncDec):
        enc = model.encoder.encoder
        dvec = None if enroll is None else model._speaker_embedding(enroll)
        feats, t = enc.encode_padded(noisy, model.drop_first_bin)
        mask = model.masker.forward_padded(feats, t, dvec)
        enh = hip.complex_mask(feats, mask, mask_act) if pairing == "complex" else hip.real_mask(feats, mask, mask_act)
        return enc.decode_padded(enh, t, model.drop_first_bin, "none")
    need = model.masker.padded_frames_needed if isinstance(model.masker, (PA.NS.DPRNN, PA.NS.SkiM)) else None
    dvec, kw = None, {}
    if enroll is not None and model.embedding_free_tse:
        dvec, te = model.encoder.encode_padded(enroll, need)
        kw = dict(embed_frames=te)
    elif enroll is not None:
        dvec = model._speaker_embedding(enroll, 0)
    feats, t = model.encoder.encode_padded(noisy, need)
    if getattr(model.masker, "takes_input_range", False) and hasattr(model.encoder, "feature_bound"):
        kw["x_amax"] = model.encoder.feature_bound(noisy)
    mask = model.masker.forward_padded(feats, t, dvec, lane=0, **kw)
    return model.encoder.decode_padded(feats, t, mask, mask_act, "none")


@torch.no_grad()
def _run(PA, dev, name, prec, noisy, enroll, coop=True):
    """-> {"pre": pre-clamp waveform, "dvec": embedding or None, "routes": recurrence kernels that were launched} of one call,
    all on the CPU; what inference() returns is the clamp of "pre", bit for bit.  coop = False: inside hip.coop_lstm_off(), as
    the lanes of a split batch run (the H = 256 / 192 recurrences stream W_hh, whatever their size)."""
    from puresound_amd import hip
    model = _model(PA, dev, name).set_gemm_precision(prec)
    noisy, enroll = noisy.to(dev).contiguous(), None if enroll is None else enroll.to(dev).contiguous()
    routes = set()
    with _recorded_launches(routes), (contextlib.nullcontext() if coop else hip.coop_lstm_off()):
        pre = _preclamp(PA, model, noisy, enroll)
        dvec = model.inference_tse_embedding(enroll)[..., 0] if W.has_speaker_net(name) else None
        out = model.inference(noisy, enroll)
    torch.cuda.synchronize(dev)
    assert out.dtype == torch.float32 and torch.equal(out, pre.clamp(min=-1.0, max=1.0)), (name, prec)
    return {"pre": pre.cpu(), "dvec": None if dvec is None else dvec.cpu(), "routes": routes}


def _case(PA, dev, name, prec, amp, batch=W.BATCH, coop=True):
    """The run of part (1), made once: part (3) reads the same runs."""
    key = (name, prec, amp, batch, coop)
    if key not in _RUNS:
        noisy, enroll, _ = W.problem(name, amp, batch)
        _RUNS[key] = _run(PA, dev, name, prec, noisy, enroll, coop)
    return _RUNS[key]


def _held(what, name, prec, got, ref, bound=None):
    """Shape, finiteness and every metric of `got` against the float64 results `ref`; prints and records each figure first
    -> the misses."""
    bound = W.bound(name, prec) if bound is None else bound
    assert got["pre"].dtype == torch.float32 and got["pre"].shape == ref["pre"].shape, (what, got["pre"].shape)
    assert bool(torch.isfinite(got["pre"]).all()), (what, name, prec)
    err = W.errors(name, got["pre"].numpy(), ref["pre"].numpy())
    if ref["dvec"] is not None:
        assert got["dvec"].shape == ref["dvec"].shape and bool(torch.isfinite(got["dvec"]).all()), (what, name, prec)
        err["dvec"] = W.embedding_error(got["dvec"].numpy(), ref["dvec"].numpy())
    row = (f"{what:<34} {name:<26} {prec:<7} " + " ".join(f"{m} {v:.3e}" for m, v in err.items())
           + f"  bound {bound:.1e}" + (f"  lstm {'+'.join(sorted(got['routes']))}" if got.get("routes") else ""))
    print(row)
    _ROWS.append(row)
    return [(what, name, prec, m, v, bound) for m, v in err.items() if not v < bound]


# ---- (1) every preset, every arithmetic, two amplitudes ---------------------------------------------------------------------
@pytest.mark.parametrize("prec", W.PRECISIONS)
@pytest.mark.parametrize("name,amp", W.all_cases())
def test_preset_with_trained_weights(PA, dev, name, amp, prec):
    _, _, ref = W.problem(name, amp)
    missed = _held(f"(1) amp {amp:g}", name, prec, _case(PA, dev, name, prec, amp), ref)
    assert not missed, missed


# ---- (2) the kernels the fixture size does not choose by itself -------------------------------------------------------------
def _under(PA, dev, what, name, precisions, flags=0):
    from puresound_amd import _abi
    missed = []
    for amp in W.AMPS:
        noisy, enroll, ref = W.problem(name, amp)
        for prec in precisions:
            with _abi.debug(flags):
                got = _run(PA, dev, name, prec, noisy, enroll)
            missed += _held(f"(2) {what}, amp {amp:g}", name, prec, got, ref)
    assert not missed, missed


def _gemm_settings():
    from puresound_amd import _abi
    return {"persistent GEMM": (_abi.PS_DBG_GEMM_ANY_SIZE, ("bf16x3", "fp16x2")),
            "persistent GEMM, no reg-B": (_abi.PS_DBG_GEMM_ANY_SIZE | _abi.PS_DBG_GEMM_NO_RB, ("bf16x3", "fp16x2")),
            "simple GEMM": (_abi.PS_DBG_GEMM_SIMPLE, ("bf16x3", "fp16x2")),
            "workgroup depthwise": (_abi.PS_DBG_DWCONV_WG, ("fp32", "fp16x2"))}


@pytest.mark.parametrize("what", ["persistent GEMM", "persistent GEMM, no reg-B", "simple GEMM", "workgroup depthwise"])
@pytest.mark.parametrize("name", ["cfg2_short", "cfg3_causal_short"])
def test_tcn_presets_under_the_other_gemm_and_depthwise_kernels(PA, dev, name, what):
    flags, precisions = _gemm_settings()[what]
    _under(PA, dev, what, name, precisions, flags)


@pytest.mark.parametrize("what", ["PS_DBG_ATTN_GENERAL", "PS_DBG_ATTN_NARROW"])
def test_dparn_under_the_other_attention_kernels(PA, dev, what):
    from puresound_amd import _abi
    _under(PA, dev, what[7:].lower().replace("_", " "), "ns_dparn_short", W.PRECISIONS, getattr(_abi, what))


@pytest.mark.parametrize("name", [n for n in W.PRESETS if W.has_speaker_net(n)])
def test_speaker_presets_under_the_three_pass_pooling(PA, dev, name):
    from puresound_amd import _abi
    _under(PA, dev, "three-pass pooling", name, W.PRECISIONS, _abi.PS_DBG_POOL_THREE_PASS)


RECURRENT = [n for n in W.PRESETS if cases.CASES[n]["masker"].get("cls") in ("DPRNN", "SkiM", "DPCRN", "DPARN")]


@pytest.mark.parametrize("off", [("FUSE_PROJ_LN",), ("FUSE_PROJ_LN", "FUSE_GEMM_LN")], ids=["gemm_ln", "gemm_chan_ln"])
@pytest.mark.parametrize("name", RECURRENT)
def test_recurrent_presets_without_the_fused_projection_norms(PA, dev, monkeypatch, name, off):
    """Without the projection + LayerNorm row kernel a recurrence's second half is the one-launch fp16x2 GEMM + LayerNorm
    (128 output rows; a launch of this size takes it under PS_DBG_GEMM_ANY_SIZE only: two utterances are too few tiles for
    the chip) or, that one off too, the GEMM and chan_layernorm as two launches.  Which of the two _proj_norm launched is
    counted (its own calls only: DPARN's attention layers launch the same kernels themselves, whatever the switches)."""
    import sys
    from puresound_amd import _abi, hip
    from puresound_amd.nnet import _plans
    assert len(RECURRENT) == 7
    for switch in off:
        assert getattr(_plans, switch) is True
        monkeypatch.setattr(_plans, switch, False)
    calls = {"conv1x1_f16x2_ln": 0, "chan_layernorm": 0, "proj_layernorm": 0}
    for fn in calls:
        def counted(*args, _fn=fn, _inner=getattr(hip, fn), **kw):
            calls[_fn] += sys._getframe(1).f_code is _plans._proj_norm.__code__
            return _inner(*args, **kw)
        monkeypatch.setattr(hip, fn, counted)
    _under(PA, dev, "no " + " / ".join(s[5:] for s in off), name, W.PRECISIONS, _abi.PS_DBG_GEMM_ANY_SIZE)
    row = f"(2) no {' / '.join(s[5:] for s in off)}: {name}: _proj_norm launched {calls}"
    print(row)
    _ROWS.append(row)
    assert calls["proj_layernorm"] == 0 and calls["chan_layernorm"] > 0    # ("fp32" and "bf16x3" have no one-launch form)
    assert (calls["conv1x1_f16x2_ln"] > 0) == (len(off) == 1), calls


# ---- (3) every recurrence kernel --------------------------------------------------------------------------------------------
def test_every_recurrence_kernel_ran_under_the_law(PA, dev):
    """What is recorded is the launch, not the route's answer (_recorded_launches).  The presets at B = 2 reach three of the six.
    ps_lstm_h256_f32 takes a pass of 128 sequences or more in "fp32": the causal SkiM's two segments of 64 utterances.  The
    frame-major H = 256 / 192 recurrences stand behind the frame-major fp16x2 GEMM, which wants 128 pairs of tiles:
    tse_skim_v1's speaker LSTM (1536 gate rows = 6 tiles, 186 frames = one pair) has them from 22 utterances on, its segment
    LSTMs from 16 on -- 32 utterances, two whole groups of 16 sequences.  Every one of those passes fits the cooperative
    kernel (it takes up to 64 groups of 16 sequences at H = 256: the streamed-weight kernel by itself starts past 1024
    sequences), so the streamed kernel runs the same batch inside hip.coop_lstm_off(), as the lanes of a split batch do."""
    from puresound_amd import hip
    amp = W.AMPS[1]
    seen = {}
    for name in RECURRENT:
        for prec in ("fp32", "fp16x2"):
            for k in _case(PA, dev, name, prec, amp)["routes"]:
                seen.setdefault(k, []).append(f"{name} [{prec}]")
    assert hip.H256_F32_MIN_SEQS[(256, 1)] == 128
    missed = []
    for name, prec, batch, coop in (("tse_skim_causal_short", "fp32", 64, True), ("tse_skim_v1_short", "fp16x2", 32, True),
                                    ("tse_skim_v1_short", "fp16x2", 32, False)):
        _, _, ref = W.problem(name, amp, batch)
        got = _case(PA, dev, name, prec, amp, batch, coop)
        how = f"B = {batch}" + ("" if coop else ", coop_lstm_off")
        missed += _held(f"(3) {how}, amp {amp:g}", name, prec, got, ref)
        assert ("coop" in got["routes"]) == (coop and prec == "fp16x2"), got["routes"]
        for k in got["routes"]:
            seen.setdefault(k, []).append(f"{name} [{prec}] {how}")
    for k in KERNELS:
        row = f"(3) lstm kernel {k:<14} " + (", ".join(seen[k]) if k in seen else "NOT VISITED")
        print(row)
        _ROWS.append(row)
    assert sorted(seen) == sorted(KERNELS), seen
    assert not missed, missed


# ---- (4) per-utterance ranges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", W.RANGE_PRESETS)
def test_a_quiet_utterance_between_two_loud_ones(PA, dev, name):
    prec = "fp16x2"
    noisy, enroll, ref = W.problem(name, W.RANGE_AMP, 3, 1)
    tops = ref["pre"].abs().amax(dim=1)
    assert float(tops[1]) < 1e-2 * float(min(tops[0], tops[2]))
    whole = _run(PA, dev, name, prec, noisy, enroll)
    missed = []
    for b in range(3):
        row = lambda r: {k: (v[b:b + 1] if torch.is_tensor(v) else None) for k, v in r.items() if k != "routes"}  # noqa: E731
        missed += _held(f"(4) row {b} of 3, middle x {W.QUIET:g}", name, prec, row(whole), row(ref))
        alone = _run(PA, dev, name, prec, noisy[b:b + 1], None if enroll is None else enroll[b:b + 1])
        alone.pop("routes")
        missed += _held(f"(4) row {b} of 3 against alone", name, prec, row(whole), alone, W.ROW_TOL)
    assert not missed, missed


# ---- (5) the streaming classes ----------------------------------------------------------------------------------------------
def _streamed(s, x, chunk, **init):
    """Stream x [B, L] (L a multiple of the hop) in chunks of `chunk` hops -> emitted samples ‖ flush(), [B, L_out]"""
    hop = s.hop_length
    s.init_streams(streams=x.shape[0], **init)
    outs, hops = [], x.shape[1] // hop
    for i in range(0, hops, chunk):
        y = s.step_chunk(x[:, i * hop:min(hops, i + chunk) * hop])
        if y is not None:
            outs.append(y)
    outs.append(s.flush())
    return torch.cat(outs, dim=1)


@pytest.mark.parametrize("kind", list(W.STREAMED))
@torch.no_grad()
def test_streaming_class_with_trained_weights(PA, dev, kind):
    from puresound_amd import streaming
    amp = W.STREAMED[kind][1]
    cls = {"tcn": "StreamingConvTasNet", "dprnn": "StreamingDPRNN", "skim": "StreamingSkiMExtractor",
           "spectral": "StreamingSeparator", "unet_tcn": "StreamingUnetTcn"}[kind]
    name, noisy, enroll, ref = W.stream_problem(kind)   # (inside the clamp: the streamed waveform is the one in front of it)
    s = getattr(streaming, cls)(_model(PA, dev, name))
    hop = s.hop_length
    x = noisy[:, :noisy.shape[1] // hop * hop].contiguous().to(dev)
    y = _streamed(s, x, 5, **({} if enroll is None else {"enroll": enroll.to(dev)})).cpu()
    missed = _held(f"(5) {cls}, amp {amp:g}", name, "fp32", {"pre": y, "dvec": None},
                   {"pre": ref["pre"].clamp(min=-1.0, max=1.0), "dvec": None}, W.STREAM_TOL)
    assert not missed, missed
