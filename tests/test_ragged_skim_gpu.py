"""Batches of utterances of unequal length through the SkiM speaker extractors on the MI355X: SoTaskWrapModule.inference(noisy,
enroll, lengths=..., enroll_lengths=...) and inference_scored_ragged on tse_skim_v0_causal, tse_skim_v0, tse_skim_v0_causal_vad
and tse_skim_v1_causal at preset size (ragged_skim_cases.py), every row against the float64 oracle of the utterance alone: a
batch of one, with no hand-over from the row above.

Bounds: edge_length_cases.bounds(name, "fp32") = FP32_TOL 2e-5 is the project's bound for tse_skim_causal_short in the exact-fp32
arithmetic (test_edge_lengths_gpu.py), and the ragged path forms the same products.  The three other presets have not been
held to it by plain inference so far: the test first measures plain fp32 inference of each utterance alone against the
oracle and holds the ragged row to the larger of FP32_TOL and twice that figure, never above PROJECT_TOL 1e-4; both figures
are printed.  The junk behind an utterance is 20 x the signal's amplitude, or NaN (the same bits are asserted);
test_ragged_skim.py shows that zero-padding moves the oracle's answer by >= 0.12 on every short row of this batch, and that
the reference's hand-over moves rows 1 and 2 of the equal-length batch by >= 0.4."""
import pytest
import torch
import torch.nn as nn

import cases
import edge_length_cases as E
import ragged_skim_cases as K

pytestmark = pytest.mark.gpu
NAN = float("nan")
SWITCH_TOL = 2e-5     # ragged against plain fp32 inference where both compute the same thing on other kernels
CAUSAL = "tse_skim_causal_short"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def PA():
    import puresound_amd.nnet as PA
    from puresound_amd import hip
    hip.lib()
    return PA


@pytest.fixture(autouse=True)
def _nan_in_the_allocator_cache(dev):
    """NaN-filled blocks in torch's caching allocator: `torch.empty` scratch and outputs start as NaN, not as zeros."""
    junk = [torch.full((1 << 22,), NAN, device=dev) for _ in range(16)]
    del junk
    yield


_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _give_the_device_memory_back(dev):
    yield
    import gc
    _MODELS.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _model(PA, dev, name):
    """one model per name for the module, in the default arithmetic (fp16x2) unless a test says otherwise and puts it back"""
    if name not in _MODELS:
        model = cases.build(PA.NS, name).eval()
        model.load_state_dict(E.weights(name)[0])
        _MODELS[name] = model.to(dev)
    assert _MODELS[name].masker.gemm_precision == "fp16x2"
    return _MODELS[name]


def _ragged(model, dev, b):
    noisy, lens, enroll, e_lens, _ = b
    return model.inference(noisy.to(dev), enroll.to(dev), lengths=lens, enroll_lengths=e_lens)


def _rows_against_the_oracle(model, dev, name, b, frames, what):
    """-> the rows that miss their bound; prints (row, plain fp32 alone, ragged, bound)"""
    noisy, lens, enroll, e_lens, refs = b
    got = _ragged(model, dev, b).cpu()
    outs = [E.out_length(name, t) for t in frames]
    assert got.dtype == torch.float32 and got.shape == (len(lens), max(outs))
    assert model.output_lengths(lens) == outs
    missed = []
    for n, t in enumerate(frames):
        assert float(got[n, outs[n]:].abs().max() if outs[n] < got.shape[1] else 0.0) == 0.0, (n, t)
        assert E.clamped_share(name, refs[n].numpy()) <= E.CLAMP_CAP
        bound, alone_err = E.bounds(name, "fp32")["rel_max"], float("nan")
        if name != CAUSAL:
            try:
                model.set_gemm_precision("fp32")
                alone = model.inference(noisy[n:n + 1, :lens[n]].to(dev), enroll[n:n + 1, :e_lens[n]].to(dev)).cpu()
            finally:
                model.set_gemm_precision("fp16x2")
            alone_err = E.errors(name, alone.numpy(), refs[n].numpy())["rel_max"]
            bound = min(max(E.FP32_TOL, 2.0 * alone_err), E.PROJECT_TOL)
        err = E.errors(name, got[n:n + 1, :outs[n]].numpy(), refs[n].numpy())["rel_max"]
        print(f"{name} {what} row {n} (T = {t}, T' = {e_lens[n]} samples): plain fp32 alone {alone_err:.3e}, ragged {err:.3e}, "
              f"bound {bound:.1e}")
        if not err <= bound:
            missed.append((n, t, err, bound))
    return missed


@pytest.mark.parametrize("name", K.NAMES)
def test_every_row_is_its_utterance_alone(PA, dev, name):
    """parity with the float64 oracle of each utterance alone, exact zeros behind it (under the Sigmoid output constraint of
    tse_skim_vad_short too), the same bits with NaN for junk and in either arithmetic setting"""
    model = _model(PA, dev, name)
    b = K.batch(name)
    missed = _rows_against_the_oracle(model, dev, name, b, K.SKIM_T, "ragged batch")
    got = _ragged(model, dev, b)
    assert torch.equal(_ragged(model, dev, K.batch(name, "nan")), got), "the junk reached the result"
    try:
        model.set_gemm_precision("fp32")
        assert torch.equal(_ragged(model, dev, b), got), "gemm_precision changed the bits"
    finally:
        model.set_gemm_precision("fp16x2")
    assert torch.equal(_ragged(model, dev, b), got)
    assert not missed, missed


@pytest.mark.parametrize("name", K.NAMES)
def test_plain_inference_is_untouched_by_a_ragged_call(PA, dev, name):
    model = _model(PA, dev, name)
    noisy, enroll = E.inputs(name, E.length_of(name, 151), 3, E.length_of(name, 50))
    noisy, enroll = noisy.to(dev), enroll.to(dev)
    before = model.inference(noisy, enroll)                # the default arithmetic, the model's own plans and kept rows
    ragged = _ragged(model, dev, K.batch(name))
    assert torch.equal(model.inference(noisy, enroll), before), "a ragged call changed plain inference"
    assert torch.equal(_ragged(model, dev, K.batch(name)), ragged)
    assert torch.equal(model.inference(noisy, enroll), before)


@pytest.mark.parametrize("name", [CAUSAL, "tse_skim_v0_short"])
def test_equal_lengths(PA, dev, name):
    """three rows of one length: every row is its utterance alone -- for the causal preset that is where the per-row
    hand-over shows (the plain batch hands row n the last segment of row n - 1, as the reference does)"""
    model = _model(PA, dev, name)
    b = K.equal_batch(name)
    noisy, lens, enroll, e_lens, _ = b
    assert len(set(lens)) == 1 and len(set(e_lens)) == 1
    missed = _rows_against_the_oracle(model, dev, name, b, K.EQUAL_T, "equal lengths")
    assert not missed, missed
    got = _ragged(model, dev, b).cpu()
    try:
        model.set_gemm_precision("fp32")
        plain = model.inference(noisy.to(dev), enroll.to(dev)).cpu()
    finally:
        model.set_gemm_precision("fp16x2")
    assert plain.shape == got.shape
    rows = range(len(lens)) if name != CAUSAL else [0]
    for n in rows:
        err = E.errors(name, got[n:n + 1].numpy(), plain[n:n + 1].numpy())["rel_max"]
        print(f"{name} equal lengths row {n}: ragged against plain fp32 inference of the batch, rel_max {err:.3e}")
        assert err <= SWITCH_TOL, (n, err)


@pytest.mark.parametrize("name", [CAUSAL, "tse_skim_v0_short"])
def test_enough_segments_for_the_h256_kernel(PA, dev, name):
    """32 rows of 1 ... 751 frames: 192 segment sequences, past hip.H256_F32_MIN_SEQS, so the Seg-LSTMs take ps_lstm_h256_f32
    (with the per-row shifted states of the causal preset) where the batches above take the thread-per-gate-row kernel.  No
    oracle at this size: each row against plain fp32 inference of the utterance alone (which the tests above hold to the
    oracle), within SWITCH_TOL."""
    from puresound_amd import hip
    model = _model(PA, dev, name)
    n = 32
    frames = [1 + 750 * i // (n - 1) for i in range(n)]
    e_frames = [1 + 185 * ((7 * i) % n) // (n - 1) for i in range(n)]
    assert n * (max(frames) // K.SEG + 1) >= hip.H256_F32_MIN_SEQS[(256, 1)] and max(frames) % K.SEG != 0
    lens, e_lens = [E.length_of(name, t) for t in frames], [E.length_of(name, t) for t in e_frames]
    noisy, enroll = E.inputs(name, max(lens), n, max(e_lens))
    noisy, enroll = noisy.to(dev), enroll.to(dev)
    for i in range(n):                       # junk behind every utterance
        noisy[i, lens[i]:] = NAN
        enroll[i, e_lens[i]:] = NAN
    got = model.inference(noisy, enroll, lengths=lens, enroll_lengths=e_lens)
    outs = model.output_lengths(lens)
    worst = 0.0
    try:
        model.set_gemm_precision("fp32")
        for i in range(n):
            alone = model.inference(noisy[i:i + 1, :lens[i]], enroll[i:i + 1, :e_lens[i]])
            assert float(got[i, outs[i]:].abs().max() if outs[i] < got.shape[1] else 0.0) == 0.0
            err = E.errors(name, got[i:i + 1, :outs[i]].cpu().numpy(), alone.cpu().numpy())["rel_max"]
            worst = max(worst, err)
            assert err <= SWITCH_TOL, (i, frames[i], err)
    finally:
        model.set_gemm_precision("fp16x2")
    print(f"{name}: 32 rows of 1 ... 751 frames against plain fp32 inference of each alone, worst rel_max {worst:.3e}")


def test_inference_scored_ragged(PA, dev):
    name = "tse_skim_v0_short"
    model = _model(PA, dev, name)
    noisy, lens, enroll, e_lens, _ = K.batch(name)
    clean = torch.full((len(lens), max(lens)), NAN)
    for n, length in enumerate(lens):
        clean[n, :length] = E.inputs(name, length, 1, row=n + 40)[0][0]
    want = model.inference(noisy.to(dev), enroll.to(dev), lengths=lens, enroll_lengths=e_lens)
    enh, score = model.inference_scored_ragged(noisy.to(dev), clean.to(dev), enroll.to(dev),
                                               loss_func=PA.SDRLoss.init_mode("sisnr", reduction=False), lengths=lens,
                                               enroll_lengths=e_lens)
    assert torch.equal(enh, want)
    assert score.numel() == len(lens) and bool(torch.isfinite(score).all())


def test_refusals_on_device_tensors_launch_nothing(PA, dev, monkeypatch):
    from puresound_amd import hip as hip_module
    noisy, enroll, lens, e_lens = torch.zeros(2, 200, device=dev), torch.zeros(2, 160, device=dev), [200, 100], [160, 80]

    def skim(speaker_net, **kw):
        args = dict(n_blocks=2, seg_size=10, seg_overlap=False, causal=True, embed_dim=6, embed_norm=True, block_with_embed=[1, 1],
                    embed_fusion="FiLM")
        args.update(kw)
        return PA.SoTaskWrapModule(encoder=PA.FreeEncDec(win_length=16, hop_length=8, laten_length=24),
                                   masker=PA.SkiM(24, 8, 24, **args), verbose=False, speaker_net=speaker_net,
                                   mask_constraint="ReLU").eval().to(dev)
    tcn = lambda: nn.ModuleList([PA.TCN(24, 12, 3, 1), PA.AttentiveStatisticsPooling(24, 8),  # noqa: E731
                                 nn.Conv1d(48, 6, 1, bias=False)])
    gru = nn.ModuleList([PA.SingleRNN("GRU", 24, 8, bidirectional=True), PA.AttentiveStatisticsPooling(24, 8),
                         nn.Conv1d(48, 6, 1, bias=False)])
    models = [(skim(tcn(), seg_overlap=True), "seg_overlap=True"), (skim(tcn(), embed_fusion="Gate"), "Gate fusion"),
              (skim(gru), "not an LSTM"), (skim(None), "needs a speaker_net")]
    big = [(cases.build(PA.NS, "tse_skim_v2_short").eval().to(dev), "SpecAugment"),
           (cases.build(PA.NS, "tse_skim_fbank_short").eval().to(dev), "got FbankEnc"),
           (cases.build(PA.NS, "cfg4_short").eval().to(dev), "DPRNN")]
    good = _model(PA, dev, CAUSAL)
    noisy4, enroll3 = torch.zeros(2, 4000, device=dev), torch.zeros(2, 3000, device=dev)

    def lib():
        raise AssertionError("the HIP library was called")
    monkeypatch.setattr(hip_module, "lib", lib)
    for model, text in models:
        with pytest.raises(NotImplementedError, match=text):
            model.inference(noisy, enroll, lengths=lens, enroll_lengths=e_lens)
        with pytest.raises(NotImplementedError, match="inference with lengths"):
            model.inference_scored_ragged(noisy, noisy, enroll, lengths=lens, enroll_lengths=e_lens)
    for model, text in big:
        with pytest.raises(NotImplementedError, match="inference with lengths.*" + text):
            model.inference(noisy4, None if text == "DPRNN" else enroll3, lengths=[4000, 2000])
    with pytest.raises(RuntimeError, match="shorter than the window 32"):
        good.inference(noisy4, enroll3, lengths=[4000, 31])
    with pytest.raises(ValueError, match="exceeds the row length"):
        good.inference(noisy4, enroll3, lengths=[4000, 2000], enroll_lengths=[3001, 100])
