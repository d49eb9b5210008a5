"""Batches of utterances of unequal length through the egs/ns noise suppressors on the MI355X: SoTaskWrapModule.inference(...,
lengths=...) and inference_scored_ragged on ns_dpcrn_v0_causal, ns_dparn_v0_causal and their transpose_delay=True copies
(ragged_ns_cases.py), every row against the float64 oracle of the utterance alone.

Bounds, none of them new: edge_length_cases.bounds(name, "fp32") -- rel_max 1e-4 behind the 16-sample cut, the window-weighted
metric 2e-5 -- are the project's bounds for these presets in the exact-fp32 arithmetic at these lengths (test_edge_lengths_gpu.py),
and the ragged path forms the same products; stft_loss_ref.FP32_TOL is the bound test_ragged_scores_gpu.py holds the same score
to.  The junk behind an utterance is 20 x the signal's amplitude, or NaN (the same bits are asserted); test_ragged_ns.py shows
that zero-padding moves the oracle's answer by >= 0.05 on every short row of this batch."""
import numpy as np
import pytest
import torch

import cases
import edge_length_cases as E
import ragged_ns_cases as C
import stft_loss_ref as SR

pytestmark = pytest.mark.gpu
NAN = float("nan")


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
    """The four models, their two sets of plans and the kept rows go when the module is done, and the allocator's cached
    blocks with them: test files that compare uninitialised pad columns bit by bit (test_streaming_long_run_gpu.py) count on a
    pool that holds nothing but their own NaN blocks."""
    yield
    import gc
    _MODELS.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _model(PA, dev, name):
    """one model per name for the module, in the default arithmetic (fp16x2) unless a test says otherwise and puts it back"""
    if name not in _MODELS:
        model = C.build(PA.NS, name).eval()
        model.load_state_dict(C.weights(name)[0])
        _MODELS[name] = model.to(dev)
    assert _MODELS[name].masker.gemm_precision == "fp16x2"
    return _MODELS[name]


def _within(name, got, ref, what):
    err, bound = E.errors(C.BASE[name], got, ref), E.bounds(C.BASE[name], "fp32")
    print(f"{name} {what}: " + ", ".join(f"{k} {v:.3e} (bound {bound[k]:.0e})" for k, v in err.items()))
    return [f"{what}: {k} {v:.3e} > {bound[k]:.0e}" for k, v in err.items() if not v <= bound[k]]


@pytest.mark.parametrize("name", C.NAMES)
def test_every_row_is_its_utterance_alone(PA, dev, name):
    """parity with the float64 oracle of each utterance alone, exact zeros behind it, the same bits with NaN for junk and in
    either arithmetic setting (the ragged path computes exact fp32 products whatever gemm_precision says)"""
    model = _model(PA, dev, name)
    lens, outs = C.lengths(), C.out_lengths()
    assert model.output_lengths(lens) == outs
    got = model.inference(C.batch("noise").to(dev), lengths=lens)
    assert got.dtype == torch.float32 and got.shape == (len(lens), max(outs))
    assert torch.equal(model.inference(C.batch("nan").to(dev), lengths=torch.tensor(lens)), got), "the junk reached the result"
    try:
        model.set_gemm_precision("fp32")
        assert torch.equal(model.inference(C.batch("noise").to(dev), lengths=lens), got), "gemm_precision changed the bits"
    finally:
        model.set_gemm_precision("fp16x2")
    assert torch.equal(model.inference(C.batch("noise").to(dev), lengths=lens), got)
    got = got.cpu()
    missed = []
    for n, t in enumerate(C.FRAMES):
        ref = C.alone(name, n)[1]
        assert float(got[n, outs[n]:].abs().max() if outs[n] < got.shape[1] else 0.0) == 0.0, (n, t)
        assert E.clamped_share(C.BASE[name], ref.numpy()) <= E.CLAMP_CAP
        missed += _within(name, got[n:n + 1, :outs[n]].numpy(), ref.numpy(), f"row {n} (T = {t}) of the ragged batch")
    assert not missed, missed


@pytest.mark.parametrize("name", C.LOOKAHEAD)
def test_plain_inference_of_the_lookahead_copies_alone(PA, dev, name):
    """the references of the test above are only as good as the oracle's transpose_delay: plain inference of each utterance
    alone, in the exact-fp32 arithmetic, meets the same bounds"""
    model = _model(PA, dev, name)
    missed = []
    try:
        model.set_gemm_precision("fp32")
        for n, t in enumerate(C.FRAMES):
            noisy, ref = C.alone(name, n)
            got = model.inference(noisy.to(dev)).cpu()
            assert got.shape == ref.shape
            missed += _within(name, got.numpy(), ref.numpy(), f"utterance {n} (T = {t}) alone, plain inference")
    finally:
        model.set_gemm_precision("fp16x2")
    assert not missed, missed


@pytest.mark.parametrize("name", C.NAMES)
def test_equal_lengths_and_no_leak_into_plain_inference(PA, dev, name):
    model = _model(PA, dev, name)
    t = 33
    noisy = E.inputs(C.BASE[name], E.length_of(C.BASE[name], t), 3)[0].to(dev)
    before = model.inference(noisy)                       # the default arithmetic, the model's own plans
    ragged = model.inference(C.batch("noise").to(dev), lengths=C.lengths())
    assert torch.equal(model.inference(noisy), before), "a ragged call changed plain inference"
    assert torch.equal(model.inference(C.batch("noise").to(dev), lengths=C.lengths()), ragged)
    # all rows of one length: every launch is the plain path's, or its twin with T_n = T (test_ragged_ns_kernels_gpu.py)
    try:
        model.set_gemm_precision("fp32")
        plain32 = model.inference(noisy)
        equal = model.inference(noisy, lengths=[noisy.shape[1]] * 3)
    finally:
        model.set_gemm_precision("fp16x2")
    assert equal.shape == plain32.shape == (3, E.out_length(C.BASE[name], t))
    assert torch.equal(equal, plain32)
    assert torch.equal(model.inference(noisy), before)


def test_inference_scored_ragged_with_the_recipes_score(PA, dev):
    """a MultiResolutionSTFTLoss over the rows of ns_dpcrn_short: `enhanced` is inference(lengths=...) bit for bit, the score
    within stft_loss_ref.FP32_TOL of the float64 sums of each (enhanced, aligned reference) row alone"""
    from puresound_amd.nnet.loss import stft_loss as S
    name = "ns_dpcrn_short"
    model = _model(PA, dev, name)
    lens, outs = C.lengths(), C.out_lengths()
    noisy = C.batch("noise").to(dev)
    clean = torch.full((len(lens), max(lens)), NAN)
    for n, length in enumerate(lens):
        clean[n, :length] = E.inputs(name, length, 1, row=n + 40)[0][0]
    want = model.inference(noisy, lengths=lens)
    resolutions = [(64, 16, 48), (32, 8, 32)]
    mr = S.MultiResolutionSTFTLoss(*[list(v) for v in zip(*resolutions)])
    enh, total = model.inference_scored_ragged(noisy, clean.to(dev), loss_func=mr, lengths=lens)
    assert torch.equal(enh, want)
    vals = []
    for res in resolutions:
        s = np.concatenate([SR.sums(want[n:n + 1, :o].cpu().numpy(), clean[n:n + 1, :o].numpy(), *res) for n, o in enumerate(outs)])
        count = (res[0] // 2 + 1) * sum(SR.frames(o, res[0], res[1]) for o in outs)
        vals.append((np.sqrt(s[:, 0].sum()) / np.sqrt(s[:, 1].sum()), s[:, 2].sum() / count))
    want_total = SR.FACTOR_SC * float(np.mean([v[0] for v in vals])) + SR.FACTOR_MAG * float(np.mean([v[1] for v in vals]))
    print(f"multi-resolution STFT score through the wrapper: {float(total):.8g} (float64 {want_total:.8g})")
    assert SR.rel(float(total), want_total) < SR.FP32_TOL
    # an SDRLoss and a closure that takes lengths go the same way
    enh, score = model.inference_scored_ragged(noisy, clean.to(dev), loss_func=PA.SDRLoss.init_mode("sisnr", reduction=False),
                                               lengths=lens)
    assert torch.equal(enh, want) and score.numel() == len(lens) and bool(torch.isfinite(score).all())
    enh, score = model.inference_scored_ragged(noisy, clean.to(dev), lengths=lens,
                                               loss_func=lambda est, ref, unused, lengths=None: mr(est, ref, lengths=lengths))
    assert torch.equal(enh, want) and torch.equal(score, total)


def test_refusals_on_device_tensors_launch_nothing(PA, dev, monkeypatch):
    from puresound_amd import hip as hip_module
    noisy, lens = torch.zeros(2, 4000, device=dev), [4000, 2000]
    kw = dict(C.spec("ns_dpcrn_short")["masker"]["kw"])

    def wrap(masker, **more):
        args = dict(mask_constraint="linear", f_type="Complex", mask_type="Complex", drop_first_bin=True)
        args.update(more)
        return PA.SoTaskWrapModule(encoder=cases.build_encoder(PA.NS, dict(kind="stft", n_fft=512, hop=128)), masker=masker,
                                   verbose=False, **args).eval().to(dev)
    models = [(wrap(PA.DPCRN(**dict(kw, norm_type="gLN"))), "gLN"), (wrap(PA.DPCRN(**dict(kw, skip_conv=True))), "skip_conv"),
              (wrap(PA.Unet()), "got Unet"), (wrap(PA.DPCRN(**kw), f_type="real", mask_type="real"), "complex, complex"),
              (cases.build(PA.NS, "tse_unet_tcn_causal_short").eval().to(dev), "got UnetTcn"),
              (cases.build(PA.NS, "cfg1_short").eval().to(dev), "in front of a ConvTasNet")]
    good = _model(PA, dev, "ns_dpcrn_short")

    def lib():
        raise AssertionError("the HIP library was called")
    monkeypatch.setattr(hip_module, "lib", lib)
    for model, text in models:
        with pytest.raises(NotImplementedError, match=text):
            model.inference(noisy, lengths=lens)
        with pytest.raises(NotImplementedError, match="inference with lengths"):
            model.inference_scored_ragged(noisy, noisy, lengths=lens)
    with pytest.raises(NotImplementedError, match="an enrolment is not covered"):
        good.inference(noisy, torch.zeros(2, 3000, device=dev), lengths=lens)
    with pytest.raises(RuntimeError, match="shorter than the window 512"):
        good.inference(noisy, lengths=[4000, 511])
    with pytest.raises(ValueError, match="exceeds the row length"):
        good.inference(noisy, lengths=[4001, 2000])
