"""The spectral scores on the device: the two launching entries through their hip.py wrappers at their edge shapes, the
modules of puresound_amd.nnet.loss.stft_loss against the recorded values of the reference and the float64 restatement
(tests/stft_loss_ref.py, proven without a GPU by test_stft_loss.py), and inference_scored with the recipe's closure.

House rules of test_abi_kernels_gpu.py: seeded Philox inputs, NaN in the caching allocator, NaN in the pad columns an entry
promises not to read, exact zeros asserted where it promises them.  Bounds: stft_loss_ref.FP32_TOL / GOLDEN_TOL."""
import os

import numpy as np
import pytest
import torch

import cases
import stft_loss_ref as R
from abi_refs import rand as _rand
from conftest import rel_max
from detweights import det_state_dict, det_wave

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def H():
    from puresound_amd import hip
    hip.lib()
    return hip


@pytest.fixture(scope="module")
def S():
    from puresound_amd.nnet.loss import stft_loss
    return stft_loss


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "loss_stft.npz")))


@pytest.fixture(autouse=True)
def _nan_in_the_allocator_cache(dev):
    """NaN-filled blocks in torch's caching allocator: `torch.empty` scratch and outputs start as NaN, not as zeros."""
    junk = [torch.full((1 << 22,), NAN, device=dev) for _ in range(16)]
    junk += [torch.full((n,), NAN, device=dev) for n in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20)]
    del junk
    yield


# ------------------------------------------------------------------------------------------------
# ps_frame_reflect_f32
# ------------------------------------------------------------------------------------------------
def _gather(wav, n_fft, hop, win):
    """frames[r][k][t] = wav[r][reflect(t * hop + k + off - n_fft // 2)] in numpy"""
    length = wav.shape[1]
    t = R.frames(length, n_fft, hop)
    pos = (np.arange(t) * hop)[None, :] + np.arange(win)[:, None] + (n_fft - win) // 2 - n_fft // 2
    pos = np.abs(pos)
    pos = np.where(pos >= length, 2 * (length - 1) - pos, pos)
    assert pos.min() >= 0 and pos.max() < length
    return wav[:, pos]


FRAME_SHAPES = [(16, 4, 16, 9),          # L = n_fft / 2 + 1, the smallest legal length: every frame reflects on both sides
                (64, 12, 40, 33), (64, 12, 40, 1000),    # a hop that divides nothing, win < n_fft
                (16, 4, 16, 508), (16, 4, 16, 512),      # T = 128 and 129: across the 128-frame row padding
                (2048, 240, 1200, 1025),
                # an odd n_fft where hop divides L has one frame fewer than 1 + L // hop; at L = n_fft // 2 + 1 a frame more
                # would reach index -1
                (15, 4, 15, 8), (15, 4, 11, 8), (33, 5, 20, 100)]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("n_fft,hop,win,length", FRAME_SHAPES)
def test_frame_reflect_is_the_numpy_gather(H, dev, n_fft, hop, win, length, n):
    a, b = _rand((n, length), 11), _rand((n, length), 12)
    frames, t = H.frame_reflect(a.to(dev), b.to(dev), n_fft, win, hop)
    assert t == R.frames(length, n_fft, hop) and tuple(frames.shape) == (2 * n, win, H.padded_frames(t))
    want = _gather(torch.cat([a, b]).numpy(), n_fft, hop, win)
    assert np.array_equal(frames[..., :t].cpu().numpy(), want)
    assert not bool(frames[..., t:].any()), "pad columns are zero"
    # one waveform batch alone: N rows, the same bits; rows of a longer buffer (a row stride that is not L)
    wide = torch.full((n, length + 5), NAN, device=dev)
    wide[:, :length] = a.to(dev)
    alone, _ = H.frame_reflect(wide[:, :length], None, n_fft, win, hop)
    assert tuple(alone.shape) == (n, win, frames.shape[2]) and torch.equal(alone, frames[:n])


def test_frame_reflect_refusals(H, dev):
    x = torch.zeros(2, 64, device=dev)
    with pytest.raises(RuntimeError, match="length 32"):
        H.frame_reflect(x[:, :32].contiguous(), None, 64, 64, 16)       # L = n_fft / 2: one sample short
    with pytest.raises(RuntimeError, match="win"):
        H.frame_reflect(x, None, 32, 48, 16)
    with pytest.raises(RuntimeError, match="one shape"):
        H.frame_reflect(x, x[:1], 32, 32, 16)
    with pytest.raises(RuntimeError, match="out"):
        H.frame_reflect(x, None, 32, 32, 16, out=torch.zeros(2, 32, 64, device=dev))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        H.frame_reflect(x.cpu(), None, 32, 32, 16)


# ------------------------------------------------------------------------------------------------
# ps_spec_pair_moments_f64
# ------------------------------------------------------------------------------------------------
N_ROWS = 3


def _spectra(bins, t, ldt):
    """[2N, 2 bins, ldt] fp32 with NaN pads: unit-scale entries, a quarter of the bins of every row far below the clamp
    (power 1e-10 against 1e-7), reference row 1 all zero"""
    spec = torch.full((2 * N_ROWS, 2 * bins, ldt), NAN)
    body = _rand((2 * N_ROWS, 2 * bins, t), 21)
    scale = torch.where(torch.arange(bins) % 4 == 1, 1e-5, 1.0)
    body *= torch.cat([scale, scale])[None, :, None]
    body[N_ROWS + 1] = 0.0
    spec[..., :t] = body
    return spec


def _sums64(spec, bins, t, p):
    s = spec[..., :t].double().numpy()
    mags = np.sqrt(np.maximum(s[:, :bins] ** 2 + s[:, bins:] ** 2, R.CLAMP))     # [2N, bins, t]
    return R.sums_of(mags[:N_ROWS], mags[N_ROWS:], p), mags


@pytest.mark.parametrize("bins", [9, 33, 257])
@pytest.mark.parametrize("t", [1, 127, 128, 129])
def test_spec_pair_moments_against_float64(H, dev, t, bins):
    ldt = H.padded_frames(t)
    spec = _spectra(bins, t, ldt)
    on_dev = spec.to(dev)
    for p in (0.5, 1.0):
        want, mags = _sums64(spec, bins, t, p)
        assert want[1, 3] == 0.0 and (want[:, :3] > 0).all()
        mag = torch.full((2 * N_ROWS, bins, ldt), NAN, device=dev)
        got = H.spec_pair_moments(on_dev, bins, t, p, mag=mag)
        assert got.dtype == torch.float64 and tuple(got.shape) == (N_ROWS, 4)
        err = R.rel_each(got.cpu().numpy(), want)
        print(f"T={t} bins={bins} p={p}: S0..S3 per row, largest relative error {err:.3e}")
        assert err < R.FP32_TOL
        mag_err = R.rel_each(mag[..., :t].cpu().numpy(), mags)   # element by element: the clamped entries count as much
        print(f"    magnitudes, largest element-wise relative error {mag_err:.3e}")
        assert mag_err < R.FP32_TOL
        assert torch.equal(H.spec_pair_moments(on_dev, bins, t, p), got), "the sums do not depend on the optional output"
        # what the pad columns hold changes no bit
        clean = on_dev.clone()
        clean[..., t:] = 0.0
        assert torch.equal(H.spec_pair_moments(clean, bins, t, p), got)
        # a row alone gives the bits it gives inside the batch
        for n in range(N_ROWS):
            alone = on_dev[[n, N_ROWS + n]].contiguous()
            assert torch.equal(H.spec_pair_moments(alone, bins, t, p), got[n:n + 1])
    # identical halves: exactly zero distance
    same = torch.cat([on_dev[:N_ROWS], on_dev[:N_ROWS]])
    z = H.spec_pair_moments(same, bins, t, 0.5)
    assert bool((z[:, [0, 2, 3]] == 0).all()) and bool((z[:, 1] > 0).all())


def test_spec_pair_moments_refusals(H, dev):
    spec = torch.zeros(2, 18, 128, device=dev)
    with pytest.raises(RuntimeError, match="2N, 2\\*bins, ldt"):
        H.spec_pair_moments(spec, 8, 5)
    with pytest.raises(RuntimeError, match="2N, 2\\*bins, ldt"):
        H.spec_pair_moments(spec[:1], 9, 5)
    with pytest.raises(RuntimeError, match="mag"):
        H.spec_pair_moments(spec, 9, 5, mag=torch.zeros(2, 9, 256, device=dev))
    with pytest.raises(RuntimeError, match="bad argument"):
        H.spec_pair_moments(spec, 9, 129)                # T beyond the rows
    with pytest.raises(RuntimeError, match="bad argument"):
        H.spec_pair_moments(spec, 9, 5, p=0.0)


# ------------------------------------------------------------------------------------------------
# the modules
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES) + ["long"])
def test_modules_on_the_device(S, dev, golden, name):
    R.check_scores(S, name, golden, move=lambda t: t.to(dev))


def test_stft_on_the_device(S, dev, golden):
    x, y = R.pair("short")
    n_fft, hop, win = R.MAG_RESOLUTION
    for wave, key in ((x, "short.x_mag"), (y, "short.y_mag")):
        got = S.stft(wave.to(dev), n_fft, hop, win, torch.hann_window(win))
        assert got.device.type == "cuda" and tuple(got.shape) == golden[key].shape
        assert rel_max(got.cpu().numpy(), golden[key]) < R.GOLDEN_TOL
        assert rel_max(got.cpu().numpy(), R.magnitudes(wave.numpy(), n_fft, hop, win)) < R.FP32_TOL
    # at the defaults and L = 7999, with the window buffer on the device too
    long_x, _ = R.pair("long")
    for res in R.RESOLUTIONS + (R.OV_RESOLUTION,):
        f = S.STFTLoss(*res).to(dev)
        got = f.magnitudes(long_x.to(dev))
        want = R.magnitudes(long_x.numpy(), *res)
        assert tuple(got.shape) == want.shape
        err = rel_max(got.cpu().numpy(), want)
        print(f"stft {res} L=7999: rel_max {err:.3e}")
        assert err < R.FP32_TOL
        assert torch.equal(S.stft(long_x.to(dev), *res, f.window), got)


def test_identical_and_silent_signals_score_exactly_zero(S, dev):
    """Rows n and N + n of one launch hold the same signal: the same tile positions, the same bits, zero distance."""
    x, _ = R.pair("plain")
    for a in (x.to(dev), torch.zeros(2, 1100, device=dev)):
        mr = S.MultiResolutionSTFTLoss()
        for f in mr.stft_losses:
            sc, mag = f(a, a)
            assert float(sc) == 0.0 and float(mag) == 0.0
        assert float(mr(a, a)) == 0.0
        assert float(S.over_suppression_loss(a, a)) == 0.0
        assert float(S.over_suppression_loss(a, a, p=1.0)) == 0.0


def test_scores_do_not_depend_on_what_the_kept_scratch_held(S, dev):
    x, y = (t.to(dev) for t in R.pair("plain"))
    mr = S.MultiResolutionSTFTLoss()
    first = [f.moments(x, y) for f in mr.stft_losses]
    total, ov = mr(x, y), S.over_suppression_loss(x, y)
    for f, m in zip(mr.stft_losses, first):   # a second call, behind the other resolutions' use of the scratch
        assert torch.equal(f.moments(x, y), m)
    for buf in S._WORK.values():
        buf.fill_(NAN)
    assert torch.equal(mr(x, y), total) and torch.equal(S.over_suppression_loss(x, y), ov)
    # a changed window buffer is a changed basis
    f = mr.stft_losses[2]
    before = f.moments(x, y)
    with torch.no_grad():
        f.window.mul_(0.5)
    assert R.rel_each(f.moments(x, y).cpu().numpy(), (before * torch.tensor([0.25, 0.25, 1.0, 0.5], device=dev)).cpu().numpy()) < 1e-3
    # refusals come before any launch, on the device as on the CPU
    with pytest.raises(RuntimeError, match="length 1024 with fft_size 2048"):
        mr(x[:, :1024], y[:, :1024])
    with pytest.raises(RuntimeError, match="one shape"):
        mr(x, y.cpu())


@pytest.mark.parametrize("n_fft,hop,win,length", [(15, 4, 15, 8), (15, 4, 11, 8), (33, 5, 20, 100)])
def test_an_odd_fft_size_on_the_device(S, dev, n_fft, hop, win, length):
    """The frame count of torch.stft for an odd n_fft (one fewer where hop divides L), down to the shortest legal length."""
    x, y = R.pair("plain")
    x, y = x[:, :length].contiguous(), y[:, :length].contiguous()
    f = S.STFTLoss(n_fft, hop, win)
    got = f.magnitudes(x.to(dev))
    assert tuple(got.shape) == (x.shape[0], R.frames(length, n_fft, hop), n_fft // 2 + 1)
    assert rel_max(got.cpu().numpy(), R.magnitudes(x.numpy(), n_fft, hop, win)) < R.FP32_TOL
    m = f.moments(x.to(dev), y.to(dev))
    assert R.rel_each(m.cpu().numpy(), R.sums(x.numpy(), y.numpy(), n_fft, hop, win)) < R.FP32_TOL
    assert R.rel_each(m.cpu().numpy(), f.moments(x, y).numpy()) < R.FP32_TOL     # the CPU path counts the same frames
    for a, b in zip(f(x.to(dev), y.to(dev)), f(x, y)):
        assert R.rel(float(a), float(b)) < R.FP32_TOL


def test_release_scratch_frees_what_the_file_keeps(S, dev):
    x, y = (t.to(dev) for t in R.pair("short"))
    mr = S.MultiResolutionSTFTLoss()
    before = (mr(x, y), S.over_suppression_loss(x, y))
    kept = S.kept_tensors()
    assert kept and all(t.device == x.device for t in kept)
    S.release_scratch()
    assert S.kept_tensors() == []
    assert torch.equal(mr(x, y), before[0]) and torch.equal(S.over_suppression_loss(x, y), before[1])


# ------------------------------------------------------------------------------------------------
# inference_scored
# ------------------------------------------------------------------------------------------------
def _model(dev, name):
    import puresound_amd.nnet as PA
    model = cases.build(PA.NS, name).eval()
    model.load_state_dict(det_state_dict(model))
    return model.to(dev)


@pytest.mark.parametrize("name", ["ns_dpcrn_short", "tiny_free"])
def test_inference_scored_with_the_stft_ov_closure(S, dev, name):
    import puresound_amd.nnet as PA
    c = cases.CASES[name]
    model = _model(dev, name)
    noisy = (det_wave(c["seed"], c["B"], 4000) * 0.1).to(dev)
    want = model.inference(noisy)
    ref = (0.6 * want + 0.05 * det_wave(c["seed"] + 5, c["B"], want.shape[-1]).to(dev))[:, :-7]
    closure = R.stft_ov_closure(S)
    enh, score = model.inference_scored(noisy, ref, loss_func=closure)
    assert torch.equal(enh, want)
    aligned = torch.nn.functional.pad(ref, (7, 0))
    assert torch.equal(score, closure(want, aligned, None)) and float(score) > 0
    # against the same closure on CPU tensors (stock ATen): the device path within the fp32 class
    assert R.rel(float(score), float(closure(want.cpu(), aligned.cpu(), None))) < R.FP32_TOL
    mr = S.MultiResolutionSTFTLoss()
    assert torch.equal(model.inference_scored(noisy, ref, loss_func=mr)[1], mr(want, aligned))
    # routing only: an SDRLoss still goes through the decoder's moments and from_moments (the values of that path are the
    # existing SDRLoss tests' business)
    sdr = PA.SDRLoss.init_mode("sisnr", reduction=False)
    enh2, snr = model.inference_scored(noisy, ref, loss_func=sdr)
    wav, moments = model._inference(noisy, None, ref.float())
    assert torch.equal(enh2, want) and torch.equal(wav, want)
    assert torch.equal(snr, sdr.from_moments(moments, want.shape[-1], None))
    assert torch.equal(model.inference_scored(noisy, ref)[1], PA.SDRLoss.init_mode("sisnr").from_moments(moments, want.shape[-1]))
