"""puresound_amd.nnet.loss.stft_loss without a GPU: the float64 restatement (tests/stft_loss_ref.py) against the values the
reference recorded (tests/golden/loss_stft.npz), the module on CPU tensors against both, the reference's names, defaults and
state_dict keys, the refusals, the imports and the init_loss branches of egs/ns/model.py in a fresh process with compat/ on
the path, and inference_scored with the recipe's `stft_ov` closure.

The bounds are stft_loss_ref's, none of them new."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases
import stft_loss_ref as R
from detweights import det_state_dict, det_wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_TOL, FP32_TOL = R.GOLDEN_TOL, R.FP32_TOL


@pytest.fixture(scope="module")
def S():
    from puresound_amd.nnet.loss import stft_loss
    return stft_loss


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "loss_stft.npz")))


@pytest.mark.parametrize("n_fft,hop,win,length", [(15, 4, 15, 8),      # odd n_fft, hop divides L: one frame fewer than 1 + L // hop,
                                                   (15, 4, 11, 8),      # L = n_fft // 2 + 1, the shortest legal length
                                                   (15, 4, 15, 9), (33, 5, 20, 100), (16, 4, 16, 12)])
def test_frame_count_of_an_odd_fft_size(S, n_fft, hop, win, length):
    """torch.stft makes 1 + (L + 2 (n_fft // 2) - n_fft) // hop frames: the restatement, the CPU path and hip.stft_frames agree"""
    from puresound_amd import hip
    x, y = R.pair("plain")
    x, y = x[:, :length].contiguous(), y[:, :length].contiguous()
    t = torch.stft(x, n_fft, hop, win, torch.hann_window(win), return_complex=True).shape[-1]
    assert t == R.frames(length, n_fft, hop) == hip.stft_frames(length, n_fft, hop)
    assert (t == 1 + length // hop) == (n_fft % 2 == 0 or length % hop != 0)
    f = S.STFTLoss(n_fft, hop, win)
    assert tuple(f.magnitudes(x).shape) == (x.shape[0], t, n_fft // 2 + 1)
    assert R.rel(f.magnitudes(x).numpy(), R.magnitudes(x.numpy(), n_fft, hop, win)) < FP32_TOL
    assert R.rel_each(f.moments(x, y).numpy(), R.sums(x.numpy(), y.numpy(), n_fft, hop, win)) < FP32_TOL


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_matches_the_reference_recorded_values(golden, name):
    want = R.scores(name)
    for i in range(len(R.RESOLUTIONS)):
        assert R.rel(want["sc"][i], golden[f"{name}.sc"][i]) < GOLDEN_TOL
        assert R.rel(want["mag"][i], golden[f"{name}.mag"][i]) < GOLDEN_TOL
    assert R.rel(want["mr"], golden[f"{name}.mr"]) < GOLDEN_TOL
    for i, p in enumerate(R.OV_POWERS):
        assert R.rel(want["ov"][p], golden[f"{name}.ov"][i]) < GOLDEN_TOL


def test_restatement_magnitudes_match_the_recorded_ones(golden):
    x, y = R.pair("short")
    assert golden["short.x_mag"].shape == (1, 1 + 1025 // R.MAG_RESOLUTION[1], R.MAG_RESOLUTION[0] // 2 + 1)
    assert R.rel(R.magnitudes(x.numpy(), *R.MAG_RESOLUTION), golden["short.x_mag"]) < GOLDEN_TOL
    assert R.rel(R.magnitudes(y.numpy(), *R.MAG_RESOLUTION), golden["short.y_mag"]) < GOLDEN_TOL


@pytest.mark.parametrize("name", sorted(R.CASES) + ["long"])
def test_module_on_cpu_tensors(S, golden, name):
    R.check_scores(S, name, golden)


def test_stft_on_cpu_tensors(S, golden):
    x, _ = R.pair("short")
    n_fft, hop, win = R.MAG_RESOLUTION
    got = S.stft(x, n_fft, hop, win, torch.hann_window(win))
    assert tuple(got.shape) == golden["short.x_mag"].shape
    assert R.rel(got.numpy(), golden["short.x_mag"]) < GOLDEN_TOL
    assert R.rel(got.numpy(), R.magnitudes(x.numpy(), n_fft, hop, win)) < FP32_TOL
    assert torch.equal(S.STFTLoss(n_fft, hop, win).magnitudes(x), got)
    # the two small loss modules on magnitudes, as the reference composes them
    y_mag = torch.tensor(golden["short.y_mag"])
    s = R.sums_of(got.numpy(), golden["short.y_mag"])
    assert R.rel(float(S.SpectralConvergengeLoss()(got, y_mag)), np.sqrt(s[0, 0] / s[0, 1])) < FP32_TOL
    assert R.rel(float(S.LogSTFTMagnitudeLoss()(got, y_mag)), s[0, 2] / got[0].numel()) < FP32_TOL


def test_fourier_basis_is_the_windowed_dft(S):
    """rows m and bins + m against exp(2 pi i m (k + off) / n_fft) in float64, where win < n_fft and the offset is odd"""
    n_fft, win = 64, 38
    w = torch.hann_window(win)
    b = S.fourier_basis(w, n_fft).double().numpy()
    off, bins = (n_fft - win) // 2, n_fft // 2 + 1
    assert b.shape == (2 * bins, win) and off == 13
    ang = 2 * np.pi * np.outer(np.arange(bins), np.arange(win) + off) / n_fft
    assert np.abs(b[:bins] - np.cos(ang) * w.double().numpy()).max() < 1e-7
    assert np.abs(b[bins:] - np.sin(ang) * w.double().numpy()).max() < 1e-7


def test_names_defaults_and_state_dict_keys(S):
    f = S.STFTLoss()
    assert (f.fft_size, f.shift_size, f.win_length) == (1024, 120, 600)
    assert list(f.state_dict()) == ["window"] and torch.equal(f.window, torch.hann_window(600))
    assert isinstance(f.spectral_convergenge_loss, S.SpectralConvergengeLoss)
    assert isinstance(f.log_stft_magnitude_loss, S.LogSTFTMagnitudeLoss)
    g = S.STFTLoss(256, 64, 200, "hamming_window")
    assert (g.fft_size, g.shift_size, g.win_length) == (256, 64, 200) and torch.equal(g.window, torch.hamming_window(200))
    mr = S.MultiResolutionSTFTLoss()
    assert isinstance(mr.stft_losses, torch.nn.ModuleList) and (mr.factor_sc, mr.factor_mag) == (0.1, 0.1)
    assert list(mr.state_dict()) == ["stft_losses.0.window", "stft_losses.1.window", "stft_losses.2.window"]
    assert [tuple(v.shape) for v in mr.state_dict().values()] == [(600,), (1200,), (240,)]
    two = S.MultiResolutionSTFTLoss([64, 128], [16, 32], [40, 128], "hann_window", 0.5, 0.25)
    assert [(f.fft_size, f.shift_size, f.win_length) for f in two.stft_losses] == [(64, 16, 40), (128, 32, 128)]
    assert (two.factor_sc, two.factor_mag) == (0.5, 0.25)
    import inspect
    ov = inspect.signature(S.over_suppression_loss).parameters
    assert list(ov) == ["enh", "ref", "p", "fft_size", "hop_size", "win_length"]
    assert [ov[k].default for k in list(ov)[2:]] == [0.5, 512, 128, 512]
    assert list(inspect.signature(S.stft).parameters) == ["x", "fft_size", "hop_size", "win_length", "window"]
    import puresound_amd.nnet as PA
    assert PA.MultiResolutionSTFTLoss is S.MultiResolutionSTFTLoss and PA.over_suppression_loss is S.over_suppression_loss


def test_loss_of_a_signal_against_itself_and_of_silence_is_zero(S):
    x, _ = R.pair("plain")
    zero = torch.zeros(2, 1100)
    for a in (x, zero):
        for f in S.MultiResolutionSTFTLoss().stft_losses:
            sc, mag = f(a, a)
            assert float(sc) == 0.0 and float(mag) == 0.0
        assert float(S.MultiResolutionSTFTLoss()(a, a)) == 0.0
        assert float(S.over_suppression_loss(a, a)) == 0.0


def test_refusals(S):
    f = S.STFTLoss()
    x = torch.zeros(2, 4000)
    with pytest.raises(RuntimeError, match="batch, length"):
        f(x[0], x[0])
    with pytest.raises(RuntimeError, match="batch, length"):
        S.MultiResolutionSTFTLoss()(x[None], x[None])
    with pytest.raises(RuntimeError, match="one shape"):
        f(x, x[:, :-1])
    with pytest.raises(RuntimeError, match="one shape"):
        S.over_suppression_loss(x, x[:1])
    with pytest.raises(RuntimeError, match=r"length 512 with fft_size 1024"):
        f(x[:, :512], x[:, :512])
    f(x[:, :513], x[:, :513])
    with pytest.raises(RuntimeError, match=r"length 1024 with fft_size 2048"):
        S.MultiResolutionSTFTLoss()(x[:, :1024], x[:, :1024])
    with pytest.raises(RuntimeError, match=r"length 256 with fft_size 512"):
        S.over_suppression_loss(x[:, :256], x[:, :256])
    with pytest.raises(RuntimeError, match="win_length 600 exceeds fft_size 512"):
        S.STFTLoss(512, 120, 600)(x, x)
    with pytest.raises(RuntimeError, match="win_length 600 exceeds fft_size 512"):
        S.stft(x, 512, 120, 600, torch.hann_window(600))
    with pytest.raises(RuntimeError, match="win_length 64 exceeds fft_size 32"):
        S.over_suppression_loss(x, x, fft_size=32, win_length=64)
    with pytest.raises(RuntimeError, match="must hold win_length"):
        S.stft(x, 512, 120, 400, torch.hann_window(300))


RECIPE = r'''
import os
import puresound
assert os.path.basename(os.path.dirname(os.path.dirname(puresound.__file__))) == "compat", puresound.__file__
import torch
import torch.nn as nn
# the six puresound.* import lines of egs/ns/model.py
from puresound.nnet.base_nn import SoTaskWrapModule
from puresound.nnet.dparn import DPARN
from puresound.nnet.dpcrn import DPCRN
from puresound.nnet.lobe.encoder import ConvEncDec
from puresound.nnet.loss.sdr import SDRLoss
from puresound.nnet.loss.stft_loss import MultiResolutionSTFTLoss, over_suppression_loss
import puresound_amd.nnet.loss.stft_loss as mirror
assert MultiResolutionSTFTLoss is mirror.MultiResolutionSTFTLoss and over_suppression_loss is mirror.over_suppression_loss


def multi_resolution(with_over_suppression):
    mr = MultiResolutionSTFTLoss()
    if with_over_suppression:
        return lambda est, clean, unused: mr(est, clean) + over_suppression_loss(est, clean)
    return lambda est, clean, unused: mr(est, clean)


# what the recipe's `sig_loss` names stand for, each a callable of (estimate, reference, labels) as the wrapper's forward calls it
BUILD = {"sisnr": lambda: SDRLoss.init_mode("sisnr", threshold=None),
         "stft": lambda: multi_resolution(False),
         "stft_ov": lambda: multi_resolution(True)}

g = torch.Generator().manual_seed(3)
enh = torch.rand(2, 1600, generator=g) - 0.5
ref = 0.7 * enh + 0.2 * (torch.rand(2, 1600, generator=g) - 0.5)
values = {}
for name, build in BUILD.items():
    out = build()(enh, ref, None)
    assert torch.is_tensor(out) and out.dim() == 0 and bool(torch.isfinite(out)), (name, out)
    values[name] = float(out)
assert values["sisnr"] < 0 < values["stft"] < values["stft_ov"], values
print("RECIPE-OK", values)
'''


def test_the_imports_and_losses_of_the_ns_recipe_in_a_fresh_process(tmp_path):
    """egs/ns/model.py's imports with compat/ first on the path (the README's "imports swapped"), and the three losses its
    `sig_loss` setting can name, built from those imports and called on CPU tensors with the wrapper's three arguments.  The
    reference checkout is not on the path and is not read."""
    script = tmp_path / "recipe.py"
    script.write_text(RECIPE)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "compat"), ROOT]), PYTHONDONTWRITEBYTECODE="1")
    done = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, cwd=str(tmp_path))
    assert done.returncode == 0, done.stdout + done.stderr
    assert "RECIPE-OK" in done.stdout


@pytest.mark.parametrize("name", ["tiny_stft", "tiny_free"])
def test_inference_scored_with_the_stft_ov_closure_on_cpu_tensors(S, name):
    import puresound_amd.nnet as PA
    c = cases.CASES[name]
    model = cases.build(PA.NS, name).eval()
    model.load_state_dict(det_state_dict(model))
    noisy = det_wave(c["seed"], c["B"], 1500)
    want = model.inference(noisy)
    ref = (0.6 * want + 0.05 * det_wave(c["seed"] + 5, c["B"], want.shape[-1]))[:, :-7]
    closure = R.stft_ov_closure(S)
    enh, score = model.inference_scored(noisy, ref, loss_func=closure)
    assert torch.equal(enh, want)
    aligned = torch.nn.functional.pad(ref, (7, 0))
    assert torch.equal(score, closure(want, aligned, None)) and float(score) > 0
    # the two module classes given directly take two arguments; loss_func_wav is the default
    mr = S.MultiResolutionSTFTLoss()
    assert torch.equal(model.inference_scored(noisy, ref, loss_func=mr)[1], mr(want, aligned))
    one = S.STFTLoss(256, 64, 256)
    got = model.inference_scored(noisy, ref, loss_func=one)[1]
    assert isinstance(got, tuple) and all(torch.equal(a, b) for a, b in zip(got, one(want, aligned)))
    model.loss_func_wav = closure
    assert torch.equal(model.inference_scored(noisy, ref)[1], score)
    with pytest.raises(NotImplementedError, match="lengths"):
        model.inference_scored(noisy, ref, loss_func=closure, lengths=[1500] * c["B"])
    with pytest.raises(NotImplementedError, match="source-aggregated"):
        model.inference_scored(noisy, ref, loss_func=PA.SDRLoss.init_mode("sasdr"))
