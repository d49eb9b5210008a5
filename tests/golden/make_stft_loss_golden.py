"""Generate tests/golden/loss_stft.npz from the REAL reference's loss/stft_loss.py (mcw519/PureSound, /root/reference).

Run in the build container only (the reference does not travel to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_stft_loss_golden.py

The reference calls torch.stft without return_complex, which the installed torch refuses.  Inside this generator only,
torch.stft is wrapped so that such a call returns torch.view_as_real(torch.stft(..., return_complex=True)): what the
reference's torch returned.  The inputs are formula-generated (tests/stft_loss_ref.pair) and not stored; the fixture
holds the reference's values only: per case and resolution (sc, mag), the multi-resolution value, over_suppression_loss at
two powers, and the magnitudes of case "short" at one small resolution.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import stft_loss_ref as R  # noqa: E402

_stft = torch.stft


def _stft_as_real(*args, **kwargs):
    if kwargs.get("return_complex") is None:
        kwargs["return_complex"] = True
        return torch.view_as_real(_stft(*args, **kwargs))
    return _stft(*args, **kwargs)


def _reference():
    # (the file alone: it imports torch only, the package around it imports torchaudio)
    spec = importlib.util.spec_from_file_location(
        "reference_stft_loss", os.path.join("/root/reference", "puresound", "nnet", "loss", "stft_loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    torch.stft = _stft_as_real
    ref = _reference()
    out = {}
    with torch.no_grad():
        mr = ref.MultiResolutionSTFTLoss()
        assert [(f.fft_size, f.shift_size, f.win_length) for f in mr.stft_losses] == list(R.RESOLUTIONS)
        for name in R.CASES:
            x, y = R.pair(name)
            per = [f(x, y) for f in mr.stft_losses]
            out[f"{name}.sc"] = np.array([float(sc) for sc, _ in per], dtype=np.float32)
            out[f"{name}.mag"] = np.array([float(mag) for _, mag in per], dtype=np.float32)
            out[f"{name}.mr"] = np.float32(float(mr(x, y)))
            out[f"{name}.ov"] = np.array([float(ref.over_suppression_loss(x, y, p=p)) for p in R.OV_POWERS], dtype=np.float32)
        x, y = R.pair("short")
        n_fft, hop, win = R.MAG_RESOLUTION
        out["short.x_mag"] = ref.stft(x, n_fft, hop, win, torch.hann_window(win)).contiguous().numpy()
        out["short.y_mag"] = ref.stft(y, n_fft, hop, win, torch.hann_window(win)).contiguous().numpy()
    path = os.path.join(HERE, "loss_stft.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
