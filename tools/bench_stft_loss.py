"""Timing of the recipes' `stft_ov` score (not the bench.py headline): MultiResolutionSTFTLoss()(enh, ref) +
over_suppression_loss(enh, ref) on --rows utterances of --seconds at 16 kHz.

  (1) hip       the score on the HIP path (puresound_amd.nnet.loss.stft_loss), and once per run its split per kernel family
                through ps_profile_read: the exact-fp32 GEMM ("conv1x1") against "frame_reflect" and "spec_pair_moments",
  (2) torch     the same formula in stock torch ops on the same device (torch.stft(..., return_complex=True) and
                elementwise ops); if that does not run on the device the line says why,
  (3) scored    inference_scored with that score against plain inference on the `ns_dpcrn_short` model at that batch.

Every figure is the median over --steps calls after --warmup, each call bracketed by device synchronisation, repeated --runs
times.  One JSON line per run."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
KERNELS = ("frame_reflect", "conv1x1", "spec_pair_moments")


def torch_score(enh, ref, windows):
    """The recipe's formula in stock torch ops on the tensors' device, reductions over the whole batch."""
    def mag(x, n_fft, hop, win):
        spec = torch.stft(x, n_fft, hop, win, windows[win], return_complex=True)
        return torch.sqrt(torch.clamp(spec.real ** 2 + spec.imag ** 2, min=1e-7)).transpose(2, 1)

    sc = mg = 0.0
    for n_fft, hop, win in RESOLUTIONS:
        x, y = mag(enh, n_fft, hop, win), mag(ref, n_fft, hop, win)
        sc = sc + torch.norm(y - x, p="fro") / torch.norm(y, p="fro")
        mg = mg + torch.nn.functional.l1_loss(torch.log(y), torch.log(x))
    x, y = mag(enh, 512, 128, 512), mag(ref, 512, 128, 512)
    ov = torch.mean(torch.relu(y.pow(0.5) - x.pow(0.5)).pow(2))
    return 0.1 * sc / len(RESOLUTIONS) + 0.1 * mg / len(RESOLUTIONS) + ov


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-model", action="store_true", help="skip (3)")
    args = ap.parse_args()
    tree = os.path.abspath(os.path.join(HERE, ".."))
    sys.path[:0] = [tree, os.path.join(tree, "tests", "golden")]
    import cases
    import puresound_amd.nnet as PA
    from detweights import det_state_dict, det_wave
    from puresound_amd import _abi
    from puresound_amd.nnet.loss.stft_loss import MultiResolutionSTFTLoss, over_suppression_loss
    if not torch.cuda.is_available():
        raise SystemExit("bench_stft_loss.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    n, length = args.rows, int(args.seconds * 16000)
    enh = (det_wave(1234, n, length) * 0.3).to(dev)
    ref = 0.7 * enh + 0.2 * (det_wave(1235, n, length) * 0.3).to(dev)
    loss = MultiResolutionSTFTLoss()

    def score(a, b, dummy=None):
        return loss(a, b) + over_suppression_loss(a, b)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ms = []
        for _ in range(args.steps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms)

    def kernel_split():
        lib = _abi.lib()
        lib.ps_profile_enable(1)
        score(enh, ref)
        torch.cuda.synchronize(dev)
        out = {}
        for k in KERNELS:
            ms, count = ctypes.c_double(0.0), ctypes.c_int(0)
            _abi.check(lib.ps_profile_read(k.encode(), ctypes.byref(ms), ctypes.byref(count)), "ps_profile_read")
            out[k] = {"ms": round(ms.value, 4), "launches": count.value}
        lib.ps_profile_enable(0)
        return out

    windows = {win: torch.hann_window(win, device=dev) for win in (600, 1200, 240, 512)}
    torch_note = None
    try:
        want = float(torch_score(enh, ref, windows))
        got = float(score(enh, ref))
        torch_note = {"value_torch": want, "value_hip": got, "rel_diff": abs(got - want) / abs(want)}
    except Exception as e:   # recorded, not hidden: the comparison is part of the result
        torch_note = {"error": f"{type(e).__name__}: {e}"[:300]}

    model = None
    if not args.no_model:
        model = cases.build(PA.NS, "ns_dpcrn_short").eval()
        model.load_state_dict(det_state_dict(model))
        model.to(dev)
        noisy = (det_wave(1236, n, length) * 0.1).to(dev)

    for run in range(args.runs):
        ms = {"hip": round(timed(lambda: score(enh, ref)), 3)}
        if "error" not in torch_note:
            ms["torch"] = round(timed(lambda: torch_score(enh, ref, windows)), 3)
        if model is not None:
            ms["inference"] = round(timed(lambda: model.inference(noisy)), 3)
            ms["inference_scored"] = round(timed(lambda: model.inference_scored(noisy, ref, loss_func=score)), 3)
        line = {"run": run, "rows": n, "samples": length, "ms": ms, "kernels": kernel_split(), "torch": torch_note}
        if "torch" in ms:
            line["torch_over_hip"] = round(ms["torch"] / ms["hip"], 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
