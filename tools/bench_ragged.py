"""Timing of ragged batches through SoTaskWrapModule.inference(noisy, lengths=...) (not the bench.py headline): the BASELINE
Conv-TasNet (cases "cfg2_full"), 32 rows, lengths spaced evenly over 1 - 4 s, fp32 arithmetic.

  (a) ragged    one inference(noisy, lengths=lengths) call,
  (b) one_by_one the 32 rows through inference(noisy[n:n+1, :lengths[n]]) one after the other: what a user who wants the
                 reference's result for every utterance runs without (a),
  (c) padded    the plain inference(noisy) call over the padded batch: its results are WRONG for the short rows (the global
                 norms and the depthwise taps see the padding); a time reference only,
and, separately, lengths = [64000] * 32 against the plain fp32 step (`equal`: the cost of the ragged path itself -- two more
reads of a hidden map per block for the statistics the GEMM epilogues otherwise leave behind).

Every figure is the median over --steps calls after --warmup, each call bracketed by device synchronisation, repeated --runs
times; the (b) loop is timed as a whole.  --tree DIR imports puresound_amd from another checkout (the parent commit, built):
such a tree has no `lengths` argument and gets (b), (c) and the plain step only.  One JSON line per run.

--scored times the evaluation loop instead, every row against a clean reference of its own length:
  scored_sisnr     inference_scored_ragged with an SI-SNR SDRLoss (reduction=False),
  scored_stft_ov   the same with MultiResolutionSTFTLoss() + over_suppression_loss through a closure that takes `lengths`,
  rows_sisnr / rows_stft_ov   what a tree without inference_scored_ragged can do: inference(noisy, lengths=...), then every row
                   sliced, aligned and scored on its own with the same loss,
  ragged           the plain inference(noisy, lengths=...) call; scored_sisnr - ragged is the cost of alignment + moments.
A --tree without inference_scored_ragged gets the rows_* loops and `ragged` only."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.join(HERE, ".."), help="checkout to import puresound_amd and the cases from")
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--seconds", type=float, nargs=2, default=(1.0, 4.0), help="shortest and longest utterance")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--scored", action="store_true", help="time the scored evaluation loop (see above)")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path[:0] = [tree, os.path.join(tree, "tests", "golden")]
    import cases
    import puresound_amd.nnet as PA
    from detweights import det_wave
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = cases.build(PA.NS, "cfg2_full").eval().to(dev)
    model.set_gemm_precision("fp32")
    has_lengths = hasattr(model, "output_lengths")

    n, rate = args.rows, 16000
    lo, hi = (int(s * rate) for s in args.seconds)
    lengths = [lo + (hi - lo) * i // max(n - 1, 1) for i in range(n)]
    noisy = (det_wave(1234, n, hi) * 0.1).to(dev)
    rows = [noisy[i:i + 1, :lengths[i]].contiguous() for i in range(n)]

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

    calls = {"one_by_one": lambda: [model.inference(r) for r in rows], "padded": lambda: model.inference(noisy)}
    if has_lengths:
        calls["ragged"] = lambda: model.inference(noisy, lengths=lengths)
        calls["equal_ragged"] = lambda: model.inference(noisy, lengths=[hi] * n)
    if args.scored:
        calls = scored_calls(PA, model, noisy, (det_wave(1235, n, hi) * 0.1).to(dev), lengths)
    for run in range(args.runs):
        ms = {k: round(timed(fn), 3) for k, fn in calls.items()}
        line = {"tree": os.path.relpath(tree, os.getcwd()), "run": run, "rows": n, "samples_valid": sum(lengths),
                "samples_padded": n * hi, "ms": ms}
        if args.scored:
            for kind in ("sisnr", "stft_ov"):
                if "scored_" + kind in ms:
                    line[f"speedup_scored_{kind}_over_rows"] = round(ms["rows_" + kind] / ms["scored_" + kind], 2)
            if "scored_sisnr" in ms:
                line["align_and_moments_ms"] = round(ms["scored_sisnr"] - ms["ragged"], 3)
        elif has_lengths:
            line["speedup_ragged_over_one_by_one"] = round(ms["one_by_one"] / ms["ragged"], 2)
            line["equal_ragged_over_padded"] = round(ms["equal_ragged"] / ms["padded"], 3)
            line["valid_msamples_per_s_ragged"] = round(sum(lengths) / ms["ragged"] / 1e3, 1)
        print(json.dumps(line), flush=True)


def scored_calls(PA, model, noisy, clean, lengths):
    """The calls --scored times, by name (the module's docstring)."""
    from puresound_amd import hip
    from puresound_amd.nnet.loss import stft_loss as S
    n = noisy.shape[0]
    out = model.output_lengths(lengths)
    sisnr = PA.SDRLoss.init_mode("sisnr", reduction=False)
    mr = S.MultiResolutionSTFTLoss()

    def rows_scored(score):
        enh = model.inference(noisy, lengths=lengths)
        return [score(enh[i:i + 1, :out[i]], hip.align_reference(clean[i:i + 1, :lengths[i]], out[i])) for i in range(n)]

    calls = {"ragged": lambda: model.inference(noisy, lengths=lengths),
             "rows_sisnr": lambda: rows_scored(sisnr),
             "rows_stft_ov": lambda: rows_scored(lambda e, r: mr(e, r) + S.over_suppression_loss(e, r))}
    if hasattr(model, "inference_scored_ragged"):
        def stft_ov(est, ref, unused, lengths=None):
            return mr(est, ref, lengths=lengths) + S.over_suppression_loss_ragged(est, ref, lengths=lengths)
        calls["scored_sisnr"] = lambda: model.inference_scored_ragged(noisy, clean, loss_func=sisnr, lengths=lengths)
        calls["scored_stft_ov"] = lambda: model.inference_scored_ragged(noisy, clean, loss_func=stft_ov, lengths=lengths)
    return calls


if __name__ == "__main__":
    main()
