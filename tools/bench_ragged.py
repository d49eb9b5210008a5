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
such a tree has no `lengths` argument and gets (b), (c) and the plain step only.  One JSON line per run."""
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
    for run in range(args.runs):
        ms = {k: round(timed(fn), 3) for k, fn in calls.items()}
        line = {"tree": os.path.relpath(tree, os.getcwd()), "run": run, "rows": n, "samples_valid": sum(lengths),
                "samples_padded": n * hi, "ms": ms}
        if has_lengths:
            line["speedup_ragged_over_one_by_one"] = round(ms["one_by_one"] / ms["ragged"], 2)
            line["equal_ragged_over_padded"] = round(ms["equal_ragged"] / ms["padded"], 3)
            line["valid_msamples_per_s_ragged"] = round(sum(lengths) / ms["ragged"] / 1e3, 1)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
