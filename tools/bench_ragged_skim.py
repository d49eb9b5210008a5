"""Timing of ragged batches through the SkiM speaker extractors (not the bench.py headline): tse_skim_v0, tse_skim_v0_causal,
tse_skim_v1_causal and tse_skim_v0_causal_vad at preset size (the *_short cases of tests/golden/cases.py), 32 rows, mixtures
and enrolments spaced evenly over 1 - 4 s.

  (a) ragged        one inference(noisy, enroll, lengths=..., enroll_lengths=...) call (exact fp32 products whatever
                    gemm_precision says),
  (b) one_by_one    the 32 rows through inference(noisy[n:n+1, :lengths[n]], enroll[n:n+1, :enroll_lengths[n]]) one after the
                    other in fp32: what a user who wants every utterance's own result runs without (a),
  (c) padded_fp32 / padded_fp16x2   the plain inference(noisy, enroll) call over the padded batch in either arithmetic: its
                    results are WRONG for the short rows (the Mem-LSTMs and the speaker net see the padding, the causal
                    presets hand states from row to row); time references only.

Every figure is the median over --steps calls after --warmup, each call bracketed by device synchronisation, repeated --runs
times; the (b) loop is timed as a whole.  --tree DIR imports puresound_amd from another checkout (the parent commit, built):
a tree that refuses these models with lengths gets (b) and (c) only.  One JSON line per model and run."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = {"tse_skim_v0": "tse_skim_v0_short", "tse_skim_v0_causal": "tse_skim_causal_short",
          "tse_skim_v1_causal": "tse_skim_v1_short", "tse_skim_v0_causal_vad": "tse_skim_vad_short"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.join(HERE, ".."), help="checkout to import puresound_amd and the cases from")
    ap.add_argument("--models", nargs="+", default=list(MODELS), choices=list(MODELS))
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--seconds", type=float, nargs=2, default=(1.0, 4.0), help="shortest and longest utterance / enrolment")
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
        raise SystemExit("bench_ragged_skim.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")

    n, rate = args.rows, 16000
    lo, hi = (int(s * rate) for s in args.seconds)
    lengths = [lo + (hi - lo) * i // max(n - 1, 1) for i in range(n)]
    e_lengths = lengths[::-1]          # (the longest mixture with the shortest enrolment)
    noisy = (det_wave(1234, n, hi) * 0.05).to(dev)
    enroll = (det_wave(1235, n, hi) * 0.05).to(dev)
    rows = [(noisy[i:i + 1, :lengths[i]].contiguous(), enroll[i:i + 1, :e_lengths[i]].contiguous()) for i in range(n)]

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

    for name in args.models:
        torch.manual_seed(0)
        model = cases.build(PA.NS, MODELS[name]).eval().to(dev)
        try:
            model.inference(noisy[:2, :lo], enroll[:2, :lo], lengths=[lo, lo], enroll_lengths=[lo, lo])
            has_ragged = True
        except (NotImplementedError, TypeError):
            has_ragged = False

        def in_precision(precision, fn):
            def call():
                model.set_gemm_precision(precision)
                return fn()
            return call

        calls = {"one_by_one": in_precision("fp32", lambda: [model.inference(x, e) for x, e in rows]),
                 "padded_fp32": in_precision("fp32", lambda: model.inference(noisy, enroll)),
                 "padded_fp16x2": in_precision("fp16x2", lambda: model.inference(noisy, enroll))}
        if has_ragged:
            calls["ragged"] = in_precision("fp16x2", lambda: model.inference(noisy, enroll, lengths=lengths,
                                                                             enroll_lengths=e_lengths))
        for run in range(args.runs):
            ms = {k: round(timed(fn), 3) for k, fn in calls.items()}
            line = {"tree": os.path.relpath(tree, os.getcwd()), "model": name, "run": run, "rows": n,
                    "samples_valid": sum(lengths), "samples_padded": n * hi, "ms": ms}
            if has_ragged:
                line["speedup_ragged_over_one_by_one"] = round(ms["one_by_one"] / ms["ragged"], 2)
                line["ragged_over_padded_fp32"] = round(ms["ragged"] / ms["padded_fp32"], 3)
                line["ragged_over_padded_fp16x2"] = round(ms["ragged"] / ms["padded_fp16x2"], 3)
            print(json.dumps(line), flush=True)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
