"""One NaN / infinity in a live input sample, on the GPU: per wrapper case, scenario and arithmetic the reference's NaN count
(tests/golden/nonfinite_masks.json), the HIP path's, and the largest error of the HIP path's finite elements against the
fp64 oracle, relative to the oracle's largest finite element (GPU box).  tests/test_nonfinite_gpu.py asserts on the same
quantities; this prints them.   python tools/nonfinite_report.py [out.txt] [case ...]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import nonfinite_cases as NF  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    names = sys.argv[2:] or NF.CASES
    head = f"{'case':26s} {'scenario':17s} {'arith':8s} {'ref NaN':>7s} {'HIP NaN':>7s} {'HIP inf':>7s} {'missed':>6s} " \
           f"{'finite err':>10s} {'clean rows':>10s}"
    print(head, file=out, flush=True)
    for name in names:
        for prec in NF.precisions(name):
            model = NF.hip_model(name, dev)  # (a fresh one: "default" is what the constructors leave)
            if prec is not None:
                model.set_gemm_precision(prec)
            clean = NF.hip_out(model, name, None, dev)
            for sc in NF.scenarios(name):
                nan, inf = NF.golden_masks(name, sc)
                got = NF.hip_out(model, name, sc, dev)
                want = NF.oracle_out(name, sc)
                missed = int((np.isfinite(got) & ~np.isfinite(want)).sum())  # finite where the reference has no number
                err, den = NF.finite_error(name, got, want)
                rows = ~(nan | inf).any(axis=1)
                same = "-" if not rows.any() else ("equal" if np.array_equal(got[rows], clean[rows]) else "DIFFER")
                print(f"{name:26s} {sc:17s} {prec or 'default':8s} {int(nan.sum()):7d} {int(np.isnan(got).sum()):7d} "
                      f"{int(np.isinf(got).sum()):7d} {missed:6d} {err / den:10.2e} {same:>10s}", file=out, flush=True)
            del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
