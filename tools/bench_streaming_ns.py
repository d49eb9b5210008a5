"""Per-hop latency of hop-by-hop streaming (puresound_amd/streaming/spectral.py) for the egs/ns presets ns_dpcrn_v0_causal and
ns_dparn_v0_causal (tests/golden/cases.py, deterministic weights), against the hop's real-time budget (hop / 16 kHz = 8 ms).

For each model and B: step() and step_chunk() with 4 and 16 hops, graph replays, a device synchronise after every call;
p50 / p90 / p99 of the per-hop wall time (a chunk's time / its hops) over --replays calls after --warmup.  Then the largest B
(doubling from the largest measured one) whose step() p99 stays under the budget, and offline `inference` on the same 10 s
signals for context.  Prints a plain-text report (profiles/streaming_ns.txt holds one run)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests", "golden"))
import cases  # noqa: E402
from detweights import det_state_dict, det_wave  # noqa: E402
import puresound_amd.nnet as PA  # noqa: E402
from puresound_amd.streaming import StreamingSeparator  # noqa: E402

PRESETS = {"ns_dpcrn_v0_causal": "ns_dpcrn_short", "ns_dparn_v0_causal": "ns_dparn_short"}
SR, SECONDS = 16000, 10


def percentiles(ms):
    a = np.asarray(ms)
    return {p: float(np.percentile(a, p)) for p in (50, 90, 99)}


def time_mode(sep, x, streams, chunk_hops, replays, warmup):
    """Per-hop ms of `replays` calls (step() when chunk_hops == 1, else step_chunk of chunk_hops hops)."""
    hop = sep.hop_length
    sep.init_streams(streams=streams, use_graph=True)
    total_hops = x.shape[1] // hop
    pos = 0

    def call():
        nonlocal pos
        if pos + chunk_hops > total_hops:
            pos = 0
        piece = x[:, pos * hop:(pos + chunk_hops) * hop]
        pos += chunk_hops
        return sep.step(piece) if chunk_hops == 1 else sep.step_chunk(piece)

    for _ in range(sep.prime_hops):
        sep.step(x[:, pos * hop:(pos + 1) * hop])
        pos += 1
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(replays):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / chunk_hops)
    return percentiles(ms)


def offline_ms(model, x, reps=5):
    model.inference(x)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        model.inference(x)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batches", default="1,16,64,256")
    ap.add_argument("--chunks", default="1,4,16", help="hops per call (1 = step())")
    ap.add_argument("--replays", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--max-search", type=int, default=4096, help="largest B the real-time search tries")
    ap.add_argument("--models", default=",".join(PRESETS))
    ap.add_argument("--tree", default="", help="source revision to print in the header")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    budget = 1e3 * 128 / SR
    batches = [int(b) for b in args.batches.split(",")]
    chunks = [int(c) for c in args.chunks.split(",")]
    print(f"# tools/bench_streaming_ns.py  tree {args.tree or '(not given)'}  device {torch.cuda.get_device_name(dev)}")
    print(f"# per-hop wall ms (a chunk call / its hops), graph replays, device sync per call; {args.replays} calls after "
          f"{args.warmup} warm-up; real-time budget {budget:.1f} ms per 128-sample hop at {SR} Hz")
    for label in args.models.split(","):
        name = PRESETS[label]
        model = cases.build(PA.NS, name).eval()
        model.load_state_dict(det_state_dict(model))
        model.to(dev)
        sep = StreamingSeparator(model)
        print(f"\n## {label}  (n_fft {sep.n_fft}, hop {sep.hop_length}, latency {sep.latency_samples} samples)")
        print(f"{'B':>6} {'hops/call':>9} {'p50':>8} {'p90':>8} {'p99':>8}  real-time")
        xs = {}
        best = 0
        for b in batches:
            xs[b] = det_wave(100 + b, b, SR * SECONDS).to(dev)
            for k in chunks:
                p = time_mode(sep, xs[b], b, k, args.replays, args.warmup)
                ok = p[99] < budget
                if k == 1 and ok:
                    best = max(best, b)
                print(f"{b:>6} {k:>9} {p[50]:>8.3f} {p[90]:>8.3f} {p[99]:>8.3f}  {'yes' if ok else 'no'}", flush=True)
        # the largest real-time B for step(): double past the largest measured B while p99 stays under the budget
        b = max(batches)
        last_ok = best if best == max(batches) else None
        while last_ok is not None and 2 * b <= args.max_search:
            b *= 2
            xb = det_wave(100 + b, b, SR * SECONDS).to(dev)
            p = time_mode(sep, xb, b, 1, args.replays, args.warmup)
            ok = p[99] < budget
            print(f"{b:>6} {1:>9} {p[50]:>8.3f} {p[90]:>8.3f} {p[99]:>8.3f}  {'yes' if ok else 'no'}  (search)", flush=True)
            del xb
            if not ok:
                break
            last_ok = b
        if last_ok is not None:
            best = last_ok
        print(f"largest real-time B for step() (p99 < {budget:.1f} ms): {best}"
              + (f" (search capped at {args.max_search})" if best >= args.max_search else ""))
        sep = None
        torch.cuda.empty_cache()
        print(f"offline inference of the same {SECONDS} s signals (median of 5):")
        for b in batches:
            for prec in ("fp16x2", "fp32"):
                model.set_gemm_precision(prec)
                ms = offline_ms(model, xs[b])
                print(f"  B {b:>4} {prec:>6}: {ms:9.2f} ms  ({b * SECONDS * 1e3 / ms:8.1f} x real time in total)", flush=True)
            model.set_gemm_precision("fp16x2")
        xs = None
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
