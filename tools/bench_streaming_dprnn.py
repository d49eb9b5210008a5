"""Per-call latency of hop-by-hop streaming (puresound_amd/streaming/dprnn.py) for the causal DPRNN speaker extractor
veve_dprnn_v0_causal (tests/golden/cases.py "cfg4_tse_short", deterministic weights), against the call's real-time budget
(the audio it carries: 1 ms per 16-sample hop at 16 kHz).

For each B: step() (one hop per call) and step_chunk() of --chunk hops, graph replays, a device synchronise after every call;
p50 / p90 / p99 of the per-call wall time over --replays calls after --warmup.  Prints a plain-text report
(profiles/streaming_dprnn.txt holds one run).  --slots: the same calls on a slot session of capacity B (init_slots), once
with every slot opened with its own 1 s enrolment and once with the first quarter of the slots open (the other columns idle:
whole tiles of 16 columns are dead), none ended.  --profile-only B,K: a short run of K-hop chunks at B streams and nothing
else, for rocprofv3."""
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
from puresound_amd.streaming import StreamingDPRNN  # noqa: E402

SR, SECONDS = 16000, 2


def time_mode(s, b, chunk_hops, replays, warmup, dev, open_slots=None):
    """Per-call ms of `replays` calls (step() when chunk_hops == 1, else step_chunk of chunk_hops hops).  open_slots: a slot
    session of capacity b with slots 0 .. open_slots - 1 open (None: a block session of b streams)."""
    x = det_wave(100 + b, b, SR * SECONDS).to(dev)
    enroll = det_wave(200 + b, b, SR).to(dev)
    if open_slots is None:
        s.init_streams(streams=b, enroll=enroll, use_graph=True)
    else:
        s.init_slots(b, use_graph=True)
        for i in range(open_slots):
            s.open(i, enroll[i])
    hop = s.hop_length
    total = x.shape[1] // hop
    pos = 0

    def call():
        nonlocal pos
        if pos + chunk_hops > total:
            pos = s.prime_hops
        piece = x[:, pos * hop:(pos + chunk_hops) * hop]
        pos += chunk_hops
        return s.step(piece) if chunk_hops == 1 else s.step_chunk(piece)

    for _ in range(s.prime_hops if open_slots is None else 0):     # (a slot session has no priming phase)
        s.step(x[:, pos * hop:(pos + 1) * hop])
        pos += 1
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(replays):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    a = np.asarray(ms)
    return {p: float(np.percentile(a, p)) for p in (50, 90, 99)}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batches", default="1,16,64,256,1024")
    ap.add_argument("--chunk", type=int, default=8, help="hops per step_chunk call")
    ap.add_argument("--replays", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--slots", action="store_true", help="slot sessions of capacity B: every slot open, then a quarter")
    ap.add_argument("--profile-only", default="", help="B,K: 200 calls of K-hop chunks at B streams (--slots: B open slots), no report")
    ap.add_argument("--tree", default="", help="source revision to print in the header")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = cases.build(PA.NS, "cfg4_tse_short").eval()
    model.load_state_dict(det_state_dict(model))
    model.to(dev)
    s = StreamingDPRNN(model)
    if args.profile_only:
        b, k = (int(v) for v in args.profile_only.split(","))
        time_mode(s, b, k, 200, 20, dev, b if args.slots else None)
        return
    hop_ms = 1e3 * s.hop_length / SR
    print(f"# tools/bench_streaming_dprnn.py  tree {args.tree or '(not given)'}  device {torch.cuda.get_device_name(dev)}")
    print(f"# veve_dprnn_v0_causal (win {s.win_length}, hop {s.hop_length}, latency {s.latency_samples} samples); "
          f"per-call wall ms, graph replays, device sync per call; {args.replays} calls after {args.warmup} warm-up; "
          f"real-time budget {hop_ms:.1f} ms per hop")
    batches = [int(v) for v in args.batches.split(",")]
    # (what the header says, how many slots of a capacity-B session are open); a block session: None
    modes = [("block session (init_streams)", lambda b: None)]
    if args.slots:
        modes = [("slot session (init_slots), every slot open", lambda b: b),
                 ("slot session (init_slots), the first quarter of the slots open", lambda b: max(1, b // 4))]
    for title, opened in modes:
        print(f"# {title}")
        print(f"{'B':>6} {'hops/call':>9} {'budget':>7} {'p50':>8} {'p90':>8} {'p99':>8}  real-time")
        for k in (1, args.chunk):
            budget = hop_ms * k
            best = 0
            for b in batches:
                p = time_mode(s, b, k, args.replays, args.warmup, dev, opened(b))
                ok = p[99] < budget
                best = b if ok and b > best else best
                print(f"{b:>6} {k:>9} {budget:>7.1f} {p[50]:>8.3f} {p[90]:>8.3f} {p[99]:>8.3f}  {'yes' if ok else 'no'}",
                      flush=True)
            print(f"largest measured real-time B for {k}-hop calls (p99 < {budget:.1f} ms): {best}", flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
