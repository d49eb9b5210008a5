"""Per-call latency of hop-by-hop streaming (puresound_amd/streaming/tcn.py) for the causal Conv-TasNet speaker extractor
td_tse_conv_tasnet_v0_causal (tests/golden/cases.py "cfg3_causal_short", deterministic weights), against the call's real-time
budget (the audio it carries: 1 ms per 16-sample hop at 16 kHz).

For each B: step() (one hop per call) and step_chunk() of --chunk hops, graph replays, a device synchronise after every call;
p50 / p90 / p99 of the per-call wall time over --replays calls after --warmup.  Then the largest B (doubling from the largest
measured one) whose p99 stays under the budget, for each call size.  Prints a plain-text report (profiles/streaming_tcn.txt
holds one run).  --profile-only B,K: a short run of K-hop chunks at B streams and nothing else, for rocprofv3.

--slots: the same loop on a slot session (init_slots, every slot opened with its own enrolment), then the host wall time of
open() and of close() on one slot of a running session, a device synchronise after each, with the speaker branch (the preset)
and without one (tiny_free_relu_causal): profiles/streaming_tcn_slots.txt holds one run next to the block sessions'."""
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
from puresound_amd.streaming import StreamingConvTasNet  # noqa: E402

SR, SECONDS = 16000, 2


def session(s, b, dev, slots=False):
    x = det_wave(100 + b, b, SR * SECONDS).to(dev)
    e = det_wave(200 + b, b, SR).to(dev)
    if slots:
        s.init_slots(b, use_graph=True)
        for i in range(b):
            s.open(i, e[i])
    else:
        s.init_streams(streams=b, enroll=e, use_graph=True)
    return x


def time_mode(s, b, chunk_hops, replays, warmup, dev, slots=False):
    """Per-call ms of `replays` calls (step() when chunk_hops == 1, else step_chunk of chunk_hops hops)."""
    x = session(s, b, dev, slots)
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

    for _ in range(s.prime_hops):                    # (a slot session has no priming phase: these hops return samples)
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


def time_open_close(s, capacity, enroll, chunk_hops, n, dev):
    """Host wall ms of n open() and n close() calls on slot 0 of a running slot session of `capacity` slots (the others
    open), a device synchronise after each; a chunk runs between the two (a stream needs a window before it can close)."""
    others = None if enroll is None else det_wave(300, capacity, enroll.numel()).to(dev)
    s.init_slots(capacity, use_graph=True)
    for i in range(1, capacity):
        s.open(i, None if others is None else others[i])
    x = det_wave(301, capacity, chunk_hops * s.hop_length).to(dev)
    t_open, t_close = [], []
    for i in range(n + 5):                            # (5 warm-up rounds: graph capture, allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.open(0, enroll)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        s.step_chunk(x)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        s.close(0)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if i >= 5:
            t_open.append((t1 - t0) * 1e3)
            t_close.append((t3 - t2) * 1e3)
    return [{p: float(np.percentile(np.asarray(t), p)) for p in (50, 99)} for t in (t_open, t_close)]


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batches", default="1,16,64,256,1024")
    ap.add_argument("--chunk", type=int, default=8, help="hops per step_chunk call")
    ap.add_argument("--replays", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--max-search", type=int, default=4096, help="largest B the real-time search tries")
    ap.add_argument("--profile-only", default="", help="B,K: 200 calls of K-hop chunks at B streams, no report")
    ap.add_argument("--tree", default="", help="source revision to print in the header")
    ap.add_argument("--slots", action="store_true", help="a slot session with every slot open, then open() / close() times")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = cases.build(PA.NS, "cfg3_causal_short").eval()
    model.load_state_dict(det_state_dict(model))
    model.to(dev)
    s = StreamingConvTasNet(model)
    if args.profile_only:
        b, k = (int(v) for v in args.profile_only.split(","))
        time_mode(s, b, k, 200, 20, dev, args.slots)
        return
    hop_ms = 1e3 * s.hop_length / SR
    print(f"# tools/bench_streaming_tcn.py  tree {args.tree or '(not given)'}  device {torch.cuda.get_device_name(dev)}")
    print(f"# td_tse_conv_tasnet_v0_causal (win {s.win_length}, hop {s.hop_length}, latency {s.latency_samples} samples); "
          f"per-call wall ms, graph replays, device sync per call; {args.replays} calls after {args.warmup} warm-up; "
          f"real-time budget {hop_ms:.1f} ms per hop")
    if args.slots:
        print("# slot session (init_slots): every slot opened with its own 1 s enrolment, none ended")
    print(f"{'B':>6} {'hops/call':>9} {'budget':>7} {'p50':>8} {'p90':>8} {'p99':>8}  real-time")
    for k in (1, args.chunk):
        budget = hop_ms * k
        best = 0
        for b in [int(v) for v in args.batches.split(",")]:
            p = time_mode(s, b, k, args.replays, args.warmup, dev, args.slots)
            ok = p[99] < budget
            best = b if ok and b > best else best
            print(f"{b:>6} {k:>9} {budget:>7.1f} {p[50]:>8.3f} {p[90]:>8.3f} {p[99]:>8.3f}  {'yes' if ok else 'no'}", flush=True)
        b = best
        while b and b == best and 2 * b <= args.max_search and b >= max(int(v) for v in args.batches.split(",")):
            b *= 2
            p = time_mode(s, b, k, args.replays, args.warmup, dev, args.slots)
            ok = p[99] < budget
            print(f"{b:>6} {k:>9} {budget:>7.1f} {p[50]:>8.3f} {p[90]:>8.3f} {p[99]:>8.3f}  {'yes' if ok else 'no'}  (search)",
                  flush=True)
            if ok:
                best = b
        print(f"largest real-time B for {k}-hop calls (p99 < {budget:.1f} ms): {best}", flush=True)
        torch.cuda.empty_cache()
    if args.slots:
        tiny = cases.build(PA.NS, "tiny_free_relu_causal").eval()
        tiny.load_state_dict(det_state_dict(tiny))
        tiny.to(dev)
        print(f"# open() / close() of one slot, host wall ms with a device synchronise after each, 100 of each, capacity 64, "
              f"{args.chunk}-hop chunks")
        print(f"{'model':>44} {'open p50':>9} {'open p99':>9} {'close p50':>10} {'close p99':>10}")
        for label, st, enroll in (("preset, speaker branch, 1 s enrolment", s, det_wave(302, 1, SR)[0].to(dev)),
                                  ("tiny_free_relu_causal, no speaker branch", StreamingConvTasNet(tiny), None)):
            o, c = time_open_close(st, 64, enroll, args.chunk, 100, dev)
            print(f"{label:>44} {o[50]:>9.3f} {o[99]:>9.3f} {c[50]:>10.3f} {c[99]:>10.3f}", flush=True)


if __name__ == "__main__":
    main()
