"""Per-hop latency of hop-by-hop streaming (puresound_amd/streaming/spectral.py) for the egs/ns presets ns_dpcrn_v0_causal and
ns_dparn_v0_causal (tests/golden/cases.py, deterministic weights), against the hop's real-time budget (hop / 16 kHz = 8 ms).

For each model and B: step() and step_chunk() with 4 and 16 hops, graph replays, a device synchronise after every call;
p50 / p90 / p99 of the per-hop wall time (a chunk's time / its hops) over --replays calls after --warmup.  Then the largest B
(doubling from the largest measured one) whose step() p99 stays under the budget, and offline `inference` on the same 10 s
signals for context.  Prints a plain-text report (profiles/streaming_ns.txt holds one run).

--slots: the report on slot sessions (profiles/streaming_ns_slots.txt holds one run).  For each model, B and step() / 16-hop
chunks, p50 / p99 per hop of (a) the block session, (b) a slot session of capacity B with every slot opened together and (c)
a slot session in which one slot in eight is closed and reopened every 32 hops (the close() / open() calls are inside the
timed call they precede), the difference of (b) and (c) to (a) per hop, whether p99 stays under the budget, the host time of
one open() and one close(), and the device time of the state-gate launch alone (the library's launch timers, eager hops).
--block-only prints (a) alone: the same table from the parent revision's checkout, run in the same job, is what (b) and (c)
are compared with."""
import argparse
import ctypes
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


def time_slots(sep, x, streams, chunk_hops, replays, warmup, churn_every=0):
    """Per-hop ms of `replays` calls of a slot session with every slot open; churn_every = n > 0: before the first call at or
    past every n-th hop one slot in eight is closed and reopened, inside that call's timed window -> (percentiles, host
    seconds of each open(), of each close())."""
    hop = sep.hop_length
    sep.init_slots(streams, use_graph=True)
    for slot in range(streams):
        sep.open(slot)
    total_hops = x.shape[1] // hop
    pos = hops_done = 0
    next_churn = churn_every
    opens, closes = [], []

    def call():
        nonlocal pos, hops_done, next_churn
        if churn_every and hops_done >= next_churn:
            next_churn += churn_every
            for slot in range(0, streams, 8):
                t0 = time.perf_counter()
                sep.close(slot)
                t1 = time.perf_counter()
                sep.open(slot)
                closes.append(t1 - t0)
                opens.append(time.perf_counter() - t1)
        if pos + chunk_hops > total_hops:
            pos = 0
        piece = x[:, pos * hop:(pos + chunk_hops) * hop]
        pos += chunk_hops
        hops_done += chunk_hops
        return sep.step(piece) if chunk_hops == 1 else sep.step_chunk(piece)

    for _ in range(max(warmup, (sep.prime_hops + chunk_hops) // chunk_hops)):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(replays):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / chunk_hops)
    return percentiles(ms), opens, closes


def gate_us(sep, x, streams, live, hops=50):
    """Device time in us of one ps_state_gate_slots_f32 launch (eager hops, the library's launch timers): every slot live, or
    every slot idle (each dead column of the four states is zeroed: the most the launch ever stores)."""
    from puresound_amd import _abi
    lib = _abi.lib()
    hop = sep.hop_length
    sep.init_slots(streams, use_graph=False)
    if live:
        for slot in range(streams):
            sep.open(slot)
    for i in range(sep.prime_hops + 2):
        sep.step(x[:, i * hop:(i + 1) * hop])
    torch.cuda.synchronize()
    lib.ps_profile_enable(1)
    for i in range(hops):
        sep.step(x[:, (8 + i) * hop:(9 + i) * hop])
    torch.cuda.synchronize()
    lib.ps_profile_enable(0)
    ms, cnt = ctypes.c_double(), ctypes.c_int()
    _abi.check(lib.ps_profile_read(b"state_gate_slots", ctypes.byref(ms), ctypes.byref(cnt)), "ps_profile_read")
    assert cnt.value == hops, cnt.value
    return ms.value / cnt.value * 1e3


def slots_report(args, dev, budget, batches):
    chunks = [int(c) for c in args.chunks.split(",")]
    for label in args.models.split(","):
        name = PRESETS[label]
        model = cases.build(PA.NS, name).eval()
        model.load_state_dict(det_state_dict(model))
        model.to(dev)
        sep = StreamingSeparator(model)
        print(f"\n## {label}  (n_fft {sep.n_fft}, hop {sep.hop_length}, latency {sep.latency_samples} samples)")
        head = f"{'B':>6} {'hops/call':>9} " + " ".join(f"{m + ' p50':>12} {m + ' p99':>12}" for m in (
            ("block",) if args.block_only else ("block", "slots", "churn")))
        print(head + ("" if args.block_only else f" {'slots-block':>12} {'churn-block':>12}  p99 < {budget:.0f} ms (block / slots / churn)"))
        host, gate = [], []
        for b in batches:
            x = det_wave(100 + b, min(b, 64), SR * 2).repeat((b + 63) // 64, 1)[:b].contiguous().to(dev)
            for k in chunks:
                a = time_mode(sep, x, b, k, args.replays, args.warmup)
                if args.block_only:
                    print(f"{b:>6} {k:>9} {a[50]:>12.3f} {a[99]:>12.3f}", flush=True)
                    continue
                f, _, _ = time_slots(sep, x, b, k, args.replays, args.warmup)
                c, opens, closes = time_slots(sep, x, b, k, args.replays, args.warmup, churn_every=32)
                if k == 1:
                    host.append((b, 1e6 * float(np.median(opens)), 1e6 * float(np.median(closes)), len(opens)))
                yes = " / ".join("yes" if p[99] < budget else "no" for p in (a, f, c))
                print(f"{b:>6} {k:>9} {a[50]:>12.3f} {a[99]:>12.3f} {f[50]:>12.3f} {f[99]:>12.3f} {c[50]:>12.3f} {c[99]:>12.3f} "
                      f"{f[50] - a[50]:>+12.3f} {c[50] - a[50]:>+12.3f}  {yes}", flush=True)
            if not args.block_only:
                gate.append((b, gate_us(sep, x, b, True), gate_us(sep, x, b, False)))
            del x
            torch.cuda.empty_cache()
        if not args.block_only:
            print("host time of one open() / one close(), us (median over the churn of the step() run; neither synchronises):")
            for b, o, c, n in host:
                print(f"  B {b:>5}: open {o:8.1f}  close {c:8.1f}   ({n} of each)")
            print("ps_state_gate_slots_f32 alone, us per launch (one launch per hop; eager hops, launch timers):")
            for b, live, idle in gate:
                print(f"  B {b:>5}: every slot live {live:7.1f}   every slot idle (all four states zeroed) {idle:7.1f}")


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
    ap.add_argument("--slots", action="store_true", help="the slot-session report (block, slots, slots with churn)")
    ap.add_argument("--block-only", action="store_true", help="with --slots: the block session's columns alone")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    budget = 1e3 * 128 / SR
    batches = [int(b) for b in args.batches.split(",")]
    chunks = [int(c) for c in args.chunks.split(",")]
    print(f"# tools/bench_streaming_ns.py  tree {args.tree or '(not given)'}  device {torch.cuda.get_device_name(dev)}")
    print(f"# per-hop wall ms (a chunk call / its hops), graph replays, device sync per call; {args.replays} calls after "
          f"{args.warmup} warm-up; real-time budget {budget:.1f} ms per 128-sample hop at {SR} Hz")
    if args.slots or args.block_only:
        return slots_report(args, dev, budget, batches)
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
