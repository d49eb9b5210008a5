"""Per-call latency of hop-by-hop streaming (puresound_amd/streaming/skim.py) for the causal SkiM speaker extractor
tse_skim_v0_causal (tests/golden/cases.py "tse_skim_causal_short", deterministic weights), against the call's real-time budget
(the audio it carries: 1 ms per 16-sample hop at 16 kHz).

For each B: step() (one hop per call), step_chunk() of 8 hops and of 16 hops, graph replays, a device synchronise after every
call; p50 / p99 of the per-call wall time over --replays calls after --warmup.  Calls whose frames hold the last frame of a
segment run the MemLSTM hand-over on top (one in 150 step() calls): they are reported on a line of their own (n of them, p50
and the slowest).  For context the demo harness (DemoTseNet.streaming_inference_chunk) at --demo-streams streams on chunks
of the same lengths, in the same run.  Prints a plain-text report (profiles/streaming_skim.txt holds one run).
--profile-only B,K: a short run of K-hop chunks at B streams and nothing else, for rocprofv3.
--slots: the slot sessions instead (init_slots / open; profiles/streaming_skim_slots.txt holds one run).  Per B and call size,
in one run: the block session (init_streams: the yardstick), a slot session with every slot opened at frame 0, one with the
births spread uniformly over the K frames of a segment, and the worst case, every tile's 16 slots born at 16 consecutive
frames (a chunk of k hops then meets min(k, 16) hand-over frames per tile).  In a staggered session most calls hold a segment
end of some slot, so every call counts: p50 / p99 / max over all of them.  Then the cost of open() with a 1 s enrolment and
with a cached embedding."""
import argparse
import contextlib
import io
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
from puresound_amd.streaming import StreamingSkiMExtractor  # noqa: E402

SR, SECONDS = 16000, 2


def time_mode(s, b, chunk_hops, replays, warmup, dev):
    """Per-call ms of `replays` calls (step() when chunk_hops == 1, else step_chunk of chunk_hops hops) -> (ms of the calls
    without a segment end, ms of those with one)."""
    x = det_wave(100 + b, b, SR * SECONDS).to(dev)
    embed = det_wave(200 + b, b, s.model.masker.embed_dim).to(dev)
    s.init_streams(streams=b, embed=embed, use_graph=True)
    hop, seg = s.hop_length, s.model.masker.seg_size
    total = x.shape[1] // hop
    pos = 0

    def call():
        nonlocal pos
        if pos + chunk_hops > total:
            pos = 0
        piece = x[:, pos * hop:(pos + chunk_hops) * hop]
        pos += chunk_hops
        first = s.frames
        s.step(piece) if chunk_hops == 1 else s.step_chunk(piece)
        return any((first + f) % seg == seg - 1 for f in range(chunk_hops))

    for _ in range(s.prime_hops):
        s.step(x[:, pos * hop:(pos + 1) * hop])
        pos += 1
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    plain, ends = [], []
    for _ in range(replays):
        t0 = time.perf_counter()
        end = call()
        torch.cuda.synchronize()
        (ends if end else plain).append((time.perf_counter() - t0) * 1e3)
    return np.asarray(plain), np.asarray(ends)


SLOT_CASES = ("block", "slots@0", "uniform", "worst")


def births(case, b, seg):
    """Per slot the frame at which it is opened."""
    if case == "uniform":
        return [(i * seg) // b for i in range(b)]
    if case == "worst":
        return [i % 16 for i in range(b)]
    return [0] * b


def time_slots(s, b, chunk_hops, case, replays, warmup, dev):
    """Per-call ms of `replays` calls in a slot session of b slots opened by `case` (or the block session), every call."""
    x = det_wave(100 + b, b, SR * SECONDS).to(dev)
    embed = det_wave(200 + b, b, s.model.masker.embed_dim).to(dev)
    hop = s.hop_length
    total = x.shape[1] // hop
    pos = 0

    def call(k):
        nonlocal pos
        if pos + k > total:
            pos = 0
        piece = x[:, pos * hop:(pos + k) * hop]
        pos += k
        s.step(piece) if k == 1 else s.step_chunk(piece)

    if case == "block":
        s.init_streams(streams=b, embed=embed, use_graph=True)
        for _ in range(s.prime_hops):
            call(1)
    else:
        s.init_slots(b, use_graph=True)
        at = births(case, b, s.model.masker.seg_size)
        for f in range(max(at) + 1):
            for i in (i for i, v in enumerate(at) if v == f):
                s.open(i, embed=embed[i])
            call(1)
    for _ in range(warmup):
        call(chunk_hops)
    torch.cuda.synchronize()
    ms = []
    for _ in range(replays):
        t0 = time.perf_counter()
        call(chunk_hops)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return np.asarray(ms)


def time_open(s, b, dev, n=200):
    """ms of open() in a running slot session of b slots: with a 1 s enrolment, with its cached embedding (a device
    synchronise after every call; close() between them is not timed)."""
    s.init_slots(b, use_graph=True)
    hop = s.hop_length
    x = det_wave(100, b, 2 * hop).to(dev)
    e = det_wave(400, 1, SR)[0].to(dev)
    d = s.model.inference_tse_embedding(e[None])
    out = {}
    for what, how in (("enroll 1 s", dict(enroll=e)), ("cached embed", dict(embed=d))):
        ms = []
        for i in range(n + 10):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.open(0, **how)
            torch.cuda.synchronize()
            if i >= 10:
                ms.append((time.perf_counter() - t0) * 1e3)
            s.step_chunk(x)
            s.close(0)
        out[what] = np.asarray(ms)
    return out


def report_slots(s, args, dev, hop_ms):
    print("# slot sessions; cases: block = init_streams (the yardstick); slots@0 = every slot opened at frame 0; uniform = births "
          "spread over the K frames of a segment; worst = every tile's 16 slots born at 16 consecutive frames")
    print(f"{'B':>6} {'hops/call':>9} {'budget':>7} {'case':>8} {'p50':>8} {'p99':>8} {'max':>8}  p99 in budget  max in budget")
    for k in (int(v) for v in args.chunks.split(",")):
        budget = hop_ms * k
        for b in (int(v) for v in args.batches.split(",")):
            for case in SLOT_CASES:
                ms = time_slots(s, b, k, case, args.replays, args.warmup, dev)
                p50, p99 = np.percentile(ms, 50), np.percentile(ms, 99)
                print(f"{b:>6} {k:>9} {budget:>7.1f} {case:>8} {p50:>8.3f} {p99:>8.3f} {ms.max():>8.3f}  "
                      f"{'yes' if p99 < budget else 'no':>13}  {'yes' if ms.max() < budget else 'no':>13}", flush=True)
        torch.cuda.empty_cache()
    print("# open() in a running session of 64 slots, ms per call with a device synchronise")
    for what, ms in time_open(s, 64, dev).items():
        print(f"{what:>14}  p50 {np.percentile(ms, 50):>8.3f}  p99 {np.percentile(ms, 99):>8.3f}", flush=True)


def time_demo(streams, chunk_hops, replays, warmup, dev):
    """Per-call ms of DemoTseNet.streaming_inference_chunk on chunks of chunk_hops hops (tools/bench_configs.py cfg5)."""
    from puresound_amd.streaming.demo import DemoTseNet
    with contextlib.redirect_stdout(io.StringIO()):          # (the constructor prints a time stamp)
        net = DemoTseNet().eval()
    net.load_state_dict(det_state_dict(net))
    net.to(dev)
    net.init_streams(streams)
    embed = det_wave(300, streams, 192).to(dev)
    n = 16 * chunk_hops
    wav = det_wave(301, streams, n * 8).to(dev)
    ms, pre = [], None
    for i in range(replays + warmup):
        chunk = wav[:, (i % 8) * n:(i % 8 + 1) * n]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = net.streaming_inference_chunk(chunk, embed, pre)
        pre = y[:, -16:]
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return np.asarray(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batches", default="1,64,256,1024")
    ap.add_argument("--chunks", default="1,8,16", help="hops per call")
    ap.add_argument("--replays", type=int, default=1500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--demo-streams", type=int, default=64)
    ap.add_argument("--profile-only", default="", help="B,K: 200 calls of K-hop chunks at B streams, no report")
    ap.add_argument("--tree", default="", help="source revision to print in the header")
    ap.add_argument("--slots", action="store_true", help="measure the slot sessions against the block session")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = cases.build(PA.NS, "tse_skim_causal_short").eval()
    model.load_state_dict(det_state_dict(model))
    model.to(dev)
    s = StreamingSkiMExtractor(model)
    if args.profile_only:
        b, k = (int(v) for v in args.profile_only.split(","))
        time_mode(s, b, k, 200, 20, dev)
        return
    hop_ms = 1e3 * s.hop_length / SR
    m = model.masker
    print(f"# tools/bench_streaming_skim.py  tree {args.tree or '(not given)'}  device {torch.cuda.get_device_name(dev)}")
    print(f"# tse_skim_v0_causal (C {m.input_size}, H {m.hidden_size}, K {m.seg_size}, {m.n_blocks} blocks; win {s.win_length}, "
          f"hop {s.hop_length}, latency {s.latency_samples} samples); per-call wall ms, graph replays, device sync per call; "
          f"{args.replays} calls after {args.warmup} warm-up; real-time budget {hop_ms:.1f} ms per hop")
    if args.slots:
        report_slots(s, args, dev, hop_ms)
        return
    print("# 'segment end': the calls whose frames hold the last frame of a segment (the MemLSTM hand-over runs on top)")
    print(f"{'B':>6} {'hops/call':>9} {'budget':>7} {'p50':>8} {'p99':>8}  real-time | segment end: {'n':>4} {'p50':>8} {'max':>8}  "
          f"real-time")
    for k in (int(v) for v in args.chunks.split(",")):
        budget = hop_ms * k
        for b in (int(v) for v in args.batches.split(",")):
            plain, ends = time_mode(s, b, k, args.replays, args.warmup, dev)
            p50, p99 = np.percentile(plain, 50), np.percentile(plain, 99)
            tail = f"{len(ends):>4} {np.percentile(ends, 50):>8.3f} {ends.max():>8.3f}  {'yes' if ends.max() < budget else 'no'}" \
                if len(ends) else f"{0:>4}"
            print(f"{b:>6} {k:>9} {budget:>7.1f} {p50:>8.3f} {p99:>8.3f}  {'yes' if p99 < budget else 'no':>9} |              {tail}",
                  flush=True)
        torch.cuda.empty_cache()
    print(f"# for context: DemoTseNet.streaming_inference_chunk, {args.demo_streams} streams (averaging overlap-add, graphs keyed "
          f"by the host's frame counter)")
    print(f"{'B':>6} {'hops/call':>9} {'budget':>7} {'p50':>8} {'p99':>8} {'max':>8}")
    for k in (int(v) for v in args.chunks.split(",")):
        if k == 1:
            continue
        ms = time_demo(args.demo_streams, k, min(args.replays, 500), args.warmup, dev)
        print(f"{args.demo_streams:>6} {k:>9} {hop_ms * k:>7.1f} {np.percentile(ms, 50):>8.3f} {np.percentile(ms, 99):>8.3f} "
              f"{ms.max():>8.3f}", flush=True)


if __name__ == "__main__":
    main()
