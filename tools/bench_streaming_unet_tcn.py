"""Per-hop latency of hop-by-hop streaming (puresound_amd/streaming/unet_tcn.py) for the egs/tse preset tse_unet_tcn_v0_causal
(tests/golden/cases.py, deterministic weights), against the hop's real-time budget (hop / 16 kHz = 8 ms).

For each B: step() and step_chunk() with 8 hops, graph replays, a device synchronise after every call; p50 / p99 of the
per-hop wall time (a chunk's time / its hops) over --replays calls after --warmup, and whether the p99 stays under the budget:
a result to read, not a threshold.  Then offline `inference` on the same signals for context.  Prints a plain-text report
(profiles/streaming_unet_tcn.txt holds one run)."""
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
from puresound_amd.streaming import StreamingUnetTcn  # noqa: E402

SR, SECONDS = 16000, 4


def time_mode(s, x, embed, chunk_hops, replays, warmup):
    """Per-hop ms of `replays` calls (step() when chunk_hops == 1, else step_chunk of chunk_hops hops)."""
    hop = s.hop_length
    s.init_streams(x.shape[0], embed=embed, use_graph=True)
    total_hops = x.shape[1] // hop
    pos = 0

    def call():
        nonlocal pos
        if pos + chunk_hops > total_hops:
            pos = 0
        piece = x[:, pos * hop:(pos + chunk_hops) * hop]
        pos += chunk_hops
        return s.step(piece) if chunk_hops == 1 else s.step_chunk(piece)

    for _ in range(s.prime_hops):                    # the window fills, the model's delay passes (eager hops)
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
        ms.append((time.perf_counter() - t0) * 1e3 / chunk_hops)
    a = np.asarray(ms)
    return float(np.percentile(a, 50)), float(np.percentile(a, 99))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batches", default="1,16,64,256,1024")
    ap.add_argument("--chunks", default="1,8", help="hops per call (1 = step())")
    ap.add_argument("--replays", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--offline-up-to", type=int, default=64, help="largest B whose offline inference is timed")
    ap.add_argument("--tree", default="", help="source revision to print in the header")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    budget = 1e3 * 128 / SR
    model = cases.build(PA.NS, "tse_unet_tcn_causal_short").eval()
    model.load_state_dict(det_state_dict(model))
    model.to(dev)
    s = StreamingUnetTcn(model)
    print(f"# tools/bench_streaming_unet_tcn.py  tree {args.tree or '(not given)'}  device {torch.cuda.get_device_name(dev)}")
    print(f"# tse_unet_tcn_v0_causal: n_fft {s.n_fft}, hop {s.hop_length}, delay {s.delay_frames} frames, latency "
          f"{s.latency_samples} samples")
    print(f"# per-hop wall ms (a chunk call / its hops), graph replays, device sync per call; {args.replays} calls after "
          f"{args.warmup} warm-up; real-time budget {budget:.1f} ms per 128-sample hop at {SR} Hz")
    print(f"{'B':>6} {'hops/call':>9} {'p50':>8} {'p99':>8}  real-time (p99 < {budget:.0f} ms)")
    for b in (int(v) for v in args.batches.split(",")):
        x = det_wave(100 + b, b, SR * SECONDS).to(dev)
        embed = model.inference_tse_embedding(det_wave(7, 1, 3000).to(dev)).expand(b, -1, -1).contiguous()
        for k in (int(v) for v in args.chunks.split(",")):
            p50, p99 = time_mode(s, x, embed, k, args.replays, args.warmup)
            print(f"{b:>6} {k:>9} {p50:>8.3f} {p99:>8.3f}  {'yes' if p99 < budget else 'NO'}", flush=True)
        if b <= args.offline_up_to:
            enroll = det_wave(7, 1, 3000).to(dev).expand(b, -1).contiguous()
            for _ in range(2):
                model.inference(x, enroll)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                model.inference(x, enroll)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / 3
            print(f"       offline inference of the same {SECONDS} s signals: {ms:9.2f} ms", flush=True)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
