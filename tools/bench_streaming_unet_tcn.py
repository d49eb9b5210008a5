"""Per-hop latency of hop-by-hop streaming (puresound_amd/streaming/unet_tcn.py) for the egs/tse preset tse_unet_tcn_v0_causal
(tests/golden/cases.py, deterministic weights), against the hop's real-time budget (hop / 16 kHz = 8 ms).

For each B: step() and step_chunk() with 8 hops, graph replays, a device synchronise after every call; p50 / p99 of the
per-hop wall time (a chunk's time / its hops) over --replays calls after --warmup, and whether the p99 stays under the budget:
a result to read, not a threshold.  Then offline `inference` on the same signals for context.  Prints a plain-text report
(profiles/streaming_unet_tcn.txt holds one run).

--slots: the same two call sizes in three sessions per B -- a block session (init_streams), a slot session with every slot
opened together, and a slot session whose births are spread over 64 consecutive frames and in which, at every timed hop, one
slot in eight is inside its D drain hops (three groups of an eighth of the slots keep ending, draining, closing and
reopening between the calls: CHURN below; close() and open() are not part of a timed call) -- then the launch timers of the
three kernel pairs over eager hops, and the time of open() with a 1 s enrolment and with a cached embedding
(profiles/streaming_unet_tcn_slots.txt holds one run)."""
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


#: the slots that keep leaving and joining in the "births spread" session: three groups of one slot in eight (i % 8), each
#: on a cycle of CYCLE hops -- (hop of the cycle at which the group closes and reopens, hops of input its stream then has).
#: With window / hop = 4 and D = 6: group 7 drains during hops 4 .. 9, group 3 during 10 .. 15, group 5 (reopened at hop 8,
#: 6 hops of input) during 14 .. 15 and 0 .. 3 of the next cycle, and each is through its drain before it closes.  So at every
#: hop one slot in eight, at hops 14 and 15 two, is inside its D drain hops, and every boundary is a multiple of 8 hops.
CYCLE = 16
CHURN = {7: (0, 4), 3: (0, 10), 5: (8, 6)}


def slot_session(s, b, embed, spread):
    """A slot session of b slots: all opened together at frame 0, or (spread) slot i opened at frame i % 64 and fed from its
    birth on -- but for the CHURN slots, which churn() opens."""
    hop = s.hop_length
    s.init_slots(b, use_graph=True)
    if not spread:
        for i in range(b):
            s.open(i, embed=embed)
        return
    assert (s.window // hop, s.delay_frames) == (4, 6), "CHURN is laid out for a 4-hop window and a delay of 6 frames"
    quiet = torch.zeros(b, hop, device=embed.device)
    for f in range(min(64, b)):
        for i in range(f, b, 64):
            if i % 8 not in CHURN:
                s.open(i, embed=embed)
        s.step(quiet)


def churn(s, embed, hops_done):
    """Before the call that begins at hop `hops_done` of the timed session (a multiple of 8): the CHURN groups due at this hop
    of their cycle close (their D drain hops were stepped), reopen with the cached embedding and are ended ahead, after the
    hops of input the table gives them.  Not part of any timed call: the device is synchronised afterwards."""
    at = hops_done % CYCLE
    for group, (when, fed) in CHURN.items():
        if when != at:
            continue
        active = set(s.active)
        for i in range(group, s.streams, 8):
            if i in active:
                s.close(i)
            s.open(i, embed=embed)
            s.end(i, fed)
    torch.cuda.synchronize()


def time_calls(s, x, chunk_hops, replays, warmup, embed=None):
    """time_mode's loop on a session that is already running; embed: the session churns (see CHURN), between the calls."""
    hop = s.hop_length
    total_hops = x.shape[1] // hop
    pos = 0
    assert embed is None or 8 % chunk_hops == 0, "the CHURN boundaries are multiples of 8 hops"

    def call():
        nonlocal pos
        if pos + chunk_hops > total_hops:
            pos = 0
        piece = x[:, pos * hop:(pos + chunk_hops) * hop]
        pos += chunk_hops
        return s.step(piece) if chunk_hops == 1 else s.step_chunk(piece)

    ms = []
    for n in range(warmup + replays):
        if embed is not None and (n * chunk_hops) % 8 == 0:
            churn(s, embed, n * chunk_hops)
        if n == warmup:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if n >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3 / chunk_hops)
    a = np.asarray(ms)
    return float(np.percentile(a, 50)), float(np.percentile(a, 99))


def launch_timers(s, x, embed, slots, hops=20):
    """us per launch of the three kernel families over `hops` eager hops of a running session."""
    from puresound_amd import _abi
    lib = _abi.lib()
    hop, b = s.hop_length, x.shape[0]
    if slots:
        s.init_slots(b, use_graph=False)
        for i in range(b):
            s.open(i, embed=embed[:1])
    else:
        s.init_streams(b, embed=embed, use_graph=False)
    for i in range(s.prime_hops + 3):
        s.step(x[:, i * hop:(i + 1) * hop])
    torch.cuda.synchronize()
    lib.ps_profile_enable(1)
    for i in range(hops):
        s.step(x[:, (20 + i) * hop:(21 + i) * hop])
    torch.cuda.synchronize()
    out = {}
    for fam in ("conv2d_step", "gated_tcn_step", "istft_step"):
        ms, cnt = ctypes.c_double(), ctypes.c_int()
        _abi.check(lib.ps_profile_read((fam + ("_slots" if slots else "")).encode(), ctypes.byref(ms), ctypes.byref(cnt)),
                   "ps_profile_read")
        out[fam] = (ms.value / max(cnt.value, 1) * 1e3, cnt.value // hops)
    lib.ps_profile_enable(0)
    return out


def open_times(s, model, dev, reps=20):
    """ms per open() (device synchronised) with a 1 s enrolment and with a cached embedding."""
    enroll = det_wave(9, 1, SR)[0].to(dev)
    embed = model.inference_tse_embedding(enroll[None])
    out = {}
    for name, kw in (("1 s enrolment", dict(enroll=enroll)), ("cached embedding", dict(embed=embed))):
        s.init_slots(reps + 2, use_graph=True)
        s.open(0, **kw)
        torch.cuda.synchronize()
        ms = []
        for i in range(1, reps + 1):
            t0 = time.perf_counter()
            s.open(i, **kw)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = (float(np.percentile(ms, 50)), float(np.max(ms)))
    return out


def main_slots(args, s, model, dev, budget):
    print(f"{'B':>6} {'session':>22} {'hops/call':>9} {'p50':>8} {'p99':>8}  real-time (p99 < {budget:.0f} ms)")
    sessions = ("block", "slots, opened together", "slots, births spread")
    one = model.inference_tse_embedding(det_wave(7, 1, 3000).to(dev))
    for b in (int(v) for v in args.batches.split(",")):
        x = det_wave(100 + b, b, SR * SECONDS).to(dev)
        for name in sessions:
            for k in (int(v) for v in args.chunks.split(",")):
                if name == "block":
                    p50, p99 = time_mode(s, x, one.expand(b, -1, -1).contiguous(), k, args.replays, args.warmup)
                else:
                    slot_session(s, b, one, spread="spread" in name)
                    p50, p99 = time_calls(s, x, k, args.replays, args.warmup, embed=one if "spread" in name else None)
                print(f"{b:>6} {name:>22} {k:>9} {p50:>8.3f} {p99:>8.3f}  {'yes' if p99 < budget else 'NO'}", flush=True)
        del x
        torch.cuda.empty_cache()
    print("# launch timers, eager hops: us per launch (launches per hop), entry without a span / *_slots_f32 entry")
    for b in (64, 1024):
        x = det_wave(100 + b, b, SR * SECONDS).to(dev)
        plain = launch_timers(s, x, one.expand(b, -1, -1).contiguous(), False)
        slots = launch_timers(s, x, one, True)
        for fam in plain:
            print(f"{b:>6} ps_{fam}_f32 {plain[fam][0]:8.1f} us ({plain[fam][1]})   ps_{fam}_slots_f32 {slots[fam][0]:8.1f} us "
                  f"({slots[fam][1]})", flush=True)
    for name, (p50, worst) in open_times(s, model, dev).items():
        print(f"# open() with a {name}: p50 {p50:.2f} ms, worst {worst:.2f} ms (20 calls, device synchronised)", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batches", default="1,16,64,256,1024")
    ap.add_argument("--chunks", default="1,8", help="hops per call (1 = step())")
    ap.add_argument("--replays", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--offline-up-to", type=int, default=64, help="largest B whose offline inference is timed")
    ap.add_argument("--tree", default="", help="source revision to print in the header")
    ap.add_argument("--slots", action="store_true", help="block session against slot sessions, launch timers, open() time")
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
    if args.slots:
        return main_slots(args, s, model, dev, budget)
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
