"""One launch per branch of the recurrence entries' kernel choice, on zero inputs: which kernel runs, on what grid.

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/lstm_dispatch_cases.py     (GPU: makes the launches)
  python tools/lstm_dispatch_cases.py --ledger DIR/*/*kernel_trace.csv                           (formats the trace)

The ledger is one line per recurrence kernel in launch order: case | kernel with template arguments | grid | workgroup |
LDS bytes.  Two trees choose alike when their ledgers are equal line for line (profiles/lstm_dispatch_ledger.txt).  The
cooperative kernel runs only at the (H, D, N, Q, steps) tests/test_round4_gpu.py launches it at."""
import csv
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCALAR, WIDE, M4, B4 = 1 << 1, 1 << 2, 1 << 3, 1 << 20   # PS_DBG_LSTM_SCALAR / _WIDE / _M4 / _4B_STORES
SEG = dict(n=16, q=256, q_stride=20, steps=20)             # 4096 sequences of 20 consecutive frames
STRIDED = dict(n=2, q=20, q_stride=1, steps=8, step_stride=20)
SHORT = dict(n=1, q=4, q_stride=8, steps=8)
ACROSS = dict(n=1, q=8, q_stride=1, steps=4, step_stride=8)

# (name, wrapper, arguments: n, h, d, q, q_stride, steps, step_stride = 1, f16x2, flags, kind, coop)
CASES = [(f"lstm H={h}", "lstm", dict(SHORT, h=h)) for h in (32, 96)]
CASES += [(f"lstm H=64 4096 segments of 20{' f16x2' if f else ''} D={d}", "lstm", dict(SEG, h=64, d=d, f16x2=f))
          for f in (False, True) for d in (1, 2)]
CASES += [
    ("lstm H=64 4096 sequences of 8", "lstm", dict(SEG, h=64, steps=8)),
    ("lstm H=64 4095 sequences of 8", "lstm", dict(SEG, h=64, n=15, q=273, steps=8)),
    ("lstm H=64 strided", "lstm", dict(STRIDED, h=64)),
    ("lstm H=64 strided f16x2", "lstm", dict(STRIDED, h=64, f16x2=True)),
    ("lstm H=64 strided f16x2 4B_STORES", "lstm", dict(STRIDED, h=64, f16x2=True, flags=B4)),
    ("lstm H=128 consecutive", "lstm", dict(SHORT, h=128)),
    ("lstm H=128 strided", "lstm", dict(STRIDED, h=128)),
    ("lstm H=64 steps=6 D=2", "lstm", dict(SHORT, h=64, d=2, steps=6)),
    ("lstm H=64 steps=6 D=1 room in the row", "lstm", dict(SHORT, h=64, steps=6)),
    ("lstm H=64 q_stride=6", "lstm", dict(SHORT, h=64, q_stride=6, steps=4)),
    ("lstm H=64 strided WIDE", "lstm", dict(STRIDED, h=64, flags=WIDE)),
    ("lstm H=128 WIDE", "lstm", dict(SHORT, h=128, flags=WIDE)),
    ("lstm H=64 4096 segments of 20 WIDE 4B_STORES", "lstm", dict(SEG, h=64, flags=WIDE | B4)),
    ("lstm H=64 4096 sequences of 8 M4", "lstm", dict(SEG, h=64, steps=8, flags=M4)),
    ("lstm H=64 SCALAR", "lstm", dict(SHORT, h=64, flags=SCALAR)),
    ("lstm H=128 SCALAR", "lstm", dict(SHORT, h=128, flags=SCALAR)),
    ("rnn GRU H=8", "rnn", dict(SHORT, h=8, kind="GRU")),
    ("rnn RNN H=8", "rnn", dict(SHORT, h=8, kind="RNN")),
    ("lstm_fmajor consecutive", "lstm_fmajor", dict(SHORT, h=128)),
    ("lstm_fmajor across", "lstm_fmajor", dict(ACROSS, h=128)),
    ("lstm_fmajor consecutive 4B_STORES", "lstm_fmajor", dict(SHORT, h=128, flags=B4)),
]
CASES += [(f"lstm_fmajor_h256 streamed H={h} {name}", "lstm_fmajor_h256", dict(walk, h=h))
          for h in (256, 192) for name, walk in (("consecutive", SHORT), ("across", ACROSS))]
# (n, q = segments, steps = segment length) of test_lstm_h256_streamed_weights_kernel, test_cooperative_lstm_gives_up_loudly
# and test_cooperative_lstm_many_groups_back_to_back
COOP = [(256, 2, 2, 9, 8), (256, 1, 3, 5, 7), (256, 2, 1, 20, 6), (256, 1, 2, 3, 30), (192, 2, 3, 1, 90), (192, 1, 2, 4, 9),
        (192, 2, 32, 1, 300), (256, 1, 4, 1, 6), (256, 1, 32, 27, 150), (256, 2, 32, 27, 50)]
CASES += [(f"lstm_fmajor_h256 cooperative H={h} D={d} N={n} Q={q} steps={s}{' 4B_STORES' if f else ''}", "lstm_fmajor_h256",
           dict(h=h, d=d, n=n, q=q, q_stride=s, steps=s, coop=True, flags=f))
          for h, d, n, q, s in COOP for f in ((0, B4) if (h, d, n, q) in ((256, 2, 2, 9), (256, 1, 32, 27)) else (0,))]


def launch(wrapper, n, h, q, q_stride, steps, d=1, step_stride=1, f16x2=False, flags=0, kind=None, coop=False):
    import torch
    from puresound_amd import _abi, hip
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device="cuda")  # noqa: E731
    ldt = hip.padded_frames((q - 1) * q_stride + (steps - 1) * step_stride + 1)
    walk = (q, q_stride, steps, step_stride)
    hip.COOP_LSTM = coop
    with _abi.debug(flags):
        if wrapper == "lstm":
            hip.lstm(z(n, d * 4 * h, ldt), z(d, h, 4 * h), h, d, *walk, f16x2=f16x2)
        elif wrapper == "rnn":
            g = (3 if kind == "GRU" else 1) * h
            hip.rnn(z(n, d * g, ldt), z(d, h, g), kind, h, d, *walk, bhn=z(d, h) if kind == "GRU" else None)
        elif wrapper == "lstm_fmajor":
            hip.lstm_fmajor(z(n, ldt, d * 4 * h), z(d, h, 4 * h), h, d, *walk)
        else:
            img, scale = hip.pack_whh_h256(torch.zeros(d, h, 4 * h))
            hip.lstm_fmajor_h256(z(n, ldt, d * 4 * h), img.cuda(), scale, d, *walk)
        torch.cuda.synchronize()


def ledger(trace):
    rows = [r for r in csv.DictReader(open(trace)) if re.search(r"lstm_|rnn_kernel|zero_words_kernel", r["Kernel_Name"])]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    lds = "LDS_Block_Size" if rows and "LDS_Block_Size" in rows[0] else "Group_Segment_Size"
    it = iter(rows)
    r = next(it, None)
    for name, _, kw in CASES:
        # a case is one kernel; a cooperative one is zero_words_kernel and one lstm_coop_kernel per launch (one per direction
        # when both do not fit the chip at once)
        take = 1
        while r is not None and take:
            k = re.sub(r"^void |\(.*$", "", r["Kernel_Name"])
            print(f'{name} | {k} | grid {r["Grid_Size_X"]}x{r["Grid_Size_Y"]}x{r["Grid_Size_Z"]} | wg {r["Workgroup_Size_X"]} | '
                  f'lds {r[lds]}')
            r = next(it, None)
            take = kw.get("coop") and r is not None and "lstm_coop_kernel" in r["Kernel_Name"]
    assert r is None, "more recurrence kernels in the trace than the cases account for"


if __name__ == "__main__":
    if sys.argv[1:2] == ["--ledger"]:
        ledger(sys.argv[2])
    else:
        for name, wrapper, kw in CASES:
            print("case", name, flush=True)
            launch(wrapper, **kw)
