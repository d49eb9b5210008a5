"""One launch per branch of the depthwise-conv, encoder / decoder and conv2d entries' kernel choice, on zero inputs: which
kernel runs, on what grid.

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/conv_dispatch_cases.py     (GPU: makes the launches)
  python tools/conv_dispatch_cases.py --ledger DIR/*/*kernel_trace.csv                           (formats the trace)

The ledger is one line per kernel of these entries in launch order: case | kernel with template arguments | grid |
workgroup | LDS bytes.  Two trees choose alike when their ledgers are equal line for line
(profiles/conv_dispatch_ledger.txt).  The shapes are those of tests/test_conv_dispatch_gpu.py (conv2d: its two preset
geometries)."""
import csv
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WG = 1 << 0   # PS_DBG_DWCONV_WG
DW = dict(n=2, h=17, t=1025)
C2D = dict(f=11, t=100, c1=3, c2=2, geometry=(5, 2, 2, 1, 1, 2, 1))   # kf, kt, stride_f, dil_f, dil_t, pad_f, pad_t

# (name, wrapper, arguments, kernels the case launches)
CASES = []
for dil in (4, 1):
    CASES += [(f"dwconv {name} dilation={dil}", "dwconv", dict(DW, dil=dil, **kw), 1) for name, kw in (
        ("fp32 wave", {}), ("fp32 workgroup", dict(flags=WG)), ("bf16 wave", dict(xb=True, yb=True)),
        ("bf16 workgroup", dict(xb=True, yb=True, flags=WG)), ("bf16 to fp32", dict(xb=True)), ("fp32 to bf16", dict(yb=True)),
        ("amax", dict(amax=True)))]
CASES += [(f"dwconv large halo dilation={dil}", "dwconv", dict(DW, dil=dil), 1) for dil in (256, 150)]
CASES += [("dwconv P=5 dilation=9", "dwconv", dict(DW, p=5, dil=9), 1)]
CASES += [(f"free_encode {win}/{hop} N={n} L={length} C={c}", "free_encode", dict(n=n, length=length, c=c, win=win, hop=hop), 1)
          for n, length, c, win, hop in ((2, 1040, 32, 32, 16), (2, 1024, 32, 32, 16), (2, 1040, 33, 32, 16), (2, 600, 24, 16, 8),
                                         (2, 211, 9, 20, 6), (1, 64, 4032, 32, 16), (1, 64, 4033, 32, 16))]
DECODE = ((16, 63, 32, 16, 1), (17, 64, 32, 16, 1), (16, 70, 16, 8, 1), (16, 5, 64, 64, 1), (9, 33, 20, 6, 1), (16, 64, 32, 16, 2),
          (16, 65, 32, 16, 2), (16, 97, 32, 16, 2))   # (the matrix-pipe decoder is two kernels: tiles, then their boundaries)
CASES += [(f"free_decode {win}/{hop} C={c} T={t}", "free_decode", dict(c=c, t=t, win=win, hop=hop), k) for c, t, win, hop, k in DECODE]
CASES += [(f"free_decode_moments 32/16 C=16 T={t}", "free_decode_moments", dict(c=16, t=t, win=32, hop=16), k)
          for t, k in ((64, 2), (65, 2), (97, 2), (63, 1))]
for tr in (False, True):
    CASES += [(f"conv2d{' transposed' if tr else ''} M={m}{' stats' if st else ''}", "conv2d", dict(C2D, m=m, stats=st, transposed=tr), 1)
              for m, st in ((2, False), (4, False), (4, True), (33, False), (65, True))]
    CASES += [(f"conv2d_f16x2{' transposed' if tr else ''} M={m}", "conv2d_f16x2", dict(C2D, m=m, transposed=tr), 1)
              for m in (32, 64, 65)]
CASES += [("pad_rows", "pad_rows", {}, 1), ("unpad_rows", "unpad_rows", {}, 1)]


def launch(wrapper, **a):
    import torch
    from puresound_amd import _abi, hip
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device="cuda")  # noqa: E731
    with _abi.debug(a.get("flags", 0)):
        if wrapper == "dwconv":
            p, bf16 = a.get("p", 3), torch.bfloat16
            hip.dwconv(z(a["n"], a["h"], hip.padded_frames(a["t"]), dtype=bf16 if a.get("xb") else torch.float32), a["t"],
                       z(a["h"], 1, p), z(a["h"]), a["dil"], (p - 1) // 2 * a["dil"], None, not a.get("amax"),
                       out_dtype=bf16 if a.get("yb") else torch.float32, want_amax=bool(a.get("amax")))
        elif wrapper == "free_encode":
            hip.free_encode(z(a["n"], a["length"]), z(a["c"], 1, a["win"]), a["hop"], True)
        elif wrapper in ("free_decode", "free_decode_moments"):
            feats, w = z(2, a["c"], hip.padded_frames(a["t"])), z(a["c"], 1, a["win"])
            if wrapper == "free_decode":
                hip.free_decode(feats, a["t"], w, a["hop"], feats, "relu", "linear")
            else:
                hip.free_decode_moments(feats, a["t"], w, a["hop"], z(2, (a["t"] - 1) * a["hop"] + a["win"]), feats, "relu", "linear")
        elif wrapper in ("conv2d", "conv2d_f16x2"):
            kf, kt, sf, df, dt, pf, pt = a["geometry"]
            tr, m, k = a["transposed"], a["m"], (a["c1"] + a["c2"]) * kf * kt
            f_out = (a["f"] - 1) * sf - 2 * pf + df * (kf - 1) + (sf - kf + 2 * pf) + 1 if tr else (a["f"] + 2 * pf - df * (kf - 1) - 1) // sf + 1
            x1, x2 = z(1, a["c1"], a["f"], 128), z(1, a["c2"], a["f"], 128)
            tail = (m, a["t"], f_out, kf, kt, sf, df, dt, pf, pt, tr)
            if wrapper == "conv2d_f16x2":
                img, w_exp = hip.pack_conv2d_f16x2(z(m, k) + 1.0)
                hip.conv2d_f16x2(x1, x2, img, w_exp, z(m), *tail, "prelu", z(1))
            elif a["stats"]:
                hip.conv2d_stats(x1, x2, hip.pack_wt(z(m, k)), z(m), *tail)
            else:
                hip.conv2d(x1, x2, hip.pack_wt(z(m, k)), z(m), *tail, "prelu", z(1))
        elif wrapper == "pad_rows":
            hip.pad_rows(z(3, 5, 100))
        else:
            hip.unpad_rows(z(3, 5, 128), 100)
        torch.cuda.synchronize()


def ledger(trace):
    ours = r"dwconv_|free_encode_|free_decode_|conv2d_|pad_rows_kernel"
    rows = [r for r in csv.DictReader(open(trace)) if re.search(ours, r["Kernel_Name"])]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    lds = "LDS_Block_Size" if rows and "LDS_Block_Size" in rows[0] else "Group_Segment_Size"
    assert len(rows) == sum(c[3] for c in CASES), "the trace holds another number of kernels than the cases account for"
    it = iter(rows)
    for name, _, _, kernels in CASES:
        for _ in range(kernels):
            r = next(it)
            k = re.sub(r"^void |\(.*$", "", r["Kernel_Name"])
            print(f'{name} | {k} | grid {r["Grid_Size_X"]}x{r["Grid_Size_Y"]}x{r["Grid_Size_Z"]} | wg {r["Workgroup_Size_X"]} | '
                  f'lds {r[lds]}')


if __name__ == "__main__":
    if sys.argv[1:2] == ["--ledger"]:
        ledger(sys.argv[2])
    else:
        for name, wrapper, kw, _ in CASES:
            print("case", name, flush=True)
            launch(wrapper, **kw)
