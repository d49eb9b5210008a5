"""What the 1x1-conv GEMM entries refuse, and what the weight packers produce -- both without a GPU.

Refusals: every row of CASES calls one conv1x1-family entry with arguments it must turn down before any launch or device
query; the return code and the whole ps_last_error() text are compared.  Non-null pointers are 16-byte aligned host
buffers that are never dereferenced (the call returns first).  Not in the table because they are decided by rb_ok() /
device_cus(), which ask the device: "this launch cannot run on the register-B kernel" of ps_conv1x1_f16x2_fmajor_f32
(its 2 GiB slab rule included), ps_conv1x1_f16_rows and ps_conv1x1_f16x2_ln_f32.  Nor N = 65536 for ps_conv1x1_f32: its
persistent grid does not put N into a grid dimension, so it accepts that call and goes on to launch.

Packers: SHA-256 of each packed image's bytes at the packers' edge shapes, plus the exponent / scales.

EXPECTED and PACKED were recorded from commit ad87148 (the library built from it, its hip.py on the CPU)."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

from puresound_amd import _abi, hip

_BUF = C.create_string_buffer(4096 + 16)
BUF = (C.addressof(_BUF) + 15) // 16 * 16   # 16-byte aligned host memory; BUF + 4 is the misaligned pointer
N, K, M, T, LDT = 2, 64, 256, 129, 384

GLOBAL, AFFINE = _abi.PS_NORM_GLOBAL, _abi.PS_NORM_AFFINE


def _pro(**kw):
    p = _abi.Prologue()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _rng(w_exp=0, x_bound=1.0, x_amax=None, x_amax_parts=0):
    return _abi.F16x2Range(w_exp, x_bound, x_amax, x_amax_parts, None)


PRO_FAULTS = {
    "global_incomplete": dict(norm=GLOBAL, stats=BUF, parts=0, count=1.0, gamma=BUF, beta=BUF),
    "affine_no_beta": dict(norm=AFFINE, gamma=BUF),
    "prelu_no_slope": dict(prelu=1),
}
RANGE_FAULTS = {
    "range_null": None,
    "range_w_exp": dict(w_exp=101),
    "range_negative_bound": dict(x_bound=-1.0),
    "range_amax_parts": dict(x_bound=0.0, x_amax=BUF, x_amax_parts=0),
}

# entry -> (argument names in call order, defaults of a valid call)
_GEMM = dict(x=BUF, wt=BUF, y=BUF, N=N, K=K, M=M, T=T, ldt=LDT, pro=None, bias=None, bias_n=None, res=None, ostats=None,
             stream=None)
ENTRIES = {
    "ps_conv1x1_f32": ("x wt y N K M T ldt pro bias bias_n res ostats stream", _GEMM),
    "ps_conv1x1_bf16_f32": ("x wt y N K M T ldt planes pro bias bias_n res ostats stream", dict(_GEMM, planes=3)),
    "ps_conv1x1_bf16_io": ("x x_bf16 wt y y_bf16 N K M T ldt planes pro bias bias_n res ostats stream",
                           dict(_GEMM, planes=1, x_bf16=0, y_bf16=0)),
    "ps_conv1x1_f16x2_f32": ("x wt rng y N K M T ldt pro bias bias_n res ostats stream", dict(_GEMM, rng={})),
    "ps_conv1x1_f16_rows": ("x wt rng y N K M T ldt pro bias bias_n res ostats stream", dict(_GEMM, rng={})),
    "ps_conv1x1_f16x2_fmajor_f32": ("x wt rng y N K M T ldt ldm bias stream",
                                    dict(x=BUF, wt=BUF, rng={}, y=BUF, N=N, K=K, M=M, T=T, ldt=LDT, ldm=M, bias=None,
                                         stream=None)),
    "ps_conv1x1_f16x2_ln_f32": ("x wt rng y N K C T ldt pro bias gamma beta eps res res_inside stream",
                                dict(x=BUF, wt=BUF, rng={}, y=BUF, N=N, K=K, C=128, T=T, ldt=LDT, pro=None, bias=None,
                                     gamma=BUF, beta=BUF, eps=1e-5, res=None, res_inside=0, stream=None)),
}
RANGED = ("ps_conv1x1_f16x2_f32", "ps_conv1x1_f16x2_fmajor_f32", "ps_conv1x1_f16x2_ln_f32", "ps_conv1x1_f16_rows")


def _cases():
    out = []
    for e, (_, d) in ENTRIES.items():
        out += [(e, "null_x", dict(x=None)), (e, "null_wt", dict(wt=None)), (e, "null_y", dict(y=None))]
        out += [(e, f"{k}_zero", {k: 0}) for k in ("N", "K", "M", "T") if k in d]
        out += [(e, "T_negative", dict(T=-1)), (e, "ldt_below_T", dict(T=385)), (e, "ldt_not_128", dict(ldt=200)),
                (e, "wt_misaligned", dict(wt=BUF + 4))]
        if e != "ps_conv1x1_f32":   # (its grid has no such limit)
            out.append((e, "N_65536", dict(N=65536)))
        if "ostats" in d:
            out.append((e, "res_with_ostats", dict(res=BUF, ostats=BUF)))
            out += [(e, f"pro_{k}", dict(pro=v)) for k, v in PRO_FAULTS.items()]
            out.append((e, "K_576_with_prologue", dict(K=576, pro=dict(prelu=1, slope=BUF))))
    for e in ("ps_conv1x1_bf16_f32", "ps_conv1x1_bf16_io"):
        out += [(e, f"planes_{p}", dict(planes=p)) for p in (0, 2, 4)]
    out += [("ps_conv1x1_bf16_io", "bf16_rows_planes_3", dict(planes=3, x_bf16=1, y_bf16=1)),
            ("ps_conv1x1_bf16_io", "bf16_x_planes_3", dict(planes=3, x_bf16=1))]
    for e in RANGED:
        out += [(e, k, dict(rng=v)) for k, v in RANGE_FAULTS.items()]
    out += [("ps_conv1x1_f16_rows", "range_no_source", dict(rng=dict(x_bound=0.0))),
            ("ps_conv1x1_f16x2_fmajor_f32", "ldm_below_M", dict(ldm=252)),
            ("ps_conv1x1_f16x2_fmajor_f32", "ldm_not_4", dict(ldm=258)),
            ("ps_conv1x1_f16x2_ln_f32", "C_64", dict(C=64)),
            ("ps_conv1x1_f16x2_ln_f32", "null_gamma", dict(gamma=None)),
            ("ps_conv1x1_f16x2_ln_f32", "pro_pre_relu", dict(pro=dict(pre_relu=1))),
            ("ps_conv1x1_f16x2_ln_f32", "pro_global", dict(pro=dict(norm=GLOBAL))),
            ("ps_conv1x1_f16x2_ln_f32", "pro_prelu_no_slope", dict(pro=dict(prelu=1))),
            ("ps_conv1x1_f16x2_ln_f32", "K_576_with_prologue", dict(K=576, pro=dict(prelu=1, slope=BUF)))]
    return out


CASES = _cases()


def refuse(entry, overrides):
    names, defaults = ENTRIES[entry]
    a = dict(defaults, **overrides)
    keep = []   # (the structures must outlive the call)
    if isinstance(a.get("pro"), dict):
        keep.append(_pro(**a["pro"]))
        a["pro"] = C.byref(keep[-1])
    if "rng" in a and a["rng"] is not None:
        keep.append(_rng(**a["rng"]))
        a["rng"] = C.byref(keep[-1])
    lib = _abi.lib()
    rc = getattr(lib, entry)(*[a[k] for k in names.split()])
    return rc, lib.ps_last_error().decode()


EXPECTED = {
    "ps_conv1x1_f32:null_x": (-1, "ps_conv1x1_f32: null pointer or non-positive size (N=2 K=64 M=256 T=129)"),
    "ps_conv1x1_f32:null_wt": (-1, "ps_conv1x1_f32: null pointer or non-positive size (N=2 K=64 M=256 T=129)"),
    "ps_conv1x1_f32:null_y": (-1, "ps_conv1x1_f32: null pointer or non-positive size (N=2 K=64 M=256 T=129)"),
    "ps_conv1x1_f32:N_zero": (-1, "ps_conv1x1_f32: null pointer or non-positive size (N=0 K=64 M=256 T=129)"),
    "ps_conv1x1_f32:K_zero": (-1, "ps_conv1x1_f32: null pointer or non-positive size (N=2 K=0 M=256 T=129)"),
    "ps_conv1x1_f32:M_zero": (-1, "ps_conv1x1_f32: null pointer or non-positive size (N=2 K=64 M=0 T=129)"),
    "ps_conv1x1_f32:T_zero": (-1, "ps_conv1x1_f32: null pointer or non-positive size (N=2 K=64 M=256 T=0)"),
    "ps_conv1x1_f32:T_negative": (-1, "ps_conv1x1_f32: null pointer or non-positive size (N=2 K=64 M=256 T=-1)"),
    "ps_conv1x1_f32:ldt_below_T": (-2,
        "ps_conv1x1_f32: ldt=384 must be a multiple of 128 >= T=385 and pointers 16-byte aligned"),
    "ps_conv1x1_f32:ldt_not_128": (-2,
        "ps_conv1x1_f32: ldt=200 must be a multiple of 128 >= T=129 and pointers 16-byte aligned"),
    "ps_conv1x1_f32:wt_misaligned": (-2,
        "ps_conv1x1_f32: ldt=384 must be a multiple of 128 >= T=129 and pointers 16-byte aligned"),
    "ps_conv1x1_f32:res_with_ostats": (-3,
        "ps_conv1x1_f32: residual and output statistics cannot be combined (no Conv-TasNet stage needs both)"),
    "ps_conv1x1_f32:pro_global_incomplete": (-1,
        "ps_conv1x1_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_conv1x1_f32:pro_affine_no_beta": (-1, "ps_conv1x1_f32: PS_NORM_AFFINE prologue needs gamma/beta"),
    "ps_conv1x1_f32:pro_prelu_no_slope": (-1, "ps_conv1x1_f32: prelu prologue needs slope"),
    "ps_conv1x1_f32:K_576_with_prologue": (-3,
        "ps_conv1x1_f32: K=576 exceeds the 512 input channels the prologue keeps scale/shift tables for"),
    "ps_conv1x1_bf16_f32:null_x": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=129)"),
    "ps_conv1x1_bf16_f32:null_wt": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=129)"),
    "ps_conv1x1_bf16_f32:null_y": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=129)"),
    "ps_conv1x1_bf16_f32:N_zero": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=0 K=64 M=256 T=129)"),
    "ps_conv1x1_bf16_f32:K_zero": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=0 M=256 T=129)"),
    "ps_conv1x1_bf16_f32:M_zero": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=0 T=129)"),
    "ps_conv1x1_bf16_f32:T_zero": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=0)"),
    "ps_conv1x1_bf16_f32:T_negative": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=-1)"),
    "ps_conv1x1_bf16_f32:ldt_below_T": (-2,
        "ps_conv1x1_bf16_f32: ldt=384 must be a multiple of 128 >= T=385, weights 16-byte aligned"),
    "ps_conv1x1_bf16_f32:ldt_not_128": (-2,
        "ps_conv1x1_bf16_f32: ldt=200 must be a multiple of 128 >= T=129, weights 16-byte aligned"),
    "ps_conv1x1_bf16_f32:wt_misaligned": (-2,
        "ps_conv1x1_bf16_f32: ldt=384 must be a multiple of 128 >= T=129, weights 16-byte aligned"),
    "ps_conv1x1_bf16_f32:N_65536": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=65536 K=64 M=256 T=129)"),
    "ps_conv1x1_bf16_f32:res_with_ostats": (-3,
        "ps_conv1x1_bf16_f32: residual and output statistics cannot be combined"),
    "ps_conv1x1_bf16_f32:pro_global_incomplete": (-1,
        "ps_conv1x1_bf16_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_conv1x1_bf16_f32:pro_affine_no_beta": (-1, "ps_conv1x1_bf16_f32: PS_NORM_AFFINE prologue needs gamma/beta"),
    "ps_conv1x1_bf16_f32:pro_prelu_no_slope": (-1, "ps_conv1x1_bf16_f32: prelu prologue needs slope"),
    "ps_conv1x1_bf16_f32:K_576_with_prologue": (-3,
        "ps_conv1x1_bf16_f32: K=576 exceeds the 512 input channels the prologue keeps tables for"),
    "ps_conv1x1_bf16_io:null_x": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=129)"),
    "ps_conv1x1_bf16_io:null_wt": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=129)"),
    "ps_conv1x1_bf16_io:null_y": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=129)"),
    "ps_conv1x1_bf16_io:N_zero": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=0 K=64 M=256 T=129)"),
    "ps_conv1x1_bf16_io:K_zero": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=0 M=256 T=129)"),
    "ps_conv1x1_bf16_io:M_zero": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=0 T=129)"),
    "ps_conv1x1_bf16_io:T_zero": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=0)"),
    "ps_conv1x1_bf16_io:T_negative": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=-1)"),
    "ps_conv1x1_bf16_io:ldt_below_T": (-2,
        "ps_conv1x1_bf16_f32: ldt=384 must be a multiple of 128 >= T=385, weights 16-byte aligned"),
    "ps_conv1x1_bf16_io:ldt_not_128": (-2,
        "ps_conv1x1_bf16_f32: ldt=200 must be a multiple of 128 >= T=129, weights 16-byte aligned"),
    "ps_conv1x1_bf16_io:wt_misaligned": (-2,
        "ps_conv1x1_bf16_f32: ldt=384 must be a multiple of 128 >= T=129, weights 16-byte aligned"),
    "ps_conv1x1_bf16_io:N_65536": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=65536 K=64 M=256 T=129)"),
    "ps_conv1x1_bf16_io:res_with_ostats": (-3,
        "ps_conv1x1_bf16_f32: residual and output statistics cannot be combined"),
    "ps_conv1x1_bf16_io:pro_global_incomplete": (-1,
        "ps_conv1x1_bf16_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_conv1x1_bf16_io:pro_affine_no_beta": (-1, "ps_conv1x1_bf16_f32: PS_NORM_AFFINE prologue needs gamma/beta"),
    "ps_conv1x1_bf16_io:pro_prelu_no_slope": (-1, "ps_conv1x1_bf16_f32: prelu prologue needs slope"),
    "ps_conv1x1_bf16_io:K_576_with_prologue": (-3,
        "ps_conv1x1_bf16_f32: K=576 exceeds the 512 input channels the prologue keeps tables for"),
    "ps_conv1x1_f16x2_f32:null_x": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=129)"),
    "ps_conv1x1_f16x2_f32:null_wt": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=129)"),
    "ps_conv1x1_f16x2_f32:null_y": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=129)"),
    "ps_conv1x1_f16x2_f32:N_zero": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=0 K=64 M=256 T=129)"),
    "ps_conv1x1_f16x2_f32:K_zero": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=0 M=256 T=129)"),
    "ps_conv1x1_f16x2_f32:M_zero": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=0 T=129)"),
    "ps_conv1x1_f16x2_f32:T_zero": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=0)"),
    "ps_conv1x1_f16x2_f32:T_negative": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=-1)"),
    "ps_conv1x1_f16x2_f32:ldt_below_T": (-2,
        "ps_conv1x1_bf16_f32: ldt=384 must be a multiple of 128 >= T=385, weights 16-byte aligned"),
    "ps_conv1x1_f16x2_f32:ldt_not_128": (-2,
        "ps_conv1x1_bf16_f32: ldt=200 must be a multiple of 128 >= T=129, weights 16-byte aligned"),
    "ps_conv1x1_f16x2_f32:wt_misaligned": (-2,
        "ps_conv1x1_bf16_f32: ldt=384 must be a multiple of 128 >= T=129, weights 16-byte aligned"),
    "ps_conv1x1_f16x2_f32:N_65536": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=65536 K=64 M=256 T=129)"),
    "ps_conv1x1_f16x2_f32:res_with_ostats": (-3,
        "ps_conv1x1_bf16_f32: residual and output statistics cannot be combined"),
    "ps_conv1x1_f16x2_f32:pro_global_incomplete": (-1,
        "ps_conv1x1_bf16_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_conv1x1_f16x2_f32:pro_affine_no_beta": (-1, "ps_conv1x1_bf16_f32: PS_NORM_AFFINE prologue needs gamma/beta"),
    "ps_conv1x1_f16x2_f32:pro_prelu_no_slope": (-1, "ps_conv1x1_bf16_f32: prelu prologue needs slope"),
    "ps_conv1x1_f16x2_f32:K_576_with_prologue": (-3,
        "ps_conv1x1_bf16_f32: K=576 exceeds the 512 input channels the prologue keeps tables for"),
    "ps_conv1x1_f16_rows:null_x": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=129)"),
    "ps_conv1x1_f16_rows:null_wt": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=129)"),
    "ps_conv1x1_f16_rows:null_y": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=129)"),
    "ps_conv1x1_f16_rows:N_zero": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=0 K=64 M=256 T=129)"),
    "ps_conv1x1_f16_rows:K_zero": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=0 M=256 T=129)"),
    "ps_conv1x1_f16_rows:M_zero": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=0 T=129)"),
    "ps_conv1x1_f16_rows:T_zero": (-1, "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=0)"),
    "ps_conv1x1_f16_rows:T_negative": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=-1)"),
    "ps_conv1x1_f16_rows:ldt_below_T": (-2,
        "ps_conv1x1_bf16_f32: ldt=384 must be a multiple of 128 >= T=385, weights 16-byte aligned"),
    "ps_conv1x1_f16_rows:ldt_not_128": (-2,
        "ps_conv1x1_bf16_f32: ldt=200 must be a multiple of 128 >= T=129, weights 16-byte aligned"),
    "ps_conv1x1_f16_rows:wt_misaligned": (-2,
        "ps_conv1x1_bf16_f32: ldt=384 must be a multiple of 128 >= T=129, weights 16-byte aligned"),
    "ps_conv1x1_f16_rows:N_65536": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=65536 K=64 M=256 T=129)"),
    "ps_conv1x1_f16_rows:res_with_ostats": (-3,
        "ps_conv1x1_bf16_f32: residual and output statistics cannot be combined"),
    "ps_conv1x1_f16_rows:pro_global_incomplete": (-1,
        "ps_conv1x1_bf16_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_conv1x1_f16_rows:pro_affine_no_beta": (-1, "ps_conv1x1_bf16_f32: PS_NORM_AFFINE prologue needs gamma/beta"),
    "ps_conv1x1_f16_rows:pro_prelu_no_slope": (-1, "ps_conv1x1_bf16_f32: prelu prologue needs slope"),
    "ps_conv1x1_f16_rows:K_576_with_prologue": (-3,
        "ps_conv1x1_bf16_f32: K=576 exceeds the 512 input channels the prologue keeps tables for"),
    "ps_conv1x1_f16x2_fmajor_f32:null_x": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=129)"),
    "ps_conv1x1_f16x2_fmajor_f32:null_wt": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=129)"),
    "ps_conv1x1_f16x2_fmajor_f32:null_y": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=129)"),
    "ps_conv1x1_f16x2_fmajor_f32:N_zero": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=0 K=64 M=256 T=129)"),
    "ps_conv1x1_f16x2_fmajor_f32:K_zero": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=0 M=256 T=129)"),
    "ps_conv1x1_f16x2_fmajor_f32:M_zero": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=0 T=129)"),
    "ps_conv1x1_f16x2_fmajor_f32:T_zero": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=0)"),
    "ps_conv1x1_f16x2_fmajor_f32:T_negative": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=2 K=64 M=256 T=-1)"),
    "ps_conv1x1_f16x2_fmajor_f32:ldt_below_T": (-2,
        "ps_conv1x1_bf16_f32: ldt=384 must be a multiple of 128 >= T=385, weights 16-byte aligned"),
    "ps_conv1x1_f16x2_fmajor_f32:ldt_not_128": (-2,
        "ps_conv1x1_bf16_f32: ldt=200 must be a multiple of 128 >= T=129, weights 16-byte aligned"),
    "ps_conv1x1_f16x2_fmajor_f32:wt_misaligned": (-2,
        "ps_conv1x1_bf16_f32: ldt=384 must be a multiple of 128 >= T=129, weights 16-byte aligned"),
    "ps_conv1x1_f16x2_fmajor_f32:N_65536": (-1,
        "ps_conv1x1_bf16_f32: null pointer or non-positive size (N=65536 K=64 M=256 T=129)"),
    "ps_conv1x1_f16x2_ln_f32:null_x": (-1,
        "ps_conv1x1_f16x2_ln_f32: null pointer or non-positive size (N=2 K=64 C=128 T=129)"),
    "ps_conv1x1_f16x2_ln_f32:null_wt": (-1,
        "ps_conv1x1_f16x2_ln_f32: null pointer or non-positive size (N=2 K=64 C=128 T=129)"),
    "ps_conv1x1_f16x2_ln_f32:null_y": (-1,
        "ps_conv1x1_f16x2_ln_f32: null pointer or non-positive size (N=2 K=64 C=128 T=129)"),
    "ps_conv1x1_f16x2_ln_f32:N_zero": (-1,
        "ps_conv1x1_f16x2_ln_f32: null pointer or non-positive size (N=0 K=64 C=128 T=129)"),
    "ps_conv1x1_f16x2_ln_f32:K_zero": (-1,
        "ps_conv1x1_f16x2_ln_f32: null pointer or non-positive size (N=2 K=0 C=128 T=129)"),
    "ps_conv1x1_f16x2_ln_f32:T_zero": (-1,
        "ps_conv1x1_f16x2_ln_f32: null pointer or non-positive size (N=2 K=64 C=128 T=0)"),
    "ps_conv1x1_f16x2_ln_f32:T_negative": (-1,
        "ps_conv1x1_f16x2_ln_f32: null pointer or non-positive size (N=2 K=64 C=128 T=-1)"),
    "ps_conv1x1_f16x2_ln_f32:ldt_below_T": (-3,
        "ps_conv1x1_f16x2_ln_f32: C = 128 channels, ldt a multiple of 128 >= T, 16-byte aligned parameters "
        "(ps_conv1x1_f16x2_ln_ok)"),
    "ps_conv1x1_f16x2_ln_f32:ldt_not_128": (-3,
        "ps_conv1x1_f16x2_ln_f32: C = 128 channels, ldt a multiple of 128 >= T, 16-byte aligned parameters "
        "(ps_conv1x1_f16x2_ln_ok)"),
    "ps_conv1x1_f16x2_ln_f32:wt_misaligned": (-3,
        "ps_conv1x1_f16x2_ln_f32: C = 128 channels, ldt a multiple of 128 >= T, 16-byte aligned parameters "
        "(ps_conv1x1_f16x2_ln_ok)"),
    "ps_conv1x1_f16x2_ln_f32:N_65536": (-1,
        "ps_conv1x1_f16x2_ln_f32: null pointer or non-positive size (N=65536 K=64 C=128 T=129)"),
    "ps_conv1x1_bf16_f32:planes_0": (-1,
        "ps_conv1x1_bf16_f32: planes must be 1 (bf16 products) or 3 (fp32-accurate 3-way split), got 0"),
    "ps_conv1x1_bf16_f32:planes_2": (-1,
        "ps_conv1x1_bf16_f32: planes must be 1 (bf16 products) or 3 (fp32-accurate 3-way split), got 2"),
    "ps_conv1x1_bf16_f32:planes_4": (-1,
        "ps_conv1x1_bf16_f32: planes must be 1 (bf16 products) or 3 (fp32-accurate 3-way split), got 4"),
    "ps_conv1x1_bf16_io:planes_0": (-1,
        "ps_conv1x1_bf16_f32: planes must be 1 (bf16 products) or 3 (fp32-accurate 3-way split), got 0"),
    "ps_conv1x1_bf16_io:planes_2": (-1,
        "ps_conv1x1_bf16_f32: planes must be 1 (bf16 products) or 3 (fp32-accurate 3-way split), got 2"),
    "ps_conv1x1_bf16_io:planes_4": (-1,
        "ps_conv1x1_bf16_f32: planes must be 1 (bf16 products) or 3 (fp32-accurate 3-way split), got 4"),
    "ps_conv1x1_bf16_io:bf16_rows_planes_3": (-3,
        "ps_conv1x1_bf16_io: bf16 activation rows go with planes = 1 (got 3)"),
    "ps_conv1x1_bf16_io:bf16_x_planes_3": (-3, "ps_conv1x1_bf16_io: bf16 activation rows go with planes = 1 (got 3)"),
    "ps_conv1x1_f16x2_f32:range_null": (-1,
        "ps_conv1x1_f16x2_f32: range descriptor missing or out of range (w_exp within +-100, x_bound >= 0)"),
    "ps_conv1x1_f16x2_f32:range_w_exp": (-1,
        "ps_conv1x1_f16x2_f32: range descriptor missing or out of range (w_exp within +-100, x_bound >= 0)"),
    "ps_conv1x1_f16x2_f32:range_negative_bound": (-1,
        "ps_conv1x1_f16x2_f32: range descriptor missing or out of range (w_exp within +-100, x_bound >= 0)"),
    "ps_conv1x1_f16x2_f32:range_amax_parts": (-1,
        "ps_conv1x1_f16x2_f32: range descriptor missing or out of range (w_exp within +-100, x_bound >= 0)"),
    "ps_conv1x1_f16x2_fmajor_f32:range_null": (-1,
        "ps_conv1x1_f16x2_fmajor_f32: range descriptor missing or out of range (w_exp within +-100, x_bound "
        ">= 0)"),
    "ps_conv1x1_f16x2_fmajor_f32:range_w_exp": (-1,
        "ps_conv1x1_f16x2_fmajor_f32: range descriptor missing or out of range (w_exp within +-100, x_bound "
        ">= 0)"),
    "ps_conv1x1_f16x2_fmajor_f32:range_negative_bound": (-1,
        "ps_conv1x1_f16x2_fmajor_f32: range descriptor missing or out of range (w_exp within +-100, x_bound "
        ">= 0)"),
    "ps_conv1x1_f16x2_fmajor_f32:range_amax_parts": (-1,
        "ps_conv1x1_f16x2_fmajor_f32: range descriptor missing or out of range (w_exp within +-100, x_bound "
        ">= 0)"),
    "ps_conv1x1_f16x2_ln_f32:range_null": (-1,
        "ps_conv1x1_f16x2_ln_f32: range descriptor missing or out of range (w_exp within +-100, x_bound >= 0)"),
    "ps_conv1x1_f16x2_ln_f32:range_w_exp": (-1,
        "ps_conv1x1_f16x2_ln_f32: range descriptor missing or out of range (w_exp within +-100, x_bound >= 0)"),
    "ps_conv1x1_f16x2_ln_f32:range_negative_bound": (-1,
        "ps_conv1x1_f16x2_ln_f32: range descriptor missing or out of range (w_exp within +-100, x_bound >= 0)"),
    "ps_conv1x1_f16x2_ln_f32:range_amax_parts": (-1,
        "ps_conv1x1_f16x2_ln_f32: range descriptor missing or out of range (w_exp within +-100, x_bound >= 0)"),
    "ps_conv1x1_f16_rows:range_null": (-1,
        "ps_conv1x1_f16_rows: range descriptor missing or incomplete (w_exp within +-100 and x_bound > 0 or "
        "x_amax)"),
    "ps_conv1x1_f16_rows:range_w_exp": (-1,
        "ps_conv1x1_f16_rows: range descriptor missing or incomplete (w_exp within +-100 and x_bound > 0 or "
        "x_amax)"),
    "ps_conv1x1_f16_rows:range_negative_bound": (-1,
        "ps_conv1x1_f16_rows: range descriptor missing or incomplete (w_exp within +-100 and x_bound > 0 or "
        "x_amax)"),
    "ps_conv1x1_f16_rows:range_amax_parts": (-1,
        "ps_conv1x1_f16_rows: range descriptor missing or incomplete (w_exp within +-100 and x_bound > 0 or "
        "x_amax)"),
    "ps_conv1x1_f16_rows:range_no_source": (-1,
        "ps_conv1x1_f16_rows: range descriptor missing or incomplete (w_exp within +-100 and x_bound > 0 or "
        "x_amax)"),
    "ps_conv1x1_f16x2_fmajor_f32:ldm_below_M": (-1,
        "ps_conv1x1_f16x2_fmajor_f32: ldm=252 must be a multiple of 4 >= M=256"),
    "ps_conv1x1_f16x2_fmajor_f32:ldm_not_4": (-1,
        "ps_conv1x1_f16x2_fmajor_f32: ldm=258 must be a multiple of 4 >= M=256"),
    "ps_conv1x1_f16x2_ln_f32:C_64": (-3,
        "ps_conv1x1_f16x2_ln_f32: C = 128 channels, ldt a multiple of 128 >= T, 16-byte aligned parameters "
        "(ps_conv1x1_f16x2_ln_ok)"),
    "ps_conv1x1_f16x2_ln_f32:null_gamma": (-1,
        "ps_conv1x1_f16x2_ln_f32: null pointer or non-positive size (N=2 K=64 C=128 T=129)"),
    "ps_conv1x1_f16x2_ln_f32:pro_pre_relu": (-3,
        "ps_conv1x1_f16x2_ln_f32: the prologue may be a per-channel affine map and / or a PReLU (a ReLU is "
        "the PReLU of slope 0)"),
    "ps_conv1x1_f16x2_ln_f32:pro_global": (-3,
        "ps_conv1x1_f16x2_ln_f32: the prologue may be a per-channel affine map and / or a PReLU (a ReLU is "
        "the PReLU of slope 0)"),
    "ps_conv1x1_f16x2_ln_f32:pro_prelu_no_slope": (-3,
        "ps_conv1x1_f16x2_ln_f32: the prologue may be a per-channel affine map and / or a PReLU (a ReLU is "
        "the PReLU of slope 0)"),
    "ps_conv1x1_f16x2_ln_f32:K_576_with_prologue": (-3,
        "ps_conv1x1_f16x2_ln_f32: the prologue may be a per-channel affine map and / or a PReLU (a ReLU is "
        "the PReLU of slope 0)"),
}


def test_the_table_and_the_recorded_answers_name_the_same_cases():
    assert sorted(f"{e}:{k}" for e, k, _ in CASES) == sorted(EXPECTED) and len(EXPECTED) == len(CASES)


@pytest.mark.parametrize("entry,case,overrides", CASES, ids=[f"{e}:{k}" for e, k, _ in CASES])
def test_gemm_entry_refuses_before_any_launch(entry, case, overrides):
    assert refuse(entry, overrides) == EXPECTED[f"{entry}:{case}"]


# ---- packers ---------------------------------------------------------------------------------------------------------
def _weight(*shape):
    """seeded, with magnitudes over several binades so that every plane of a split is populated"""
    r = np.random.RandomState(sum(shape) * 7919 + len(shape))
    w = r.standard_normal(shape) * np.exp2(r.randint(-6, 3, size=shape))
    return torch.from_numpy(w.astype(np.float32))


def _sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def packed(name, *shape):
    """-> [hash of the image, exponent / scales] (or [hash] alone)"""
    if name == "bf16x1":
        return [_sha(hip.pack_wt_bf16(_weight(*shape), 1))]
    if name == "bf16x3":
        return [_sha(hip.pack_wt_bf16(_weight(*shape).unsqueeze(2), 3))]
    if name == "whh":
        h, = shape
        img, scales = hip.pack_whh_h256(_weight(2, h, 4 * h))
        return [_sha(img), [float(s) for s in scales]]
    img, w_exp = (hip.pack_wt_f16x2 if name == "f16x2" else hip.pack_conv2d_f16x2)(_weight(*shape))
    return [_sha(img), int(w_exp)]


PACK_CASES = ([(n, m, k) for n in ("bf16x1", "bf16x3", "f16x2") for m in (1, 255, 256, 257) for k in (1, 15, 16, 33)]
              + [("whh", 192), ("whh", 256)] + [("conv2d", m, k) for m in (32, 33, 65) for k in (1, 15, 16, 33)])
PACKED = {
    "bf16x1-1-1": ["210db4a0f78414507eaf47e42b9998f2645aa74d6865c348b823279eb3cac1c7"],
    "bf16x1-1-15": ["b4becc40dbd937276c389e2c66d35d67e50299c2cedeefc55639a246f02964ab"],
    "bf16x1-1-16": ["0ff17b2790e49a24e3e9742720e7ea2abda997ec77d773fc81af209dc8c9f828"],
    "bf16x1-1-33": ["434e55bb8524b67eb037f2adcf052a108604a4b94f562d60408dc54dcd966191"],
    "bf16x1-255-1": ["ee0699c07f54f8d45f35a23ed6d6018a9481832061a769515ecddd55f8887f62"],
    "bf16x1-255-15": ["25a22f69160b21d6c3977382db627fc0ed30512cde2ce82edb52e863f2019bc3"],
    "bf16x1-255-16": ["1acec343e0cd8fa9de267e6bdc473f8a3ec79525a1e1c8bd364a3673752e6d14"],
    "bf16x1-255-33": ["8b961d13ba4273a5d5ec12bb014af2ff54bf79cdf1912a01d0e13d526199afb6"],
    "bf16x1-256-1": ["0565799fcc4e8e67fcceaf1b920042ea863ecf017235b633da92f9826421b5bb"],
    "bf16x1-256-15": ["530f33d31af71b043c67dfd4d7f197f242fa202d02c28a74391f0151009faa34"],
    "bf16x1-256-16": ["81aa50eab7e6d29b1e26b5fb9a4c4d17c8186ca701bb406ff81e5263d534e6c5"],
    "bf16x1-256-33": ["398492b2e98e31c4d5971750f98e3b29ec85fc525d456708cc686d301db349a6"],
    "bf16x1-257-1": ["6985c38dca333ccd19982a6a37fe2f7869ae0913166372a9cb8b8f45e41330c6"],
    "bf16x1-257-15": ["10f1573d6d4475ce25f4b72f9661ac3981f3f0b398e226f86821c508357c05ba"],
    "bf16x1-257-16": ["5fd67fc51909d039aaedc8e6239b5f58ae0f18604925840ed11759da80167beb"],
    "bf16x1-257-33": ["c7b0e7d1e8543ec49fffd0ed23b2c2ec4cfe89e5f248fa13821f18908a239b7e"],
    "bf16x3-1-1": ["b22de83b0329e61923643a99e4a8239a804eefe33f600176bd645efd6c17467b"],
    "bf16x3-1-15": ["71d13e5e004730ad8288d7ef380b45f368e6325a97496014348ad0b3bbffd61a"],
    "bf16x3-1-16": ["3a78f7b02bcb5dbe14da77c51af1b95fed6cfc13d8d8aeb127209f5aa21ee35e"],
    "bf16x3-1-33": ["c0461bac5c4e7cf4df4730eddedf72bbe87d81447500dadf8df54ddbf084bbc4"],
    "bf16x3-255-1": ["546008dd40f299e719ffa25ec705a8e94a7b97bfe7cce4d523452da05489a079"],
    "bf16x3-255-15": ["fc859ed7c9ac22438a6d83b1c09d0217d4e1c5a426118a866567dacd688076b1"],
    "bf16x3-255-16": ["93f94d07a08cb7267df3f56687770a0a256e3c09fb1cc8aaf62f16dc9e441595"],
    "bf16x3-255-33": ["cb3d39682a5bb267394c506bba80a711bc5d1a3de16435b168c12d5ec8625509"],
    "bf16x3-256-1": ["ecc75e6bb747e6e8bf15f40d18f628ae36e3ce7db34e7901e24bdc35feab0fbc"],
    "bf16x3-256-15": ["d1a58588c6375d9d8815a70cdc6811d5f2323c0d6fcd7343ff73e2a4c088def8"],
    "bf16x3-256-16": ["a39ee8ca919f7db0bc5be92670b601b86194cb1840499cb0ff388701f1091cfd"],
    "bf16x3-256-33": ["7fa01d2ded0fe4e24c4232ef628ab78df9f5b6841b4cb544003c8642a4590ab0"],
    "bf16x3-257-1": ["1ca6039d6619dbbd43f8a1732feb99a01077d98282458c4048915b0f21d188a2"],
    "bf16x3-257-15": ["a0e26ff6c8e23f5a62a649190a73d0d1b9bcb829ec52703b1d2d6174f9ae246a"],
    "bf16x3-257-16": ["925e5cc76f08878f330eb61069cd91b3c62d32b46947f2e3d688ac5479f183ac"],
    "bf16x3-257-33": ["d69edcbcd3908be0eba0ab5d979fb0f5f1395c3b012cb6336c03964af41e7623"],
    "f16x2-1-1": ["6dd1dfdeae92447c45d5c4abf1122fd8668322c138a8ea3a63b32d095611dc6e", 12],
    "f16x2-1-15": ["0edc3853b8b70b8bb58a39a13000216e00c0698be28dd877f4682245016f55fe", 12],
    "f16x2-1-16": ["7d244e0590f2e23688a501f7e173fea2108c1a06e321afa0012a72f0441ba05c", 11],
    "f16x2-1-33": ["1cca53205260b0504ba92fc275d2bd58fd08c83bbad01d6f91d2640c1739735d", 11],
    "f16x2-255-1": ["4cbdfe0dc20cb25f391d3a97af372153da783dde3efe7f56b30b1e0a256aa7c7", 10],
    "f16x2-255-15": ["732dfda540e2c38430276c74f0c3858ae36cbd8b8f2a797cb29f3028b1ec8606", 10],
    "f16x2-255-16": ["9d421a6b9f0b7fd5256fd3f70a380faeb21684e8de88b3a60dec73e8e0b5f010", 10],
    "f16x2-255-33": ["7b40d620507b47ddf335f1b6a28bae41b738ece7667e20e623074cde083c79b7", 10],
    "f16x2-256-1": ["3614f5bd90fc5e84fc6e8dbdbbde5674987beae881c3f071fd54f545d54baf72", 11],
    "f16x2-256-15": ["0d504ed1d9679bd71686c72e34d692cb523f33037e64e02cc9f9131784f194bf", 10],
    "f16x2-256-16": ["cac590ddcb3467572e69f64c9158dca3c891d7e2220310c0402ea7cac7f13940", 10],
    "f16x2-256-33": ["68eeea135fe6df03407857be64d0ed4b309d6e646f9f38b112702790131622be", 10],
    "f16x2-257-1": ["5724d2ffb5881353321025ae37308e56e6b4eabd56ddb7d4945e8e8181e98e4d", 10],
    "f16x2-257-15": ["d9d8ac73edf883121f8c2f49f87764d0dd6b8b5c51f65dd39d9b6600c3d4352b", 10],
    "f16x2-257-16": ["219be62c81f6261fef28851bb560d6bfb409746cf07c4e163c6cb9e87a4e8cd4", 10],
    "f16x2-257-33": ["21f1559ddc49c92d22722088268fa67988a4c5872af499a3cca22c9da7b7cb02", 10],
    "whh-192": ["7110ba5ad8e405639b4149ccebc596e86a841b3681d24ee255d590faac37b6e3", [524288.0, 524288.0]],
    "whh-256": ["e4e38005a79e95ed7d6a952e8db0276c850cb5194a62f90495254e614f42c7d1", [262144.0, 262144.0]],
    "conv2d-32-1": ["757d3ab28a61dfb51f92a97b06c4e90e1f91127f2a1ddaa5df40faafa7d5fd1a", 11],
    "conv2d-32-15": ["4932bb538f436345927afc23700bd944a09a6f5b9c7ba8ac9250dbbfb5c1702f", 10],
    "conv2d-32-16": ["f52f05ff3d1b171d18c99c44f7fc0c1e529dd0abdfe6d71b54d3138aa4c28cb0", 10],
    "conv2d-32-33": ["eb9da9bc499d614d5295cb1e9a4c5695ecd700f7b6f305fd7088f7dce5fefac3", 10],
    "conv2d-33-1": ["9b7a2021a3780239b227eb035ba6bad0a40ee3b031910609542aff3552aab00a", 11],
    "conv2d-33-15": ["1fc46579babbb42ddb2655612b0cbd438ae10663d135cbeb09f7cbd073bd4196", 11],
    "conv2d-33-16": ["036c08c9ade1d63789c618bb833d9ad599c664052ee8753fc1ed66554e8fd2f8", 10],
    "conv2d-33-33": ["587f9efe490178fbbf14e5d78ff1b4e2c1c70a6eb24408a33265e95a0524ea8a", 10],
    "conv2d-65-1": ["f40497fbdc0fbc2fe2400750310882a59c07255369ca23a388614e1f22280e08", 10],
    "conv2d-65-15": ["2c9fda579a93dd0b2ba77d23830cb73d9714b5b9b72063906c25c7e6350b1377", 10],
    "conv2d-65-16": ["a6fa7b3ad6293c5447a616abbdce8f69b8a115f21b4893311da029b45670f106", 10],
    "conv2d-65-33": ["1432c67e879768dc421057b78793e458a6167a644d95bc19ed0fa2cdf607e6f6", 10],
}


@pytest.mark.parametrize("case", PACK_CASES, ids=["-".join(map(str, c)) for c in PACK_CASES])
def test_packed_weight_images_are_bit_identical(case):
    """Hashes and exponents / scales recorded from commit ad87148's hip.py on the CPU."""
    assert packed(*case) == PACKED["-".join(map(str, case))]


def test_packers_refuse_inf_and_nan_by_name():
    for fn, who in ((hip.pack_wt_f16x2, "pack_wt_f16x2"), (hip.pack_conv2d_f16x2, "pack_conv2d_f16x2")):
        for bad in (float("inf"), float("nan")):
            w = _weight(3, 5)
            w[1, 2] = bad
            with pytest.raises(ValueError, match=f"^{who}: the weight holds inf / NaN$"):
                fn(w)
    w = _weight(1, 192, 768)
    w[0, 0, 0] = float("nan")
    with pytest.raises(ValueError, match="^pack_whh_h256: the weight holds inf / NaN$"):
        hip.pack_whh_h256(w)
    zero, w_exp = hip.pack_wt_f16x2(torch.zeros(4, 4))
    assert w_exp == 0 and not zero.any()
