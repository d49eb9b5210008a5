"""What the depthwise-conv, encoder / decoder and conv2d entries refuse, and what their predicates and sizers answer -- both
without a GPU.

Refusals: every row of CASES calls one entry with arguments it must turn down before any launch; the return code and the
whole ps_last_error() text are compared.  Non-null pointers are aligned host buffers that are never dereferenced (the call
returns first), so every row has to BE a refusal: a call these entries accept would launch on those buffers.  That is why
the table holds no ps_free_decode_ws_f32 row whose shape the matrix-pipe predicate rejects and ps_free_decode_f32 then
accepts, and why the bf16 rows of ps_dwconv_io outside the wave-private kernel use a halo beyond the small build.

Values: GRIDS calls the five predicates / sizers over points on both sides of every threshold.

EXPECTED and VALUES were recorded from commit 58cc688 (the library built from it).  Four kinds of row record that commit's
return code with the text of the commit that gave these entries one check path; each carries a comment:
- the prologue defects of the three dwconv entries (check_prologue's messages);
- ps_free_decode_ws_f32's own "bad argument" (ps_free_decode_f32's form, with win / hop);
- ps_conv2d_f16x2_f32's Kp and 2^30 limits (the fp32 entry's two messages)."""
import ctypes as C
import itertools

import pytest

from puresound_amd import _abi

_BUF = C.create_string_buffer(4096 + 256)
BUF = (C.addressof(_BUF) + 255) // 256 * 256   # aligned host memory; BUF + 4 etc. are the misaligned pointers

_DW = dict(x=BUF, x_bf16=0, w=BUF, b=None, y=BUF, y_bf16=0, N=2, H=4, T=100, ldt=128, P=3, dilation=2, left=2, pro=None,
           ostats=None, y_amax=BUF, stream=None)
_DW_ARGS = "x w b y N H T ldt P dilation left pro"
_ENC = dict(wav=BUF, w=BUF, feats=BUF, N=2, L=1000, C=8, win=32, hop=16, T=61, ldt=128, relu=0, stream=None)
_DEC = dict(feats=BUF, mask=None, mask_act=0, w=BUF, out=BUF, N=2, C=16, T=64, ldt=128, win=32, hop=16, out_mode=2,
            workspace=BUF, workspace_bytes=4096, ref=BUF, ldr=1100, ref_len=1040, partials=BUF, stream=None)
_DEC_ARGS = "feats mask mask_act w out N C T ldt win hop out_mode"
_ROWS = dict(src=BUF, dst=BUF, rows=4, T=100, ldt=128, stream=None)
_C2D = dict(x1=BUF, C1=2, x2=None, C2=0, wt=BUF, wimg=BUF, w_exp=0, bias=None, y=BUF, N=1, M=4, Fin=8, T_in=100, T=100, ld=128,
            kf=3, kt=2, stride_f=1, dil_f=1, dil_t=1, pad_f=1, pad_t=1, Fout=8, transposed=0, act=0, slope=None, ostats=BUF,
            stream=None)
_C2D_GEOMETRY = "N M Fin T_in T ld kf kt stride_f dil_f dil_t pad_f pad_t Fout transposed"
# entry -> (arguments in call order, defaults of a valid call)
ENTRIES = {
    "ps_dwconv_f32": (_DW_ARGS + " ostats stream", _DW),
    "ps_dwconv_io": ("x x_bf16 w b y y_bf16 N H T ldt P dilation left pro ostats stream", _DW),
    "ps_dwconv_amax_f32": (_DW_ARGS + " y_amax stream", _DW),
    "ps_free_encode_f32": ("wav w feats N L C win hop T ldt relu stream", _ENC),
    "ps_free_decode_f32": (_DEC_ARGS + " stream", _DEC),
    "ps_free_decode_ws_f32": (_DEC_ARGS + " workspace workspace_bytes stream", _DEC),
    "ps_free_decode_moments_f32": (_DEC_ARGS + " ref ldr ref_len partials workspace workspace_bytes stream", _DEC),
    "ps_pad_rows_f32": ("src dst rows T ldt stream", _ROWS),
    "ps_unpad_rows_f32": ("src dst rows T ldt stream", _ROWS),
    "ps_conv2d_f32": ("x1 C1 x2 C2 wt bias y " + _C2D_GEOMETRY + " act slope stream", _C2D),
    "ps_conv2d_stats_f32": ("x1 C1 x2 C2 wt bias y " + _C2D_GEOMETRY + " ostats stream", _C2D),
    "ps_conv2d_f16x2_f32": ("x1 C1 x2 C2 wimg w_exp bias y " + _C2D_GEOMETRY + " act slope ostats stream", _C2D),
}
GLOBAL, AFFINE = _abi.PS_NORM_GLOBAL, _abi.PS_NORM_AFFINE
_PRO = dict(norm=GLOBAL, prelu=1, stats=BUF, parts=4, count=400.0, eps=1e-8, gamma=BUF, beta=BUF, slope=BUF)


def _cases():
    out = []
    for e in ("ps_dwconv_f32", "ps_dwconv_io", "ps_dwconv_amax_f32"):
        out += [(e, f"null_{k}", {k: None}) for k in ("x", "w", "y")]
        out += [(e, f"{k}_zero", {k: 0}) for k in ("N", "H", "T", "P", "dilation")]
        out += [(e, "P_9", dict(P=9, left=0)), (e, "left_negative", dict(left=-1)),
                (e, "left_beyond_the_receptive_field", dict(left=5)), (e, "halo_beyond_the_tile", dict(dilation=509)),
                (e, "ldt_below_T", dict(T=129)), (e, "ldt_192", dict(ldt=192)), (e, "x_misaligned", dict(x=BUF + 4)),
                (e, "y_misaligned", dict(y=BUF + 8))]
        out += [(e, f"global_prologue_{k}", dict(pro=dict(_PRO, **{k: 0}))) for k in ("stats", "parts", "count", "gamma", "beta")]
        out += [(e, f"affine_prologue_{k}", dict(pro=dict(_PRO, norm=AFFINE, **{k: 0}))) for k in ("gamma", "beta")]
        out += [(e, "prelu_prologue_slope", dict(pro=dict(_PRO, norm=0, slope=0))),
                (e, "norm_3_prologue_gamma", dict(pro=dict(_PRO, norm=3, gamma=0)))]
    e = "ps_dwconv_io"
    out += [(e, "bf16_in_P_5", dict(x_bf16=1, P=5, left=4)), (e, "bf16_out_P_5", dict(y_bf16=1, P=5, left=4)),
            (e, "bf16_rows_P_2", dict(x_bf16=1, y_bf16=1, P=2)),
            (e, "bf16_in_halo_beyond_the_small_build", dict(x_bf16=1, dilation=141)),
            (e, "bf16_out_halo_beyond_the_small_build", dict(y_bf16=1, dilation=141)),
            (e, "bf16_rows_halo_beyond_the_small_build", dict(x_bf16=1, y_bf16=1, dilation=141))]
    e = "ps_dwconv_amax_f32"
    out += [(e, "null_y_amax", dict(y_amax=None)), (e, "P_5", dict(P=5)), (e, "P_2", dict(P=2)),
            (e, "dilation_129", dict(dilation=129)), (e, "left_beyond_two_dilations", dict(left=5))]
    e = "ps_free_encode_f32"
    out += [(e, f"null_{k}", {k: None}) for k in ("wav", "w", "feats")]
    out += [(e, f"{k}_zero", {k: 0}) for k in ("N", "C", "win", "hop")]
    out += [(e, "L_below_win", dict(L=16)), (e, "T_60", dict(T=60)), (e, "ldt_below_T", dict(ldt=0)), (e, "ldt_192", dict(ldt=192))]
    for e in ("ps_free_decode_f32", "ps_free_decode_ws_f32"):
        out += [(e, f"null_{k}", {k: None}) for k in ("feats", "w", "out")]
        out += [(e, f"{k}_zero", {k: 0}) for k in ("N", "C", "T", "win", "hop")]
        out += [(e, "ldt_below_T", dict(ldt=32))]
    for e in ("ps_free_decode_f32", "ps_free_decode_ws_f32", "ps_free_decode_moments_f32"):
        out += [(e, "mask_act_minus_1", dict(mask_act=-1)), (e, "mask_act_3", dict(mask_act=3)),
                (e, "out_mode_minus_1", dict(out_mode=-1)), (e, "out_mode_3", dict(out_mode=3))]
    e = "ps_free_decode_ws_f32"   # (without the workspace the call is ps_free_decode_f32's)
    out += [(e, "no_workspace_null_feats", dict(workspace=None, feats=None)), (e, "no_workspace_mask_act_3", dict(workspace=None, mask_act=3))]
    e = "ps_free_decode_moments_f32"
    out += [(e, "T_63", dict(T=63)), (e, "C_8", dict(C=8)), (e, "C_zero", dict(C=0)), (e, "N_zero", dict(N=0)),
            (e, "N_65536", dict(N=65536)), (e, "win_16_hop_8", dict(win=16, hop=8)), (e, "ldt_below_T", dict(ldt=32)),
            (e, "utterance_2GiB", dict(C=4194304))]
    out += [(e, f"null_{k}", {k: None}) for k in ("feats", "w", "out", "ref", "partials", "workspace")]
    out += [(e, "ref_len_zero", dict(ref_len=0)), (e, "ldr_below_ref_len", dict(ldr=1039)), (e, "short_workspace", dict(workspace_bytes=383)),
            (e, "out_misaligned", dict(out=BUF + 4)), (e, "workspace_misaligned", dict(workspace=BUF + 8))]
    for e in ("ps_pad_rows_f32", "ps_unpad_rows_f32"):
        out += [(e, "null_src", dict(src=None)), (e, "null_dst", dict(dst=None)), (e, "rows_zero", dict(rows=0)),
                (e, "T_zero", dict(T=0)), (e, "ldt_below_T", dict(ldt=99)), (e, "rows_2_31", dict(rows=1 << 31))]
    for e, w in (("ps_conv2d_f32", "wt"), ("ps_conv2d_stats_f32", "wt"), ("ps_conv2d_f16x2_f32", "wimg")):
        out += [(e, f"null_{k}", {k: None}) for k in ("x1", w, "y")]
        out += [(e, f"{k}_zero", {k: 0}) for k in ("N", "M", "C1", "Fin", "Fout", "T", "T_in", "kf", "kt", "stride_f", "dil_f", "dil_t")]
        out += [(e, "C2_negative", dict(C2=-1)), (e, "C2_without_x2", dict(C2=2)), (e, "ld_below_T", dict(ld=0)),
                (e, "ld_below_T_in", dict(T_in=200)), (e, "ld_192", dict(ld=192)), (e, "Fout_65536", dict(Fout=65536)),
                (e, "Kp_4200", dict(C1=700)), (e, "utterance_2_30_elements", dict(C1=128, Fin=65536)),
                (e, "grid_limit", dict(N=65536))]
    for e in ("ps_conv2d_f32", "ps_conv2d_f16x2_f32"):
        out += [(e, "act_minus_1", dict(act=-1)), (e, "act_6", dict(act=6)), (e, "prelu_without_slope", dict(act=2))]
    e = "ps_conv2d_f16x2_f32"
    out += [(e, "w_exp_101", dict(w_exp=101)), (e, "w_exp_minus_101", dict(w_exp=-101)), (e, "wimg_misaligned", dict(wimg=BUF + 8))]
    out += [("ps_conv2d_stats_f32", "null_ostats", dict(ostats=None))]
    return out


CASES = _cases()


def refuse(entry, overrides):
    names, defaults = ENTRIES[entry]
    a = dict(defaults, **overrides)
    if a.get("pro"):
        pro = _abi.Prologue()
        for k, v in a["pro"].items():
            setattr(pro, k, None if v == 0 and k in ("stats", "gamma", "beta", "slope") else v)
        a["pro"] = C.byref(pro)
    lib = _abi.lib()
    rc = getattr(lib, entry)(*[a[k] for k in names.split()])
    return rc, lib.ps_last_error().decode()


# ---- the predicates and sizers -----------------------------------------------------------------------------------------
GRIDS = {
    "ps_dwconv_amax_ok": [(p, d, left) for p in (2, 3, 5) for d in (0, 1, 4, 127, 128, 129)
                          for left in (-1, 0, d, 2 * d, 2 * d + 1)],
    "ps_dwconv_stats_parts": list(itertools.product((0, 1, 16, 17), (0, 1, 1024, 1025))),
    "ps_free_decode_workspace_bytes": list(itertools.product((0, 1, 65535, 65536), (0, 63, 64, 65), (32, 16), (16, 8))),
    # N, C (odd and even against 2 * DM_UC = 16), T, ldt (below T, above), win, hop; then the longer rows and the 2 GiB limit
    "ps_free_decode_moments_parts": [p + wh for p in itertools.product((0, 1, 65535, 65536), (0, 8, 15, 16, 17, 32), (63, 64),
                                                                        (32, 128)) for wh in ((32, 16), (16, 8))]
                                    + [(2, 16, t, 128, 32, 16) for t in (65, 96, 97, 128, 129)]
                                    + [(1, 4194304 - 16, 64, 128, 32, 16), (1, 4194304, 64, 128, 32, 16)],
    "ps_conv2d_stats_parts": list(itertools.product((0, 1, 32, 33, 64, 65, 128, 129), (0, 1, 5), (0, 128, 192, 384))),
}
POINTS = [(f, p) for f, grid in GRIDS.items() for p in grid]


def value(fn, point):
    return getattr(_abi.lib(), fn)(*point)


EXPECTED = {
    "ps_dwconv_f32:null_x": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=100 P=3 dilation=2 left=2)"),
    "ps_dwconv_f32:null_w": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=100 P=3 dilation=2 left=2)"),
    "ps_dwconv_f32:null_y": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=100 P=3 dilation=2 left=2)"),
    "ps_dwconv_f32:N_zero": (-1, "ps_dwconv_f32: bad argument (N=0 H=4 T=100 P=3 dilation=2 left=2)"),
    "ps_dwconv_f32:H_zero": (-1, "ps_dwconv_f32: bad argument (N=2 H=0 T=100 P=3 dilation=2 left=2)"),
    "ps_dwconv_f32:T_zero": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=0 P=3 dilation=2 left=2)"),
    "ps_dwconv_f32:P_zero": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=100 P=0 dilation=2 left=2)"),
    "ps_dwconv_f32:dilation_zero": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=100 P=3 dilation=0 left=2)"),
    "ps_dwconv_f32:P_9": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=100 P=9 dilation=2 left=0)"),
    "ps_dwconv_f32:left_negative": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=100 P=3 dilation=2 left=-1)"),
    "ps_dwconv_f32:left_beyond_the_receptive_field": (-1, "ps_dwconv_f32: left=5 exceeds the receptive field (P-1)*dilation=4"),
    "ps_dwconv_f32:halo_beyond_the_tile": (-3,
        "ps_dwconv_f32: (P-1)*dilation=1018 exceeds the 1016-frame halo the LDS tile holds"),
    "ps_dwconv_f32:ldt_below_T": (-2, "ps_dwconv_f32: ldt=128 must be a multiple of 128 >= T=129 and pointers 16-byte aligned"),
    "ps_dwconv_f32:ldt_192": (-2, "ps_dwconv_f32: ldt=192 must be a multiple of 128 >= T=100 and pointers 16-byte aligned"),
    "ps_dwconv_f32:x_misaligned": (-2, "ps_dwconv_f32: ldt=128 must be a multiple of 128 >= T=100 and pointers 16-byte aligned"),
    "ps_dwconv_f32:y_misaligned": (-2, "ps_dwconv_f32: ldt=128 must be a multiple of 128 >= T=100 and pointers 16-byte aligned"),
    "ps_dwconv_f32:global_prologue_stats": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_dwconv_f32:global_prologue_parts": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_dwconv_f32:global_prologue_count": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_dwconv_f32:global_prologue_gamma": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_dwconv_f32:global_prologue_beta": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_dwconv_f32:affine_prologue_gamma": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_AFFINE prologue needs gamma/beta"),
    "ps_dwconv_f32:affine_prologue_beta": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_AFFINE prologue needs gamma/beta"),
    "ps_dwconv_f32:prelu_prologue_slope": (-1, "ps_dwconv_f32: prelu prologue needs slope"),
    "ps_dwconv_f32:norm_3_prologue_gamma": (-1, "ps_dwconv_f32: norm prologue needs gamma/beta"),
    "ps_dwconv_io:null_x": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=100 P=3 dilation=2 left=2)"),
    "ps_dwconv_io:null_w": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=100 P=3 dilation=2 left=2)"),
    "ps_dwconv_io:null_y": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=100 P=3 dilation=2 left=2)"),
    "ps_dwconv_io:N_zero": (-1, "ps_dwconv_f32: bad argument (N=0 H=4 T=100 P=3 dilation=2 left=2)"),
    "ps_dwconv_io:H_zero": (-1, "ps_dwconv_f32: bad argument (N=2 H=0 T=100 P=3 dilation=2 left=2)"),
    "ps_dwconv_io:T_zero": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=0 P=3 dilation=2 left=2)"),
    "ps_dwconv_io:P_zero": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=100 P=0 dilation=2 left=2)"),
    "ps_dwconv_io:dilation_zero": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=100 P=3 dilation=0 left=2)"),
    "ps_dwconv_io:P_9": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=100 P=9 dilation=2 left=0)"),
    "ps_dwconv_io:left_negative": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=100 P=3 dilation=2 left=-1)"),
    "ps_dwconv_io:left_beyond_the_receptive_field": (-1, "ps_dwconv_f32: left=5 exceeds the receptive field (P-1)*dilation=4"),
    "ps_dwconv_io:halo_beyond_the_tile": (-3,
        "ps_dwconv_f32: (P-1)*dilation=1018 exceeds the 1016-frame halo the LDS tile holds"),
    "ps_dwconv_io:ldt_below_T": (-2, "ps_dwconv_f32: ldt=128 must be a multiple of 128 >= T=129 and pointers 16-byte aligned"),
    "ps_dwconv_io:ldt_192": (-2, "ps_dwconv_f32: ldt=192 must be a multiple of 128 >= T=100 and pointers 16-byte aligned"),
    "ps_dwconv_io:x_misaligned": (-2, "ps_dwconv_f32: ldt=128 must be a multiple of 128 >= T=100 and pointers 16-byte aligned"),
    "ps_dwconv_io:y_misaligned": (-2, "ps_dwconv_f32: ldt=128 must be a multiple of 128 >= T=100 and pointers 16-byte aligned"),
    "ps_dwconv_io:global_prologue_stats": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_dwconv_io:global_prologue_parts": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_dwconv_io:global_prologue_count": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_dwconv_io:global_prologue_gamma": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_dwconv_io:global_prologue_beta": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_dwconv_io:affine_prologue_gamma": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_AFFINE prologue needs gamma/beta"),
    "ps_dwconv_io:affine_prologue_beta": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_AFFINE prologue needs gamma/beta"),
    "ps_dwconv_io:prelu_prologue_slope": (-1, "ps_dwconv_f32: prelu prologue needs slope"),
    "ps_dwconv_io:norm_3_prologue_gamma": (-1, "ps_dwconv_f32: norm prologue needs gamma/beta"),
    "ps_dwconv_amax_f32:null_x": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=100 P=3 dilation=2 left=2)"),
    "ps_dwconv_amax_f32:null_w": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=100 P=3 dilation=2 left=2)"),
    "ps_dwconv_amax_f32:null_y": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=100 P=3 dilation=2 left=2)"),
    "ps_dwconv_amax_f32:N_zero": (-1, "ps_dwconv_f32: bad argument (N=0 H=4 T=100 P=3 dilation=2 left=2)"),
    "ps_dwconv_amax_f32:H_zero": (-1, "ps_dwconv_f32: bad argument (N=2 H=0 T=100 P=3 dilation=2 left=2)"),
    "ps_dwconv_amax_f32:T_zero": (-1, "ps_dwconv_f32: bad argument (N=2 H=4 T=0 P=3 dilation=2 left=2)"),
    "ps_dwconv_amax_f32:P_zero": (-3,
        "ps_dwconv_amax_f32: the maxima are an output of the wave-private kernel only (P = 3, 2 * dilation <= 256; "
        "ps_dwconv_amax_ok); got P=0 dilation=2 left=2"),
    "ps_dwconv_amax_f32:dilation_zero": (-3,
        "ps_dwconv_amax_f32: the maxima are an output of the wave-private kernel only (P = 3, 2 * dilation <= 256; "
        "ps_dwconv_amax_ok); got P=3 dilation=0 left=2"),
    "ps_dwconv_amax_f32:P_9": (-3,
        "ps_dwconv_amax_f32: the maxima are an output of the wave-private kernel only (P = 3, 2 * dilation <= 256; "
        "ps_dwconv_amax_ok); got P=9 dilation=2 left=0"),
    "ps_dwconv_amax_f32:left_negative": (-3,
        "ps_dwconv_amax_f32: the maxima are an output of the wave-private kernel only (P = 3, 2 * dilation <= 256; "
        "ps_dwconv_amax_ok); got P=3 dilation=2 left=-1"),
    "ps_dwconv_amax_f32:left_beyond_the_receptive_field": (-3,
        "ps_dwconv_amax_f32: the maxima are an output of the wave-private kernel only (P = 3, 2 * dilation <= 256; "
        "ps_dwconv_amax_ok); got P=3 dilation=2 left=5"),
    "ps_dwconv_amax_f32:halo_beyond_the_tile": (-3,
        "ps_dwconv_amax_f32: the maxima are an output of the wave-private kernel only (P = 3, 2 * dilation <= 256; "
        "ps_dwconv_amax_ok); got P=3 dilation=509 left=2"),
    "ps_dwconv_amax_f32:ldt_below_T": (-2,
        "ps_dwconv_f32: ldt=128 must be a multiple of 128 >= T=129 and pointers 16-byte aligned"),
    "ps_dwconv_amax_f32:ldt_192": (-2, "ps_dwconv_f32: ldt=192 must be a multiple of 128 >= T=100 and pointers 16-byte aligned"),
    "ps_dwconv_amax_f32:x_misaligned": (-2,
        "ps_dwconv_f32: ldt=128 must be a multiple of 128 >= T=100 and pointers 16-byte aligned"),
    "ps_dwconv_amax_f32:y_misaligned": (-2,
        "ps_dwconv_f32: ldt=128 must be a multiple of 128 >= T=100 and pointers 16-byte aligned"),
    "ps_dwconv_amax_f32:global_prologue_stats": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_dwconv_amax_f32:global_prologue_parts": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_dwconv_amax_f32:global_prologue_count": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_dwconv_amax_f32:global_prologue_gamma": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_dwconv_amax_f32:global_prologue_beta": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_GLOBAL prologue needs stats/parts/count/gamma/beta"),
    "ps_dwconv_amax_f32:affine_prologue_gamma": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_AFFINE prologue needs gamma/beta"),
    "ps_dwconv_amax_f32:affine_prologue_beta": (-1,   # (check_prologue's text; the code is 58cc688's)
        "ps_dwconv_f32: PS_NORM_AFFINE prologue needs gamma/beta"),
    "ps_dwconv_amax_f32:prelu_prologue_slope": (-1, "ps_dwconv_f32: prelu prologue needs slope"),
    "ps_dwconv_amax_f32:norm_3_prologue_gamma": (-1, "ps_dwconv_f32: norm prologue needs gamma/beta"),
    "ps_dwconv_io:bf16_in_P_5": (-3, "ps_dwconv_io: bf16 rows are built for P = 3 with (P-1)*dilation <= 280"),
    "ps_dwconv_io:bf16_out_P_5": (-3, "ps_dwconv_io: bf16 rows are built for P = 3 with (P-1)*dilation <= 280"),
    "ps_dwconv_io:bf16_rows_P_2": (-3, "ps_dwconv_io: bf16 rows are built for P = 3 with (P-1)*dilation <= 280"),
    "ps_dwconv_io:bf16_in_halo_beyond_the_small_build": (-3,
        "ps_dwconv_io: bf16 rows are built for P = 3 with (P-1)*dilation <= 280"),
    "ps_dwconv_io:bf16_out_halo_beyond_the_small_build": (-3,
        "ps_dwconv_io: bf16 rows are built for P = 3 with (P-1)*dilation <= 280"),
    "ps_dwconv_io:bf16_rows_halo_beyond_the_small_build": (-3,
        "ps_dwconv_io: bf16 rows are built for P = 3 with (P-1)*dilation <= 280"),
    "ps_dwconv_amax_f32:null_y_amax": (-3,
        "ps_dwconv_amax_f32: the maxima are an output of the wave-private kernel only (P = 3, 2 * dilation <= 256; "
        "ps_dwconv_amax_ok); got P=3 dilation=2 left=2"),
    "ps_dwconv_amax_f32:P_5": (-3,
        "ps_dwconv_amax_f32: the maxima are an output of the wave-private kernel only (P = 3, 2 * dilation <= 256; "
        "ps_dwconv_amax_ok); got P=5 dilation=2 left=2"),
    "ps_dwconv_amax_f32:P_2": (-3,
        "ps_dwconv_amax_f32: the maxima are an output of the wave-private kernel only (P = 3, 2 * dilation <= 256; "
        "ps_dwconv_amax_ok); got P=2 dilation=2 left=2"),
    "ps_dwconv_amax_f32:dilation_129": (-3,
        "ps_dwconv_amax_f32: the maxima are an output of the wave-private kernel only (P = 3, 2 * dilation <= 256; "
        "ps_dwconv_amax_ok); got P=3 dilation=129 left=2"),
    "ps_dwconv_amax_f32:left_beyond_two_dilations": (-3,
        "ps_dwconv_amax_f32: the maxima are an output of the wave-private kernel only (P = 3, 2 * dilation <= 256; "
        "ps_dwconv_amax_ok); got P=3 dilation=2 left=5"),
    "ps_free_encode_f32:null_wav": (-1, "ps_free_encode_f32: bad argument (N=2 L=1000 C=8 win=32 hop=16)"),
    "ps_free_encode_f32:null_w": (-1, "ps_free_encode_f32: bad argument (N=2 L=1000 C=8 win=32 hop=16)"),
    "ps_free_encode_f32:null_feats": (-1, "ps_free_encode_f32: bad argument (N=2 L=1000 C=8 win=32 hop=16)"),
    "ps_free_encode_f32:N_zero": (-1, "ps_free_encode_f32: bad argument (N=0 L=1000 C=8 win=32 hop=16)"),
    "ps_free_encode_f32:C_zero": (-1, "ps_free_encode_f32: bad argument (N=2 L=1000 C=0 win=32 hop=16)"),
    "ps_free_encode_f32:win_zero": (-1, "ps_free_encode_f32: bad argument (N=2 L=1000 C=8 win=0 hop=16)"),
    "ps_free_encode_f32:hop_zero": (-1, "ps_free_encode_f32: bad argument (N=2 L=1000 C=8 win=32 hop=0)"),
    "ps_free_encode_f32:L_below_win": (-1, "ps_free_encode_f32: bad argument (N=2 L=16 C=8 win=32 hop=16)"),
    "ps_free_encode_f32:T_60": (-1,
        "ps_free_encode_f32: T=60 must equal floor((L-win)/hop)+1=61, ldt=128 a multiple of 128 >= T"),
    "ps_free_encode_f32:ldt_below_T": (-1,
        "ps_free_encode_f32: T=61 must equal floor((L-win)/hop)+1=61, ldt=0 a multiple of 128 >= T"),
    "ps_free_encode_f32:ldt_192": (-1,
        "ps_free_encode_f32: T=61 must equal floor((L-win)/hop)+1=61, ldt=192 a multiple of 128 >= T"),
    "ps_free_decode_f32:null_feats": (-1, "ps_free_decode_f32: bad argument (N=2 C=16 T=64 win=32 hop=16)"),
    "ps_free_decode_f32:null_w": (-1, "ps_free_decode_f32: bad argument (N=2 C=16 T=64 win=32 hop=16)"),
    "ps_free_decode_f32:null_out": (-1, "ps_free_decode_f32: bad argument (N=2 C=16 T=64 win=32 hop=16)"),
    "ps_free_decode_f32:N_zero": (-1, "ps_free_decode_f32: bad argument (N=0 C=16 T=64 win=32 hop=16)"),
    "ps_free_decode_f32:C_zero": (-1, "ps_free_decode_f32: bad argument (N=2 C=0 T=64 win=32 hop=16)"),
    "ps_free_decode_f32:T_zero": (-1, "ps_free_decode_f32: bad argument (N=2 C=16 T=0 win=32 hop=16)"),
    "ps_free_decode_f32:win_zero": (-1, "ps_free_decode_f32: bad argument (N=2 C=16 T=64 win=0 hop=16)"),
    "ps_free_decode_f32:hop_zero": (-1, "ps_free_decode_f32: bad argument (N=2 C=16 T=64 win=32 hop=0)"),
    "ps_free_decode_f32:ldt_below_T": (-1, "ps_free_decode_f32: bad argument (N=2 C=16 T=64 win=32 hop=16)"),
    "ps_free_decode_ws_f32:null_feats": (-1,   # (ps_free_decode_f32's form; the code is 58cc688's)
        "ps_free_decode_ws_f32: bad argument (N=2 C=16 T=64 win=32 hop=16)"),
    "ps_free_decode_ws_f32:null_w": (-1,   # (ps_free_decode_f32's form; the code is 58cc688's)
        "ps_free_decode_ws_f32: bad argument (N=2 C=16 T=64 win=32 hop=16)"),
    "ps_free_decode_ws_f32:null_out": (-1,   # (ps_free_decode_f32's form; the code is 58cc688's)
        "ps_free_decode_ws_f32: bad argument (N=2 C=16 T=64 win=32 hop=16)"),
    "ps_free_decode_ws_f32:N_zero": (-1, "ps_free_decode_f32: bad argument (N=0 C=16 T=64 win=32 hop=16)"),
    "ps_free_decode_ws_f32:C_zero": (-1,   # (ps_free_decode_f32's form; the code is 58cc688's)
        "ps_free_decode_ws_f32: bad argument (N=2 C=0 T=64 win=32 hop=16)"),
    "ps_free_decode_ws_f32:T_zero": (-1, "ps_free_decode_f32: bad argument (N=2 C=16 T=0 win=32 hop=16)"),
    "ps_free_decode_ws_f32:win_zero": (-1, "ps_free_decode_f32: bad argument (N=2 C=16 T=64 win=0 hop=16)"),
    "ps_free_decode_ws_f32:hop_zero": (-1, "ps_free_decode_f32: bad argument (N=2 C=16 T=64 win=32 hop=0)"),
    "ps_free_decode_ws_f32:ldt_below_T": (-1,   # (ps_free_decode_f32's form; the code is 58cc688's)
        "ps_free_decode_ws_f32: bad argument (N=2 C=16 T=64 win=32 hop=16)"),
    "ps_free_decode_f32:mask_act_minus_1": (-1, "ps_free_decode_f32: unknown mask_act=-1 or out_mode=2"),
    "ps_free_decode_f32:mask_act_3": (-1, "ps_free_decode_f32: unknown mask_act=3 or out_mode=2"),
    "ps_free_decode_f32:out_mode_minus_1": (-1, "ps_free_decode_f32: unknown mask_act=0 or out_mode=-1"),
    "ps_free_decode_f32:out_mode_3": (-1, "ps_free_decode_f32: unknown mask_act=0 or out_mode=3"),
    "ps_free_decode_ws_f32:mask_act_minus_1": (-1, "ps_free_decode_ws_f32: unknown mask_act=-1 or out_mode=2"),
    "ps_free_decode_ws_f32:mask_act_3": (-1, "ps_free_decode_ws_f32: unknown mask_act=3 or out_mode=2"),
    "ps_free_decode_ws_f32:out_mode_minus_1": (-1, "ps_free_decode_ws_f32: unknown mask_act=0 or out_mode=-1"),
    "ps_free_decode_ws_f32:out_mode_3": (-1, "ps_free_decode_ws_f32: unknown mask_act=0 or out_mode=3"),
    "ps_free_decode_moments_f32:mask_act_minus_1": (-1, "ps_free_decode_moments_f32: unknown mask_act=-1 or out_mode=2"),
    "ps_free_decode_moments_f32:mask_act_3": (-1, "ps_free_decode_moments_f32: unknown mask_act=3 or out_mode=2"),
    "ps_free_decode_moments_f32:out_mode_minus_1": (-1, "ps_free_decode_moments_f32: unknown mask_act=0 or out_mode=-1"),
    "ps_free_decode_moments_f32:out_mode_3": (-1, "ps_free_decode_moments_f32: unknown mask_act=0 or out_mode=3"),
    "ps_free_decode_ws_f32:no_workspace_null_feats": (-1, "ps_free_decode_f32: bad argument (N=2 C=16 T=64 win=32 hop=16)"),
    "ps_free_decode_ws_f32:no_workspace_mask_act_3": (-1, "ps_free_decode_f32: unknown mask_act=3 or out_mode=2"),
    "ps_free_decode_moments_f32:T_63": (-3,
        "ps_free_decode_moments_f32: shape outside the fused kernel (N=2 C=16 T=63 ldt=128 win=32 hop=16): decode, then"
        " ps_wave_moments_f64"),
    "ps_free_decode_moments_f32:C_8": (-3,
        "ps_free_decode_moments_f32: shape outside the fused kernel (N=2 C=8 T=64 ldt=128 win=32 hop=16): decode, then "
        "ps_wave_moments_f64"),
    "ps_free_decode_moments_f32:C_zero": (-3,
        "ps_free_decode_moments_f32: shape outside the fused kernel (N=2 C=0 T=64 ldt=128 win=32 hop=16): decode, then "
        "ps_wave_moments_f64"),
    "ps_free_decode_moments_f32:N_zero": (-3,
        "ps_free_decode_moments_f32: shape outside the fused kernel (N=0 C=16 T=64 ldt=128 win=32 hop=16): decode, then"
        " ps_wave_moments_f64"),
    "ps_free_decode_moments_f32:N_65536": (-3,
        "ps_free_decode_moments_f32: shape outside the fused kernel (N=65536 C=16 T=64 ldt=128 win=32 hop=16): decode, "
        "then ps_wave_moments_f64"),
    "ps_free_decode_moments_f32:win_16_hop_8": (-3,
        "ps_free_decode_moments_f32: shape outside the fused kernel (N=2 C=16 T=64 ldt=128 win=16 hop=8): decode, then "
        "ps_wave_moments_f64"),
    "ps_free_decode_moments_f32:ldt_below_T": (-3,
        "ps_free_decode_moments_f32: shape outside the fused kernel (N=2 C=16 T=64 ldt=32 win=32 hop=16): decode, then "
        "ps_wave_moments_f64"),
    "ps_free_decode_moments_f32:utterance_2GiB": (-3,
        "ps_free_decode_moments_f32: shape outside the fused kernel (N=2 C=4194304 T=64 ldt=128 win=32 hop=16): decode,"
        " then ps_wave_moments_f64"),
    "ps_free_decode_moments_f32:null_feats": (-1,
        "ps_free_decode_moments_f32: null / unaligned pointer, short workspace or bad reference row (ref_len=1040 "
        "ldr=1100)"),
    "ps_free_decode_moments_f32:null_w": (-1,
        "ps_free_decode_moments_f32: null / unaligned pointer, short workspace or bad reference row (ref_len=1040 "
        "ldr=1100)"),
    "ps_free_decode_moments_f32:null_out": (-1,
        "ps_free_decode_moments_f32: null / unaligned pointer, short workspace or bad reference row (ref_len=1040 "
        "ldr=1100)"),
    "ps_free_decode_moments_f32:null_ref": (-1,
        "ps_free_decode_moments_f32: null / unaligned pointer, short workspace or bad reference row (ref_len=1040 "
        "ldr=1100)"),
    "ps_free_decode_moments_f32:null_partials": (-1,
        "ps_free_decode_moments_f32: null / unaligned pointer, short workspace or bad reference row (ref_len=1040 "
        "ldr=1100)"),
    "ps_free_decode_moments_f32:null_workspace": (-1,
        "ps_free_decode_moments_f32: null / unaligned pointer, short workspace or bad reference row (ref_len=1040 "
        "ldr=1100)"),
    "ps_free_decode_moments_f32:ref_len_zero": (-1,
        "ps_free_decode_moments_f32: null / unaligned pointer, short workspace or bad reference row (ref_len=0 "
        "ldr=1100)"),
    "ps_free_decode_moments_f32:ldr_below_ref_len": (-1,
        "ps_free_decode_moments_f32: null / unaligned pointer, short workspace or bad reference row (ref_len=1040 "
        "ldr=1039)"),
    "ps_free_decode_moments_f32:short_workspace": (-1,
        "ps_free_decode_moments_f32: null / unaligned pointer, short workspace or bad reference row (ref_len=1040 "
        "ldr=1100)"),
    "ps_free_decode_moments_f32:out_misaligned": (-1,
        "ps_free_decode_moments_f32: null / unaligned pointer, short workspace or bad reference row (ref_len=1040 "
        "ldr=1100)"),
    "ps_free_decode_moments_f32:workspace_misaligned": (-1,
        "ps_free_decode_moments_f32: null / unaligned pointer, short workspace or bad reference row (ref_len=1040 "
        "ldr=1100)"),
    "ps_pad_rows_f32:null_src": (-1, "ps_pad_rows_f32: bad argument"),
    "ps_pad_rows_f32:null_dst": (-1, "ps_pad_rows_f32: bad argument"),
    "ps_pad_rows_f32:rows_zero": (-1, "ps_pad_rows_f32: bad argument"),
    "ps_pad_rows_f32:T_zero": (-1, "ps_pad_rows_f32: bad argument"),
    "ps_pad_rows_f32:ldt_below_T": (-1, "ps_pad_rows_f32: bad argument"),
    "ps_pad_rows_f32:rows_2_31": (-1, "ps_pad_rows_f32: bad argument"),
    "ps_unpad_rows_f32:null_src": (-1, "ps_unpad_rows_f32: bad argument"),
    "ps_unpad_rows_f32:null_dst": (-1, "ps_unpad_rows_f32: bad argument"),
    "ps_unpad_rows_f32:rows_zero": (-1, "ps_unpad_rows_f32: bad argument"),
    "ps_unpad_rows_f32:T_zero": (-1, "ps_unpad_rows_f32: bad argument"),
    "ps_unpad_rows_f32:ldt_below_T": (-1, "ps_unpad_rows_f32: bad argument"),
    "ps_unpad_rows_f32:rows_2_31": (-1, "ps_unpad_rows_f32: bad argument"),
    "ps_conv2d_f32:null_x1": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f32:null_wt": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f32:null_y": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f32:N_zero": (-1, "ps_conv2d_f32: bad argument (N=0 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f32:M_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=0 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f32:C1_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=0+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f32:Fin_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=0->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f32:Fout_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->0 T=100 k=3x2 act=0)"),
    "ps_conv2d_f32:T_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=0 k=3x2 act=0)"),
    "ps_conv2d_f32:T_in_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f32:kf_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=0x2 act=0)"),
    "ps_conv2d_f32:kt_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x0 act=0)"),
    "ps_conv2d_f32:stride_f_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f32:dil_f_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f32:dil_t_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f32:C2_negative": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+-1 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f32:C2_without_x2": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+2 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f32:ld_below_T": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f32:ld_below_T_in": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f32:ld_192": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f32:Fout_65536": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->65536 T=100 k=3x2 act=0)"),
    "ps_conv2d_f32:Kp_4200": (-3, "ps_conv2d_f32: Cin*kf*kt = 4200 exceeds 4096"),
    "ps_conv2d_f32:utterance_2_30_elements": (-3, "ps_conv2d_f32: one utterance of the input exceeds 2^30 elements"),
    "ps_conv2d_f32:grid_limit": (-3, "ps_conv2d_f32: N * channel tiles exceeds the grid limit"),
    "ps_conv2d_stats_f32:null_x1": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:null_wt": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:null_y": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:N_zero": (-1, "ps_conv2d_f32: bad argument (N=0 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:M_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=0 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:C1_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=0+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:Fin_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=0->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:Fout_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->0 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:T_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=0 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:T_in_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:kf_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=0x2 act=0)"),
    "ps_conv2d_stats_f32:kt_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x0 act=0)"),
    "ps_conv2d_stats_f32:stride_f_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:dil_f_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:dil_t_zero": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:C2_negative": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+-1 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:C2_without_x2": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+2 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:ld_below_T": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:ld_below_T_in": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:ld_192": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:Fout_65536": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->65536 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:Kp_4200": (-3, "ps_conv2d_f32: Cin*kf*kt = 4200 exceeds 4096"),
    "ps_conv2d_stats_f32:utterance_2_30_elements": (-3, "ps_conv2d_f32: one utterance of the input exceeds 2^30 elements"),
    "ps_conv2d_stats_f32:grid_limit": (-3, "ps_conv2d_f32: N * channel tiles exceeds the grid limit"),
    "ps_conv2d_f16x2_f32:null_x1": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:null_wimg": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:null_y": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:N_zero": (-1, "ps_conv2d_f16x2_f32: bad argument (N=0 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:M_zero": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=0 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:C1_zero": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=0+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:Fin_zero": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=0->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:Fout_zero": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->0 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:T_zero": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=0 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:T_in_zero": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:kf_zero": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=0x2 act=0)"),
    "ps_conv2d_f16x2_f32:kt_zero": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x0 act=0)"),
    "ps_conv2d_f16x2_f32:stride_f_zero": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:dil_f_zero": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:dil_t_zero": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:C2_negative": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+-1 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:C2_without_x2": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+2 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:ld_below_T": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:ld_below_T_in": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:ld_192": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:Fout_65536": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->65536 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:Kp_4200": (-3,   # (the fp32 entry's text; the code is 58cc688's)
        "ps_conv2d_f16x2_f32: Cin*kf*kt = 4200 exceeds 4096"),
    "ps_conv2d_f16x2_f32:utterance_2_30_elements": (-3,   # (the fp32 entry's text; the code is 58cc688's)
        "ps_conv2d_f16x2_f32: one utterance of the input exceeds 2^30 elements"),
    "ps_conv2d_f16x2_f32:grid_limit": (-3, "ps_conv2d_f16x2_f32: N * channel tiles exceeds the grid limit"),
    "ps_conv2d_f32:act_minus_1": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=-1)"),
    "ps_conv2d_f32:act_6": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=6)"),
    "ps_conv2d_f32:prelu_without_slope": (-1, "ps_conv2d_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=2)"),
    "ps_conv2d_f16x2_f32:act_minus_1": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=-1)"),
    "ps_conv2d_f16x2_f32:act_6": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=6)"),
    "ps_conv2d_f16x2_f32:prelu_without_slope": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=2)"),
    "ps_conv2d_f16x2_f32:w_exp_101": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:w_exp_minus_101": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_f16x2_f32:wimg_misaligned": (-1, "ps_conv2d_f16x2_f32: bad argument (N=1 M=4 C=2+0 F=8->8 T=100 k=3x2 act=0)"),
    "ps_conv2d_stats_f32:null_ostats": (-1, "ps_conv2d_stats_f32: ostats is NULL"),
}
VALUES = {
    "ps_dwconv_amax_ok": {
        (2, 0, -1): 0, (2, 0, 0): 0, (2, 0, 1): 0, (2, 1, -1): 0, (2, 1, 0): 0, (2, 1, 1): 0, (2, 1, 2): 0, (2, 1, 3): 0,
        (2, 4, -1): 0, (2, 4, 0): 0, (2, 4, 4): 0, (2, 4, 8): 0, (2, 4, 9): 0, (2, 127, -1): 0, (2, 127, 0): 0,
        (2, 127, 127): 0, (2, 127, 254): 0, (2, 127, 255): 0, (2, 128, -1): 0, (2, 128, 0): 0, (2, 128, 128): 0,
        (2, 128, 256): 0, (2, 128, 257): 0, (2, 129, -1): 0, (2, 129, 0): 0, (2, 129, 129): 0, (2, 129, 258): 0,
        (2, 129, 259): 0, (3, 0, -1): 0, (3, 0, 0): 0, (3, 0, 1): 0, (3, 1, -1): 0, (3, 1, 0): 1, (3, 1, 1): 1, (3, 1, 2): 1,
        (3, 1, 3): 0, (3, 4, -1): 0, (3, 4, 0): 1, (3, 4, 4): 1, (3, 4, 8): 1, (3, 4, 9): 0, (3, 127, -1): 0, (3, 127, 0): 1,
        (3, 127, 127): 1, (3, 127, 254): 1, (3, 127, 255): 0, (3, 128, -1): 0, (3, 128, 0): 1, (3, 128, 128): 1,
        (3, 128, 256): 1, (3, 128, 257): 0, (3, 129, -1): 0, (3, 129, 0): 0, (3, 129, 129): 0, (3, 129, 258): 0,
        (3, 129, 259): 0, (5, 0, -1): 0, (5, 0, 0): 0, (5, 0, 1): 0, (5, 1, -1): 0, (5, 1, 0): 0, (5, 1, 1): 0, (5, 1, 2): 0,
        (5, 1, 3): 0, (5, 4, -1): 0, (5, 4, 0): 0, (5, 4, 4): 0, (5, 4, 8): 0, (5, 4, 9): 0, (5, 127, -1): 0, (5, 127, 0): 0,
        (5, 127, 127): 0, (5, 127, 254): 0, (5, 127, 255): 0, (5, 128, -1): 0, (5, 128, 0): 0, (5, 128, 128): 0,
        (5, 128, 256): 0, (5, 128, 257): 0, (5, 129, -1): 0, (5, 129, 0): 0, (5, 129, 129): 0, (5, 129, 258): 0,
        (5, 129, 259): 0,
    },
    "ps_dwconv_stats_parts": {
        (0, 0): 0, (0, 1): 0, (0, 1024): 0, (0, 1025): 0, (1, 0): 0, (1, 1): 1, (1, 1024): 1, (1, 1025): 2, (16, 0): 0,
        (16, 1): 1, (16, 1024): 1, (16, 1025): 2, (17, 0): 0, (17, 1): 2, (17, 1024): 2, (17, 1025): 4,
    },
    "ps_free_decode_workspace_bytes": {
        (0, 0, 32, 16): 0, (0, 0, 32, 8): 0, (0, 0, 16, 16): 0, (0, 0, 16, 8): 0, (0, 63, 32, 16): 0, (0, 63, 32, 8): 0,
        (0, 63, 16, 16): 0, (0, 63, 16, 8): 0, (0, 64, 32, 16): 0, (0, 64, 32, 8): 0, (0, 64, 16, 16): 0, (0, 64, 16, 8): 0,
        (0, 65, 32, 16): 0, (0, 65, 32, 8): 0, (0, 65, 16, 16): 0, (0, 65, 16, 8): 0, (1, 0, 32, 16): 0, (1, 0, 32, 8): 0,
        (1, 0, 16, 16): 0, (1, 0, 16, 8): 0, (1, 63, 32, 16): 128, (1, 63, 32, 8): 0, (1, 63, 16, 16): 0, (1, 63, 16, 8): 0,
        (1, 64, 32, 16): 192, (1, 64, 32, 8): 0, (1, 64, 16, 16): 0, (1, 64, 16, 8): 0, (1, 65, 32, 16): 192,
        (1, 65, 32, 8): 0, (1, 65, 16, 16): 0, (1, 65, 16, 8): 0, (65535, 0, 32, 16): 0, (65535, 0, 32, 8): 0,
        (65535, 0, 16, 16): 0, (65535, 0, 16, 8): 0, (65535, 63, 32, 16): 8388480, (65535, 63, 32, 8): 0,
        (65535, 63, 16, 16): 0, (65535, 63, 16, 8): 0, (65535, 64, 32, 16): 12582720, (65535, 64, 32, 8): 0,
        (65535, 64, 16, 16): 0, (65535, 64, 16, 8): 0, (65535, 65, 32, 16): 12582720, (65535, 65, 32, 8): 0,
        (65535, 65, 16, 16): 0, (65535, 65, 16, 8): 0, (65536, 0, 32, 16): 0, (65536, 0, 32, 8): 0, (65536, 0, 16, 16): 0,
        (65536, 0, 16, 8): 0, (65536, 63, 32, 16): 8388608, (65536, 63, 32, 8): 0, (65536, 63, 16, 16): 0,
        (65536, 63, 16, 8): 0, (65536, 64, 32, 16): 12582912, (65536, 64, 32, 8): 0, (65536, 64, 16, 16): 0,
        (65536, 64, 16, 8): 0, (65536, 65, 32, 16): 12582912, (65536, 65, 32, 8): 0, (65536, 65, 16, 16): 0,
        (65536, 65, 16, 8): 0,
    },
    "ps_free_decode_moments_parts": {
        (0, 0, 63, 32, 32, 16): 0, (0, 0, 63, 32, 16, 8): 0, (0, 0, 63, 128, 32, 16): 0, (0, 0, 63, 128, 16, 8): 0,
        (0, 0, 64, 32, 32, 16): 0, (0, 0, 64, 32, 16, 8): 0, (0, 0, 64, 128, 32, 16): 0, (0, 0, 64, 128, 16, 8): 0,
        (0, 8, 63, 32, 32, 16): 0, (0, 8, 63, 32, 16, 8): 0, (0, 8, 63, 128, 32, 16): 0, (0, 8, 63, 128, 16, 8): 0,
        (0, 8, 64, 32, 32, 16): 0, (0, 8, 64, 32, 16, 8): 0, (0, 8, 64, 128, 32, 16): 0, (0, 8, 64, 128, 16, 8): 0,
        (0, 15, 63, 32, 32, 16): 0, (0, 15, 63, 32, 16, 8): 0, (0, 15, 63, 128, 32, 16): 0, (0, 15, 63, 128, 16, 8): 0,
        (0, 15, 64, 32, 32, 16): 0, (0, 15, 64, 32, 16, 8): 0, (0, 15, 64, 128, 32, 16): 0, (0, 15, 64, 128, 16, 8): 0,
        (0, 16, 63, 32, 32, 16): 0, (0, 16, 63, 32, 16, 8): 0, (0, 16, 63, 128, 32, 16): 0, (0, 16, 63, 128, 16, 8): 0,
        (0, 16, 64, 32, 32, 16): 0, (0, 16, 64, 32, 16, 8): 0, (0, 16, 64, 128, 32, 16): 0, (0, 16, 64, 128, 16, 8): 0,
        (0, 17, 63, 32, 32, 16): 0, (0, 17, 63, 32, 16, 8): 0, (0, 17, 63, 128, 32, 16): 0, (0, 17, 63, 128, 16, 8): 0,
        (0, 17, 64, 32, 32, 16): 0, (0, 17, 64, 32, 16, 8): 0, (0, 17, 64, 128, 32, 16): 0, (0, 17, 64, 128, 16, 8): 0,
        (0, 32, 63, 32, 32, 16): 0, (0, 32, 63, 32, 16, 8): 0, (0, 32, 63, 128, 32, 16): 0, (0, 32, 63, 128, 16, 8): 0,
        (0, 32, 64, 32, 32, 16): 0, (0, 32, 64, 32, 16, 8): 0, (0, 32, 64, 128, 32, 16): 0, (0, 32, 64, 128, 16, 8): 0,
        (1, 0, 63, 32, 32, 16): 0, (1, 0, 63, 32, 16, 8): 0, (1, 0, 63, 128, 32, 16): 0, (1, 0, 63, 128, 16, 8): 0,
        (1, 0, 64, 32, 32, 16): 0, (1, 0, 64, 32, 16, 8): 0, (1, 0, 64, 128, 32, 16): 0, (1, 0, 64, 128, 16, 8): 0,
        (1, 8, 63, 32, 32, 16): 0, (1, 8, 63, 32, 16, 8): 0, (1, 8, 63, 128, 32, 16): 0, (1, 8, 63, 128, 16, 8): 0,
        (1, 8, 64, 32, 32, 16): 0, (1, 8, 64, 32, 16, 8): 0, (1, 8, 64, 128, 32, 16): 0, (1, 8, 64, 128, 16, 8): 0,
        (1, 15, 63, 32, 32, 16): 0, (1, 15, 63, 32, 16, 8): 0, (1, 15, 63, 128, 32, 16): 0, (1, 15, 63, 128, 16, 8): 0,
        (1, 15, 64, 32, 32, 16): 0, (1, 15, 64, 32, 16, 8): 0, (1, 15, 64, 128, 32, 16): 0, (1, 15, 64, 128, 16, 8): 0,
        (1, 16, 63, 32, 32, 16): 0, (1, 16, 63, 32, 16, 8): 0, (1, 16, 63, 128, 32, 16): 0, (1, 16, 63, 128, 16, 8): 0,
        (1, 16, 64, 32, 32, 16): 0, (1, 16, 64, 32, 16, 8): 0, (1, 16, 64, 128, 32, 16): 4, (1, 16, 64, 128, 16, 8): 0,
        (1, 17, 63, 32, 32, 16): 0, (1, 17, 63, 32, 16, 8): 0, (1, 17, 63, 128, 32, 16): 0, (1, 17, 63, 128, 16, 8): 0,
        (1, 17, 64, 32, 32, 16): 0, (1, 17, 64, 32, 16, 8): 0, (1, 17, 64, 128, 32, 16): 0, (1, 17, 64, 128, 16, 8): 0,
        (1, 32, 63, 32, 32, 16): 0, (1, 32, 63, 32, 16, 8): 0, (1, 32, 63, 128, 32, 16): 0, (1, 32, 63, 128, 16, 8): 0,
        (1, 32, 64, 32, 32, 16): 0, (1, 32, 64, 32, 16, 8): 0, (1, 32, 64, 128, 32, 16): 4, (1, 32, 64, 128, 16, 8): 0,
        (65535, 0, 63, 32, 32, 16): 0, (65535, 0, 63, 32, 16, 8): 0, (65535, 0, 63, 128, 32, 16): 0,
        (65535, 0, 63, 128, 16, 8): 0, (65535, 0, 64, 32, 32, 16): 0, (65535, 0, 64, 32, 16, 8): 0,
        (65535, 0, 64, 128, 32, 16): 0, (65535, 0, 64, 128, 16, 8): 0, (65535, 8, 63, 32, 32, 16): 0,
        (65535, 8, 63, 32, 16, 8): 0, (65535, 8, 63, 128, 32, 16): 0, (65535, 8, 63, 128, 16, 8): 0,
        (65535, 8, 64, 32, 32, 16): 0, (65535, 8, 64, 32, 16, 8): 0, (65535, 8, 64, 128, 32, 16): 0,
        (65535, 8, 64, 128, 16, 8): 0, (65535, 15, 63, 32, 32, 16): 0, (65535, 15, 63, 32, 16, 8): 0,
        (65535, 15, 63, 128, 32, 16): 0, (65535, 15, 63, 128, 16, 8): 0, (65535, 15, 64, 32, 32, 16): 0,
        (65535, 15, 64, 32, 16, 8): 0, (65535, 15, 64, 128, 32, 16): 0, (65535, 15, 64, 128, 16, 8): 0,
        (65535, 16, 63, 32, 32, 16): 0, (65535, 16, 63, 32, 16, 8): 0, (65535, 16, 63, 128, 32, 16): 0,
        (65535, 16, 63, 128, 16, 8): 0, (65535, 16, 64, 32, 32, 16): 0, (65535, 16, 64, 32, 16, 8): 0,
        (65535, 16, 64, 128, 32, 16): 4, (65535, 16, 64, 128, 16, 8): 0, (65535, 17, 63, 32, 32, 16): 0,
        (65535, 17, 63, 32, 16, 8): 0, (65535, 17, 63, 128, 32, 16): 0, (65535, 17, 63, 128, 16, 8): 0,
        (65535, 17, 64, 32, 32, 16): 0, (65535, 17, 64, 32, 16, 8): 0, (65535, 17, 64, 128, 32, 16): 0,
        (65535, 17, 64, 128, 16, 8): 0, (65535, 32, 63, 32, 32, 16): 0, (65535, 32, 63, 32, 16, 8): 0,
        (65535, 32, 63, 128, 32, 16): 0, (65535, 32, 63, 128, 16, 8): 0, (65535, 32, 64, 32, 32, 16): 0,
        (65535, 32, 64, 32, 16, 8): 0, (65535, 32, 64, 128, 32, 16): 4, (65535, 32, 64, 128, 16, 8): 0,
        (65536, 0, 63, 32, 32, 16): 0, (65536, 0, 63, 32, 16, 8): 0, (65536, 0, 63, 128, 32, 16): 0,
        (65536, 0, 63, 128, 16, 8): 0, (65536, 0, 64, 32, 32, 16): 0, (65536, 0, 64, 32, 16, 8): 0,
        (65536, 0, 64, 128, 32, 16): 0, (65536, 0, 64, 128, 16, 8): 0, (65536, 8, 63, 32, 32, 16): 0,
        (65536, 8, 63, 32, 16, 8): 0, (65536, 8, 63, 128, 32, 16): 0, (65536, 8, 63, 128, 16, 8): 0,
        (65536, 8, 64, 32, 32, 16): 0, (65536, 8, 64, 32, 16, 8): 0, (65536, 8, 64, 128, 32, 16): 0,
        (65536, 8, 64, 128, 16, 8): 0, (65536, 15, 63, 32, 32, 16): 0, (65536, 15, 63, 32, 16, 8): 0,
        (65536, 15, 63, 128, 32, 16): 0, (65536, 15, 63, 128, 16, 8): 0, (65536, 15, 64, 32, 32, 16): 0,
        (65536, 15, 64, 32, 16, 8): 0, (65536, 15, 64, 128, 32, 16): 0, (65536, 15, 64, 128, 16, 8): 0,
        (65536, 16, 63, 32, 32, 16): 0, (65536, 16, 63, 32, 16, 8): 0, (65536, 16, 63, 128, 32, 16): 0,
        (65536, 16, 63, 128, 16, 8): 0, (65536, 16, 64, 32, 32, 16): 0, (65536, 16, 64, 32, 16, 8): 0,
        (65536, 16, 64, 128, 32, 16): 0, (65536, 16, 64, 128, 16, 8): 0, (65536, 17, 63, 32, 32, 16): 0,
        (65536, 17, 63, 32, 16, 8): 0, (65536, 17, 63, 128, 32, 16): 0, (65536, 17, 63, 128, 16, 8): 0,
        (65536, 17, 64, 32, 32, 16): 0, (65536, 17, 64, 32, 16, 8): 0, (65536, 17, 64, 128, 32, 16): 0,
        (65536, 17, 64, 128, 16, 8): 0, (65536, 32, 63, 32, 32, 16): 0, (65536, 32, 63, 32, 16, 8): 0,
        (65536, 32, 63, 128, 32, 16): 0, (65536, 32, 63, 128, 16, 8): 0, (65536, 32, 64, 32, 32, 16): 0,
        (65536, 32, 64, 32, 16, 8): 0, (65536, 32, 64, 128, 32, 16): 0, (65536, 32, 64, 128, 16, 8): 0,
        (2, 16, 65, 128, 32, 16): 4, (2, 16, 96, 128, 32, 16): 5, (2, 16, 97, 128, 32, 16): 5, (2, 16, 128, 128, 32, 16): 6,
        (2, 16, 129, 128, 32, 16): 0, (1, 4194288, 64, 128, 32, 16): 4, (1, 4194304, 64, 128, 32, 16): 0,
    },
    "ps_conv2d_stats_parts": {
        (0, 0, 0): 0, (0, 0, 128): 0, (0, 0, 192): 0, (0, 0, 384): 0, (0, 1, 0): 0, (0, 1, 128): 0, (0, 1, 192): 0,
        (0, 1, 384): 0, (0, 5, 0): 0, (0, 5, 128): 0, (0, 5, 192): 0, (0, 5, 384): 0, (1, 0, 0): 0, (1, 0, 128): 0,
        (1, 0, 192): 0, (1, 0, 384): 0, (1, 1, 0): 0, (1, 1, 128): 1, (1, 1, 192): 0, (1, 1, 384): 3, (1, 5, 0): 0,
        (1, 5, 128): 5, (1, 5, 192): 0, (1, 5, 384): 15, (32, 0, 0): 0, (32, 0, 128): 0, (32, 0, 192): 0, (32, 0, 384): 0,
        (32, 1, 0): 0, (32, 1, 128): 1, (32, 1, 192): 0, (32, 1, 384): 3, (32, 5, 0): 0, (32, 5, 128): 5, (32, 5, 192): 0,
        (32, 5, 384): 15, (33, 0, 0): 0, (33, 0, 128): 0, (33, 0, 192): 0, (33, 0, 384): 0, (33, 1, 0): 0, (33, 1, 128): 1,
        (33, 1, 192): 0, (33, 1, 384): 3, (33, 5, 0): 0, (33, 5, 128): 5, (33, 5, 192): 0, (33, 5, 384): 15, (64, 0, 0): 0,
        (64, 0, 128): 0, (64, 0, 192): 0, (64, 0, 384): 0, (64, 1, 0): 0, (64, 1, 128): 1, (64, 1, 192): 0, (64, 1, 384): 3,
        (64, 5, 0): 0, (64, 5, 128): 5, (64, 5, 192): 0, (64, 5, 384): 15, (65, 0, 0): 0, (65, 0, 128): 0, (65, 0, 192): 0,
        (65, 0, 384): 0, (65, 1, 0): 0, (65, 1, 128): 1, (65, 1, 192): 0, (65, 1, 384): 3, (65, 5, 0): 0, (65, 5, 128): 5,
        (65, 5, 192): 0, (65, 5, 384): 15, (128, 0, 0): 0, (128, 0, 128): 0, (128, 0, 192): 0, (128, 0, 384): 0,
        (128, 1, 0): 0, (128, 1, 128): 1, (128, 1, 192): 0, (128, 1, 384): 3, (128, 5, 0): 0, (128, 5, 128): 5,
        (128, 5, 192): 0, (128, 5, 384): 15, (129, 0, 0): 0, (129, 0, 128): 0, (129, 0, 192): 0, (129, 0, 384): 0,
        (129, 1, 0): 0, (129, 1, 128): 2, (129, 1, 192): 0, (129, 1, 384): 6, (129, 5, 0): 0, (129, 5, 128): 10,
        (129, 5, 192): 0, (129, 5, 384): 30,
    },
}


def test_the_table_and_the_recorded_answers_name_the_same_cases():
    assert sorted(f"{e}:{k}" for e, k, _ in CASES) == sorted(EXPECTED) and len(EXPECTED) == len(CASES)
    assert {f: len(set(g)) for f, g in GRIDS.items()} == {f: len(v) for f, v in VALUES.items()}


def test_every_recorded_answer_is_a_refusal():
    assert all(rc in (-1, -2, -3) for rc, _ in EXPECTED.values())   # PS_E_INVALID, PS_E_ALIGN, PS_E_UNSUPPORTED


@pytest.mark.parametrize("entry,case,overrides", CASES, ids=[f"{e}:{k}" for e, k, _ in CASES])
def test_conv_entry_refuses_before_any_launch(entry, case, overrides):
    assert refuse(entry, overrides) == EXPECTED[f"{entry}:{case}"]


@pytest.mark.parametrize("fn", list(GRIDS))
def test_predicates_and_sizers_answer_as_recorded(fn):
    assert {p: value(fn, p) for p in GRIDS[fn]} == VALUES[fn]
