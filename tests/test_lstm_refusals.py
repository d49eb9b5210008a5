"""What the recurrence entries refuse, and what the two Python predicates answer -- both without a GPU.

Refusals: every row of CASES calls one entry of the recurrence family with arguments it must turn down before any launch;
the return code and the whole ps_last_error() text are compared.  Non-null pointers are aligned host buffers that are
never dereferenced (the call returns first).  The two predicates' rows compare their return value (1 or 0) alone.
ps_lstm_fmajor_coop_f16x2_f32 prints device_cus() in the message of every shape it turns down; the number is replaced by
<CUs> before the comparison.

Not in the table, because the call is accepted or its outcome depends on device_cus():
- a null whh_t for ps_lstm_fmajor_h256_f16x2_f32 (args->whh_t is not read: the call is accepted and launches; the row of
  ps_lstm_fmajor_h256_ok records the 1) and for the cooperative entry (accepted: it goes on to size its workspace);
- H = 86 for the GRU: 3H = 258 gate rows fit the 1024 threads of a workgroup, so ps_rnn_f32 accepts it ("GRU: <= 256" in
  its message is the bound on H); H = 257 stands in its place;
- "workspace too small" and the accumulator scales of the cooperative entry, which come after its waves-per-workgroup
  choice, and every call that choice turns down for want of CUs.

Python against C: hip.lstm_fmajor_ok / hip.lstm_fmajor_h256_ok against ps_lstm_fmajor_ok / ps_lstm_fmajor_h256_ok over a
grid of sizes and walks.  hip.lstm_fmajor_h256_ok has no hidden-size parameter (its caller has H from the weight image),
so it says True at H = 64 and 128 where the C predicate says 0: DISAGREE lists those points with both answers.

EXPECTED and DISAGREE were recorded from commit 846b7ec (the library built from it, its hip.py on the CPU)."""
import ctypes as C
import re

import pytest

from puresound_amd import _abi, hip

_BUF = C.create_string_buffer(4096 + 256)
BUF = (C.addressof(_BUF) + 255) // 256 * 256   # aligned host memory; BUF + 4 etc. are the misaligned pointers
NAN = float("nan")

_ARGS = dict(gx=BUF, whh_t=BUF, hout=BUF, h0=None, c0=None, h_last=None, c_last=None, N=2, H=64, D=1, Q=4, q_stride=20,
             steps=20, step_stride=1, ldt=128, ldq=128, state_shift=0)
_FM = dict(_ARGS, H=128, ldm=512)
_H256 = dict(_ARGS, H=256, ldm=1024, image=BUF, scale=(1.0, 1.0))
# entry -> (arguments after args in call order, defaults of a valid call)
ENTRIES = {
    "ps_lstm_f32": ("stream", _ARGS),
    "ps_lstm_f16x2_f32": ("stream", _ARGS),
    "ps_rnn_f32": ("kind bhn stream", dict(_ARGS, kind=0, bhn=None)),
    "ps_lstm_fmajor_f16x2_f32": ("ldm stream", _FM),
    "ps_lstm_fmajor_ok": ("ldm", _FM),
    "ps_lstm_fmajor_h256_f16x2_f32": ("ldm image scale stream", _H256),
    "ps_lstm_fmajor_h256_ok": ("ldm", _H256),
    "ps_lstm_fmajor_coop_f16x2_f32": ("ldm image scale workspace workspace_bytes stream",
                                      dict(_H256, workspace=BUF, workspace_bytes=0)),
}
LAUNCHERS = [e for e in ENTRIES if not e.endswith("_ok")]
PREDICATES = [e for e in ENTRIES if e.endswith("_ok")]
GRU = 2


def _cases():
    out = []
    for e in ENTRIES:
        out += [(e, "null_args", dict(args=None)), (e, "null_gx", dict(gx=None)), (e, "null_hout", dict(hout=None))]
        out += [(e, f"{k}_zero", {k: 0}) for k in ("N", "H", "Q", "steps")]
        out += [(e, "D_zero", dict(D=0)), (e, "D_three", dict(D=3)), (e, "q_stride_negative", dict(q_stride=-1)),
                (e, "step_stride_negative", dict(step_stride=-1)), (e, "ldt_zero", dict(ldt=0)),
                (e, "last_frame_outside", dict(Q=40))]
    # (h256 and the cooperative entry do not read whh_t and accept the call: see the docstring)
    out += [(e, "null_whh_t", dict(whh_t=None)) for e in ENTRIES if "h256_f16x2" not in e and "coop" not in e]
    for e in ("ps_lstm_f32", "ps_lstm_f16x2_f32"):
        out += [(e, "N_65536", dict(N=65536)), (e, "H_257", dict(H=257)), (e, "h0_ldq_2", dict(h0=BUF, ldq=2)),
                (e, "state_shift_2", dict(state_shift=2))]
    e = "ps_rnn_f32"
    out += [(e, "kind_1", dict(kind=1)), (e, "gru_no_bhn", dict(kind=GRU)), (e, "c0_set", dict(c0=BUF)),
            (e, "c_last_set", dict(c_last=BUF)), (e, "state_shift_1", dict(state_shift=1)), (e, "N_65536", dict(N=65536)),
            (e, "rnn_H_257", dict(H=257)), (e, "gru_H_257", dict(kind=GRU, bhn=BUF, H=257)),
            (e, "h0_ldq_2", dict(h0=BUF, ldq=2)), (e, "h_last_ldq_2", dict(h_last=BUF, ldq=2))]
    for e in ("ps_lstm_fmajor_f16x2_f32", "ps_lstm_fmajor_ok"):
        out += [(e, "H_64", dict(H=64)), (e, "h0_set", dict(h0=BUF)), (e, "h_last_set", dict(h_last=BUF)),
                (e, "state_shift_1", dict(state_shift=1)), (e, "ldm_508", dict(ldm=508)), (e, "ldm_514", dict(ldm=514)),
                (e, "ldm_below_D_512", dict(D=2, ldm=512)), (e, "gx_misaligned", dict(gx=BUF + 4)),
                (e, "hout_misaligned", dict(hout=BUF + 2)), (e, "slab_2GiB", dict(ldt=1 << 20))]
    for e in ("ps_lstm_fmajor_h256_f16x2_f32", "ps_lstm_fmajor_h256_ok", "ps_lstm_fmajor_coop_f16x2_f32"):
        out += [(e, "H_128", dict(H=128)), (e, "ldm_1020", dict(ldm=1020)), (e, "ldm_1026", dict(ldm=1026)),
                (e, "state_shift_2", dict(state_shift=2)), (e, "h0_ldq_2", dict(h0=BUF, ldq=2)),
                (e, "c_last_ldq_2", dict(c_last=BUF, ldq=2)), (e, "gx_misaligned", dict(gx=BUF + 4)),
                (e, "hout_misaligned", dict(hout=BUF + 2))]
    for e in ("ps_lstm_fmajor_h256_f16x2_f32", "ps_lstm_fmajor_coop_f16x2_f32"):
        out += [(e, "null_image", dict(image=None)), (e, "image_misaligned", dict(image=BUF + 4)),
                (e, "null_scale", dict(scale=None))]
    e = "ps_lstm_fmajor_h256_f16x2_f32"
    out += [(e, "scale_zero", dict(scale=(0.0, 1.0))), (e, "scale_nan", dict(scale=(NAN, 1.0))),
            (e, "second_scale_zero", dict(D=2, ldm=2048, scale=(1.0, 0.0)))]
    e = "ps_lstm_fmajor_coop_f16x2_f32"
    out += [(e, "null_workspace", dict(workspace=None)), (e, "workspace_misaligned", dict(workspace=BUF + 16)),
            (e, "steps_1", dict(steps=1))]
    return out


CASES = _cases()


def refuse(entry, overrides):
    names, defaults = ENTRIES[entry]
    a = dict(defaults, **overrides)
    args = _abi.LstmArgs()
    for k, _ in _abi.LstmArgs._fields_:
        setattr(args, k, a[k])
    if a.get("scale") is not None:
        a["scale"] = (C.c_float * 2)(*a["scale"])
    lib = _abi.lib()
    rc = getattr(lib, entry)(None if "args" in overrides else C.byref(args), *[a.get(k) for k in names.split()])
    if entry in PREDICATES:
        return rc, None
    return rc, re.sub(r"at most \d+ /", "at most <CUs> /", lib.ps_last_error().decode())


EXPECTED = {
    "ps_lstm_f32:null_args": (-1, "ps_lstm_f32: null args"),
    "ps_lstm_f32:null_gx": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20)"),
    "ps_lstm_f32:null_hout": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20)"),
    "ps_lstm_f32:N_zero": (-1, "ps_lstm_f32: bad argument (N=0 H=64 D=1 Q=4 steps=20)"),
    "ps_lstm_f32:H_zero": (-1, "ps_lstm_f32: bad argument (N=2 H=0 D=1 Q=4 steps=20)"),
    "ps_lstm_f32:Q_zero": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=1 Q=0 steps=20)"),
    "ps_lstm_f32:steps_zero": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=1 Q=4 steps=0)"),
    "ps_lstm_f32:D_zero": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=0 Q=4 steps=20)"),
    "ps_lstm_f32:D_three": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=3 Q=4 steps=20)"),
    "ps_lstm_f32:q_stride_negative": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20)"),
    "ps_lstm_f32:step_stride_negative": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20)"),
    "ps_lstm_f32:ldt_zero": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20)"),
    "ps_lstm_f32:last_frame_outside": (-1, "ps_lstm_f32: the last frame 799 lies outside the row (ldt=128)"),
    "ps_lstm_f16x2_f32:null_args": (-1, "ps_lstm_f32: null args"),
    "ps_lstm_f16x2_f32:null_gx": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20)"),
    "ps_lstm_f16x2_f32:null_hout": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20)"),
    "ps_lstm_f16x2_f32:N_zero": (-1, "ps_lstm_f32: bad argument (N=0 H=64 D=1 Q=4 steps=20)"),
    "ps_lstm_f16x2_f32:H_zero": (-1, "ps_lstm_f32: bad argument (N=2 H=0 D=1 Q=4 steps=20)"),
    "ps_lstm_f16x2_f32:Q_zero": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=1 Q=0 steps=20)"),
    "ps_lstm_f16x2_f32:steps_zero": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=1 Q=4 steps=0)"),
    "ps_lstm_f16x2_f32:D_zero": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=0 Q=4 steps=20)"),
    "ps_lstm_f16x2_f32:D_three": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=3 Q=4 steps=20)"),
    "ps_lstm_f16x2_f32:q_stride_negative": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20)"),
    "ps_lstm_f16x2_f32:step_stride_negative": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20)"),
    "ps_lstm_f16x2_f32:ldt_zero": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20)"),
    "ps_lstm_f16x2_f32:last_frame_outside": (-1, "ps_lstm_f32: the last frame 799 lies outside the row (ldt=128)"),
    "ps_rnn_f32:null_args": (-1, "ps_rnn_f32: null args or unknown cell kind 0"),
    "ps_rnn_f32:null_gx": (-1,
        "ps_rnn_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20; no cell states, the GRU needs bhn)"),
    "ps_rnn_f32:null_hout": (-1,
        "ps_rnn_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20; no cell states, the GRU needs bhn)"),
    "ps_rnn_f32:N_zero": (-1,
        "ps_rnn_f32: bad argument (N=0 H=64 D=1 Q=4 steps=20; no cell states, the GRU needs bhn)"),
    "ps_rnn_f32:H_zero": (-1, "ps_rnn_f32: bad argument (N=2 H=0 D=1 Q=4 steps=20; no cell states, the GRU needs bhn)"),
    "ps_rnn_f32:Q_zero": (-1,
        "ps_rnn_f32: bad argument (N=2 H=64 D=1 Q=0 steps=20; no cell states, the GRU needs bhn)"),
    "ps_rnn_f32:steps_zero": (-1,
        "ps_rnn_f32: bad argument (N=2 H=64 D=1 Q=4 steps=0; no cell states, the GRU needs bhn)"),
    "ps_rnn_f32:D_zero": (-1,
        "ps_rnn_f32: bad argument (N=2 H=64 D=0 Q=4 steps=20; no cell states, the GRU needs bhn)"),
    "ps_rnn_f32:D_three": (-1,
        "ps_rnn_f32: bad argument (N=2 H=64 D=3 Q=4 steps=20; no cell states, the GRU needs bhn)"),
    "ps_rnn_f32:q_stride_negative": (-1,
        "ps_rnn_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20; no cell states, the GRU needs bhn)"),
    "ps_rnn_f32:step_stride_negative": (-1,
        "ps_rnn_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20; no cell states, the GRU needs bhn)"),
    "ps_rnn_f32:ldt_zero": (-1,
        "ps_rnn_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20; no cell states, the GRU needs bhn)"),
    "ps_rnn_f32:last_frame_outside": (-1, "ps_rnn_f32: a frame lies outside the row (ldt=128) or ldq=128 < Q=40"),
    "ps_lstm_fmajor_f16x2_f32:null_args": (-1,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:null_gx": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:null_hout": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:N_zero": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:H_zero": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:Q_zero": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:steps_zero": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:D_zero": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:D_three": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:q_stride_negative": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:step_stride_negative": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:ldt_zero": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:last_frame_outside": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_ok:null_args": (0, None),
    "ps_lstm_fmajor_ok:null_gx": (0, None),
    "ps_lstm_fmajor_ok:null_hout": (0, None),
    "ps_lstm_fmajor_ok:N_zero": (0, None),
    "ps_lstm_fmajor_ok:H_zero": (0, None),
    "ps_lstm_fmajor_ok:Q_zero": (0, None),
    "ps_lstm_fmajor_ok:steps_zero": (0, None),
    "ps_lstm_fmajor_ok:D_zero": (0, None),
    "ps_lstm_fmajor_ok:D_three": (0, None),
    "ps_lstm_fmajor_ok:q_stride_negative": (0, None),
    "ps_lstm_fmajor_ok:step_stride_negative": (0, None),
    "ps_lstm_fmajor_ok:ldt_zero": (0, None),
    "ps_lstm_fmajor_ok:last_frame_outside": (0, None),
    "ps_lstm_fmajor_h256_f16x2_f32:null_args": (-1,
        "ps_lstm_fmajor_h256_f16x2_f32: null argument or unaligned weight image"),
    "ps_lstm_fmajor_h256_f16x2_f32:null_gx": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_f16x2_f32:null_hout": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_f16x2_f32:N_zero": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_f16x2_f32:H_zero": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_f16x2_f32:Q_zero": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_f16x2_f32:steps_zero": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_f16x2_f32:D_zero": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_f16x2_f32:D_three": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_f16x2_f32:q_stride_negative": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_f16x2_f32:step_stride_negative": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_f16x2_f32:ldt_zero": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_f16x2_f32:last_frame_outside": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_ok:null_args": (0, None),
    "ps_lstm_fmajor_h256_ok:null_gx": (0, None),
    "ps_lstm_fmajor_h256_ok:null_hout": (0, None),
    "ps_lstm_fmajor_h256_ok:N_zero": (0, None),
    "ps_lstm_fmajor_h256_ok:H_zero": (0, None),
    "ps_lstm_fmajor_h256_ok:Q_zero": (0, None),
    "ps_lstm_fmajor_h256_ok:steps_zero": (0, None),
    "ps_lstm_fmajor_h256_ok:D_zero": (0, None),
    "ps_lstm_fmajor_h256_ok:D_three": (0, None),
    "ps_lstm_fmajor_h256_ok:q_stride_negative": (0, None),
    "ps_lstm_fmajor_h256_ok:step_stride_negative": (0, None),
    "ps_lstm_fmajor_h256_ok:ldt_zero": (0, None),
    "ps_lstm_fmajor_h256_ok:last_frame_outside": (0, None),
    "ps_lstm_fmajor_coop_f16x2_f32:null_args": (-1,
        "ps_lstm_fmajor_coop_f16x2_f32: null argument, unaligned weight image or workspace (256 bytes)"),
    "ps_lstm_fmajor_coop_f16x2_f32:null_gx": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_coop_f16x2_f32:null_hout": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_coop_f16x2_f32:N_zero": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_coop_f16x2_f32:H_zero": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_coop_f16x2_f32:Q_zero": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_coop_f16x2_f32:steps_zero": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_coop_f16x2_f32:D_zero": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_coop_f16x2_f32:D_three": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_coop_f16x2_f32:q_stride_negative": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_coop_f16x2_f32:step_stride_negative": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_coop_f16x2_f32:ldt_zero": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_coop_f16x2_f32:last_frame_outside": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_f32:null_whh_t": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20)"),
    "ps_lstm_f16x2_f32:null_whh_t": (-1, "ps_lstm_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20)"),
    "ps_rnn_f32:null_whh_t": (-1,
        "ps_rnn_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20; no cell states, the GRU needs bhn)"),
    "ps_lstm_fmajor_f16x2_f32:null_whh_t": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_ok:null_whh_t": (0, None),
    "ps_lstm_fmajor_h256_ok:null_whh_t": (1, None),
    "ps_lstm_f32:N_65536": (-1, "ps_lstm_f32: bad argument (N=65536 H=64 D=1 Q=4 steps=20)"),
    "ps_lstm_f32:H_257": (-3, "ps_lstm_f32: hidden size 257 > 256 is not supported"),
    "ps_lstm_f32:h0_ldq_2": (-1, "ps_lstm_f32: ldq=2 < Q=4"),
    "ps_lstm_f32:state_shift_2": (-1, "ps_lstm_f32: state_shift must be 0 or 1"),
    "ps_lstm_f16x2_f32:N_65536": (-1, "ps_lstm_f32: bad argument (N=65536 H=64 D=1 Q=4 steps=20)"),
    "ps_lstm_f16x2_f32:H_257": (-3, "ps_lstm_f32: hidden size 257 > 256 is not supported"),
    "ps_lstm_f16x2_f32:h0_ldq_2": (-1, "ps_lstm_f32: ldq=2 < Q=4"),
    "ps_lstm_f16x2_f32:state_shift_2": (-1, "ps_lstm_f32: state_shift must be 0 or 1"),
    "ps_rnn_f32:kind_1": (-1, "ps_rnn_f32: null args or unknown cell kind 1"),
    "ps_rnn_f32:gru_no_bhn": (-1,
        "ps_rnn_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20; no cell states, the GRU needs bhn)"),
    "ps_rnn_f32:c0_set": (-1,
        "ps_rnn_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20; no cell states, the GRU needs bhn)"),
    "ps_rnn_f32:c_last_set": (-1,
        "ps_rnn_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20; no cell states, the GRU needs bhn)"),
    "ps_rnn_f32:state_shift_1": (-1,
        "ps_rnn_f32: bad argument (N=2 H=64 D=1 Q=4 steps=20; no cell states, the GRU needs bhn)"),
    "ps_rnn_f32:N_65536": (-1,
        "ps_rnn_f32: bad argument (N=65536 H=64 D=1 Q=4 steps=20; no cell states, the GRU needs bhn)"),
    "ps_rnn_f32:rnn_H_257": (-3, "ps_rnn_f32: hidden size 257 is not supported (GRU: <= 256, RNN: <= 256)"),
    "ps_rnn_f32:gru_H_257": (-3, "ps_rnn_f32: hidden size 257 is not supported (GRU: <= 256, RNN: <= 256)"),
    "ps_rnn_f32:h0_ldq_2": (-1, "ps_rnn_f32: a frame lies outside the row (ldt=128) or ldq=2 < Q=4"),
    "ps_rnn_f32:h_last_ldq_2": (-1, "ps_rnn_f32: a frame lies outside the row (ldt=128) or ldq=2 < Q=4"),
    "ps_lstm_fmajor_f16x2_f32:H_64": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:h0_set": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:h_last_set": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:state_shift_1": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:ldm_508": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:ldm_514": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:ldm_below_D_512": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:gx_misaligned": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:hout_misaligned": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_f16x2_f32:slab_2GiB": (-3,
        "ps_lstm_fmajor_f16x2_f32: H = 128, D = 1 or 2, no states, every frame inside the row, slabs below 2 GiB "
        "(ps_lstm_fmajor_ok)"),
    "ps_lstm_fmajor_ok:H_64": (0, None),
    "ps_lstm_fmajor_ok:h0_set": (0, None),
    "ps_lstm_fmajor_ok:h_last_set": (0, None),
    "ps_lstm_fmajor_ok:state_shift_1": (0, None),
    "ps_lstm_fmajor_ok:ldm_508": (0, None),
    "ps_lstm_fmajor_ok:ldm_514": (0, None),
    "ps_lstm_fmajor_ok:ldm_below_D_512": (0, None),
    "ps_lstm_fmajor_ok:gx_misaligned": (0, None),
    "ps_lstm_fmajor_ok:hout_misaligned": (0, None),
    "ps_lstm_fmajor_ok:slab_2GiB": (0, None),
    "ps_lstm_fmajor_h256_f16x2_f32:H_128": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_f16x2_f32:ldm_1020": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_f16x2_f32:ldm_1026": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_f16x2_f32:state_shift_2": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_f16x2_f32:h0_ldq_2": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_f16x2_f32:c_last_ldq_2": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_f16x2_f32:gx_misaligned": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_f16x2_f32:hout_misaligned": (-3,
        "ps_lstm_fmajor_h256_f16x2_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, ldm >= D*4H "
        "(ps_lstm_fmajor_h256_ok)"),
    "ps_lstm_fmajor_h256_ok:H_128": (0, None),
    "ps_lstm_fmajor_h256_ok:ldm_1020": (0, None),
    "ps_lstm_fmajor_h256_ok:ldm_1026": (0, None),
    "ps_lstm_fmajor_h256_ok:state_shift_2": (0, None),
    "ps_lstm_fmajor_h256_ok:h0_ldq_2": (0, None),
    "ps_lstm_fmajor_h256_ok:c_last_ldq_2": (0, None),
    "ps_lstm_fmajor_h256_ok:gx_misaligned": (0, None),
    "ps_lstm_fmajor_h256_ok:hout_misaligned": (0, None),
    "ps_lstm_fmajor_coop_f16x2_f32:H_128": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_coop_f16x2_f32:ldm_1020": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_coop_f16x2_f32:ldm_1026": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_coop_f16x2_f32:state_shift_2": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_coop_f16x2_f32:h0_ldq_2": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_coop_f16x2_f32:c_last_ldq_2": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_coop_f16x2_f32:gx_misaligned": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_coop_f16x2_f32:hout_misaligned": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
    "ps_lstm_fmajor_h256_f16x2_f32:null_image": (-1,
        "ps_lstm_fmajor_h256_f16x2_f32: null argument or unaligned weight image"),
    "ps_lstm_fmajor_h256_f16x2_f32:image_misaligned": (-1,
        "ps_lstm_fmajor_h256_f16x2_f32: null argument or unaligned weight image"),
    "ps_lstm_fmajor_h256_f16x2_f32:null_scale": (-1,
        "ps_lstm_fmajor_h256_f16x2_f32: null argument or unaligned weight image"),
    "ps_lstm_fmajor_coop_f16x2_f32:null_image": (-1,
        "ps_lstm_fmajor_coop_f16x2_f32: null argument, unaligned weight image or workspace (256 bytes)"),
    "ps_lstm_fmajor_coop_f16x2_f32:image_misaligned": (-1,
        "ps_lstm_fmajor_coop_f16x2_f32: null argument, unaligned weight image or workspace (256 bytes)"),
    "ps_lstm_fmajor_coop_f16x2_f32:null_scale": (-1,
        "ps_lstm_fmajor_coop_f16x2_f32: null argument, unaligned weight image or workspace (256 bytes)"),
    "ps_lstm_fmajor_h256_f16x2_f32:scale_zero": (-1,
        "ps_lstm_fmajor_h256_f16x2_f32: accumulator scales must be positive"),
    "ps_lstm_fmajor_h256_f16x2_f32:scale_nan": (-1,
        "ps_lstm_fmajor_h256_f16x2_f32: accumulator scales must be positive"),
    "ps_lstm_fmajor_h256_f16x2_f32:second_scale_zero": (-1,
        "ps_lstm_fmajor_h256_f16x2_f32: accumulator scales must be positive"),
    "ps_lstm_fmajor_coop_f16x2_f32:null_workspace": (-1,
        "ps_lstm_fmajor_coop_f16x2_f32: null argument, unaligned weight image or workspace (256 bytes)"),
    "ps_lstm_fmajor_coop_f16x2_f32:workspace_misaligned": (-1,
        "ps_lstm_fmajor_coop_f16x2_f32: null argument, unaligned weight image or workspace (256 bytes)"),
    "ps_lstm_fmajor_coop_f16x2_f32:steps_1": (-3,
        "ps_lstm_fmajor_coop_f16x2_f32: ps_lstm_fmajor_h256_f16x2_f32's shapes with at most <CUs> / (D * H / 64) "
        "groups of 16 sequences and at least two steps (ps_lstm_fmajor_coop_workspace_bytes = 0)"),
}


def test_the_table_and_the_recorded_answers_name_the_same_cases():
    assert sorted(f"{e}:{k}" for e, k, _ in CASES) == sorted(EXPECTED) and len(EXPECTED) == len(CASES)


@pytest.mark.parametrize("entry,case,overrides", CASES, ids=[f"{e}:{k}" for e, k, _ in CASES])
def test_recurrence_entry_refuses_before_any_launch(entry, case, overrides):
    assert refuse(entry, overrides) == EXPECTED[f"{entry}:{case}"]


# ---- the Python predicates against the C ones ------------------------------------------------------------------------
LDT = 384
# (Q, q_stride, steps, step_stride) with the last frame at `last`: consecutive steps, consecutive sequences, both strided
WALKS = [w for last in (LDT - 9, LDT - 1, LDT)
         for w in ((4, 20, last - 59, 1), (last - 279, 1, 8, 40), (2, last - 21, 8, 3))]
GRID = [(h, d) + w for h in (64, 128, 192, 256) for d in (1, 2) for w in WALKS]


def predicates(h, d, q, q_stride, steps, step_stride):
    """-> ((Python, C) of lstm_fmajor_ok, (Python, C) of lstm_fmajor_h256_ok): aligned dummy pointers, no states"""
    args = _abi.LstmArgs()
    for k, v in dict(_ARGS, N=2, H=h, D=d, Q=q, q_stride=q_stride, steps=steps, step_stride=step_stride, ldt=LDT, ldq=0).items():
        setattr(args, k, v)
    ldm = hip.fmajor_ld(d * 4 * h)
    lib = _abi.lib()
    return ((hip.lstm_fmajor_ok(2, LDT, h, d, q, q_stride, steps, step_stride), bool(lib.ps_lstm_fmajor_ok(C.byref(args), ldm))),
            (hip.lstm_fmajor_h256_ok(2, LDT, d, q, q_stride, steps, step_stride), bool(lib.ps_lstm_fmajor_h256_ok(C.byref(args), ldm))))


# grid point -> ((Python, C) of lstm_fmajor_ok, (Python, C) of lstm_fmajor_h256_ok) where a pair disagrees
DISAGREE = {
    (64, 1, 4, 20, 316, 1): ((False, False), (True, False)),
    (64, 1, 96, 1, 8, 40): ((False, False), (True, False)),
    (64, 1, 2, 354, 8, 3): ((False, False), (True, False)),
    (64, 1, 4, 20, 324, 1): ((False, False), (True, False)),
    (64, 1, 104, 1, 8, 40): ((False, False), (True, False)),
    (64, 1, 2, 362, 8, 3): ((False, False), (True, False)),
    (64, 2, 4, 20, 316, 1): ((False, False), (True, False)),
    (64, 2, 96, 1, 8, 40): ((False, False), (True, False)),
    (64, 2, 2, 354, 8, 3): ((False, False), (True, False)),
    (64, 2, 4, 20, 324, 1): ((False, False), (True, False)),
    (64, 2, 104, 1, 8, 40): ((False, False), (True, False)),
    (64, 2, 2, 362, 8, 3): ((False, False), (True, False)),
    (128, 1, 4, 20, 316, 1): ((True, True), (True, False)),
    (128, 1, 96, 1, 8, 40): ((True, True), (True, False)),
    (128, 1, 2, 354, 8, 3): ((True, True), (True, False)),
    (128, 1, 4, 20, 324, 1): ((True, True), (True, False)),
    (128, 1, 104, 1, 8, 40): ((True, True), (True, False)),
    (128, 1, 2, 362, 8, 3): ((True, True), (True, False)),
    (128, 2, 4, 20, 316, 1): ((True, True), (True, False)),
    (128, 2, 96, 1, 8, 40): ((True, True), (True, False)),
    (128, 2, 2, 354, 8, 3): ((True, True), (True, False)),
    (128, 2, 4, 20, 324, 1): ((True, True), (True, False)),
    (128, 2, 104, 1, 8, 40): ((True, True), (True, False)),
    (128, 2, 2, 362, 8, 3): ((True, True), (True, False)),
}


def test_the_walks_cover_inside_the_last_frame_and_one_past_it():
    assert [(q - 1) * qs + (steps - 1) * ss for q, qs, steps, ss in WALKS] == [LDT - 9] * 3 + [LDT - 1] * 3 + [LDT] * 3
    assert len(GRID) == 72 and all(k in GRID for k in DISAGREE)


@pytest.mark.parametrize("point", GRID, ids=["-".join(map(str, p)) for p in GRID])
def test_python_predicates_answer_as_the_c_ones(point):
    got = predicates(*point)
    if point in DISAGREE:
        assert got == DISAGREE[point]
    else:
        assert got[0][0] == got[0][1] and got[1][0] == got[1][1]
