"""ps_lstm_h256_f32 / ps_lstm_h256_ok without a GPU: the declarations, the weight image's layout, the predicate against the
conditions the header states, and what the entry refuses before any launch.

Non-null pointers are aligned host buffers that are never dereferenced: every call below returns before a launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from puresound_amd import _abi, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BUF = C.create_string_buffer(4096 + 256)
BUF = (C.addressof(_BUF) + 255) // 256 * 256
_ARGS = dict(gx=BUF, whh_t=None, hout=BUF, h0=None, c0=None, h_last=None, c_last=None, N=2, H=256, D=1, Q=4, q_stride=20,
             steps=20, step_stride=1, ldt=128, ldq=128, state_shift=0)


def _args(**over):
    a = _abi.LstmArgs()
    for k, v in dict(_ARGS, **over).items():
        setattr(a, k, v)
    return a


def test_both_entries_are_declared_and_bound_with_the_same_argument_counts():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "puresound_hip.h")).read(), flags=re.S)
    for name in ("ps_lstm_h256_ok", "ps_lstm_h256_f32"):
        m = re.search(rf"^int\s+{name}\s*\(([^)]*)\)\s*;", hdr, flags=re.M)
        assert m, f"{name} is not declared in the header"
        restype, argtypes = _abi.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(m.group(1).split(","))
        assert hasattr(_abi.lib(), name)
    assert _abi.lib().ps_abi_version() == 24


def _image_numpy(whh_t):
    """The header's words: element (d, w, kg, rb, g, lane, e) = W_hh[g*H + 32 w + 16 rb + lane % 16][16 kg + 4 (lane / 16) + e],
    W_hh[row][k] = whh_t[d][k][row]."""
    d, h, _ = whh_t.shape
    img = np.empty((d, h // 32, h // 16, 2, 4, 64, 4), dtype=np.float32)
    for w in range(h // 32):
        for kg in range(h // 16):
            for rb in range(2):
                for g in range(4):
                    for lane in range(64):
                        row = g * h + 32 * w + 16 * rb + lane % 16
                        k0 = 16 * kg + 4 * (lane // 16)
                        img[:, w, kg, rb, g, lane, :] = whh_t[:, k0:k0 + 4, row]
    return img


@pytest.mark.parametrize("h,d", [(256, 1), (256, 2), (192, 1), (192, 2)])
def test_pack_whh_h256_f32_is_the_documented_layout(h, d):
    whh_t = torch.arange(d * h * 4 * h, dtype=torch.float32).reshape(d, h, 4 * h)   # (every element its own value)
    img = hip.pack_whh_h256_f32(whh_t)
    assert img.dtype is torch.float32 and img.is_contiguous() and tuple(img.shape) == (d, h // 32, h // 16, 2, 4, 64, 4)
    assert np.array_equal(img.numpy(), _image_numpy(whh_t.numpy()))


def test_pack_whh_h256_f32_refuses_other_sizes():
    with pytest.raises(ValueError):
        hip.pack_whh_h256_f32(torch.zeros(1, 128, 512))
    with pytest.raises(ValueError):
        hip.pack_whh_h256_f32(torch.zeros(1, 256, 512))


# ---- the predicate over a grid, against the header's conditions restated here -----------------------------------------------
LDT = 384
WALKS = [w for last in (LDT - 9, LDT - 1, LDT)
         for w in ((4, 20, last - 59, 1), (last - 279, 1, 8, 40), (2, last - 21, 8, 3), (1, LDT, last + 1, 1))]
GRID = [(h, d) + w for h in (64, 128, 192, 256, 257) for d in (1, 2, 3) for w in WALKS]


def _header_says(n, h, d, q, q_stride, steps, step_stride, ldt, ldq=0, state_shift=0, states=False):
    span = min(n, -(-15 // q) + 1)
    return (h in (256, 192) and d in (1, 2) and min(n, q, steps, ldt) > 0 and q_stride >= 0 and step_stride >= 0
            and (q - 1) * q_stride + (steps - 1) * step_stride < ldt and state_shift in (0, 1) and (not states or ldq >= q)
            and n * q < 2 ** 30 and span * d * 4 * h * ldt * 4 < 2 ** 31)


# (the grid holds H = 128, D = 3 and, per walk, a last frame at ldt - 9, ldt - 1 and ldt)
assert [(q - 1) * qs + (steps - 1) * ss for q, qs, steps, ss in WALKS] == [LDT - 9] * 4 + [LDT - 1] * 4 + [LDT] * 4
assert any(p[0] == 128 for p in GRID) and any(p[1] == 3 for p in GRID)


@pytest.mark.parametrize("point", GRID, ids=["-".join(map(str, p)) for p in GRID])
def test_predicate_answers_as_the_header_states(point):
    h, d, q, q_stride, steps, step_stride = point
    want = _header_says(2, h, d, q, q_stride, steps, step_stride, LDT)
    a = _args(H=h, D=d, Q=q, q_stride=q_stride, steps=steps, step_stride=step_stride, ldt=LDT, ldq=0)
    assert bool(_abi.lib().ps_lstm_h256_ok(C.byref(a))) == want
    assert hip.lstm_h256_f32_ok(2, LDT, h, d, q, q_stride, steps, step_stride) == want
    assert want == (h in (192, 256) and d < 3 and (q - 1) * q_stride + (steps - 1) * step_stride < LDT)


@pytest.mark.parametrize("over,want", [
    (dict(), 1), (dict(H=192), 1), (dict(state_shift=1), 1), (dict(state_shift=2), 0), (dict(state_shift=-1), 0),
    (dict(h0=BUF, ldq=4), 1), (dict(h0=BUF, ldq=3), 0), (dict(c_last=BUF, ldq=2), 0), (dict(ldq=0), 1),
    (dict(gx=BUF + 2), 0), (dict(hout=BUF + 2), 0), (dict(gx=BUF + 4), 1), (dict(gx=None), 0), (dict(hout=None), 0),
    (dict(N=0), 0), (dict(Q=0), 0), (dict(steps=0), 0), (dict(ldt=0), 0), (dict(q_stride=-1), 0), (dict(step_stride=-1), 0),
    # the gx of the utterances 16 sequences can touch: 2 * 1 * 1024 * ldt * 4 bytes at Q = 4 -> below 2 GiB up to ldt = 262143
    (dict(ldt=262143), 1), (dict(ldt=262144), 0), (dict(N=1, ldt=262144), 1), (dict(N=64, Q=1, q_stride=0, steps=1, ldt=32767), 1),
    (dict(N=64, Q=1, q_stride=0, steps=1, ldt=32768), 0), (dict(N=1 << 20, Q=1 << 10, q_stride=0, steps=1), 0),
])
def test_predicate_on_states_alignment_and_the_size_limits(over, want):
    assert _abi.lib().ps_lstm_h256_ok(C.byref(_args(**over))) == want
    assert _abi.lib().ps_lstm_h256_ok(None) == 0


# ---- refusals ---------------------------------------------------------------------------------------------------------------
INVALID, UNSUPPORTED = -1, -3
BAD_IMAGE = "ps_lstm_h256_f32: null argument or unaligned weight image"
NO_FIT = ("ps_lstm_h256_f32: H = 256 or 192, D = 1 or 2, every frame inside the row, the gx of 16 sequences' utterances below "
          "2 GiB (ps_lstm_h256_ok)")


@pytest.mark.parametrize("case,over,image,want", [
    ("null_args", None, BUF, (INVALID, BAD_IMAGE)),
    ("null_image", {}, None, (INVALID, BAD_IMAGE)),
    ("image_misaligned", {}, BUF + 4, (INVALID, BAD_IMAGE)),
    ("image_misaligned_8", {}, BUF + 8, (INVALID, BAD_IMAGE)),
    ("null_gx", dict(gx=None), BUF, (UNSUPPORTED, NO_FIT)),
    ("null_hout", dict(hout=None), BUF, (UNSUPPORTED, NO_FIT)),
    ("H_128", dict(H=128), BUF, (UNSUPPORTED, NO_FIT)),
    ("H_64", dict(H=64), BUF, (UNSUPPORTED, NO_FIT)),
    ("H_257", dict(H=257), BUF, (UNSUPPORTED, NO_FIT)),
    ("D_three", dict(D=3), BUF, (UNSUPPORTED, NO_FIT)),
    ("last_frame_outside", dict(Q=40), BUF, (UNSUPPORTED, NO_FIT)),
    ("state_shift_2", dict(state_shift=2), BUF, (UNSUPPORTED, NO_FIT)),
    ("h0_ldq_2", dict(h0=BUF, ldq=2), BUF, (UNSUPPORTED, NO_FIT)),
], ids=lambda v: v if isinstance(v, str) and " " not in v else "")
def test_entry_refuses_before_any_launch(case, over, image, want):
    lib = _abi.lib()
    hdr = open(os.path.join(ROOT, "include", "puresound_hip.h")).read()
    assert re.search(r"PS_E_INVALID\s*=?\s*\(?-1\b", hdr) and re.search(r"PS_E_UNSUPPORTED\s*=?\s*\(?-3\b", hdr)
    rc = lib.ps_lstm_h256_f32(None if over is None else C.byref(_args(**over)), image, None)
    assert (rc, lib.ps_last_error().decode()) == want
    assert "ps_lstm_h256_ok" in NO_FIT
