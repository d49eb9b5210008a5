"""Tensor-level front of the C ABI: each function enqueues exactly one entry point of
libpuresound_hip.so on the current HIP stream of the tensors' device.  PyTorch is used for device
memory and streams only; all arithmetic happens in the HIP kernels.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
import threading
from typing import Optional, Sequence

import torch

from . import _abi
from ._abi import (F16x2Range, LstmArgs, Prologue, RingPair, StateRows, TcnBlock, check, lib, padded_frames, ptr,
                   require_device, require_weight, stream_ptr)


def pack_wt(w: torch.Tensor) -> torch.Tensor:
    """[M,K] (or [M,K,1]) conv weight -> kernel layout [ceil(M/256)][ceil16(K)][256]: transposed (k-major),
    zero padded, one 256-channel output tile after the other (see ps_conv1x1_f32)."""
    if w.dim() == 3:
        w = w[:, :, 0]
    m, k = w.shape
    kp, mt = (k + 15) // 16 * 16, (m + 255) // 256
    out = torch.zeros(mt, kp, 256, dtype=torch.float32, device=w.device)
    wt = w.detach().to(torch.float32).t()  # [K, M]
    for i in range(mt):
        cols = min(256, m - i * 256)
        out[i, :k, :cols] = wt[:, i * 256:i * 256 + cols]
    return out


def _require_operand(who: str, device: torch.device, dtype: torch.dtype = torch.float32, **tensors) -> None:
    """Tensors whose pointers go into the call or its argument struct: on the input's device, `dtype`, contiguous.  Anything
    else reaches the kernel as a wild pointer: a GPU fault, not an error."""
    for name, t in tensors.items():
        if t is not None and not (t.dtype is dtype and t.is_contiguous() and t.device == device):
            raise RuntimeError(f"{who}: {name} must be a contiguous {dtype} tensor on {device} "
                               f"(got {t.dtype} on {t.device}, strides {tuple(t.stride())})")


def _stats_buffer(n: int, parts: int, device: torch.device, zeroed: bool = False) -> torch.Tensor:
    """[N, parts, 2] fp64: the partial (sum, sum of squares) slots a producer leaves for the next global norm."""
    return (torch.zeros if zeroed else torch.empty)(n, parts, 2, dtype=torch.float64, device=device)


def pad_rows(x: torch.Tensor, min_frames: int = 0) -> torch.Tensor:
    """compact [..., T] -> padded [..., ldt] (zeros in the pad); ldt also covers `min_frames`."""
    require_device(x, "pad_rows")
    x = x.contiguous()
    t = x.shape[-1]
    ldt = padded_frames(max(t, min_frames))
    out = torch.empty(*x.shape[:-1], ldt, dtype=torch.float32, device=x.device)
    rows = x.numel() // t
    check(lib().ps_pad_rows_f32(ptr(x), ptr(out), rows, t, ldt, stream_ptr(x.device)), "ps_pad_rows_f32")
    return out


def unpad_rows(x: torch.Tensor, t: int) -> torch.Tensor:
    require_device(x, "unpad_rows")
    ldt = x.shape[-1]
    out = torch.empty(*x.shape[:-1], t, dtype=torch.float32, device=x.device)
    rows = x.numel() // ldt
    check(lib().ps_unpad_rows_f32(ptr(x), ptr(out), rows, t, ldt, stream_ptr(x.device)), "ps_unpad_rows_f32")
    return out


def free_encode(wav: torch.Tensor, w: torch.Tensor, hop: int, relu: bool = False,
                min_frames=None) -> tuple[torch.Tensor, int]:
    """wav [N,L], w [C,1,win] -> (feats padded [N,C,ldt], T).  `min_frames`: int or callable T -> frames the
    consumer needs the (zero-filled) rows to hold (segment padding of the dual-path maskers)."""
    require_device(wav, "free_encode")
    require_weight(w, wav, "free_encode")
    wav = wav.contiguous()
    n, length = wav.shape
    c, _, win = w.shape
    if length < win:
        raise RuntimeError(f"free_encode: input length {length} is shorter than the window {win}")
    t = (length - win) // hop + 1
    need = min_frames(t) if callable(min_frames) else (min_frames or 0)
    ldt = padded_frames(max(t, need))
    # frames beyond T: zero when a consumer asked for them (segment padding: only those columns are cleared, the kernel
    # writes [0, T) and nothing else), otherwise never read as data
    feats = torch.empty(n, c, ldt, dtype=torch.float32, device=wav.device)
    if need > t:
        feats[..., t:].zero_()
    check(lib().ps_free_encode_f32(ptr(wav), ptr(w), ptr(feats), n, length, c, win, hop, t, ldt, int(relu),
                                   stream_ptr(wav.device)), "ps_free_encode_f32")
    return feats, t


def _decode_buffers(who: str, feats: torch.Tensor, t: int, win: int, hop: int, out: Optional[torch.Tensor]):
    """-> (out [N, (T-1)*hop+win], workspace or None, its bytes): the matrix-pipe decoder (win = 32, hop = 16, long rows)
    completes tile boundaries through a small side buffer."""
    n = feats.shape[0]
    if out is None:
        out = torch.empty(n, (t - 1) * hop + win, dtype=torch.float32, device=feats.device)
    elif tuple(out.shape) != (n, (t - 1) * hop + win) or not out.is_contiguous():
        raise RuntimeError(f"{who}: `out` must be a contiguous [N, (T-1)*hop+win] tensor")
    ws_bytes = lib().ps_free_decode_workspace_bytes(n, t, win, hop)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=feats.device) if ws_bytes else None
    return out, ws, ws_bytes


def free_decode(feats: torch.Tensor, t: int, w: torch.Tensor, hop: int, mask: Optional[torch.Tensor] = None,
                mask_act: str = "linear", out_mode: str = "none", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """feats/mask padded [N,C,ldt] -> waveform [N,(T-1)*hop+win] (into `out` if given: contiguous rows)."""
    require_device(feats, "free_decode")
    require_weight(w, feats, "free_decode")
    _require_operand("free_decode", feats.device, mask=mask)
    n, c, ldt = feats.shape
    win = w.shape[-1]
    out, ws, ws_bytes = _decode_buffers("free_decode", feats, t, win, hop, out)
    check(lib().ps_free_decode_ws_f32(ptr(feats), ptr(mask), _abi.PS_ACT[mask_act], ptr(w), ptr(out), n, c, t, ldt,
                                      win, hop, _abi.PS_OUT[out_mode], ptr(ws), ws_bytes, stream_ptr(feats.device)),
          "ps_free_decode_ws_f32")
    return out


def align_reference(ref: torch.Tensor, length: int) -> torch.Tensor:
    """_align_waveform's rule for the reference (base_nn.py:398-412): shorter than the estimate it is left-padded with
    zeros, longer it is cut."""
    have = ref.shape[-1]
    if have < length:
        return torch.nn.functional.pad(ref, (length - have, 0))
    return ref[..., :length]


def free_decode_moments(feats: torch.Tensor, t: int, w: torch.Tensor, hop: int, ref: torch.Tensor,
                        mask: Optional[torch.Tensor] = None, mask_act: str = "linear", out_mode: str = "none",
                        out: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """free_decode + the moments [N, 5] (fp64: sum a, sum b, sum a^2, sum b^2, sum ab over the (T-1)*hop+win output
    samples) of the estimate a and the reference b = ref [N, L_ref] aligned by the reference's rule (align_reference).
    One pass: the moments are the decoder's epilogue (ps_free_decode_moments_f32) where that kernel exists, otherwise
    the decoder followed by ps_wave_moments_f64."""
    require_device(feats, "free_decode_moments")
    require_device(ref, "free_decode_moments")
    require_weight(w, feats, "free_decode_moments")
    _require_operand("free_decode_moments", feats.device, mask=mask)
    if ref.device != feats.device:   # (its rows may be strided: ldr goes with the pointer)
        raise RuntimeError(f"free_decode_moments: ref must be on {feats.device} (got {ref.device})")
    n, c, ldt = feats.shape
    win = w.shape[-1]
    lout = (t - 1) * hop + win
    if ref.dim() != 2 or ref.shape[0] != n or ref.dtype != torch.float32 or ref.shape[1] < 1:
        raise RuntimeError("free_decode_moments: `ref` must be an fp32 [N, L_ref] tensor")
    parts = lib().ps_free_decode_moments_parts(n, c, t, ldt, win, hop)
    if parts == 0:
        out = free_decode(feats, t, w, hop, mask, mask_act, out_mode, out)
        return out, wave_moments(out, align_reference(ref, lout))
    out, ws, ws_bytes = _decode_buffers("free_decode_moments", feats, t, win, hop, out)
    if ref.stride(1) != 1:
        ref = ref.contiguous()
    part = torch.empty(n, parts, 5, dtype=torch.float64, device=feats.device)
    check(lib().ps_free_decode_moments_f32(ptr(feats), ptr(mask), _abi.PS_ACT[mask_act], ptr(w), ptr(out), n, c, t, ldt,
                                           win, hop, _abi.PS_OUT[out_mode], ptr(ref), ref.stride(0), ref.shape[1],
                                           ptr(part), ptr(ws), ws_bytes, stream_ptr(feats.device)),
          "ps_free_decode_moments_f32")
    return out, part.sum(dim=1)


def frame(wav: torch.Tensor, win: int, hop: int) -> tuple[torch.Tensor, int]:
    """wav [N,L] -> (frames padded [N,win,ldt], T): frames[n][k][t] = wav[n][t*hop+k]."""
    require_device(wav, "frame")
    wav = wav.contiguous()
    n, length = wav.shape
    if length < win:
        raise RuntimeError(f"frame: input length {length} is shorter than the window {win}")
    t = (length - win) // hop + 1
    ldt = padded_frames(t)
    out = torch.empty(n, win, ldt, dtype=torch.float32, device=wav.device)
    check(lib().ps_frame_f32(ptr(wav), ptr(out), n, length, win, hop, t, ldt, stream_ptr(wav.device)), "ps_frame_f32")
    return out, t


def complex_mask(feats: torch.Tensor, mask: torch.Tensor, mask_act: str = "linear") -> torch.Tensor:
    """[re;im] channel halves, padded [N,2H,ldt] x mask [N,2H,ldt] -> complex product, same layout."""
    require_device(feats, "complex_mask")
    n, c2, ldt = feats.shape
    if c2 % 2 or mask.shape != feats.shape:
        raise RuntimeError("complex_mask: feats and mask must be [N, 2*half, ldt] with equal shapes")
    out = torch.empty_like(feats)
    check(lib().ps_complex_mask_f32(ptr(feats), ptr(mask), ptr(out), n, c2 // 2, ldt, _abi.PS_ACT[mask_act],
                                    stream_ptr(feats.device)), "ps_complex_mask_f32")
    return out


def polar_mask(feats: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """[re;im] channel halves, padded [N,2H,ldt], x mask in the same layout -> polar-form product (base_nn.py:161-190)."""
    require_device(feats, "polar_mask")
    n, c2, ldt = feats.shape
    if c2 % 2 or mask.shape != feats.shape:
        raise RuntimeError("polar_mask: feats and mask must be [N, 2*half, ldt] with equal shapes")
    out = torch.empty_like(feats)
    check(lib().ps_polar_mask_f32(ptr(feats), ptr(mask), ptr(out), n, c2 // 2, ldt, stream_ptr(feats.device)),
          "ps_polar_mask_f32")
    return out


def magphase(spec: torch.Tensor, take_sqrt: bool) -> torch.Tensor:
    """analysis product [re;im] padded [N,2H,ldt] -> [mags;phase] in the same layout (lobe/encoder.py:384-389)."""
    require_device(spec, "magphase")
    n, c2, ldt = spec.shape
    out = torch.empty_like(spec)
    check(lib().ps_magphase_f32(ptr(spec), ptr(out), n, c2 // 2, ldt, int(take_sqrt), stream_ptr(spec.device)),
          "ps_magphase_f32")
    return out


def istft_ola(frames: torch.Tensor, t: int, window: torch.Tensor, hop: int, out_mode: str = "none") -> torch.Tensor:
    """synthesis frames padded [N,n_fft,ldt] -> waveform [N,(T-1)*hop+n_fft] (window, /n_fft, OLA, /window-sum)."""
    require_device(frames, "istft_ola")
    _require_operand("istft_ola", frames.device, window=window)
    n, n_fft, ldt = frames.shape
    out = torch.empty(n, (t - 1) * hop + n_fft, dtype=torch.float32, device=frames.device)
    check(lib().ps_istft_ola_f32(ptr(frames), ptr(window), ptr(out), n, n_fft, hop, t, ldt, _abi.PS_OUT[out_mode],
                                 stream_ptr(frames.device)), "ps_istft_ola_f32")
    return out


def make_prologue(norm: int = 0, prelu: bool = False, stats: Optional[torch.Tensor] = None, count: float = 0.0,
                  eps: float = 1e-8, gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None,
                  slope: Optional[torch.Tensor] = None, pre_relu: bool = False, post_tanh: bool = False) -> Prologue:
    p = Prologue()
    p.pre_relu, p.post_tanh = int(pre_relu), int(post_tanh)
    p.norm, p.prelu = norm, int(prelu)
    p.stats = ptr(stats)
    p.parts = 0 if stats is None else stats.shape[1]
    p.count, p.eps = float(count), float(eps)
    p.gamma, p.beta, p.slope = ptr(gamma), ptr(beta), ptr(slope)
    return p


def conv1x1(x: torch.Tensor, t: int, wt: torch.Tensor, m: int, pro: Optional[Prologue] = None,
            bias: Optional[torch.Tensor] = None, bias_n: Optional[torch.Tensor] = None,
            res: Optional[torch.Tensor] = None, want_stats: bool = False,
            out: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, Optional[torch.Tensor]]:
    """x padded [N,K,ldt], wt packed (pack_wt) -> y padded [N,M,ldt] (+ partial stats [N,parts,2] fp64)."""
    require_device(x, "conv1x1")
    n, k, ldt = x.shape
    y = out if out is not None else torch.zeros(n, m, ldt, dtype=torch.float32, device=x.device)
    stats = _stats_buffer(n, lib().ps_conv1x1_stats_parts(m, t), x.device, zeroed=True) if want_stats else None
    check(lib().ps_conv1x1_f32(ptr(x), ptr(wt), ptr(y), n, k, m, t, ldt, C.byref(pro) if pro is not None else None,
                               ptr(bias), ptr(bias_n), ptr(res), ptr(stats), stream_ptr(x.device)), "ps_conv1x1_f32")
    return y, stats


def _split_planes(rest: torch.Tensor, dtype: torch.dtype, planes: int) -> list:
    """fp32 `rest` -> `planes` tensors of `dtype`: each holds the rounding of what the planes before it left over."""
    out = []
    for _ in range(planes):
        h = rest.to(dtype)
        out.append(h)
        rest = rest - h.float()
    return out


def _f16_weight_exponent(w: torch.Tensor, who: str) -> int:
    """w_exp that puts max |2^w_exp w| into [2^13, 2^14) (0 for an all-zero weight); reads the maximum back to the host."""
    wmax = float(w.detach().abs().max())
    if not (wmax < float("inf")):
        raise ValueError(f"{who}: the weight holds inf / NaN")
    return 13 - math.frexp(wmax)[1] + 1 if wmax > 0 else 0  # frexp: wmax = f * 2^e, f in [0.5, 1)


def _plane_image(w: torch.Tensor, dtype: torch.dtype, planes: int) -> torch.Tensor:
    """[M, K] fp32 -> the conv1x1 plane image [ceil(M/256)][ceil(K/16)][planes][256][16], zero padded"""
    m, k = w.shape
    mt, ks = (m + 255) // 256, (k + 15) // 16
    rest = torch.zeros(mt * 256, ks * 16, dtype=torch.float32, device=w.device)
    rest[:m, :k] = w
    img = torch.stack(_split_planes(rest, dtype, planes), 0).reshape(planes, mt, 256, ks, 16)
    return img.permute(1, 3, 0, 2, 4).contiguous()


def pack_wt_bf16(w: torch.Tensor, planes: int) -> torch.Tensor:
    """[M,K] (or [M,K,1]) fp32 weight -> bf16 plane image [ceil(M/256)][ceil(K/16)][planes][256][16] for
    ps_conv1x1_bf16_f32: plane p holds bf16 of what the planes before it left over (planes = 1: plain rounding)."""
    if w.dim() == 3:
        w = w[:, :, 0]
    return _plane_image(w.detach().float(), torch.bfloat16, planes)


def pack_wt_f16x2(w: torch.Tensor) -> tuple[torch.Tensor, int]:
    """[M,K] (or [M,K,1]) fp32 weight -> (two-plane fp16 image [ceil(M/256)][ceil(K/16)][2][256][16] of 2^w_exp * W, w_exp)
    for ps_conv1x1_f16x2_f32: plane 0 = fp16(w'), plane 1 = fp16(w' - plane 0); w_exp puts max |w'| into [2^13, 2^14).
    (Reads the maximum back to the host: plan-build time only.)"""
    if w.dim() == 3:
        w = w[:, :, 0]
    w_exp = _f16_weight_exponent(w, "pack_wt_f16x2")
    return _plane_image(torch.ldexp(w.detach().float(), torch.tensor(w_exp, device=w.device)), torch.float16, 2), w_exp


def _f16x2_range(w_exp: int, x_bound: float, x_amax: Optional[torch.Tensor], y_amax: Optional[torch.Tensor],
                 amax_map: Optional[tuple] = None) -> F16x2Range:
    rng = F16x2Range(int(w_exp), float(x_bound), ptr(x_amax), x_amax.shape[1] if x_amax is not None else 0, ptr(y_amax))
    if amax_map is not None:
        rng.amax_mul, rng.amax_add = float(amax_map[0]), float(amax_map[1])
    return rng


def conv1x1_f16x2(x: torch.Tensor, t: int, wt_planes: torch.Tensor, w_exp: int, m: int,
                  pro: Optional[Prologue] = None, bias: Optional[torch.Tensor] = None,
                  bias_n: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
                  want_stats: bool = False, out: Optional[torch.Tensor] = None, x_bound: float = 0.0,
                  x_amax: Optional[torch.Tensor] = None, want_amax: bool = False,
                  amax_map: Optional[tuple] = None):
    """ps_conv1x1_f32's contract in the fp16x2 arithmetic (ps_conv1x1_f16x2_f32; weights from pack_wt_f16x2).
    x_bound / x_amax: how the activations are brought into fp16's range (see include/puresound_hip.h); x_amax is an
    [N, parts] tensor of partial maxima (absmax(), or the y_amax of the producing launch); amax_map = (mul, add): the
    maxima are those of x in front of an affine prologue whose output is bounded by mul * max|x| + add.
    Returns (y, stats, y_amax)."""
    require_device(x, "conv1x1_f16x2")
    n, k, ldt = x.shape
    y = out if out is not None else torch.empty(n, m, ldt, dtype=torch.float32, device=x.device)
    stats = _stats_buffer(n, lib().ps_conv1x1_stats_parts(m, t), x.device, zeroed=True) if want_stats else None
    amax = None
    if want_amax:
        amax = torch.zeros(n, lib().ps_conv1x1_stats_parts(m, t), dtype=torch.float32, device=x.device)
    if x_amax is not None:
        require_device(x_amax, "conv1x1_f16x2 (x_amax)")
        if x_amax.dim() != 2 or x_amax.shape[0] != n or not x_amax.is_contiguous():
            raise ValueError(f"conv1x1_f16x2: x_amax must be a contiguous [N={n}, parts] tensor, got {tuple(x_amax.shape)}")
    rng = _f16x2_range(w_exp, x_bound, x_amax, amax, amax_map)
    check(lib().ps_conv1x1_f16x2_f32(ptr(x), ptr(wt_planes), C.byref(rng), ptr(y), n, k, m, t, ldt,
                                     C.byref(pro) if pro is not None else None, ptr(bias), ptr(bias_n), ptr(res),
                                     ptr(stats), stream_ptr(x.device)), "ps_conv1x1_f16x2_f32")
    return y, stats, amax


FMAJOR_PAD = int(os.environ.get("PS_FMAJOR_PAD", "0"))   # floats between the M outputs of consecutive frames


def fmajor_ld(m: int) -> int:
    """Frame stride of the frame-major gate pre-activations: M (+ PS_FMAJOR_PAD floats; a 256-byte skew between frames was
    tried against a suspected 4 KiB channel stride and made no difference: 1.40 / 1.39 / 1.31 ms per launch at 64 / 0 / 32)."""
    return m + FMAJOR_PAD


def conv1x1_f16x2_fmajor_ok(n: int, k: int, m: int, t: int, ldt: int) -> bool:
    return bool(lib().ps_conv1x1_f16x2_fmajor_ok(n, k, m, t, ldt, fmajor_ld(m)))


def conv1x1_f16x2_fmajor(x: torch.Tensor, t: int, wt_planes: torch.Tensor, w_exp: int, m: int,
                         bias: Optional[torch.Tensor] = None, x_bound: float = 0.0,
                         x_amax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ps_conv1x1_f16x2_fmajor_f32: the fp16x2 GEMM writing y FRAME-MAJOR, a [N, ldt, M] view of rows fmajor_ld(M) apart
    (the gate pre-activations of lstm_fmajor).  Raises when the launch does not qualify (conv1x1_f16x2_fmajor_ok)."""
    require_device(x, "conv1x1_f16x2_fmajor")
    n, k, ldt = x.shape
    ldm = fmajor_ld(m)
    y = torch.empty(n, ldt, ldm, dtype=torch.float32, device=x.device)[..., :m]
    rng = _f16x2_range(w_exp, x_bound, x_amax, None)
    check(lib().ps_conv1x1_f16x2_fmajor_f32(ptr(x), ptr(wt_planes), C.byref(rng), ptr(y), n, k, m, t, ldt, ldm, ptr(bias),
                                            stream_ptr(x.device)), "ps_conv1x1_f16x2_fmajor_f32")
    return y


def conv1x1_f16x2_ln_ok(n: int, k: int, c: int, t: int) -> bool:
    return bool(lib().ps_conv1x1_f16x2_ln_ok(n, k, c, t))


def conv1x1_f16x2_ln(x: torch.Tensor, t: int, wt_planes: torch.Tensor, w_exp: int, c: int, bias: Optional[torch.Tensor],
                     gamma: torch.Tensor, beta: torch.Tensor, eps: float, res: Optional[torch.Tensor],
                     x_bound: float = 0.0, x_amax: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None, want_amax: bool = False, pro: Optional[Prologue] = None,
                     res_inside: bool = False):
    """ps_conv1x1_f16x2_ln_f32: y = res + LayerNorm_channels(W x + b) in one launch (C = 128; wt_planes = pack_wt_f16x2 of
    W zero padded to 256 rows), or y = LayerNorm(W x + b + res) with res_inside; `pro`: affine / PReLU prologue on x.
    Raises when the launch does not qualify (conv1x1_f16x2_ln_ok).  want_amax: returns (y, [N, parts] partial maxima of
    |y|) -- the x_amax of the next fp16x2 GEMM."""
    require_device(x, "conv1x1_f16x2_ln")
    n, k, ldt = x.shape
    y = out if out is not None else torch.empty(n, c, ldt, dtype=torch.float32, device=x.device)
    if res is not None and (tuple(res.shape) != (n, c, ldt) or not res.is_contiguous()):
        raise ValueError(f"conv1x1_f16x2_ln: the residual must be a contiguous {(n, c, ldt)} tensor")
    amax = torch.zeros(n, lib().ps_conv1x1_stats_parts(256, t), dtype=torch.float32, device=x.device) if want_amax else None
    rng = _f16x2_range(w_exp, x_bound, x_amax, amax)
    check(lib().ps_conv1x1_f16x2_ln_f32(ptr(x), ptr(wt_planes), C.byref(rng), ptr(y), n, k, c, t, ldt,
                                        C.byref(pro) if pro is not None else None, ptr(bias), ptr(gamma), ptr(beta), float(eps),
                                        ptr(res), int(res_inside), stream_ptr(x.device)), "ps_conv1x1_f16x2_ln_f32")
    return (y, amax) if want_amax else y


def absmax(x: torch.Tensor, t: int) -> torch.Tensor:
    """padded rows [N, C, ldt] -> [N, ps_absmax_parts()] partial maxima of |x| over the t valid frames."""
    require_device(x, "absmax")
    n, c, ldt = x.shape
    out = torch.empty(n, lib().ps_absmax_parts(), dtype=torch.float32, device=x.device)
    check(lib().ps_absmax_f32(ptr(x), ptr(out), n, c, t, ldt, stream_ptr(x.device)), "ps_absmax_f32")
    return out


def conv1x1_bf16(x: torch.Tensor, t: int, wt_planes: torch.Tensor, m: int, pro: Optional[Prologue] = None,
                 bias: Optional[torch.Tensor] = None, bias_n: Optional[torch.Tensor] = None,
                 res: Optional[torch.Tensor] = None, want_stats: bool = False,
                 out: Optional[torch.Tensor] = None,
                 out_dtype: torch.dtype = torch.float32) -> tuple[torch.Tensor, Optional[torch.Tensor]]:
    """ps_conv1x1_f32's contract on the bf16 matrix pipe; the plane count is read off wt_planes (pack_wt_bf16).
    A torch.bfloat16 `x` / `out` (or out_dtype) selects bf16 activation rows (ps_conv1x1_bf16_io, planes = 1)."""
    require_device(x, "conv1x1_bf16", allow_bf16=True)
    n, k, ldt = x.shape
    planes = wt_planes.shape[2]
    y = out if out is not None else torch.empty(n, m, ldt, dtype=out_dtype, device=x.device)
    if res is not None and res.dtype != y.dtype:
        raise ValueError(f"conv1x1_bf16: the residual rows must have the output's dtype ({y.dtype}), got {res.dtype}")
    stats = _stats_buffer(n, lib().ps_conv1x1_stats_parts(m, t), x.device, zeroed=True) if want_stats else None
    check(lib().ps_conv1x1_bf16_io(ptr(x), int(x.dtype == torch.bfloat16), ptr(wt_planes), ptr(y),
                                   int(y.dtype == torch.bfloat16), n, k, m, t, ldt, planes,
                                   C.byref(pro) if pro is not None else None, ptr(bias), ptr(bias_n), ptr(res),
                                   ptr(stats), stream_ptr(x.device)), "ps_conv1x1_bf16_io")
    return y, stats


def dwconv(x: torch.Tensor, t: int, w: torch.Tensor, b: Optional[torch.Tensor], dilation: int, left: int,
           pro: Optional[Prologue] = None, want_stats: bool = False,
           out_dtype: Optional[torch.dtype] = None, want_amax: bool = False) -> tuple[torch.Tensor, Optional[torch.Tensor]]:
    """x padded [N,H,ldt] (fp32 or bf16 rows), w [H,1,P] -> y padded [N,H,ldt] (+ partial stats; with want_amax the
    partial maxima of |y| [N, parts] instead: ps_dwconv_amax_f32, fp32 rows, P = 3, 2 * dilation <= 256)."""
    require_device(x, "dwconv", allow_bf16=True)
    _require_operand("dwconv", x.device, w=w, b=b)
    n, h, ldt = x.shape
    p = w.shape[-1]
    y = torch.zeros(n, h, ldt, dtype=out_dtype or x.dtype, device=x.device)
    if want_amax:
        amax = torch.empty(n, lib().ps_dwconv_stats_parts(h, t), dtype=torch.float32, device=x.device)
        check(lib().ps_dwconv_amax_f32(ptr(x), ptr(w), ptr(b), ptr(y), n, h, t, ldt, p, dilation, left,
                                       C.byref(pro) if pro is not None else None, ptr(amax), stream_ptr(x.device)),
              "ps_dwconv_amax_f32")
        return y, amax
    stats = _stats_buffer(n, lib().ps_dwconv_stats_parts(h, t), x.device, zeroed=True) if want_stats else None
    check(lib().ps_dwconv_io(ptr(x), int(x.dtype == torch.bfloat16), ptr(w), ptr(b), ptr(y),
                             int(y.dtype == torch.bfloat16), n, h, t, ldt, p, dilation, left,
                             C.byref(pro) if pro is not None else None, ptr(stats), stream_ptr(x.device)),
          "ps_dwconv_io")
    return y, stats


def attn_stats_pool(logits: torch.Tensor, x: torch.Tensor, t: int, eps: float = 1e-12,
                    lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """attention logits / features padded [N,C,ldt] -> [N,2C] = cat(weighted mean, weighted std); `lengths` [N]:
    relative lengths, frames t with float(t) >= lengths[n] * T are masked out (lobe/pooling.py:100-107)."""
    require_device(x, "attn_stats_pool")
    n, c, ldt = x.shape
    out = torch.empty(n, 2 * c, dtype=torch.float32, device=x.device)
    if lengths is not None:
        require_device(lengths, "attn_stats_pool")
        if lengths.shape != (n,):
            raise RuntimeError("attn_stats_pool: lengths must be [N]")
        lengths = lengths.to(torch.float32).contiguous()
    check(lib().ps_attn_stats_pool_len_f32(ptr(logits), ptr(x), ptr(lengths), ptr(out), n, c, t, ldt, float(eps),
                                           stream_ptr(x.device)), "ps_attn_stats_pool_len_f32")
    return out


def attn_weights(logits: torch.Tensor, t: int, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """padded attention logits [N,C,ldt] (+ relative lengths [N]) -> padded softmax over the valid frames."""
    require_device(logits, "attn_weights")
    n, c, ldt = logits.shape
    out = torch.empty_like(logits)
    if lengths is not None:
        lengths = lengths.detach().to(device=logits.device, dtype=torch.float32).contiguous()
        if lengths.numel() != n:
            raise RuntimeError(f"attn_weights: lengths must hold one value per utterance ({n}), got {tuple(lengths.shape)}")
    check(lib().ps_attn_weights_f32(ptr(logits), ptr(lengths), ptr(out), n, c, t, ldt, stream_ptr(logits.device)),
          "ps_attn_weights_f32")
    return out


COOP_LSTM = os.environ.get("PS_COOP_LSTM", "1") != "0"   # the process default; 0: always the streamed-weight kernel
_COOP_OFF = type("_CoopOff", (threading.local,), {"depth": 0})()   # .depth: coop_lstm_off() blocks this thread is inside
_COOP_LAST = [None]
RNN_KINDS = {"RNN": 0, "GRU": 2}


@contextlib.contextmanager
def coop_lstm_off():
    """Inside the block, and in this thread only, lstm_fmajor_h256 takes the streamed-weight kernel whatever COOP_LSTM says."""
    _COOP_OFF.depth += 1
    try:
        yield
    finally:
        _COOP_OFF.depth -= 1


def _lstm_state_args(who: str, a: LstmArgs, n: int, rows: int, q: int, h0, c0, want_state: bool, state_out, device,
                     cell: bool = True):
    """Fills a.h0 / c0 / h_last / c_last / ldq of a launch; returns the final-state pair (h, c) or None (cell = False, the
    RNN / GRU: no c).  All state tensors of one launch share the row stride ldq (the kernels read and write every one of
    them with it)."""
    ldq = padded_frames(q)
    h_last, c_last = state_out if state_out is not None else (None, None)
    _require_operand(who, device, h0=h0, c0=c0, state_out_h=h_last, state_out_c=c_last)
    for name, t in (("h0", h0), ("c0", c0), ("state_out[0]", h_last), ("state_out[1]", c_last)):
        if t is not None and (t.dim() != 3 or tuple(t.shape[:2]) != (n, rows) or t.shape[2] < q):
            raise RuntimeError(f"{who}: {name} must be a contiguous state tensor [N, D*H, ldq >= Q]")
    if h0 is not None:
        ldq = h0.shape[2]
    elif c0 is not None:
        ldq = c0.shape[2]
    if (h0 is not None and c0 is not None) and h0.shape[2] != c0.shape[2]:
        raise RuntimeError(f"{who}: h0 and c0 must share ldq")
    if state_out is not None:
        if (h_last.shape[2] != ldq and (h0 is not None or c0 is not None)) or c_last.shape[2] != h_last.shape[2]:
            raise RuntimeError(f"{who}: state_out must share ldq with h0/c0")
        ldq = h_last.shape[2]
    elif want_state:
        h_last = torch.zeros(n, rows, ldq, dtype=torch.float32, device=device)
        c_last = torch.zeros_like(h_last) if cell else None
    a.h0, a.c0, a.h_last, a.c_last = ptr(h0), ptr(c0), ptr(h_last), ptr(c_last)
    a.ldq = ldq
    return (h_last, c_last) if h_last is not None else None


def _lstm_args(who: str, gx: torch.Tensor, n: int, ldt: int, whh_t, out, hidden: int, dirs: int, walk: tuple, h0=None, c0=None,
               want_state: bool = False, state_shift: int = 0, state_out=None, cell: bool = True):
    """The ps_lstm_args of every recurrence launch -> (args, hout, final states or None).  walk = (Q, q_stride, steps,
    step_stride); out: where hout [N, D*H, ldt] goes (None = a new tensor)."""
    _require_operand(who, gx.device, whh_t=whh_t, out=out)
    hout = out if out is not None else torch.empty(n, dirs * hidden, ldt, dtype=torch.float32, device=gx.device)
    if tuple(hout.shape) != (n, dirs * hidden, ldt):
        raise RuntimeError(f"{who}: out must be a contiguous [N, D*H, ldt] tensor")
    a = LstmArgs()
    a.gx, a.whh_t, a.hout = ptr(gx), ptr(whh_t), ptr(hout)
    a.N, a.H, a.D, a.ldt, a.state_shift = n, hidden, dirs, ldt, state_shift
    a.Q, a.q_stride, a.steps, a.step_stride = walk
    state = _lstm_state_args(who, a, n, dirs * hidden, walk[0], h0, c0, want_state, state_out, gx.device, cell)
    return a, hout, state


def _frame_rows(who: str, gx_fm: torch.Tensor) -> int:
    """ldm of frame-major gate pre-activations [N, ldt, D*4H]: the frames may be padded rows (stride(1) >= D*4H)"""
    ldm = gx_fm.stride(1)
    if gx_fm.stride(2) != 1 or gx_fm.stride(0) != gx_fm.shape[1] * ldm:
        raise RuntimeError(f"{who}: gx must be a [N, ldt, :D*4H] view of contiguous frame rows")
    return ldm


def lstm(gx: torch.Tensor, whh_t: torch.Tensor, hidden: int, dirs: int, q: int, q_stride: int, steps: int,
         step_stride: int, h0: Optional[torch.Tensor] = None, c0: Optional[torch.Tensor] = None,
         want_state: bool = False, state_shift: int = 0, state_out: Optional[tuple] = None, f16x2: bool = False,
         out: Optional[torch.Tensor] = None):
    """LSTM recurrence over gate pre-activations gx padded [N,D*4H,ldt] -> hout [N,D*H,ldt]
    (+ final (h, c) in state layout [N,D*H,ldq] when want_state / state_out).  f16x2: ps_lstm_f16x2_f32 (the
    recurrent product in two fp16 terms per operand where a kernel for it exists, else the fp32 kernels)."""
    require_device(gx, "lstm")
    n, rows, ldt = gx.shape
    if rows != dirs * 4 * hidden or tuple(whh_t.shape) != (dirs, hidden, 4 * hidden):
        raise RuntimeError("lstm: gx must be [N, D*4H, ldt] and whh_t [D, H, 4H]")
    _require_operand("lstm", gx.device, gx=gx)
    a, hout, state = _lstm_args("lstm", gx, n, ldt, whh_t, out, hidden, dirs, (q, q_stride, steps, step_stride), h0, c0,
                                want_state, state_shift, state_out)
    if f16x2:
        check(lib().ps_lstm_f16x2_f32(C.byref(a), stream_ptr(gx.device)), "ps_lstm_f16x2_f32")
    else:
        check(lib().ps_lstm_f32(C.byref(a), stream_ptr(gx.device)), "ps_lstm_f32")
    return hout, state


def lstm_rows(gx: torch.Tensor, whh_t: torch.Tensor, hidden: int, dirs: int, q: int, q_stride: int, steps: int,
              step_stride: int, steps_rows: torch.Tensor, h0: Optional[torch.Tensor] = None,
              c0: Optional[torch.Tensor] = None, want_state: bool = False, state_out: Optional[tuple] = None,
              out: Optional[torch.Tensor] = None):
    """ps_lstm_rows_f32: lstm() with a step count per utterance (steps_rows int32 [N] on the device, clamped to [0, steps]):
    row n is, on its first steps_rows[n] steps, lstm() of that utterance alone with that many steps -- direction 1 starts at
    the row's own last step -- and hout is 0.0 at the frames of the steps behind them; gx there is never read.  Final states:
    after the row's own last step."""
    require_device(gx, "lstm_rows")
    n, rows, ldt = gx.shape
    if rows != dirs * 4 * hidden or tuple(whh_t.shape) != (dirs, hidden, 4 * hidden):
        raise RuntimeError("lstm_rows: gx must be [N, D*4H, ldt] and whh_t [D, H, 4H]")
    _require_operand("lstm_rows", gx.device, gx=gx)
    _require_limits("lstm_rows", steps_rows, n, gx.device)
    a, hout, state = _lstm_args("lstm_rows", gx, n, ldt, whh_t, out, hidden, dirs, (q, q_stride, steps, step_stride), h0, c0,
                                want_state, 0, state_out)
    check(lib().ps_lstm_rows_f32(C.byref(a), ptr(steps_rows), stream_ptr(gx.device)), "ps_lstm_rows_f32")
    return hout, state


def rnn(gx: torch.Tensor, whh_t: torch.Tensor, kind: str, hidden: int, dirs: int, q: int, q_stride: int, steps: int,
        step_stride: int, bhn: Optional[torch.Tensor] = None, h0: Optional[torch.Tensor] = None, want_state: bool = False):
    """ps_rnn_f32: the recurrence of nn.RNN (tanh) / nn.GRU over pre-activations gx padded [N, D*G, ldt] (G = H or 3H) ->
    hout [N, D*H, ldt].  h0: initial state in the state layout [N, D*H, ldq >= Q] (None = zeros); want_state: returns
    (hout, h_last) with h_last in the same layout (ldq of h0, else padded_frames(Q))."""
    require_device(gx, "rnn")
    n, rows, ldt = gx.shape
    g = (3 if kind == "GRU" else 1) * hidden
    if kind not in RNN_KINDS or rows != dirs * g or tuple(whh_t.shape) != (dirs, hidden, g):
        raise RuntimeError("rnn: kind RNN / GRU, gx [N, D*G, ldt], whh_t [D, H, G]")
    _require_operand("rnn", gx.device, gx=gx, bhn=bhn)
    if bhn is not None and tuple(bhn.shape) != (dirs, hidden):
        raise RuntimeError("rnn: bhn must be a contiguous [D, H] tensor")
    a, hout, state = _lstm_args("rnn", gx, n, ldt, whh_t, None, hidden, dirs, (q, q_stride, steps, step_stride), h0, None,
                                want_state, cell=False)
    check(lib().ps_rnn_f32(C.byref(a), RNN_KINDS[kind], ptr(bhn), stream_ptr(gx.device)), "ps_rnn_f32")
    return (hout, state[0]) if want_state else hout


def lstm_fmajor_ok(n: int, ldt: int, hidden: int, dirs: int, q: int, q_stride: int, steps: int, step_stride: int) -> bool:
    """Does ps_lstm_fmajor_f16x2_f32 take this pass?  (The shape / stride conditions of lstm_fmajor_fits in csrc/rnn.hip: H =
    128, slabs < 2 GiB; tests/test_lstm_refusals.py holds it against ps_lstm_fmajor_ok.)"""
    if hidden != 128 or dirs not in (1, 2) or (q - 1) * q_stride + (steps - 1) * step_stride >= ldt:
        return False
    return ldt * fmajor_ld(dirs * 512) * 4 < 2 ** 31


def lstm_fmajor(gx_fm: torch.Tensor, whh_t: torch.Tensor, hidden: int, dirs: int, q: int, q_stride: int, steps: int,
                step_stride: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ps_lstm_fmajor_f16x2_f32: LSTM recurrence over FRAME-MAJOR gate pre-activations gx [N, ldt, D*4H] (from
    conv1x1_f16x2_fmajor; the frames may be padded rows: stride(1) >= D*4H) -> hout [N, D*H, ldt]; H = 128, zero initial
    states, fp16x2 recurrent product."""
    require_device(gx_fm, "lstm_fmajor")
    n, ldt, rows = gx_fm.shape
    if rows != dirs * 4 * hidden or tuple(whh_t.shape) != (dirs, hidden, 4 * hidden):
        raise RuntimeError("lstm_fmajor: gx must be [N, ldt, D*4H] and whh_t [D, H, 4H]")
    ldm = _frame_rows("lstm_fmajor", gx_fm)
    a, hout, _ = _lstm_args("lstm_fmajor", gx_fm, n, ldt, whh_t, out, hidden, dirs, (q, q_stride, steps, step_stride))
    check(lib().ps_lstm_fmajor_f16x2_f32(C.byref(a), ldm, stream_ptr(gx_fm.device)), "ps_lstm_fmajor_f16x2_f32")
    return hout


def pack_whh_h256(whh_t: torch.Tensor):
    """weight_hh^T [D, H, 4H], H = 256 or 192 -> (fp16 image [D, H/32, H/32, 2, 4, 2, 64, 8], acc scales [D] as a Python list)
    for lstm_fmajor_h256 (layout: include/puresound_hip.h).  Reads the maxima back to the host: plan-build time only."""
    d, hh, g = whh_t.shape
    if hh not in (256, 192) or g != 4 * hh:
        raise ValueError("pack_whh_h256: whh_t must be [D, H, 4H] with H = 256 or 192")
    nw = hh // 32
    imgs, scales = [], []
    for i in range(d):
        w = whh_t[i].detach().float().t().contiguous()            # [4H gate rows, H k]
        wmax = float(w.abs().max())
        if not (wmax < float("inf")):
            raise ValueError("pack_whh_h256: the weight holds inf / NaN")
        ex = max(math.frexp(wmax)[1], -27) if wmax > 0 else 0
        sc = math.ldexp(1.0, 13 - ex)
        pl = torch.stack(_split_planes(w * sc, torch.float16, 2), 0)  # [pl, 4H, H]
        pl = pl.reshape(2, 4, nw, 2, 16, nw, 4, 8)                  # pl, g, w, rb, row, ks, kg, e
        pl = pl.permute(2, 5, 3, 1, 0, 6, 4, 7)                     # w, ks, rb, g, pl, kg, row, e
        imgs.append(pl.reshape(nw, nw, 2, 4, 2, 64, 8))
        scales.append(sc * 1024.0)
    return torch.stack(imgs, 0).contiguous(), scales


def lstm_fmajor_h256_ok(n: int, ldt: int, dirs: int, q: int, q_stride: int, steps: int, step_stride: int) -> bool:
    """The walk conditions of lstm_h256_fits in csrc/rnn.hip (the caller has H = 256 or 192 from the weight image)."""
    return dirs in (1, 2) and (q - 1) * q_stride + (steps - 1) * step_stride < ldt


def lstm_fmajor_h256(gx_fm: torch.Tensor, whh_image: torch.Tensor, acc_scale, dirs: int, q: int, q_stride: int, steps: int,
                     step_stride: int, h0: Optional[torch.Tensor] = None, c0: Optional[torch.Tensor] = None,
                     want_state: bool = False, state_shift: int = 0, state_out: Optional[tuple] = None,
                     out: Optional[torch.Tensor] = None):
    """ps_lstm_fmajor_h256_f16x2_f32: the H = 256 recurrence over FRAME-MAJOR pre-activations gx [N, ldt, D*1024] with W_hh
    streamed from its packed image (pack_whh_h256) -> (hout [N, D*256, ldt], final (h, c) or None), states as lstm()."""
    require_device(gx_fm, "lstm_fmajor_h256")
    hidden = whh_image.shape[1] * 32
    n, ldt, rows = gx_fm.shape
    if (rows != dirs * 4 * hidden or hidden not in (256, 192)
            or tuple(whh_image.shape) != (dirs, hidden // 32, hidden // 32, 2, 4, 2, 64, 8)):
        raise RuntimeError("lstm_fmajor_h256: gx must be [N, ldt, D*4H] and the image pack_whh_h256's")
    _require_operand("lstm_fmajor_h256", gx_fm.device, torch.float16, whh_image=whh_image)
    ldm = _frame_rows("lstm_fmajor_h256", gx_fm)
    a, hout, state = _lstm_args("lstm_fmajor_h256", gx_fm, n, ldt, None, out, hidden, dirs, (q, q_stride, steps, step_stride),
                                h0, c0, want_state, state_shift, state_out)
    sc = (C.c_float * 2)(float(acc_scale[0]), float(acc_scale[-1]))
    # few sequence groups (a speaker LSTM over all frames, SkiM's Mem-LSTMs): the cooperative kernel -- W_hh resident in the
    # registers of H / 32 CUs per group -- instead of streaming 1 MiB of it through one CU every step
    ws_bytes = lib().ps_lstm_fmajor_coop_workspace_bytes(C.byref(a), ldm) if COOP_LSTM and not _COOP_OFF.depth else 0
    if ws_bytes:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=gx_fm.device)
        check(lib().ps_lstm_fmajor_coop_f16x2_f32(C.byref(a), ldm, ptr(whh_image), sc, ptr(ws), ws_bytes,
                                                  stream_ptr(gx_fm.device)), "ps_lstm_fmajor_coop_f16x2_f32")
        _COOP_LAST[0] = ws   # (tests read the error word behind the counters: its last four bytes' block)
    else:
        check(lib().ps_lstm_fmajor_h256_f16x2_f32(C.byref(a), ldm, ptr(whh_image), sc, stream_ptr(gx_fm.device)),
              "ps_lstm_fmajor_h256_f16x2_f32")
    return hout, state


H256_F32_LSTM = os.environ.get("PS_H256_F32_LSTM", "1") != "0"   # 0: the fp32 arithmetic keeps ps_lstm_f32 at H = 256 / 192
# (hidden size, directions) -> sequences per launch from which the models take ps_lstm_h256_f32; fewer, or a pair that is not
# listed, stay on ps_lstm_f32.  A 16-sequence workgroup takes 21-45 us per step however few there are, the generic kernel's
# 4-sequence workgroups ~25 us until they crowd the L2 -- which two directions do at half the sequences.  Each entry is the
# smallest measured count at which the new entry wins by more than the runs' spread on both kinds of walk (SkiM's segments; one
# sequence per utterance), with no measured loss above it; H = 192 in one direction lost at 128 on both walks and is not
# listed (tools/bench_recurrent.py --which h256, profiles/lstm_h256_f32.txt).
H256_F32_MIN_SEQS = {(256, 1): 128, (256, 2): 128, (192, 2): 128}


def pack_whh_h256_f32(whh_t: torch.Tensor) -> torch.Tensor:
    """weight_hh^T [D, H, 4H], H = 256 or 192 -> the fp32 image [D, H/32, H/16, 2, 4, 64, 4] of lstm_h256_f32 (wave, k-group,
    row block, gate, lane, e; layout: include/puresound_hip.h).  A permutation alone: no host read-back, any device."""
    d, hh, g = whh_t.shape
    if hh not in (256, 192) or g != 4 * hh:
        raise ValueError("pack_whh_h256_f32: whh_t must be [D, H, 4H] with H = 256 or 192")
    nw, kgs = hh // 32, hh // 16
    w = whh_t.detach().float().transpose(1, 2)                   # [D, 4H gate rows, H k]
    w = w.reshape(d, 4, nw, 2, 16, kgs, 4, 4)                    # d, g, w, rb, row, kg, kq, e
    w = w.permute(0, 2, 5, 3, 1, 6, 4, 7)                        # d, w, kg, rb, g, kq, row, e
    return w.reshape(d, nw, kgs, 2, 4, 64, 4).contiguous()


def lstm_h256_f32_pays(hidden: int, dirs: int, n: int, q: int) -> bool:
    """The models' choice between lstm_h256_f32 and lstm() in the fp32 arithmetic: the switch, and enough sequences."""
    return H256_F32_LSTM and n * q >= H256_F32_MIN_SEQS.get((hidden, dirs), n * q + 1)


def lstm_h256_f32_ok(n: int, ldt: int, hidden: int, dirs: int, q: int, q_stride: int, steps: int, step_stride: int,
                     ldq: int = 0, state_shift: int = 0) -> bool:
    """Does ps_lstm_h256_f32 take this pass?  Asks ps_lstm_h256_ok with aligned stand-in pointers (never dereferenced); ldq: the
    state tensors' row stride when the launch carries states (0: none)."""
    a = LstmArgs()
    a.gx = a.hout = 256
    if ldq:
        a.h0 = 256
    a.N, a.H, a.D, a.ldt, a.ldq, a.state_shift = n, hidden, dirs, ldt, ldq, state_shift
    a.Q, a.q_stride, a.steps, a.step_stride = q, q_stride, steps, step_stride
    return bool(lib().ps_lstm_h256_ok(C.byref(a)))


def lstm_h256_f32(gx: torch.Tensor, whh_image: torch.Tensor, dirs: int, q: int, q_stride: int, steps: int, step_stride: int,
                  h0: Optional[torch.Tensor] = None, c0: Optional[torch.Tensor] = None, want_state: bool = False,
                  state_shift: int = 0, state_out: Optional[tuple] = None, out: Optional[torch.Tensor] = None):
    """ps_lstm_h256_f32: the H = 256 / 192 recurrence of lstm() with the product W_hh h in exact fp32 MFMA and W_hh streamed
    from its packed image (pack_whh_h256_f32): gx padded [N, D*4H, ldt] -> (hout [N, D*H, ldt], final (h, c) or None)."""
    require_device(gx, "lstm_h256_f32")
    hidden = whh_image.shape[1] * 32
    n, rows, ldt = gx.shape
    if (rows != dirs * 4 * hidden or hidden not in (256, 192)
            or tuple(whh_image.shape) != (dirs, hidden // 32, hidden // 16, 2, 4, 64, 4)):
        raise RuntimeError("lstm_h256_f32: gx must be [N, D*4H, ldt] and the image pack_whh_h256_f32's")
    _require_operand("lstm_h256_f32", gx.device, gx=gx, whh_image=whh_image)
    a, hout, state = _lstm_args("lstm_h256_f32", gx, n, ldt, None, out, hidden, dirs, (q, q_stride, steps, step_stride),
                                h0, c0, want_state, state_shift, state_out)
    check(lib().ps_lstm_h256_f32(C.byref(a), ptr(whh_image), stream_ptr(gx.device)), "ps_lstm_h256_f32")
    return hout, state


def _coop_slices(dirs: int, groups: int, hidden: int) -> int:
    """slices per group the launcher picks: H / 32 (two waves each) while the launch fits the chip, else H / 64"""
    rounds = (groups * dirs + 7) // 8 * 8   # (both directions in one launch; one launch per direction beyond that: H / 64 too)
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return hidden // 32 if rounds * (hidden // 32) <= cus else hidden // 64


def _coop_layout(dirs: int, groups: int, hidden: int) -> tuple[int, int, int]:
    """int32 indices into the cooperative LSTM's workspace -- the Python copy of coop_layout() in csrc/rnn.hip (the h
    exchange, then D * groups barrier counters; lstm_coop.inc): (error word, first XCD id, first XCD mask)."""
    hx = (2 * dirs * groups * 2 * 16 * (hidden + 8) * 2 + 255) // 256 * 256
    err = hx // 4 + dirs * groups
    return err, err + 1, err + 1 + dirs * groups * _coop_slices(dirs, groups, hidden)


def coop_lstm_error_word(dirs: int, groups: int, hidden: int) -> int:
    """The error word of the last cooperative LSTM launch's workspace (1 = a group barrier gave up waiting); synchronises."""
    ws = _COOP_LAST[0]
    if ws is None:
        return 0
    return int(ws.view(torch.int32)[_coop_layout(dirs, groups, hidden)[0]])


def coop_lstm_xcd_ids(dirs: int, groups: int, hidden: int) -> torch.Tensor:
    """[D * groups, slices]: the XCD every slice of the last cooperative launch ran on (the light group barrier needs each
    row constant: tests check it on the target part)."""
    ws = _COOP_LAST[0]
    first = _coop_layout(dirs, groups, hidden)[1]
    ns = _coop_slices(dirs, groups, hidden)
    return ws.view(torch.int32)[first:first + dirs * groups * ns].reshape(dirs * groups, ns).cpu()


def coop_lstm_xcd_masks(dirs: int, groups: int, hidden: int) -> torch.Tensor:
    """[D * groups]: per cluster the OR of 1 << XCD over its slices (one bit = the cluster took the light barrier)."""
    ws = _COOP_LAST[0]
    first = _coop_layout(dirs, groups, hidden)[2]
    return ws.view(torch.int32)[first:first + dirs * groups].cpu()


def chan_layernorm(x: torch.Tensor, t: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                   res: Optional[torch.Tensor] = None, slope: Optional[torch.Tensor] = None, sigmoid: bool = False,
                   mul: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[res +] [mul *] act(LN over channels of every frame) on padded [N,C,ldt]."""
    require_device(x, "chan_layernorm")
    n, c, ldt = x.shape
    y = out if out is not None else torch.empty_like(x)
    check(lib().ps_chan_layernorm_f32(ptr(x), ptr(gamma), ptr(beta), float(eps), ptr(slope), int(sigmoid), ptr(mul),
                                      ptr(res), ptr(y), n, c, t, ldt, stream_ptr(x.device)), "ps_chan_layernorm_f32")
    return y


def unfold_taps(x: torch.Tensor, t: int, taps: int, dilation: int, left: int, scale: Optional[torch.Tensor] = None,
                shift: Optional[torch.Tensor] = None, embed: Optional[torch.Tensor] = None,
                t_out: Optional[int] = None) -> torch.Tensor:
    """x padded [N,K,ldt] -> [N, taps*(K+E), ldt]: tap-shifted copies (zero outside [0,T)), optional per-(n,k) affine
    before the padding, optional constant embedding rows.  t_out > t: that many output frames per row."""
    require_device(x, "unfold_taps")
    n, k, ldt = x.shape
    e = 0 if embed is None else embed.shape[1]
    y = torch.empty(n, taps * (k + e), ldt, dtype=torch.float32, device=x.device)
    if t_out is None:
        check(lib().ps_unfold_taps_f32(ptr(x), ptr(y), n, k, t, ldt, taps, dilation, left, ptr(scale), ptr(shift), ptr(embed), e,
                                       stream_ptr(x.device)), "ps_unfold_taps_f32")
        return y
    check(lib().ps_unfold_taps_out_f32(ptr(x), ptr(y), n, k, t, t_out, ldt, taps, dilation, left, ptr(scale), ptr(shift),
                                       ptr(embed), e, stream_ptr(x.device)), "ps_unfold_taps_out_f32")
    return y


def gated_product(left: torch.Tensor, right: torch.Tensor, t: int, pro_left: Prologue, pro_right: Prologue) -> torch.Tensor:
    """PReLU(norm(left)) * sigmoid(PReLU(norm(right))) on padded [N,H,ldt]."""
    require_device(left, "gated_product")
    n, h, ldt = left.shape
    y = torch.empty_like(left)
    check(lib().ps_gated_product_f32(ptr(left), ptr(right), ptr(y), n, h, t, ldt, C.byref(pro_left), C.byref(pro_right),
                                     stream_ptr(left.device)), "ps_gated_product_f32")
    return y


def overlap_geometry(t: int, k: int) -> tuple[int, int]:
    """(rest, S*K) of the 50 % overlapped segmentation of t frames into k-frame segments."""
    stride = k // 2
    rest = k - (stride + t % k) % k
    return rest, 2 * ((t + rest + stride) // k) * k


def segment_split(x: torch.Tensor, t: int, k: int) -> tuple[torch.Tensor, int]:
    """padded [N,C,ldt] with t frames -> (padded [N,C,ld'] holding S*K frames of overlapped segments, S*K)."""
    require_device(x, "segment_split")
    n, c, ldt = x.shape
    _, tp = overlap_geometry(t, k)
    y = torch.empty(n, c, padded_frames(tp), dtype=torch.float32, device=x.device)
    check(lib().ps_segment_overlap_f32(ptr(x), ptr(y), n * c, t, ldt, tp, y.shape[-1], k, 0, stream_ptr(x.device)),
          "ps_segment_overlap_f32")
    return y, tp


def segment_merge(x: torch.Tensor, tp: int, t: int, k: int) -> torch.Tensor:
    """inverse of segment_split: padded [N,C,ld'] with tp segment frames -> padded [N,C,ldt] with t frames."""
    require_device(x, "segment_merge")
    n, c, ld = x.shape
    y = torch.empty(n, c, padded_frames(t), dtype=torch.float32, device=x.device)
    check(lib().ps_segment_overlap_f32(ptr(x), ptr(y), n * c, tp, ld, t, y.shape[-1], k, 1, stream_ptr(x.device)),
          "ps_segment_overlap_f32")
    return y


def film_conv(x: torch.Tensor, t: int, wt_pairs: torch.Tensor, res_pairs: Optional[torch.Tensor],
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """FiLM (after its input norm) in one kernel: (Ws x + rs) * x + (Wb x + rb); weight rows paired (scale, bias)."""
    require_device(x, "film_conv")
    n, c, ldt = x.shape
    y = out if out is not None else torch.empty_like(x)
    check(lib().ps_film_conv_f32(ptr(x), ptr(wt_pairs), ptr(res_pairs), ptr(y), n, c, t, ldt, stream_ptr(x.device)),
          "ps_film_conv_f32")
    return y


def lstm_gates_cell(xh: torch.Tensor, t: int, wt_units: torch.Tensor, bias_units: torch.Tensor, c: torch.Tensor,
                    h: torch.Tensor, hidden: int) -> None:
    """gates GEMM over [x; h] + LSTM cell; c in place, h' into `h` (not the h rows of xh)."""
    require_device(xh, "lstm_gates_cell")
    n, k, ldt = xh.shape
    if n != 1 and (not c.is_contiguous() or not h.is_contiguous()):
        raise RuntimeError("lstm_gates_cell: state views are supported for N = 1 only")
    check(lib().ps_lstm_gates_cell_f32(ptr(xh), ptr(wt_units), ptr(bias_units), ptr(c), ptr(h), n, k, hidden, t, ldt,
                                       c.stride(1), stream_ptr(xh.device)), "ps_lstm_gates_cell_f32")


def proj_layernorm(x: torch.Tensor, t: int, wt: torch.Tensor, bias: Optional[torch.Tensor], m: int,
                   gamma: torch.Tensor, beta: torch.Tensor, eps: float, res: Optional[torch.Tensor],
                   norm2: Optional[tuple] = None, x_copy: Optional[torch.Tensor] = None, res_inside: bool = False,
                   out: Optional[torch.Tensor] = None, out2: Optional[torch.Tensor] = None, want_amax: bool = False):
    """y = res + LN(W x + b), or LN(W x + b + res) with res_inside (+ y2 = LN2(y), + copy of x); returns (y, y2);
    y is written into `out` (contiguous [N, m, ldt]) when given."""
    require_device(x, "proj_layernorm")
    n, k, ldt = x.shape
    if out is not None and (tuple(out.shape) != (n, m, ldt) or not out.is_contiguous() or out.dtype != torch.float32):
        raise ValueError(f"proj_layernorm: `out` must be a contiguous fp32 {(n, m, ldt)} tensor")
    y = out if out is not None else torch.empty(n, m, ldt, dtype=torch.float32, device=x.device)
    y2 = (out2 if out2 is not None else torch.empty_like(y)) if norm2 is not None else None
    g2, b2, e2 = norm2 if norm2 is not None else (None, None, 0.0)
    if want_amax:  # (long rows only: the row kernel; the caller falls back to absmax() when this raises PS_E_UNSUPPORTED)
        amax = torch.empty(n, lib().ps_proj_layernorm_amax_parts(t), dtype=torch.float32, device=x.device)
        check(lib().ps_proj_layernorm_amax_f32(ptr(x), ptr(wt), ptr(bias), ptr(gamma), ptr(beta), float(eps), ptr(res), ptr(y),
                                               ptr(g2), ptr(b2), float(e2), ptr(y2), ptr(x_copy), int(res_inside), n, k, m, t,
                                               ldt, ptr(amax), stream_ptr(x.device)), "ps_proj_layernorm_amax_f32")
        return y, y2, amax
    check(lib().ps_proj_layernorm_f32(ptr(x), ptr(wt), ptr(bias), ptr(gamma), ptr(beta), float(eps), ptr(res), ptr(y),
                                      ptr(g2), ptr(b2), float(e2), ptr(y2), ptr(x_copy), int(res_inside), n, k, m, t, ldt,
                                      stream_ptr(x.device)), "ps_proj_layernorm_f32")
    return y, y2


# ---- the cells of a streaming anti-diagonal: the three operators above for several one-utterance problems per launch ----
MAX_CELLS = _abi.PS_MAX_CELLS


def film_conv_cells(cells: list, t: int) -> None:
    """cells: [(xn [1,C,ld], wt_pairs, res_pairs | None, out [1,C,ld]), ...] -> one ps_film_conv_cells_f32 launch."""
    x0 = cells[0][0]
    require_device(x0, "film_conv_cells")
    _, c, ldt = x0.shape
    arr = (_abi.FilmCell * len(cells))()
    for a, (x, wt, res, y) in zip(arr, cells):
        if tuple(x.shape) != (1, c, ldt) or tuple(y.shape) != (1, c, ldt) or x.stride(1) != ldt or y.stride(1) != ldt:
            raise RuntimeError("film_conv_cells: every cell is a [1, C, ld] row block of one shape")
        a.x, a.wt_pairs, a.res_pairs, a.y = ptr(x), ptr(wt), ptr(res), ptr(y)
    check(lib().ps_film_conv_cells_f32(arr, len(cells), c, t, ldt, stream_ptr(x0.device)), "ps_film_conv_cells_f32")


def lstm_gates_cell_cells(cells: list, t: int, hidden: int) -> None:
    """cells: [(xh [1,K,ld], wt_units, bias_units, c [1,H,ld'], h [1,H,ld']), ...] -> one launch (c in place, h' out)."""
    xh0, c0 = cells[0][0], cells[0][3]
    require_device(xh0, "lstm_gates_cell_cells")
    _, k, ldt = xh0.shape
    arr = (_abi.GatesCell * len(cells))()
    for a, (xh, wt, bias, c, h) in zip(arr, cells):
        if tuple(xh.shape) != (1, k, ldt) or c.stride(1) != c0.stride(1) or h.stride(1) != c0.stride(1):
            raise RuntimeError("lstm_gates_cell_cells: every cell has the same [1, K, ld] block and state row stride")
        a.xh, a.wt_units, a.bias_units, a.c, a.h = ptr(xh), ptr(wt), ptr(bias), ptr(c), ptr(h)
    check(lib().ps_lstm_gates_cell_cells_f32(arr, len(cells), k, hidden, t, ldt, c0.stride(1), stream_ptr(xh0.device)),
          "ps_lstm_gates_cell_cells_f32")


def proj_layernorm_cells(cells: list, t: int, m: int, res_inside: bool = False) -> None:
    """cells: [dict(x, wt, bias, gamma, beta, eps, res, y, norm2 = (gamma2, beta2, eps2) | None, y2, x_copy), ...] -> one
    launch: y = res + LN(W x + b), or LN(W x + b + res) with res_inside (+ y2 = LN2(y), + x_copy = x) per cell."""
    x0 = cells[0]["x"]
    require_device(x0, "proj_layernorm_cells")
    _, k, ldt = x0.shape
    arr = (_abi.ProjLnCell * len(cells))()
    for a, c in zip(arr, cells):
        if tuple(c["x"].shape) != (1, k, ldt) or tuple(c["y"].shape) != (1, m, ldt) or not c["y"].is_contiguous():
            raise RuntimeError("proj_layernorm_cells: every cell maps a [1, K, ld] block to a contiguous [1, M, ld] block")
        g2, b2, e2 = c["norm2"] if c.get("norm2") is not None else (None, None, 0.0)
        a.x, a.wt, a.bias, a.gamma, a.beta = ptr(c["x"]), ptr(c["wt"]), ptr(c.get("bias")), ptr(c["gamma"]), ptr(c["beta"])
        a.res, a.y, a.gamma2, a.beta2 = ptr(c.get("res")), ptr(c["y"]), ptr(g2), ptr(b2)
        a.y2, a.x_copy = ptr(c.get("y2") if g2 is not None else None), ptr(c.get("x_copy"))
        a.eps, a.eps2 = float(c["eps"]), float(e2)
    check(lib().ps_proj_layernorm_cells_f32(arr, len(cells), int(res_inside), k, m, t, ldt, stream_ptr(x0.device)),
          "ps_proj_layernorm_cells_f32")


def overlap_average(prev: torch.Tensor, cur: torch.Tensor, overlap: int) -> torch.Tensor:
    """Streaming harness OLA: returns the new [B, win] block whose first `overlap` samples are the average of the
    tail of `prev` [B, L] and the head of `cur` [B, win]."""
    require_device(cur, "overlap_average")
    b, win = cur.shape
    if prev.shape[0] != b or prev.shape[1] < overlap or prev.stride(1) != 1:
        raise RuntimeError("overlap_average: prev must be [B, L >= overlap] with contiguous rows")
    cur = cur.contiguous()
    out = torch.empty_like(cur)
    tail = prev[:, prev.shape[1] - overlap:]
    check(lib().ps_overlap_average_f32(ptr(tail), prev.stride(0), ptr(cur), ptr(out), b, win, overlap,
                                       stream_ptr(cur.device)), "ps_overlap_average_f32")
    return out


def stream_windows(queue: torch.Tensor, chunk: torch.Tensor, wins: torch.Tensor, hop: int) -> None:
    """queue [B, win] ‖ chunk [B, hops * hop] -> wins [hops, B * win]: window i of stream b = samples [i hop, i hop + win) of
    queue[:, hop:] ‖ chunk (ps_stream_windows_f32; win >= hop)."""
    require_device(chunk, "stream_windows")
    b, win = queue.shape
    hops = chunk.shape[1] // hop
    if not (queue.is_contiguous() and chunk.is_contiguous() and wins.is_contiguous()) or wins.shape != (hops, b * win):
        raise RuntimeError("stream_windows: contiguous queue [B, win], chunk [B, hops * hop], wins [hops, B * win] expected")
    check(lib().ps_stream_windows_f32(ptr(queue), ptr(chunk), ptr(wins), b, hops, win, hop, stream_ptr(chunk.device)),
          "ps_stream_windows_f32")


def stream_overlap(frames: torch.Tensor, wins: torch.Tensor, tail: torch.Tensor, blocks: torch.Tensor,
                   queue: torch.Tensor, hop: int) -> None:
    """Averaging overlap-add of all hops of a chunk, in place on tail / blocks / queue (ps_stream_overlap_f32)."""
    require_device(frames, "stream_overlap")
    b, win = queue.shape
    hops = wins.shape[0]
    if not all(t.is_contiguous() for t in (frames, wins, tail, blocks, queue)) or frames.numel() != hops * b * win \
            or tail.shape != (b, hop) or blocks.shape != (b, hops * hop):
        raise RuntimeError("stream_overlap: frames [hops, B, win], tail [B, hop], blocks [B, hops * hop] (contiguous) expected")
    check(lib().ps_stream_overlap_f32(ptr(frames), ptr(wins), ptr(tail), ptr(blocks), ptr(queue), b, hops, win, hop,
                                      stream_ptr(frames.device)), "ps_stream_overlap_f32")


ACT_KINDS = {"none": 0, "relu": 1, "prelu": 2, "mish": 3, "sigmoid": 4, "tanh": 5}


def conv2d_step(x1: torch.Tensor, ring1: Optional[torch.Tensor], x2: Optional[torch.Tensor], ring2: Optional[torch.Tensor],
                wt: torch.Tensor, bias: Optional[torch.Tensor], m: int, b: int, f_out: int, kf: int, kt: int, stride_f: int,
                dil_f: int, dil_t: int, pad_f: int, transposed: bool, act: str = "none", slope: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, counter: Optional[torch.Tensor] = None,
                span: Optional[torch.Tensor] = None, shift: int = 0) -> torch.Tensor:
    """One causal frame of a Conv2d / ConvTranspose2d for b streams (ps_conv2d_step_f32): current frames x1 [1, C1, F, ld]
    (+ x2 [1, C2, F, ld]), previous frames from the rings [R, C, F, ld] (slot R - d = frame t - d) -> [1, m, f_out, ld]
    (columns b..ld of `out` are not written).  span int32 [b, 2] with the int32 frame counter: ps_conv2d_step_slots_f32, the
    current frames are frame counter[0] - shift and a tap reads frame g of stream b iff span[b, 0] <= g < span[b, 1]."""
    require_device(x1, "conv2d_step")
    _, c1, f_in, ld = x1.shape
    c2 = 0 if x2 is None else x2.shape[1]
    for src, ring in ((x1, ring1), (x2, ring2)):
        if src is None:
            continue
        if not src.is_contiguous() or src.shape[0] != 1 or (src.shape[2], src.shape[3]) != (f_in, ld):
            raise RuntimeError("conv2d_step: the sources must be contiguous [1, C, F, ld] with one F and ld")
        if ring is not None and (not ring.is_contiguous() or tuple(ring.shape[1:]) != tuple(src.shape[1:])):
            raise RuntimeError("conv2d_step: a ring must be a contiguous [R, C, F, ld] of its source's frame shape")
    y = out if out is not None else torch.zeros(1, m, f_out, ld, dtype=torch.float32, device=x1.device)
    if tuple(y.shape) != (1, m, f_out, ld) or not y.is_contiguous():
        raise RuntimeError(f"conv2d_step: out must be a contiguous {(1, m, f_out, ld)} tensor")
    r1 = 0 if ring1 is None else ring1.shape[0]
    r2 = 0 if ring2 is None else ring2.shape[0]
    slots = span is not None
    if slots:
        _check_span(span, b, x1, "conv2d_step")
        if counter is None or counter.dtype != torch.int32 or counter.device != x1.device:
            raise RuntimeError("conv2d_step: span comes with the int32 frame counter on x1's device")
    elif counter is not None or shift:
        raise RuntimeError("conv2d_step: counter and shift come with span")
    args = (ptr(x1), ptr(ring1), c1, r1, ptr(x2), ptr(ring2), c2, r2, ptr(wt), ptr(bias), ptr(y), m, f_in, b, ld, kf, kt,
            stride_f, dil_f, dil_t, pad_f, f_out, int(transposed), ACT_KINDS[act], ptr(slope),
            *((ptr(counter), ptr(span), int(shift)) if slots else ()), stream_ptr(x1.device))
    rc = lib().ps_conv2d_step_slots_f32(*args) if slots else lib().ps_conv2d_step_f32(*args)
    check(rc, "ps_conv2d_step_slots_f32" if slots else "ps_conv2d_step_f32")
    return y


def istft_step(frames: Optional[torch.Tensor], window: torch.Tensor, tail: torch.Tensor, out: torch.Tensor,
               counter: torch.Tensor, hop: int, out_mode: str = "none", flush: bool = False,
               span: Optional[torch.Tensor] = None, shift: int = 0) -> torch.Tensor:
    """Synthesis of frame t = counter[0] of every stream (ps_istft_step_f32): frames padded [1, n_fft, ldB] -> out [B, hop]
    (a row view of a wider buffer is fine), overlap-add tail [B, n_fft - hop] updated in place; flush: the tail's samples
    after the last frame -> out [B, n_fft - hop].  span int32 [B, 2]: ps_istft_step_slots_f32, stream b synthesises its own
    frame counter[0] - shift - span[b, 0] of span[b, 1] - span[b, 0] and adds it iff it is one of them."""
    require_device(tail, "istft_step")
    b, keep = tail.shape
    n_fft = keep + hop
    if not tail.is_contiguous() or out.dim() != 2 or out.shape[0] != b or out.stride(1) != 1 \
            or out.shape[1] != (keep if flush else hop) or counter.dtype != torch.int32:
        raise RuntimeError("istft_step: tail [B, n_fft - hop] contiguous, out [B, hop] (flush: [B, n_fft - hop]) with unit "
                           "column stride, int32 counter expected")
    ldf = 0
    if flush and keep == 0:
        return out
    if not flush:
        if frames is None or frames.shape[:2] != (1, n_fft) or not frames.is_contiguous():
            raise RuntimeError("istft_step: frames must be a contiguous [1, n_fft, ldB] tensor")
        ldf = frames.shape[2]
    slots = span is not None
    if slots:
        _check_span(span, b, tail, "istft_step")
    elif shift:
        raise RuntimeError("istft_step: shift comes with span")
    args = (ptr(frames), ldf, ptr(window), ptr(tail), ptr(out), out.stride(0), ptr(counter),
            *((ptr(span), int(shift)) if slots else ()), b, n_fft, hop, _abi.PS_OUT[out_mode], int(flush),
            stream_ptr(tail.device))
    rc = lib().ps_istft_step_slots_f32(*args) if slots else lib().ps_istft_step_f32(*args)
    check(rc, "ps_istft_step_slots_f32" if slots else "ps_istft_step_f32")
    return out


def commit_table(pairs: Sequence[tuple]) -> "C.Array[RingPair]":
    """[(src, ring), ...] -> the host table of ps_stream_commit_f32 (ring [R, *src.shape]: R slots of src's size)."""
    if not 0 < len(pairs) <= _abi.PS_MAX_RING_PAIRS:
        raise RuntimeError(f"commit_table: 1 .. {_abi.PS_MAX_RING_PAIRS} pairs")
    tab = (RingPair * len(pairs))()
    for e, (src, ring) in zip(tab, pairs):
        if not (src.is_contiguous() and ring.is_contiguous()) or ring.numel() % src.numel():
            raise RuntimeError("commit_table: contiguous src and ring, the ring a whole number of src-sized slots")
        e.src, e.ring, e.count, e.slots = ptr(src), ptr(ring), src.numel(), ring.numel() // src.numel()
    return tab


def stream_commit(table: "C.Array[RingPair]", counter: Optional[torch.Tensor], device: torch.device) -> None:
    """Shift every ring of the table by one frame (newest = its source) and advance the frame counter (ps_stream_commit_f32)."""
    check(lib().ps_stream_commit_f32(table, len(table), ptr(counter), stream_ptr(device)), "ps_stream_commit_f32")


def stream_commit_frames(table: "C.Array[RingPair]", counter: torch.Tensor, frames: int, device: torch.device) -> None:
    """ps_stream_commit_f32 with the frame counter advanced by `frames` (ps_stream_commit_frames_f32)."""
    check(lib().ps_stream_commit_frames_f32(table, len(table), ptr(counter), int(frames), stream_ptr(device)),
          "ps_stream_commit_frames_f32")


def state_gate(states: Sequence[torch.Tensor], counter: torch.Tensor, span: torch.Tensor, b: int, shift: int = 1,
               ld: Optional[int] = None) -> None:
    """The span rule for carried states (ps_state_gate_slots_f32): every tensor of `states` is contiguous rows of ld columns
    (ld = padded_frames(b) unless given; [1, H, F * ld] is H * F rows) with the b streams as the first b columns of a row;
    column i of every row becomes an exact 0 unless frame counter[0] - shift is live in stream i (span int32 [b, 2]).  Live
    columns and the pad columns b..ld are left as they are, nothing is read."""
    if not 0 < len(states) <= _abi.PS_MAX_RING_PAIRS:
        raise RuntimeError(f"state_gate: 1 .. {_abi.PS_MAX_RING_PAIRS} states")
    first = states[0]
    require_device(first, "state_gate")
    ld = padded_frames(int(b)) if ld is None else int(ld)
    tab = (StateRows * len(states))()
    for e, x in zip(tab, states):
        if x.dtype != torch.float32 or not x.is_contiguous() or ld <= 0 or x.numel() % ld or x.device != first.device:
            raise RuntimeError(f"state_gate: contiguous fp32 states of whole rows of ld = {ld} columns on one device expected")
        e.x, e.rows = ptr(x), x.numel() // ld
    _check_span(span, b, first, "state_gate")
    if counter is None or counter.dtype != torch.int32 or counter.device != first.device:
        raise RuntimeError("state_gate: the int32 frame counter on the states' device expected")
    check(lib().ps_state_gate_slots_f32(tab, len(tab), ptr(counter), ptr(span), int(shift), int(b), ld,
                                        stream_ptr(first.device)), "ps_state_gate_slots_f32")


def _check_span(span: torch.Tensor, streams: int, like: torch.Tensor, who: str) -> None:
    if span.dtype != torch.int32 or tuple(span.shape) != (streams, 2) or not span.is_contiguous() or span.device != like.device:
        raise RuntimeError(f"{who}: span must be a contiguous int32 [{streams}, 2] tensor (birth, death) on {like.device}")


def dwconv_step(x: torch.Tensor, ring: torch.Tensor, counter: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor],
                dilation: int, streams: int, frames: int, pro: Optional[Prologue] = None,
                out: Optional[torch.Tensor] = None, span: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Causal depthwise convolution of `frames` new frames of `streams` streams (ps_dwconv_step_f32): x [1, H, ld] (column
    f * streams + b), w [H, 1, P]; earlier frames from ring [R, H, streams] (slot g % R = frame g, activated values; the
    chunk's frames are stored there too), frame index of column 0 = counter[0] -> y [1, H, ld] (columns past
    frames * streams are not written).  span int32 [streams, 2]: ps_dwconv_step_slots_f32, a tap reads frame g of stream b
    iff span[b, 0] <= g < span[b, 1]."""
    require_device(x, "dwconv_step")
    _, h, ld = x.shape
    p = w.shape[-1]
    if not (x.is_contiguous() and ring.is_contiguous()) or ring.dim() != 3 or tuple(ring.shape[1:]) != (h, streams) \
            or counter.dtype != torch.int32:
        raise RuntimeError("dwconv_step: contiguous x [1, H, ld] and ring [R, H, streams], int32 counter expected")
    y = out if out is not None else torch.zeros_like(x)
    if y.shape != x.shape or not y.is_contiguous():
        raise RuntimeError("dwconv_step: out must be a contiguous tensor of x's shape")
    slots = span is not None
    if slots:
        _check_span(span, streams, x, "dwconv_step")
    args = (ptr(x), ptr(ring), ring.shape[0], ptr(counter), *((ptr(span),) if slots else ()), ptr(w), ptr(b), ptr(y), h,
            streams, frames, ld, p, dilation, C.byref(pro) if pro is not None else None, stream_ptr(x.device))
    rc = lib().ps_dwconv_step_slots_f32(*args) if slots else lib().ps_dwconv_step_f32(*args)
    check(rc, "ps_dwconv_step_slots_f32" if slots else "ps_dwconv_step_f32")
    return y


def gated_tcn_step(y: torch.Tensor, ring: torch.Tensor, counter: torch.Tensor, wl: torch.Tensor, wr: torch.Tensor,
                   taps: int, dilation: int, streams: int, frames: int, pro_left: Optional[Prologue] = None,
                   pro_right: Optional[Prologue] = None, emb_taps: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None, span: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The two dense dilated convolutions, norms and gate of a causal GatedTCN block for `frames` new frames of `streams`
    streams (ps_gated_tcn_step_f32): y [1, H, ld] (column f * streams + b, the output of in_conv); wl, wr = pack_wt of the
    [H, taps * H] weights with column j * H + c; earlier frames of y from ring [R, H, streams] (slot g % R = frame g; the
    chunk's frames are stored there too), frame index of column 0 = counter[0]; emb_taps [taps, H, streams]: what the
    embedding adds to the right side per tap whose frame is >= 0 -> g [1, H, ld] (columns past frames * streams are not
    written).  span int32 [streams, 2]: ps_gated_tcn_step_slots_f32, a tap reads frame g of stream b and adds its embedding
    constant iff span[b, 0] <= g < span[b, 1]."""
    require_device(y, "gated_tcn_step")
    _, h, ld = y.shape
    kp = (taps * h + 15) // 16 * 16
    _require_operand("gated_tcn_step", y.device, y=y, ring=ring, wl=wl, wr=wr, emb_taps=emb_taps, out=out)
    if ring.dim() != 3 or tuple(ring.shape[1:]) != (h, streams) or counter.dtype != torch.int32 or counter.device != y.device:
        raise RuntimeError("gated_tcn_step: ring [R, H, streams] and an int32 counter on y's device expected")
    if tuple(wl.shape) != ((h + 255) // 256, kp, 256) or wl.shape != wr.shape:
        raise RuntimeError(f"gated_tcn_step: wl, wr must be pack_wt of [H, taps * H] weights: {((h + 255) // 256, kp, 256)}")
    if emb_taps is not None and tuple(emb_taps.shape) != (taps, h, streams):
        raise RuntimeError(f"gated_tcn_step: emb_taps must be [{taps}, {h}, {streams}]")
    g = out if out is not None else torch.zeros_like(y)
    if g.shape != y.shape:
        raise RuntimeError("gated_tcn_step: out must be a contiguous tensor of y's shape")
    slots = span is not None
    if slots:
        _check_span(span, streams, y, "gated_tcn_step")
    args = (ptr(y), ptr(ring), ring.shape[0], ptr(counter), *((ptr(span),) if slots else ()), ptr(wl), ptr(wr),
            ptr(emb_taps), C.byref(pro_left) if pro_left is not None else None,
            C.byref(pro_right) if pro_right is not None else None, ptr(g), h, streams, frames, ld, taps, dilation,
            stream_ptr(y.device))
    rc = lib().ps_gated_tcn_step_slots_f32(*args) if slots else lib().ps_gated_tcn_step_f32(*args)
    check(rc, "ps_gated_tcn_step_slots_f32" if slots else "ps_gated_tcn_step_f32")
    return g


def free_decode_step(feats: Optional[torch.Tensor], mask: Optional[torch.Tensor], w: torch.Tensor, tail: torch.Tensor,
                     out: torch.Tensor, hop: int, frames: int = 0, mask_act: str = "linear", out_mode: str = "linear",
                     flush: bool = False, span: Optional[torch.Tensor] = None,
                     counter: Optional[torch.Tensor] = None) -> torch.Tensor:
    """FreeEncDec's decoder for `frames` new frames of B streams (ps_free_decode_step_f32): feats / mask [1, C, ld] (column
    f * B + b), w [C, 1, win], overlap-add tail [B, win - hop] updated in place -> out [B, frames * hop] (a row view of a
    wider buffer is fine); flush: the tail's samples -> out [B, win - hop].  span int32 [B, 2] with the int32 frame counter:
    ps_free_decode_step_slots_f32, frame f adds its product iff span[b, 0] <= counter[0] + f < span[b, 1] (not with flush)."""
    require_device(tail, "free_decode_step")
    b, keep = tail.shape
    win = w.shape[-1]
    if keep != win - hop or not tail.is_contiguous() or out.dim() != 2 or out.shape[0] != b or out.stride(1) != 1 \
            or out.shape[1] != (keep if flush else frames * hop):
        raise RuntimeError("free_decode_step: tail [B, win - hop] contiguous, out [B, frames * hop] (flush: [B, win - hop]) "
                           "with unit column stride expected")
    ld, c = 0, w.shape[0]
    if flush and keep == 0:
        return out
    if not flush:
        require_weight(w, tail, "free_decode_step")
        for t in (feats, mask):
            if t is not None and (t.dim() != 3 or t.shape[:2] != (1, c) or not t.is_contiguous()):
                raise RuntimeError(f"free_decode_step: feats / mask must be contiguous [1, {c}, ld] tensors")
        ld = feats.shape[2]
        if mask is not None and mask.shape != feats.shape:
            raise RuntimeError("free_decode_step: feats and mask of one shape expected")
    ws_bytes = 0 if flush else lib().ps_free_decode_step_workspace_bytes(b, frames, win)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=tail.device) if ws_bytes else None
    slots = span is not None
    if slots:
        _check_span(span, b, tail, "free_decode_step")
        if flush or counter is None or counter.dtype != torch.int32 or counter.device != tail.device:
            raise RuntimeError("free_decode_step: a span goes with the int32 device frame counter and never with flush")
    # (the slot entry takes the span and the counter, and no flush flag: it never flushes)
    args = (ptr(feats), ptr(mask), _abi.PS_ACT[mask_act], ld, ptr(w), ptr(tail), ptr(out), out.stride(0),
            *((ptr(span), ptr(counter)) if slots else ()), b, frames, c, win, hop, _abi.PS_OUT[out_mode],
            *(() if slots else (int(flush),)), ptr(ws), ws_bytes, stream_ptr(tail.device))
    rc = lib().ps_free_decode_step_slots_f32(*args) if slots else lib().ps_free_decode_step_f32(*args)
    check(rc, "ps_free_decode_step_slots_f32" if slots else "ps_free_decode_step_f32")
    return out


def dprnn_block_step_ok(c: int, hidden: int, seg: int) -> bool:
    """Whether ps_dprnn_block_step_f32 has a kernel for (C, H, K)."""
    return lib().ps_dprnn_block_step_ok(int(c), int(hidden), int(seg)) == 1


def pack_dprnn_pass(lstm, proj, norm, device: torch.device) -> dict:
    """One pass of a DPRNN block (a unidirectional one-layer nn.LSTM, its nn.Linear, its nn.LayerNorm) -> the fp32 tensors of
    a ps_dprnn_pass and the struct pointing at them (keep the dict alive while launches read it)."""
    f32 = lambda t: t.detach().to(dtype=torch.float32, device=device)  # noqa: E731
    p = dict(wt=torch.cat([f32(lstm.weight_ih_l0), f32(lstm.weight_hh_l0)], dim=1).t().contiguous(),   # [C + H, 4H]
             bias=(f32(lstm.bias_ih_l0) + f32(lstm.bias_hh_l0)).contiguous(),
             pt=f32(proj.weight).t().contiguous(), pbias=f32(proj.bias).contiguous(),                   # [H, C]
             gamma=f32(norm.weight).contiguous(), beta=f32(norm.bias).contiguous())
    s = _abi.DprnnPass()
    for key, t in p.items():
        setattr(s, key, ptr(t))
    s.eps = float(norm.eps)
    p["struct"] = s
    return p


def dprnn_block_step(x: torch.Tensor, counter: torch.Tensor, intra: dict, inter: dict, h_intra: torch.Tensor,
                     c_intra: torch.Tensor, h_bank: torch.Tensor, c_bank: torch.Tensor, streams: int, frames: int,
                     out: torch.Tensor, span: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One causal DPRNN block on `frames` new frames of `streams` streams (ps_dprnn_block_step_f32): x [1, C, ld] (column
    f * streams + b) -> out [1, C, ld] (columns past frames * streams are not written); intra / inter from pack_dprnn_pass;
    intra state h_intra / c_intra [H, ldb] and the inter banks h_bank / c_bank [K, H, ldb] (slot p = position p of a segment),
    updated in place; frame index of column 0 = counter[0], position = index % K.  span int32 [streams, 2]:
    ps_dprnn_block_step_slots_f32, stream b computes frame g iff span[b, 0] <= g < span[b, 1], at position
    (g - span[b, 0]) % K; a frame that is not live reads x as 0 and stores no state."""
    require_device(x, "dprnn_block_step")
    _, c, ld = x.shape
    k_seg, hidden, ldb = h_bank.shape
    for t, shape in ((h_intra, (hidden, ldb)), (c_intra, (hidden, ldb)), (c_bank, (k_seg, hidden, ldb))):
        require_weight(t, x, "dprnn_block_step")
        if tuple(t.shape) != shape:
            raise RuntimeError("dprnn_block_step: states [H, ldb] and banks [K, H, ldb] of one H and ldb expected")
    require_weight(h_bank, x, "dprnn_block_step")
    if not (x.is_contiguous() and out.is_contiguous()) or out.shape != x.shape or out.dtype != torch.float32 \
            or counter.dtype != torch.int32 or counter.device != x.device:
        raise RuntimeError("dprnn_block_step: contiguous fp32 x and out [1, C, ld], an int32 counter on their device expected")
    if tuple(intra["wt"].shape) != (c + hidden, 4 * hidden) or tuple(inter["wt"].shape) != (c + hidden, 4 * hidden) \
            or tuple(intra["pt"].shape) != (hidden, c) or tuple(inter["pt"].shape) != (hidden, c) \
            or intra["wt"].device != x.device or inter["wt"].device != x.device:
        raise RuntimeError(f"dprnn_block_step: passes packed for C = {c}, H = {hidden} on {x.device} expected")
    slots = span is not None
    if slots:
        _check_span(span, streams, x, "dprnn_block_step")
    args = (ptr(x), ptr(out), ptr(counter), *((ptr(span),) if slots else ()), C.byref(intra["struct"]),
            C.byref(inter["struct"]), ptr(h_intra), ptr(c_intra), ptr(h_bank), ptr(c_bank), c, hidden, k_seg, streams,
            frames, ld, ldb, stream_ptr(x.device))
    rc = lib().ps_dprnn_block_step_slots_f32(*args) if slots else lib().ps_dprnn_block_step_f32(*args)
    check(rc, "ps_dprnn_block_step_slots_f32" if slots else "ps_dprnn_block_step_f32")
    return out


def skim_block_step_ok(c: int, hidden: int, seg: int) -> bool:
    """Whether ps_skim_block_step_f32 has a kernel for (C, H, K)."""
    return lib().ps_skim_block_step_ok(int(c), int(hidden), int(seg)) == 1


def skim_bank_slots(frames: int, seg: int) -> int:
    """The hand-over bank slots ps_skim_block_step_f32 asks for when a launch runs up to `frames` frames."""
    return (int(frames) - 1) // int(seg) + 3


def pack_skim_block(masker, i: int, device: torch.device) -> dict:
    """Block i of a causal SkiM -> the fp32 tensors of a ps_skim_block and the struct pointing at them (keep the dict alive
    while launches read it): the feature columns of its FiLM with the input norm (a block without fusion has none), the
    SegLSTM with projection and norm, MemLSTM i when there is one (every block but the last).  `embed_wt` [2C, E]: the
    embedding columns of (cond_scale ; cond_bias), for the per-stream terms rs / rb."""
    f32 = lambda t: t.detach().to(dtype=torch.float32, device=device)  # noqa: E731
    c = masker.input_size
    seg = masker.seg_lstm[i]
    p = dict(seg=pack_dprnn_pass(seg.lstm, seg.proj, seg.norm, device), C=c, H=masker.hidden_size, film=None, mem=None)
    s = _abi.SkimBlock()
    s.seg = p["seg"]["struct"]
    if masker.embed_dim > 0 and masker.block_with_embed[i]:
        film = masker.seg_input_fusion[i]
        ws, wb = f32(film.cond_scale.weight)[:, :, 0], f32(film.cond_bias.weight)[:, :, 0]
        p["film"] = dict(wt=torch.cat([ws[:, :c], wb[:, :c]], 0).t().contiguous(),                       # [C, 2C]
                         gamma=f32(film.norm.weight).contiguous(), beta=f32(film.norm.bias).contiguous(),
                         embed_wt=torch.cat([ws[:, c:], wb[:, c:]], 0).contiguous())
        s.film_wt, s.film_gamma, s.film_beta = (ptr(p["film"][k]) for k in ("wt", "gamma", "beta"))
        s.film_eps = float(film.norm.eps)
    if i < masker.n_blocks - 1:
        m = masker.mem_lstm[i]
        p["mem"] = (pack_dprnn_pass(m.h_net, m.h_proj, m.h_norm, device), pack_dprnn_pass(m.c_net, m.c_proj, m.c_norm, device))
        s.mem_h, s.mem_c = p["mem"][0]["struct"], p["mem"][1]["struct"]
    p["struct"] = s
    return p


def skim_block_step(x: torch.Tensor, counter: torch.Tensor, block: dict, seg_state: tuple, seg: int, streams: int, frames: int,
                    out: torch.Tensor, terms: Optional[tuple] = None, bank_in: Optional[tuple] = None,
                    mem_state: Optional[tuple] = None, bank_out: Optional[tuple] = None,
                    span: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One causal SkiM block on `frames` new frames of `streams` streams (ps_skim_block_step_f32): x [1, C, ld] (column
    f * streams + b) -> out [1, C, ld] (columns past frames * streams are not written); block from pack_skim_block;
    seg_state = (seg_h, seg_c) [H, ldb]; terms = (rs, rb) [C, ldb] iff the block has FiLM; bank_in = (init_h, init_c)
    [NS, H, ldb], None for the first block; mem_state = (mh_h, mc_h, mh_c, mc_c) [H, ldb] and bank_out = the next block's
    banks iff the block has a MemLSTM.  States and bank_out are updated in place; frame index of column 0 = counter[0],
    position = index % seg.  span int32 [streams, 2]: ps_skim_block_step_slots_f32, stream b computes frame g iff
    span[b, 0] <= g < span[b, 1], as frame n = g - span[b, 0] of its own segments (position n % seg, bank slots by n // seg);
    a frame that is not live reads x as 0, stores no state and no bank slot, and returns 0."""
    who = "skim_block_step"
    require_device(x, who)
    _, c, ld = x.shape
    hidden, ldb = seg_state[0].shape
    if not (x.is_contiguous() and out.is_contiguous()) or out.shape != x.shape or out.dtype != torch.float32 \
            or counter.dtype != torch.int32 or counter.device != x.device:
        raise RuntimeError(f"{who}: contiguous fp32 x and out [1, C, ld], an int32 counter on their device expected")
    if (c, hidden) != (block["C"], block["H"]) or block["seg"]["wt"].device != x.device:
        raise RuntimeError(f"{who}: a block packed for C = {c}, H = {hidden} on {x.device} expected")
    if (terms is not None) != (block["film"] is not None) or (mem_state is not None) != (block["mem"] is not None) \
            or (bank_out is not None) != (block["mem"] is not None):
        raise RuntimeError(f"{who}: terms go with a FiLM block, mem_state and bank_out with a MemLSTM, and only with them")
    st = _abi.SkimState()
    ns = 0
    groups = (("seg_state", seg_state, ("seg_h", "seg_c"), (hidden, ldb)), ("terms", terms, ("rs", "rb"), (c, ldb)),
              ("mem_state", mem_state, ("mh_h", "mc_h", "mh_c", "mc_c"), (hidden, ldb)),
              ("bank_in", bank_in, ("init_h", "init_c"), None), ("bank_out", bank_out, ("out_h", "out_c"), None))
    for what, tensors, names, shape in groups:
        if tensors is None:
            continue
        if len(tensors) != len(names):
            raise RuntimeError(f"{who}: {what} must be {names}")
        for name, t in zip(names, tensors):
            require_weight(t, x, who)
            if shape is None:
                ns = ns or t.shape[0]
                shape_ok = t.dim() == 3 and tuple(t.shape) == (ns, hidden, ldb)
            else:
                shape_ok = tuple(t.shape) == shape
            if not shape_ok:
                raise RuntimeError(f"{who}: {what}: states [H, ldb], terms [C, ldb] and banks [NS, H, ldb] of one H, ldb and NS "
                                   f"expected (got {tuple(t.shape)} for {name})")
            setattr(st, name, ptr(t))
    slots = span is not None
    if slots:
        _check_span(span, streams, x, who)
    args = (ptr(x), ptr(out), ptr(counter), *((ptr(span),) if slots else ()), C.byref(block["struct"]), C.byref(st), c,
            hidden, int(seg), ns, streams, frames, ld, ldb, stream_ptr(x.device))
    rc = lib().ps_skim_block_step_slots_f32(*args) if slots else lib().ps_skim_block_step_f32(*args)
    check(rc, "ps_skim_block_step_slots_f32" if slots else "ps_skim_block_step_f32")
    return out


def _conv2d_sources(who: str, x1: torch.Tensor, x2: Optional[torch.Tensor]) -> tuple[int, int, int, int, int]:
    """x1 [N,C1,F,ld] (+ x2 [N,C2,F,ld], the skip connection a decoder layer concatenates) -> (N, C1, C2, F, ld)."""
    require_device(x1, who)
    n, c1, f_in, ld = x1.shape
    if x2 is None:
        return n, c1, 0, f_in, ld
    _require_operand(who, x1.device, x2=x2)
    if (x2.shape[0], x2.shape[2], x2.shape[3]) != (n, f_in, ld):
        raise RuntimeError(f"{who}: the two sources must agree in N, F and ld")
    return n, c1, x2.shape[1], f_in, ld


def unfold2d(x1: torch.Tensor, x2: Optional[torch.Tensor], t: int, f_out: int, kf: int, kt: int, stride_f: int,
             dil_f: int, dil_t: int, pad_f: int, pad_t: int, transposed: bool, t_in: Optional[int] = None) -> torch.Tensor:
    """x1 [N,C1,F,ld] (+ x2 [N,C2,F,ld]) -> tap rows [N, (C1+C2)*kf*kt, f_out*ld] for the Conv2d / ConvTranspose2d GEMM."""
    n, c1, c2, f_in, ld = _conv2d_sources("unfold2d", x1, x2)
    y = torch.empty(n, (c1 + c2) * kf * kt, f_out * ld, dtype=torch.float32, device=x1.device)
    check(lib().ps_unfold2d_f32(ptr(x1), c1, ptr(x2), c2, ptr(y), n, f_in, t if t_in is None else t_in, t, ld, kf, kt, stride_f, dil_f, dil_t, pad_f,
                                pad_t, f_out, int(transposed), stream_ptr(x1.device)), "ps_unfold2d_f32")
    return y


def conv2d(x1: torch.Tensor, x2: Optional[torch.Tensor], wt: torch.Tensor, bias: Optional[torch.Tensor], m: int, t: int,
           f_out: int, kf: int, kt: int, stride_f: int, dil_f: int, dil_t: int, pad_f: int, pad_t: int, transposed: bool,
           act: str = "none", slope: Optional[torch.Tensor] = None, t_in: Optional[int] = None) -> torch.Tensor:
    """Implicit-GEMM Conv2d / ConvTranspose2d on [N,C,F,ld] rows -> [N,M,f_out,ld] with bias + activation."""
    n, c1, c2, f_in, ld = _conv2d_sources("conv2d", x1, x2)
    _require_operand("conv2d", x1.device, wt=wt, bias=bias, slope=slope)
    y = torch.empty(n, m, f_out, ld, dtype=torch.float32, device=x1.device)
    check(lib().ps_conv2d_f32(ptr(x1), c1, ptr(x2), c2, ptr(wt), ptr(bias), ptr(y), n, m, f_in,
                              t if t_in is None else t_in, t, ld, kf, kt, stride_f, dil_f, dil_t, pad_f, pad_t, f_out,
                              int(transposed), ACT_KINDS[act], ptr(slope), stream_ptr(x1.device)), "ps_conv2d_f32")
    return y


def pack_conv2d_f16x2(w2: torch.Tensor):
    """[M, K] fp32 (BatchNorm folded) -> (image of 2^w_exp W for ps_conv2d_f16x2_f32, w_exp); layout: include/puresound_hip.h.
    Reads the maximum back to the host: plan-build time only."""
    m, k = w2.shape
    w_exp = _f16_weight_exponent(w2, "pack_conv2d_f16x2")
    mt = 32 if m <= 32 else 64 if m <= 64 else 128
    tiles, nch = (m + mt - 1) // mt, (k + 31) // 32
    rest = torch.zeros(tiles * mt, nch * 32, dtype=torch.float32, device=w2.device)
    rest[:m, :k] = torch.ldexp(w2.detach().float(), torch.tensor(w_exp, device=w2.device))
    img = torch.stack(_split_planes(rest, torch.float16, 2), 0)
    img = img.reshape(2, tiles, mt // 16, 16, nch, 4, 8)                         # pl, tile, rb, row, chunk, kg, e
    img = img.permute(1, 4, 0, 2, 5, 3, 6).contiguous()                          # tile, chunk, pl, rb, kg, row, e
    return img, w_exp


def conv2d_f16x2(x1: torch.Tensor, x2: Optional[torch.Tensor], wimg: torch.Tensor, w_exp: int, bias: Optional[torch.Tensor],
                 m: int, t: int, f_out: int, kf: int, kt: int, stride_f: int, dil_f: int, dil_t: int, pad_f: int, pad_t: int,
                 transposed: bool, act: str = "none", slope: Optional[torch.Tensor] = None, t_in: Optional[int] = None,
                 want_stats: bool = False):
    """conv2d / conv2d_stats in the fp16x2 arithmetic (ps_conv2d_f16x2_f32; weights from pack_conv2d_f16x2).  Returns y, or
    (y, stats) with want_stats (the activation should then be "none": a gLN follows)."""
    n, c1, c2, f_in, ld = _conv2d_sources("conv2d_f16x2", x1, x2)
    _require_operand("conv2d_f16x2", x1.device, torch.float16, wimg=wimg)
    _require_operand("conv2d_f16x2", x1.device, bias=bias, slope=slope)
    y = torch.empty(n, m, f_out, ld, dtype=torch.float32, device=x1.device)
    stats = _stats_buffer(n, lib().ps_conv2d_stats_parts(m, f_out, ld), x1.device) if want_stats else None
    check(lib().ps_conv2d_f16x2_f32(ptr(x1), c1, ptr(x2), c2, ptr(wimg), int(w_exp), ptr(bias), ptr(y), n, m, f_in,
                                    t if t_in is None else t_in, t, ld, kf, kt, stride_f, dil_f, dil_t, pad_f, pad_t, f_out,
                                    int(transposed), ACT_KINDS[act], ptr(slope), ptr(stats), stream_ptr(x1.device)),
          "ps_conv2d_f16x2_f32")
    return (y, stats) if want_stats else y


def conv2d_stats(x1: torch.Tensor, x2: Optional[torch.Tensor], wt: torch.Tensor, bias: Optional[torch.Tensor], m: int, t: int,
                 f_out: int, kf: int, kt: int, stride_f: int, dil_f: int, dil_t: int, pad_f: int, pad_t: int, transposed: bool,
                 t_in: Optional[int] = None):
    """conv2d without activation + the partial (sum, sum of squares) of its outputs over the t valid frames ->
    (y [N,M,f_out,ld], stats [N, parts, 2] fp64): the convolution in front of a gLN (ps_conv2d_stats_f32)."""
    n, c1, c2, f_in, ld = _conv2d_sources("conv2d_stats", x1, x2)
    _require_operand("conv2d_stats", x1.device, wt=wt, bias=bias)
    y = torch.empty(n, m, f_out, ld, dtype=torch.float32, device=x1.device)
    stats = _stats_buffer(n, lib().ps_conv2d_stats_parts(m, f_out, ld), x1.device)
    check(lib().ps_conv2d_stats_f32(ptr(x1), c1, ptr(x2), c2, ptr(wt), ptr(bias), ptr(y), n, m, f_in,
                                    t if t_in is None else t_in, t, ld, kf, kt, stride_f, dil_f, dil_t, pad_f, pad_t, f_out,
                                    int(transposed), ptr(stats), stream_ptr(x1.device)), "ps_conv2d_stats_f32")
    return y, stats


def activation_(x: torch.Tensor, kind: str, slope: Optional[torch.Tensor], t: int) -> torch.Tensor:
    """in place on [..., ld] rows."""
    require_device(x, "activation_")
    ld = x.shape[-1]
    check(lib().ps_activation_f32(ptr(x), ACT_KINDS[kind], ptr(slope), x.numel() // ld, t, ld, stream_ptr(x.device)),
          "ps_activation_f32")
    return x


def row_stats(x: torch.Tensor, t: int) -> torch.Tensor:
    """padded rows [N, rows, ld] -> [N, parts, 2] fp64 partial (sum, sum of squares) over the t valid frames."""
    require_device(x, "row_stats")
    n, rows, ld = x.shape
    out = _stats_buffer(n, lib().ps_row_stats_parts(), x.device)
    check(lib().ps_row_stats_f64(ptr(x), ptr(out), n, rows, t, ld, stream_ptr(x.device)), "ps_row_stats_f64")
    return out


def norm_activation_(x4: torch.Tensor, t: int, pro: Prologue, corr_sum: float, corr_sq: float, kind: str,
                     slope: Optional[torch.Tensor]) -> torch.Tensor:
    """gLN over [CH, F, T] + activation, in place on [N, CH, F, ld]."""
    require_device(x4, "norm_activation_")
    n, ch, f, ld = x4.shape
    check(lib().ps_norm_activation_f32(ptr(x4), C.byref(pro), float(corr_sum), float(corr_sq), f, ACT_KINDS[kind],
                                       ptr(slope), n, ch * f, t, ld, stream_ptr(x4.device)), "ps_norm_activation_f32")
    return x4


def real_mask(feats: torch.Tensor, mask: torch.Tensor, mask_act: str = "linear") -> torch.Tensor:
    """feats * act(mask) on padded rows."""
    require_device(feats, "real_mask")
    if mask.shape != feats.shape:
        raise RuntimeError("real_mask: feats and mask must have one shape")
    out = torch.empty_like(feats)
    ldt = feats.shape[-1]
    check(lib().ps_real_mask_f32(ptr(feats), ptr(mask), ptr(out), feats.numel() // ldt, ldt, _abi.PS_ACT[mask_act],
                                 stream_ptr(feats.device)), "ps_real_mask_f32")
    return out


def fill_span(x: torch.Tensor, axis: int, lo: int, hi: int, value: float) -> torch.Tensor:
    """[N, rows, ld] -> a copy with rows [lo, hi) (axis 1) or frames [lo, hi) (axis 2) set to `value` (SpecAugment)."""
    require_device(x, "fill_span")
    n, rows, ld = x.shape
    y = torch.empty_like(x)
    check(lib().ps_fill_span_f32(ptr(x), ptr(y), n, rows, ld, axis, int(lo), int(hi), float(value), stream_ptr(x.device)),
          "ps_fill_span_f32")
    return y


def magnitude(x: torch.Tensor, t: int, drop_first: bool, log1p: bool, kind: Optional[str] = None) -> torch.Tensor:
    """[re rows; im rows] padded [N,2H,ldt] -> |.| (or log1p|.|, or the power with kind="power"/"power_eps")
    padded [N,H-drop,ldt]."""
    require_device(x, "magnitude")
    n, c2, ldt = x.shape
    half = c2 // 2
    y = torch.zeros(n, half - int(drop_first), ldt, dtype=torch.float32, device=x.device)
    k = {"power": 2, "power_eps": 3}[kind] if kind else int(log1p)
    check(lib().ps_magnitude_f32(ptr(x), ptr(y), n, half, int(drop_first), k, t, ldt, stream_ptr(x.device)),
          "ps_magnitude_f32")
    return y


def add_(dst: torch.Tensor, other: torch.Tensor) -> torch.Tensor:
    """dst += other (same shape, contiguous)."""
    require_device(dst, "add_")
    if dst.shape != other.shape or not dst.is_contiguous() or not other.is_contiguous():
        raise RuntimeError("add_: contiguous tensors of one shape")
    check(lib().ps_add_f32(ptr(dst), ptr(other), ptr(dst), dst.numel(), stream_ptr(dst.device)), "ps_add_f32")
    return dst


def self_attention(qkv: torch.Tensor, e: int, heads: int, q: int, q_stride: int, length: int, pos_stride: int,
                   causal: bool = False) -> torch.Tensor:
    """qkv padded [N,3E,ld] -> attention output [N,E,ld] (sequence (n,q): positions at q*q_stride + p*pos_stride)."""
    require_device(qkv, "self_attention")
    n, rows, ld = qkv.shape
    if rows != 3 * e:
        raise RuntimeError("self_attention: qkv must be [N, 3E, ld]")
    out = torch.empty(n, e, ld, dtype=torch.float32, device=qkv.device)
    check(lib().ps_self_attention_f32(ptr(qkv), ptr(out), n, e, heads, q, q_stride, length, pos_stride, ld, int(causal),
                                      stream_ptr(qkv.device)), "ps_self_attention_f32")
    return out


def add_position(x: torch.Tensor, pe: torch.Tensor, q: int, q_stride: int, length: int, pos_stride: int) -> torch.Tensor:
    """x padded [N,E,ld] + pe[pos][c] at every sequence position."""
    require_device(x, "add_position")
    n, e, ld = x.shape
    y = x.clone()
    check(lib().ps_add_position_f32(ptr(x), ptr(pe), ptr(y), n, e, q, q_stride, length, pos_stride, ld,
                                    stream_ptr(x.device)), "ps_add_position_f32")
    return y


def wave_moments(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Rows of two waveform batches [R, L] (last-dim contiguous) -> fp64 moments [R, 5] = (sum a, sum b, sum a^2,
    sum b^2, sum ab) in one streaming pass (ps_wave_moments_f64)."""
    require_device(a, "wave_moments")
    require_device(b, "wave_moments")
    if a.dim() != 2 or a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise RuntimeError("wave_moments: two fp32 tensors of the same shape [R, L]")
    if a.stride(1) != 1:
        a = a.contiguous()
    if b.stride(1) != 1:
        b = b.contiguous()
    r, length = a.shape
    chunks = lib().ps_wave_moments_chunks(length)
    part = torch.empty(r, chunks, 5, dtype=torch.float64, device=a.device)
    check(lib().ps_wave_moments_f64(ptr(a), ptr(b), ptr(part), r, length, a.stride(0), b.stride(0),
                                    stream_ptr(a.device)), "ps_wave_moments_f64")
    return part.sum(1)


def stft_frames(length: int, n_fft: int, hop: int) -> int:
    """Frames of torch.stft(center=True): the length + 2 (n_fft // 2) padded samples hold 1 + (length - n_fft % 2) // hop
    frames of n_fft samples (an odd n_fft has one fewer when hop divides the length)."""
    return 1 + (length - n_fft % 2) // hop


def frame_reflect(a: torch.Tensor, b: Optional[torch.Tensor], n_fft: int, win: int, hop: int,
                  out: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, int]:
    """a (and b) [N, L] -> (frames padded [R, win, ldt], T): torch.stft's frames (center=True, reflect padding) on the
    support of a window of `win` samples centred in n_fft, T = stft_frames(L, n_fft, hop); R = 2N with rows N + n from b, else N
    (ps_frame_reflect_f32).  `out`: a contiguous [R, win, ldt] tensor to write into."""
    require_device(a, "frame_reflect")
    if a.dim() != 2 or (b is not None and (b.shape != a.shape or b.device != a.device or b.dtype != torch.float32)):
        raise RuntimeError("frame_reflect: fp32 waveforms [N, L] of one shape on one device")
    n, length = a.shape
    if win > n_fft or win < 1 or hop < 1:
        raise RuntimeError(f"frame_reflect: need 1 <= win <= n_fft and hop >= 1 (got win={win}, n_fft={n_fft}, hop={hop})")
    if length <= n_fft // 2:
        raise RuntimeError(f"frame_reflect: reflect padding needs more than n_fft // 2 samples (length {length}, "
                           f"fft_size {n_fft})")
    if a.stride(1) != 1:
        a = a.contiguous()
    if b is not None and b.stride(1) != 1:
        b = b.contiguous()
    rows = n if b is None else 2 * n
    t = stft_frames(length, n_fft, hop)
    ldt = padded_frames(t)
    if out is None:
        out = torch.empty(rows, win, ldt, dtype=torch.float32, device=a.device)
    elif tuple(out.shape) != (rows, win, ldt):
        raise RuntimeError(f"frame_reflect: `out` must be [{rows}, {win}, {ldt}]")
    _require_operand("frame_reflect", a.device, out=out)
    check(lib().ps_frame_reflect_f32(ptr(a), ptr(b), ptr(out), n, length, a.stride(0), 0 if b is None else b.stride(0),
                                     n_fft, win, hop, t, ldt, stream_ptr(a.device)), "ps_frame_reflect_f32")
    return out, t


def spec_pair_moments(spec: torch.Tensor, bins: int, t: int, p: float = 0.5,
                      mag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """spec padded [2N, 2*bins, ldt] ([re rows; im rows]; rows n: estimate, rows N + n: reference) -> fp64 [N, 4]:
    S0 = sum (y-x)^2, S1 = sum y^2, S2 = sum |log y - log x|, S3 = sum relu(y^p - x^p)^2 over t frames and bins of the
    clamped magnitudes x (estimate), y (reference) (ps_spec_pair_moments_f64).  `mag`: a contiguous [2N, bins, ldt] tensor
    that receives those magnitudes (columns >= t undefined)."""
    require_device(spec, "spec_pair_moments")
    if spec.dim() != 3 or spec.shape[0] % 2 or spec.shape[1] != 2 * bins or not spec.is_contiguous():
        raise RuntimeError("spec_pair_moments: spec must be a contiguous [2N, 2*bins, ldt] tensor")
    n, ldt = spec.shape[0] // 2, spec.shape[2]
    if mag is not None and tuple(mag.shape) != (2 * n, bins, ldt):
        raise RuntimeError(f"spec_pair_moments: `mag` must be [{2 * n}, {bins}, {ldt}]")
    _require_operand("spec_pair_moments", spec.device, mag=mag)
    parts = lib().ps_spec_pair_moments_parts(bins, t)
    part = torch.empty(n, max(parts, 1), 4, dtype=torch.float64, device=spec.device)
    check(lib().ps_spec_pair_moments_f64(ptr(spec), ptr(part), ptr(mag), n, bins, t, ldt, float(p),
                                         stream_ptr(spec.device)), "ps_spec_pair_moments_f64")
    return part.sum(1)


def lstm_cell(gates: torch.Tensor, c: torch.Tensor, h: torch.Tensor, hidden: int, dirs: int, t: int) -> None:
    """One cell update per (unit, frame): gates padded [N,D*4H,ld] (complete pre-activations), c in place, h out
    (both [N,D*H,ld'] rows, possibly views into larger row blocks)."""
    require_device(gates, "lstm_cell")
    n = gates.shape[0]
    if gates.shape[1] != dirs * 4 * hidden or tuple(c.shape[:2]) != (n, dirs * hidden) or c.shape != h.shape \
            or c.stride(1) != h.stride(1):
        raise RuntimeError("lstm_cell: gates [N,D*4H,ld], c/h [N,D*H,ld']")
    if n > 1 and (not c.is_contiguous() or not h.is_contiguous()):
        raise RuntimeError("lstm_cell: state views are supported for N = 1 only")
    check(lib().ps_lstm_cell_f32(ptr(gates), ptr(c), ptr(h), n, hidden, dirs, t, gates.shape[2], c.stride(1),
                                 stream_ptr(gates.device)), "ps_lstm_cell_f32")


def film_apply(x: torch.Tensor, scale_bias: torch.Tensor, t: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """scale_bias padded [N,2C,ldt] (scale rows, then bias rows), x padded [N,C,ldt] -> scale * x + bias."""
    require_device(x, "film_apply")
    n, c, ldt = x.shape
    if tuple(scale_bias.shape) != (n, 2 * c, ldt):
        raise RuntimeError("film_apply: scale_bias must be [N, 2C, ldt]")
    y = out if out is not None else torch.empty_like(x)
    check(lib().ps_film_apply_f32(ptr(x), ptr(scale_bias), ptr(y), n, c, t, ldt, stream_ptr(x.device)),
          "ps_film_apply_f32")
    return y


def embed_bias(dvec: torch.Tensor, w_embed: torch.Tensor, normalize: bool) -> torch.Tensor:
    require_device(dvec, "embed_bias")
    require_weight(w_embed, dvec, "embed_bias")
    n, e = dvec.shape
    m = w_embed.shape[0]
    out = torch.empty(n, m, dtype=torch.float32, device=dvec.device)
    check(lib().ps_embed_bias_f32(ptr(dvec.contiguous()), ptr(w_embed), ptr(out), n, e, m, int(normalize),
                                  stream_ptr(dvec.device)), "ps_embed_bias_f32")
    return out


_EYE = {}


def l2_normalize(dvec: torch.Tensor) -> torch.Tensor:
    """F.normalize(dvec, p=2, dim=1) through ps_embed_bias_f32 with an identity weight (exact: every output is one
    product with 1 plus zeros)."""
    require_device(dvec, "l2_normalize")
    e = dvec.shape[1]
    key = (str(dvec.device), e)
    if key not in _EYE:
        _EYE[key] = torch.eye(e, dtype=torch.float32, device=dvec.device)
    return embed_bias(dvec.float(), _EYE[key], True)


def conv_tasnet_workspace(n: int, c: int, h: int, t: int, device: torch.device,
                          have: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The scratch conv_tasnet needs for (n, c, h, t) on `device`: `have` when it is large enough and lives there, else a new,
    zero-filled one (three hidden maps: 415 MB at 32 x 4 s -- a caller that runs more than once keeps what this returns)."""
    need = lib().ps_conv_tasnet_workspace_bytes(n, c, h, t)
    if have is not None and have.numel() >= need and have.device == device:
        return have
    return torch.zeros(need, dtype=torch.uint8, device=device)


def _embed_sizes(blocks: "C.Array[TcnBlock]", n_blocks: int) -> frozenset:
    """The E of the blocks that take an embedding.  Kept on the array: callers hold it as long as their plans."""
    kept = getattr(blocks, "_embed_sizes", None)
    if kept is None or kept[0] != n_blocks:
        kept = blocks._embed_sizes = (n_blocks, frozenset(blocks[i].E for i in range(n_blocks) if blocks[i].in_embed_w))
    return kept[1]


def conv_tasnet(blocks: "C.Array[TcnBlock]", n_blocks: int, x_pad: torch.Tensor, t: int, c: int, h: int,
                dvec: Optional[torch.Tensor], embed_norm: bool,
                workspace: Optional[torch.Tensor] = None, x_amax: Optional[torch.Tensor] = None,
                bf16_rows: bool = False) -> torch.Tensor:
    """Run the whole masker on padded input [N,C,ldt]; returns padded mask logits [N,C,ldt] (the frames beyond T are
    not written).  x_amax [N, parts]: per utterance, values whose maximum bounds |x_pad[n]| -- the range blocks in the
    fp16x2 arithmetic scale their input by (without it they measure it with one pass over x_pad).  bf16 rows in (or
    bf16_rows): the residual stream as bf16 rows (BASELINE config 3's arithmetic), every block in the bf16 arithmetic."""
    require_device(x_pad, "conv_tasnet", allow_bf16=True)
    if x_pad.dim() != 3 or x_pad.shape[1] != c or not x_pad.is_contiguous():
        raise RuntimeError(f"conv_tasnet: x_pad must be contiguous [N, C={c}, ldt] (got {tuple(x_pad.shape)}, "
                           f"strides {x_pad.stride()})")
    n, _, ldt = x_pad.shape
    dev = x_pad.device
    if x_amax is not None and (x_amax.dim() != 2 or x_amax.shape[0] != n or not x_amax.is_contiguous()):
        raise ValueError(f"conv_tasnet: x_amax must be a contiguous [N={n}, parts] tensor, got {tuple(x_amax.shape)}")
    _require_operand("conv_tasnet", dev, dvec=dvec, x_amax=x_amax)
    if dvec is not None:
        sizes = _embed_sizes(blocks, n_blocks)
        if dvec.dim() != 2 or dvec.shape[0] != n or sizes - {dvec.shape[1]}:
            raise RuntimeError(f"conv_tasnet: dvec must be [N={n}, E], the blocks' E={sorted(sizes)} (got {tuple(dvec.shape)})")
    if bf16_rows and x_pad.dtype == torch.float32:
        # fp32 rows in, fp32 rows out, the residual stream in between as bf16 rows (two dtype casts around the stack)
        return conv_tasnet(blocks, n_blocks, x_pad.to(torch.bfloat16), t, c, h, dvec, embed_norm, workspace).float()
    workspace = conv_tasnet_workspace(n, c, h, t, dev, workspace)
    _require_operand("conv_tasnet", dev, torch.uint8, workspace=workspace)
    out = torch.empty_like(x_pad)
    if x_pad.dtype == torch.bfloat16:
        check(lib().ps_conv_tasnet_bf16_rows(blocks, n_blocks, ptr(x_pad), ptr(out), ptr(dvec), int(embed_norm), n, t, ldt,
                                             ptr(workspace), workspace.numel(), stream_ptr(dev)), "ps_conv_tasnet_bf16_rows")
    else:
        parts = 0 if x_amax is None else x_amax.shape[1]
        check(lib().ps_conv_tasnet_ranged_f32(blocks, n_blocks, ptr(x_pad), ptr(out), ptr(dvec), int(embed_norm), n, t, ldt,
                                              ptr(workspace), workspace.numel(), ptr(x_amax), parts, stream_ptr(dev)),
              "ps_conv_tasnet_ranged_f32")
    return out


# ---- batches of utterances of unequal length (csrc/ragged.hip) ----------------------------------------------------------------
def row_limits(who: str, values: Sequence[Sequence[int]], device: torch.device) -> torch.Tensor:
    """Host integers [K][N] -> one int32 device tensor [K, N] by ONE host-to-device copy: the per-row limits of a ragged call
    (frames per utterance, valid output samples, ...), already validated by the caller; row k is contiguous."""
    host = torch.tensor(values, dtype=torch.int32)
    if host.dim() != 2:
        raise ValueError(f"{who}: the limits must be K sequences of N integers")
    return host.to(device)


def _require_limits(who: str, lim: torch.Tensor, n: int, device: torch.device) -> None:
    _require_operand(who, device, torch.int32, limits=lim)
    if tuple(lim.shape) != (n,):
        raise ValueError(f"{who}: the per-row limits must be an int32 tensor [N={n}], got {tuple(lim.shape)}")


def ragged_stats(y: torch.Tensor, t: int, t_rows: torch.Tensor, parts: Optional[int] = None) -> torch.Tensor:
    """y padded [N,R,ldt], t_rows int32 [N] -> partial (sum, sum of squares) [N,parts,2] fp64 over t < t_rows[n], scaled so
    that a prologue with count = R * t derives the statistics of the R * t_rows[n] valid elements."""
    require_device(y, "ragged_stats")
    n, r, ldt = y.shape
    _require_limits("ragged_stats", t_rows, n, y.device)
    parts = lib().ps_stats_parts(r, t) if parts is None else int(parts)
    if parts <= 0 or not y.is_contiguous():
        raise RuntimeError(f"ragged_stats: contiguous rows and parts > 0 (got parts={parts}, strides {y.stride()})")
    stats = _stats_buffer(n, parts, y.device)
    check(lib().ps_ragged_stats_f32(ptr(y), ptr(t_rows), ptr(stats), n, r, t, ldt, parts, float(r) * float(t),
                                    stream_ptr(y.device)), "ps_ragged_stats_f32")
    return stats


def dwconv_ragged(x: torch.Tensor, t: int, t_rows: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], dilation: int,
                  left: int, pro: Optional[Prologue] = None, want_stats: bool = False
                  ) -> tuple[torch.Tensor, Optional[torch.Tensor]]:
    """dwconv with a per-row frame limit: x padded [N,H,ldt], w [H,1,P] -> y padded [N,H,ldt], 0 on [t_rows[n], t) (+ the
    partial statistics over t < t_rows[n], scaled as ragged_stats')."""
    require_device(x, "dwconv_ragged")
    _require_operand("dwconv_ragged", x.device, w=w, b=b)
    n, h, ldt = x.shape
    _require_limits("dwconv_ragged", t_rows, n, x.device)
    y = torch.empty_like(x)
    stats = _stats_buffer(n, lib().ps_dwconv_stats_parts(h, t), x.device) if want_stats else None
    check(lib().ps_dwconv_ragged_f32(ptr(x), ptr(w), ptr(b), ptr(y), ptr(t_rows), n, h, t, ldt, w.shape[-1], dilation, left,
                                     C.byref(pro) if pro is not None else None, ptr(stats), float(h) * float(t),
                                     stream_ptr(x.device)), "ps_dwconv_ragged_f32")
    return y, stats


def zero_tail(x: torch.Tensor, limits: torch.Tensor) -> torch.Tensor:
    """x [N,R,ld] (or a waveform batch [N,ld]), in place: 0.0 at columns >= limits[n]; nothing is read."""
    require_device(x, "zero_tail")
    if x.dim() not in (2, 3) or not x.is_contiguous():
        raise RuntimeError(f"zero_tail: a contiguous [N, R, ld] or [N, ld] tensor (got {tuple(x.shape)}, strides {x.stride()})")
    n, ld = x.shape[0], x.shape[-1]
    _require_limits("zero_tail", limits, n, x.device)
    check(lib().ps_zero_tail_f32(ptr(x), ptr(limits), n, x.numel() // (n * ld), ld, stream_ptr(x.device)), "ps_zero_tail_f32")
    return x


def conv2d_ragged(x1: torch.Tensor, x2: Optional[torch.Tensor], wt: torch.Tensor, bias: Optional[torch.Tensor], m: int, t: int,
                  t_rows: torch.Tensor, f_out: int, kf: int, kt: int, stride_f: int, dil_f: int, dil_t: int, pad_f: int,
                  pad_t: int, transposed: bool, act: str = "none", slope: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv2d with a per-row frame limit (t_rows int32 [N] on the device) in place of t_in: row n on its first t_rows[n]
    frames is conv2d of that row alone with t = t_in = t_rows[n], 0.0 behind them; what the sources hold behind a row's
    end is not read as data (ps_conv2d_ragged_f32)."""
    n, c1, c2, f_in, ld = _conv2d_sources("conv2d_ragged", x1, x2)
    _require_operand("conv2d_ragged", x1.device, wt=wt, bias=bias, slope=slope)
    _require_limits("conv2d_ragged", t_rows, n, x1.device)
    y = torch.empty(n, m, f_out, ld, dtype=torch.float32, device=x1.device)
    check(lib().ps_conv2d_ragged_f32(ptr(x1), c1, ptr(x2), c2, ptr(wt), ptr(bias), ptr(y), n, m, f_in, ptr(t_rows), t, ld, kf,
                                     kt, stride_f, dil_f, dil_t, pad_f, pad_t, f_out, int(transposed), ACT_KINDS[act],
                                     ptr(slope), stream_ptr(x1.device)), "ps_conv2d_ragged_f32")
    return y


def istft_ola_ragged(frames: torch.Tensor, t: int, t_rows: torch.Tensor, window: torch.Tensor, hop: int,
                     out_mode: str = "none") -> torch.Tensor:
    """istft_ola with a per-row frame limit: frames padded [N,n_fft,ldt] -> waveform [N,(t-1)*hop+n_fft]; row n's first
    (t_rows[n]-1)*hop+n_fft samples are istft_ola of its first t_rows[n] frames, 0.0 behind them (ps_istft_ola_ragged_f32)."""
    require_device(frames, "istft_ola_ragged")
    _require_operand("istft_ola_ragged", frames.device, window=window)
    n, n_fft, ldt = frames.shape
    _require_limits("istft_ola_ragged", t_rows, n, frames.device)
    if not frames.is_contiguous() or window.numel() != n_fft:
        raise RuntimeError(f"istft_ola_ragged: contiguous frames [N, n_fft, ldt] and a window of n_fft = {n_fft} values")
    out = torch.empty(n, (t - 1) * hop + n_fft, dtype=torch.float32, device=frames.device)
    check(lib().ps_istft_ola_ragged_f32(ptr(frames), ptr(window), ptr(out), ptr(t_rows), n, n_fft, hop, t, ldt,
                                        _abi.PS_OUT[out_mode], stream_ptr(frames.device)), "ps_istft_ola_ragged_f32")
    return out


def align_rows(ref: torch.Tensor, a_len: torch.Tensor, b_len: torch.Tensor, length: int) -> torch.Tensor:
    """align_reference per row: ref [N, L_ref] (last-dim contiguous) -> [N, length] with row n's b_len[n] reference samples
    aligned to a_len[n] valid output samples -- left-padded with zeros when shorter, cut when longer -- and exact 0.0 behind
    a_len[n]; a_len, b_len int32 [N] on the device.  What ref holds behind b_len[n] is not read (ps_align_rows_f32)."""
    require_device(ref, "align_rows")
    if ref.dim() != 2 or ref.dtype != torch.float32 or ref.shape[1] < 1 or length < 1:
        raise RuntimeError(f"align_rows: an fp32 [N, L_ref] reference and length >= 1 (got {tuple(ref.shape)} {ref.dtype}, "
                           f"length {length})")
    if ref.stride(1) != 1:
        ref = ref.contiguous()
    n, l_ref = ref.shape
    _require_limits("align_rows", a_len, n, ref.device)
    _require_limits("align_rows", b_len, n, ref.device)
    out = torch.empty(n, length, dtype=torch.float32, device=ref.device)
    check(lib().ps_align_rows_f32(ptr(ref), ptr(out), ptr(a_len), ptr(b_len), n, length, l_ref, ref.stride(0),
                                  stream_ptr(ref.device)), "ps_align_rows_f32")
    return out


def wave_moments_rows(a: torch.Tensor, b: torch.Tensor, len_rows: torch.Tensor) -> torch.Tensor:
    """wave_moments over the first len_rows[n] samples of row n (int32 [R] on the device): what the rows hold behind them, a
    NaN included, changes no bit; len_rows[n] == L gives wave_moments' bits (ps_wave_moments_rows_f64)."""
    require_device(a, "wave_moments_rows")
    require_device(b, "wave_moments_rows")
    if a.dim() != 2 or a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise RuntimeError("wave_moments_rows: two fp32 tensors of the same shape [R, L]")
    if a.stride(1) != 1:
        a = a.contiguous()
    if b.stride(1) != 1:
        b = b.contiguous()
    r, length = a.shape
    _require_limits("wave_moments_rows", len_rows, r, a.device)
    chunks = lib().ps_wave_moments_chunks(length)
    part = torch.empty(r, chunks, 5, dtype=torch.float64, device=a.device)
    check(lib().ps_wave_moments_rows_f64(ptr(a), ptr(b), ptr(len_rows), ptr(part), r, length, a.stride(0), b.stride(0),
                                         stream_ptr(a.device)), "ps_wave_moments_rows_f64")
    return part.sum(1)


def frame_reflect_rows(a: torch.Tensor, b: Optional[torch.Tensor], len_rows: torch.Tensor, n_fft: int, win: int, hop: int,
                       out: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, int]:
    """frame_reflect with rows n (and N + n) framed as utterances of len_rows[n] samples on their own (int32 [N] on the
    device, each > n_fft // 2: the host's check): stft_frames(len_rows[n], n_fft, hop) frames reflected at the row's own end,
    zeros in every column behind them; T = stft_frames(L, n_fft, hop) is the launch's (ps_frame_reflect_rows_f32)."""
    require_device(a, "frame_reflect_rows")
    if a.dim() != 2 or (b is not None and (b.shape != a.shape or b.device != a.device or b.dtype != torch.float32)):
        raise RuntimeError("frame_reflect_rows: fp32 waveforms [N, L] of one shape on one device")
    n, length = a.shape
    if win > n_fft or win < 1 or hop < 1:
        raise RuntimeError(f"frame_reflect_rows: need 1 <= win <= n_fft and hop >= 1 (got win={win}, n_fft={n_fft}, hop={hop})")
    if length <= n_fft // 2:
        raise RuntimeError(f"frame_reflect_rows: reflect padding needs more than n_fft // 2 samples (length {length}, "
                           f"fft_size {n_fft})")
    _require_limits("frame_reflect_rows", len_rows, n, a.device)
    if a.stride(1) != 1:
        a = a.contiguous()
    if b is not None and b.stride(1) != 1:
        b = b.contiguous()
    rows = n if b is None else 2 * n
    t = stft_frames(length, n_fft, hop)
    ldt = padded_frames(t)
    if out is None:
        out = torch.empty(rows, win, ldt, dtype=torch.float32, device=a.device)
    elif tuple(out.shape) != (rows, win, ldt):
        raise RuntimeError(f"frame_reflect_rows: `out` must be [{rows}, {win}, {ldt}]")
    _require_operand("frame_reflect_rows", a.device, out=out)
    check(lib().ps_frame_reflect_rows_f32(ptr(a), ptr(b), ptr(len_rows), ptr(out), n, length, a.stride(0),
                                          0 if b is None else b.stride(0), n_fft, win, hop, t, ldt, stream_ptr(a.device)),
          "ps_frame_reflect_rows_f32")
    return out, t


def spec_pair_moments_rows(spec: torch.Tensor, bins: int, t: int, t_rows: torch.Tensor, p: float = 0.5,
                           slots: bool = False) -> torch.Tensor:
    """spec_pair_moments over the first t_rows[n] <= t frames of utterance n (int32 [N] on the device): what the columns
    behind them hold changes no bit; t_rows[n] == t gives spec_pair_moments' bits (ps_spec_pair_moments_rows_f64).
    slots: the partials [N, parts, 4] as the kernel wrote them (slot (bins // 16) * ceil(t / 256) + t // 256 holds 16 bins x
    256 frames), not their sum."""
    require_device(spec, "spec_pair_moments_rows")
    if spec.dim() != 3 or spec.shape[0] % 2 or spec.shape[1] != 2 * bins or not spec.is_contiguous():
        raise RuntimeError("spec_pair_moments_rows: spec must be a contiguous [2N, 2*bins, ldt] tensor")
    n, ldt = spec.shape[0] // 2, spec.shape[2]
    _require_limits("spec_pair_moments_rows", t_rows, n, spec.device)
    parts = lib().ps_spec_pair_moments_parts(bins, t)
    part = torch.empty(n, max(parts, 1), 4, dtype=torch.float64, device=spec.device)
    check(lib().ps_spec_pair_moments_rows_f64(ptr(spec), ptr(t_rows), ptr(part), n, bins, t, ldt, float(p),
                                              stream_ptr(spec.device)), "ps_spec_pair_moments_rows_f64")
    return part if slots else part.sum(1)


def conv_tasnet_ragged(blocks: "C.Array[TcnBlock]", n_blocks: int, x_pad: torch.Tensor, t: int, c: int, h: int,
                       t_rows: torch.Tensor, dvec: Optional[torch.Tensor], embed_norm: bool,
                       workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv_tasnet for a batch whose row n holds t_rows[n] <= t valid frames (int32 [N] on the device) and anything behind
    them: padded [N,C,ldt] -> padded mask logits, row n those of its utterance alone on [0, t_rows[n]) and junk behind.
    Exact fp32 products whatever the blocks' gemm_planes."""
    require_device(x_pad, "conv_tasnet_ragged")
    if x_pad.dim() != 3 or x_pad.shape[1] != c or not x_pad.is_contiguous():
        raise RuntimeError(f"conv_tasnet_ragged: x_pad must be contiguous [N, C={c}, ldt] (got {tuple(x_pad.shape)}, "
                           f"strides {x_pad.stride()})")
    n, _, ldt = x_pad.shape
    dev = x_pad.device
    _require_limits("conv_tasnet_ragged", t_rows, n, dev)
    _require_operand("conv_tasnet_ragged", dev, dvec=dvec)
    if dvec is not None:
        sizes = _embed_sizes(blocks, n_blocks)
        if dvec.dim() != 2 or dvec.shape[0] != n or sizes - {dvec.shape[1]}:
            raise RuntimeError(f"conv_tasnet_ragged: dvec must be [N={n}, E], the blocks' E={sorted(sizes)} "
                               f"(got {tuple(dvec.shape)})")
    workspace = conv_tasnet_workspace(n, c, h, t, dev, workspace)
    _require_operand("conv_tasnet_ragged", dev, torch.uint8, workspace=workspace)
    out = torch.empty_like(x_pad)
    check(lib().ps_conv_tasnet_ragged_f32(blocks, n_blocks, ptr(x_pad), ptr(out), ptr(dvec), int(embed_norm), n, t, ldt,
                                          ptr(t_rows), ptr(workspace), workspace.numel(), stream_ptr(dev)),
          "ps_conv_tasnet_ragged_f32")
    return out
