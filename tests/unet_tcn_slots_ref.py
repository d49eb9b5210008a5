"""A pure-torch fp64 reference of the span rule StreamingUnetTcn's slot sessions run by (puresound_amd/streaming/unet_tcn.py,
ps_conv2d_step_slots_f32 / ps_gated_tcn_step_slots_f32 / ps_istft_step_slots_f32): frame g of a tensor is read as an exact 0
for stream b unless span[b, 0] <= g < span[b, 1], a select (dead frames may hold anything), and a layer that runs `shift`
frames behind the hop reads its current tensors as frame t - shift.  Written the way the kernels are specified: explicit
loops over hops and taps.  span is a [B, 2] integer tensor (birth, death)."""
import torch
import torch.nn.functional as F

import gated_tcn_step_ref as G
import unet_delay_ref as UD

INT32_MAX = 2 ** 31 - 1


def live(span, g):
    """[B] bool: frame g is live in stream b."""
    return (span[:, 0] <= g) & (g < span[:, 1])


def select(x, keep):
    """x [B, ...] with the streams outside `keep` [B] replaced by exact zeros (a select: NaN does not pass)."""
    return torch.where(keep.view(-1, *([1] * (x.dim() - 1))), x, torch.zeros_like(x))


# ---- ps_conv2d_step_slots_f32 -------------------------------------------------------------------------------------------
def conv2d_taps(cur, ring, span, t, shift):
    """cur [B, C, F] (frame t - shift), ring [R, B, C, F] (slot R - d = frame t - shift - d) -> [B, C, F, R + 1], the time
    axis oldest first, dead frames selected to zero."""
    r = ring.shape[0]
    seq = [select(ring[r - d], live(span, t - shift - d)) for d in range(r, 0, -1)] + [select(cur, live(span, t - shift))]
    return torch.stack(seq, dim=-1)


def conv2d_last_frame(seq, w, bias, slope, transposed, kf, sf, df, dt):
    """The newest output frame of the causal Conv2d / trimmed ConvTranspose2d + bias + PReLU on seq [B, C, F, hist + 1] whose
    earlier frames are the zero padding -> [B, M, Fout]."""
    pf, hist = kf // 2, seq.shape[-1] - 1
    if transposed:
        op = sf - kf + 2 * pf
        y = F.conv_transpose2d(seq, w, stride=(sf, 1), padding=(pf, 0), output_padding=(op, 0), dilation=(df, dt))[..., hist]
    else:
        y = F.conv2d(F.pad(seq, (hist, 0, pf, pf)), w, stride=(sf, 1), dilation=(df, dt))[..., hist]
    return F.prelu(y + bias.view(1, -1, 1), slope)


# ---- the up path: n delayed transposed convolutions, layer j with shift j -------------------------------------------------
def up_path_slots(x, skips, layers, span, hops):
    """x, skips[j] [B, C, F, hops]: what hop s holds for every stream, dead frames included (anything).  Layer j at hop s
    reads cat(x_j, skip_j) at frame s - j (current) and s - j - 1, each live or zero by its stream's span; x_0<s> = x[..., s],
    x_j<s> = layer j - 1's result of this hop.  -> [B, C, F, hops]: hop s holds frame s - n of the output."""
    n = len(layers)
    zero = torch.zeros_like(x[..., 0])
    at = lambda t, s: t[..., s] if 0 <= s < hops else zero  # noqa: E731
    prev_x = [zero] * n
    out = []
    for s in range(hops):
        xj = x[..., s]
        for j, lay in enumerate(layers):
            cur = select(torch.cat([xj, at(skips[j], s - j)], dim=1), live(span, s - j))
            prev = select(torch.cat([prev_x[j], at(skips[j], s - j - 1)], dim=1), live(span, s - j - 1))
            prev_x[j] = xj
            xj = UD._frame(lay, cur, prev)
        out.append(xj)
    return torch.stack(out, dim=-1)


# ---- ps_gated_tcn_step_slots_f32 ----------------------------------------------------------------------------------------
def block_step_slots(y, t0, blk, ring, span, emb=None):
    """gated_tcn_step_ref.block_step with "frame g exists" = live in its stream: y [k, H, B], ring [R, H, B] -> g [k, H, B]."""
    k, h, b = y.shape
    p, d, r = blk["P"], blk["dilation"], ring.shape[0]
    assert r >= (p - 1) * d + k
    taps = None if emb is None else G.emb_taps(blk, emb)
    out = torch.empty_like(y)
    for f in range(k):
        left = torch.zeros(h, b, dtype=y.dtype)
        right = torch.zeros(h, b, dtype=y.dtype)
        for j in range(p):
            fs = f - (p - 1 - j) * d
            g = t0 + fs
            keep = live(span, g)
            if g < 0 or not bool(keep.any()):
                continue
            v = torch.where(keep[None, :], y[fs] if fs >= 0 else ring[g % r], torch.zeros(h, b, dtype=y.dtype))
            left += blk["wl"][:, :, j] @ v
            right += blk["wr"][:, :h, j] @ v
            if taps is not None:
                right += torch.where(keep[None, :], taps[j], torch.zeros(h, b, dtype=y.dtype))
        out[f] = G.gate(left, right, blk)
    for f in range(k):
        ring[(t0 + f) % r] = y[f]
    return out


def align(y, span):
    """y [T, H, B] in session frames -> [T, H, B] with stream b's live frames moved to 0 .. T_b - 1 and zeros after them: the
    stream on its own, as an entry without a span (or an offline call) takes it."""
    t = y.shape[0]
    out = torch.zeros_like(y)
    for b in range(y.shape[2]):
        lo, hi = max(int(span[b, 0]), 0), min(int(span[b, 1]), t)
        if hi > lo:
            out[:hi - lo, :, b] = y[lo:hi, :, b]
    return out


# ---- ps_istft_step_slots_f32 --------------------------------------------------------------------------------------------
def constrain(v, out_mode):
    return {"linear": lambda u: u.clamp(-1, 1), "sigmoid": torch.sigmoid, "none": lambda u: u}[out_mode](v)


def window_sum(window, hop, u_b, t_b, emit, flush):
    """S of the `emit` samples from u_b * hop on: the frames 0 <= u <= min(g / hop, u_last) covering each, u_last = u_b (step)
    or u_b - 1 (flush), capped at t_b - 1; none for u_b < 0."""
    n_fft = window.shape[0]
    s = torch.zeros(emit, dtype=window.dtype)
    if u_b < 0:
        return s
    u_last = min(u_b - 1 if flush else u_b, t_b - 1)
    for j in range(emit):
        g = u_b * hop + j
        for u in range(max(0, -((n_fft - 1 - g) // hop)), min(g // hop, u_last) + 1):
            s[j] += window[g - u * hop] ** 2
    return s


def istft_slots(frames, window, span, shift, hop, out_mode):
    """frames [hops, B, n_fft] (dead frames anything) -> (out [B, hops * hop], tails [hops + 1, B, n_fft - hop]: the tail before
    every hop and after the last)."""
    hops, b, n_fft = frames.shape
    keep = n_fft - hop
    tail = torch.zeros(b, keep, dtype=frames.dtype)
    out, tails = torch.zeros(b, hops * hop, dtype=frames.dtype), [tail.clone()]
    for t in range(hops):
        for i in range(b):
            u_b, t_b = t - shift - int(span[i, 0]), int(span[i, 1]) - int(span[i, 0])
            acc = torch.cat([tail[i], torch.zeros(hop, dtype=frames.dtype)])
            if 0 <= u_b < t_b:
                acc = acc + frames[t, i] * window / n_fft
            s = window_sum(window, hop, u_b, t_b, hop, False)
            head = acc[:hop]
            out[i, t * hop:(t + 1) * hop] = constrain(torch.where(s > 1e-10, head / s.clamp_min(1e-30), head), out_mode)
            tail[i] = acc[hop:]
        tails.append(tail.clone())
    return out, torch.stack(tails)


def istft_flush_slots(tail_row, window, span_row, t, shift, hop, out_mode):
    """The flush of one stream's tail [n_fft - hop] at session frame t."""
    u_b, t_b = t - shift - int(span_row[0]), int(span_row[1]) - int(span_row[0])
    s = window_sum(window, hop, u_b, t_b, tail_row.shape[0], True)
    return constrain(torch.where(s > 1e-10, tail_row / s.clamp_min(1e-30), tail_row), out_mode)


def ola_alone(frames, window, hop, out_mode):
    """ConvSTFT.inverse of one stream on its own: frames [T, n_fft] -> [(T - 1) * hop + n_fft]."""
    t, n_fft = frames.shape
    y = torch.zeros((t - 1) * hop + n_fft, dtype=frames.dtype)
    s = torch.zeros_like(y)
    for u in range(t):
        y[u * hop:u * hop + n_fft] += frames[u] * window / n_fft
        s[u * hop:u * hop + n_fft] += window ** 2
    return constrain(torch.where(s > 1e-10, y / s.clamp_min(1e-30), y), out_mode)
