"""A pure-torch fp64 reference of what ps_gated_tcn_step_f32 computes (the middle of one causal GatedTCN block with eval
BatchNorm1d: conv_tasnet.py:129-215), written the way the kernel is specified: explicit loops over the frames of a chunk, a
frame counter, a circular ring of earlier frames.  `offline` is the same block on whole sequences through F.conv1d with
left padding, the embedding concatenated to the right convolution's input and zero-padded with it, as the model does it."""
import torch
import torch.nn.functional as F


def make_block(h, e, p, dilation, seed=0, dtype=torch.float64):
    """Random weights of one block: Wl [H, H, P], Wr [H, H + E, P], per side the folded norm (scale, shift) and a slope."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1  # noqa: E731
    blk = dict(H=h, E=e, P=p, dilation=dilation, wl=r(h, h, p) / (h * p) ** 0.5, wr=r(h, h + e, p) / ((h + e) * p) ** 0.5)
    for side, slope in (("l", 0.25), ("r", 0.1)):
        blk["sc_" + side], blk["sh_" + side] = r(h) * 0.5 + 1.5, r(h) * 0.3
        blk["slope_" + side] = torch.tensor([slope], dtype=torch.float64)
    return {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in blk.items()}


def _act(v, sc, sh, slope):
    z = v * sc + sh
    return torch.where(z >= 0, z, slope * z)


def gate(left, right, blk):
    """[..., H, B] sums of the two convolutions -> PReLU(aff_l(L)) * sigmoid(PReLU(aff_r(Rt)))."""
    lv = _act(left, blk["sc_l"][:, None], blk["sh_l"][:, None], blk["slope_l"])
    rv = _act(right, blk["sc_r"][:, None], blk["sh_r"][:, None], blk["slope_r"])
    return lv * torch.sigmoid(rv)


def offline(y, blk, emb=None):
    """y [B, H, T] (the output of in_conv), emb [B, E] -> g [B, H, T]."""
    pad = (blk["P"] - 1) * blk["dilation"]
    left = F.conv1d(F.pad(y, (pad, 0)), blk["wl"], dilation=blk["dilation"])
    yr = y if emb is None else torch.cat([y, emb[:, :, None].expand(-1, -1, y.shape[2])], dim=1)
    right = F.conv1d(F.pad(yr, (pad, 0)), blk["wr"], dilation=blk["dilation"])
    return gate(left.permute(2, 1, 0), right.permute(2, 1, 0), blk).permute(2, 1, 0)


def emb_taps(blk, emb):
    """[P, H, B]: what tap j of the right convolution adds for the embedding of stream b."""
    h = blk["H"]
    return torch.einsum("hej,be->jhb", blk["wr"][:, h:, :], emb)


def block_step(y, t0, blk, ring, emb=None):
    """y [k, H, B]: frames t0 .. t0 + k - 1 of every stream; ring [R, H, B]: slot g % R = frame g -> g [k, H, B].  Frames of
    the chunk come from y, earlier frames >= 0 from the ring, frames < 0 are zeros (and add no embedding term); every frame of
    the chunk is stored to its slot afterwards."""
    k, h, b = y.shape
    p, d, r = blk["P"], blk["dilation"], ring.shape[0]
    assert r >= (p - 1) * d + k
    taps = None if emb is None else emb_taps(blk, emb)
    out = torch.empty_like(y)
    for f in range(k):
        left = torch.zeros(h, b, dtype=y.dtype)
        right = torch.zeros(h, b, dtype=y.dtype)
        for j in range(p):
            fs = f - (p - 1 - j) * d
            g = t0 + fs
            if g < 0:
                continue
            v = y[fs] if fs >= 0 else ring[g % r]
            left += blk["wl"][:, :, j] @ v
            right += blk["wr"][:, :h, j] @ v
            if taps is not None:
                right += taps[j]
        out[f] = gate(left, right, blk)
    for f in range(k):
        ring[(t0 + f) % r] = y[f]
    return out
