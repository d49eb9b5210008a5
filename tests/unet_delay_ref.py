"""A pure-torch reference of the hop schedule StreamingUnetTcn runs its up path by (puresound_amd/streaming/unet_tcn.py):
n transposed convolutions of two frames in time whose FIRST output frame is trimmed (transpose_delay=True, unet.py:514-528),
each followed by an eval BatchNorm2d and a PReLU, each reading cat(x, skip).  `offline` is F.conv_transpose2d on whole
sequences; `stream` walks the hops with rings and then the n flush hops."""
import torch
import torch.nn.functional as F


def make_decoder(n, ch, seed=0, dtype=torch.float64):
    """n layers: ConvTranspose2d(2 * ch -> ch, (3, 2), padding (1, 0)) + folded norm (scale, shift) + a PReLU slope."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1).to(dtype)  # noqa: E731
    return [dict(w=r(2 * ch, ch, 3, 2) / (12 * ch) ** 0.5, b=r(ch) * 0.1, sc=r(ch) * 0.5 + 1.5, sh=r(ch) * 0.2, slope=0.2 + 0.05 * j)
            for j in range(n)]


def _post(y, lay):
    z = y * lay["sc"][None, :, None, None] + lay["sh"][None, :, None, None]
    return torch.where(z >= 0, z, lay["slope"] * z)


def offline(x, skips, layers):
    """x [B, C, F, T], skips[j] [B, C, F, T] for layer j -> [B, C, F, T]."""
    for lay, s in zip(layers, skips):
        y = F.conv_transpose2d(torch.cat([x, s], dim=1), lay["w"], lay["b"], padding=(1, 0))   # T + 1 frames
        x = _post(y[..., 1:], lay)                                                               # the first one trimmed
    return x


def _frame(lay, cur, prev):
    """One output frame of a layer: act(bias + W0 . cur + W1 . prev), [B, 2C, F] each."""
    w = lay["w"]
    y = (F.conv_transpose2d(cur[..., None], w[..., 0:1], lay["b"], padding=(1, 0))
         + F.conv_transpose2d(prev[..., None], w[..., 1:2], None, padding=(1, 0)))
    return _post(y, lay)[..., 0]


def stream(x, skips, layers):
    """The same through the hop schedule: hop s feeds frame s of x and of every skip; layer j computes frame s - j - 1 of
    its output from in<s> and in<s-1>, in = cat(x_j<s>, skip_j<s>), skip_j<s> = frame s - j of its skip (a ring of j + 1
    frames).  The first n hops emit nothing; n flush hops follow the last input: at flush hop i the layers j < i are
    skipped, layer i reads an all-zero current input.  -> [B, C, F, T]."""
    n, t = len(layers), x.shape[-1]
    zero = torch.zeros_like(x[..., 0])
    rings = [[zero] * (j + 1) for j in range(n)]     # skip ring of layer j: [-1] = frame s - 1, [-(j+1)] = frame s - j - 1
    prev_x = [zero] * n                              # x_j<s-1>
    out = []
    for s in range(t + n):
        flush = s - t                                # >= 0: flush hop i = s - t
        now_x = [None] * n
        result = None
        for j, lay in enumerate(layers):
            if flush >= 0 and j < flush:
                continue
            xj = (x[..., s] if s < t else None) if j == 0 else result
            skip_hist = rings[j] + [skips[j][..., s] if s < t else zero]     # [..., frame s-1, frame s]
            sk_cur, sk_prev = skip_hist[-1 - j], skip_hist[-2 - j]
            if flush >= 0 and j == flush:
                cur = torch.zeros_like(torch.cat([zero, zero], dim=1))
            else:
                cur = torch.cat([xj, sk_cur], dim=1)
            now_x[j] = xj if xj is not None else zero
            result = _frame(lay, cur, torch.cat([prev_x[j], sk_prev], dim=1))
        for j in range(n):
            rings[j] = (rings[j] + [skips[j][..., s] if s < t else zero])[-(j + 1):]
            if now_x[j] is not None:
                prev_x[j] = now_x[j]
        if s >= n:
            out.append(result)
    return torch.stack(out, dim=-1)
