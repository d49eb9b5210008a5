"""Plain float64 references for the direct C-ABI kernel tests (test_abi_kernels_gpu.py).  Everything here is torch / numpy on
the CPU and uses no project code; test_abi_references.py checks each of them against an independent formulation, so the
reference side is proven on a machine without a GPU."""
import numpy as np
import torch

ACT_KINDS = ("none", "relu", "prelu", "mish", "sigmoid", "tanh")


def rand(shape, seed, lo=-1.0, hi=1.0):
    g = np.random.Generator(np.random.Philox(key=seed))
    return torch.tensor(g.uniform(lo, hi, shape), dtype=torch.float32)


def activation(x: torch.Tensor, kind: str, slope: float = 0.0) -> torch.Tensor:
    """lobe/activation.py in float64; mish = x tanh(softplus(x)) with the overflow-free softplus."""
    x = x.double()
    if kind == "relu":
        return x.clamp(min=0)
    if kind == "prelu":
        return torch.where(x >= 0, x, slope * x)
    if kind == "mish":
        return x * torch.tanh(x.clamp(min=0) + torch.log1p(torch.exp(-x.abs())))
    if kind == "sigmoid":
        return torch.sigmoid(x)
    if kind == "tanh":
        return torch.tanh(x)
    assert kind == "none", kind
    return x


# ---- GRU / Elman cells ---------------------------------------------------------------------------------------------------
def rnn_fold(mod: torch.nn.Module):
    """nn.GRU / nn.RNN (one layer, float64) -> (w_ih [D*G, C], bias [D*G], whh_t [D, H, G], bhn [D, H] | None): what
    ps_rnn_f32 takes.  b_ih + b_hh go into the projection's bias, except the GRU's n gate: its b_hn stays inside the reset
    product (n = tanh(W_in x + b_in + r (W_hn h + b_hn))) and travels on its own as bhn."""
    gru = isinstance(mod, torch.nn.GRU)
    hid = mod.hidden_size
    w_ih, bias, whh_t, bhn = [], [], [], []
    for sfx in ("", "_reverse")[: 2 if mod.bidirectional else 1]:
        b_ih = getattr(mod, "bias_ih_l0" + sfx).detach().double()
        b_hh = getattr(mod, "bias_hh_l0" + sfx).detach().double()
        b = b_ih + b_hh
        if gru:
            b = torch.cat([b[: 2 * hid], b_ih[2 * hid:]])
            bhn.append(b_hh[2 * hid:].clone())
        w_ih.append(getattr(mod, "weight_ih_l0" + sfx).detach().double())
        bias.append(b)
        whh_t.append(getattr(mod, "weight_hh_l0" + sfx).detach().double().t().contiguous())
    return torch.cat(w_ih), torch.cat(bias), torch.stack(whh_t), (torch.stack(bhn) if gru else None)


def rnn_from_gx(gx: torch.Tensor, whh_t: torch.Tensor, bhn, h0=None):
    """The recurrence ps_rnn_f32 documents, step by step: gx [B, steps, D*G], whh_t [D, H, G], bhn [D, H] (GRU) or None
    (tanh RNN), h0 [D, B, H] -> (out [B, steps, D*H], h_last [D, B, H]).  Direction 1 walks the steps backwards."""
    d, hid, g = whh_t.shape
    b, steps, _ = gx.shape
    out = torch.zeros(b, steps, d * hid, dtype=torch.float64)
    last = []
    for di in range(d):
        h = torch.zeros(b, hid, dtype=torch.float64) if h0 is None else h0[di].double()
        for s in (range(steps) if di == 0 else reversed(range(steps))):
            pre = gx[:, s, di * g:(di + 1) * g].double()
            rec = h @ whh_t[di]
            if bhn is None:
                h = torch.tanh(pre + rec)
            else:
                r = torch.sigmoid(pre[:, :hid] + rec[:, :hid])
                z = torch.sigmoid(pre[:, hid:2 * hid] + rec[:, hid:2 * hid])
                n = torch.tanh(pre[:, 2 * hid:] + r * (rec[:, 2 * hid:] + bhn[di]))
                h = (1 - z) * n + z * h
            out[:, s, di * hid:(di + 1) * hid] = h
        last.append(h)
    return out, torch.stack(last)


# ---- 2-D convolutions on [N, C, F, T] maps -------------------------------------------------------------------------------
def conv2d_out_rows(f_in: int, kf: int, sf: int, df: int, pf: int, transposed: bool) -> int:
    """Frequency rows of the output: nn.Conv2d behind ZeroPad2d(pf), or nn.ConvTranspose2d(padding=pf, output_padding =
    sf - kf + 2 pf) as the U-Net decoder builds it."""
    if not transposed:
        return (f_in + 2 * pf - df * (kf - 1) - 1) // sf + 1
    return (f_in - 1) * sf - 2 * pf + df * (kf - 1) + (sf - kf + 2 * pf) + 1


def conv2d_taps(x, w2, bias, t, f_out, kf, kt, sf, df, dt, pf, pt, transposed):
    """y[n][m][fo][t'] = bias[m] + sum_k w2[m][k] tap_k, k = (ci kf + jf) kt + jt, by the tap definition of ps_unfold2d_f32:
    conv: fi = fo sf + jf df - pf, ti = t' + jt dt - pt; transposed: fi = (fo + pf - jf df) / sf when divisible,
    ti = t' + pt - jt dt; zero outside the input.  x [N, C, F, T_in] -> [N, M, f_out, t], float64."""
    x, w2 = x.double(), w2.double()
    n, c, f_in, t_in = x.shape
    m = w2.shape[0]
    w4 = w2.reshape(m, c, kf, kt)
    y = torch.zeros(n, m, f_out, t, dtype=torch.float64)
    fo, tt = torch.arange(f_out), torch.arange(t)
    for jf in range(kf):
        if not transposed:
            fi, okf = fo * sf + jf * df - pf, torch.ones(f_out, dtype=torch.bool)
        else:
            num = fo + pf - jf * df
            okf = (num >= 0) & (num % sf == 0)
            fi = torch.div(num, sf, rounding_mode="floor")
        okf = okf & (fi >= 0) & (fi < f_in)
        for jt in range(kt):
            ti = tt + jt * dt - pt if not transposed else tt + pt - jt * dt
            okt = (ti >= 0) & (ti < t_in)
            tap = x[:, :, fi.clamp(0, f_in - 1)][:, :, :, ti.clamp(0, t_in - 1)]
            tap = tap * (okf.reshape(-1, 1) & okt.reshape(1, -1))
            y += torch.einsum("mc,ncft->nmft", w4[:, :, jf, jt], tap)
    if bias is not None:
        y += bias.double().reshape(1, -1, 1, 1)
    return y


# ---- gLN over [CH, F, T] and the pad-column correction -------------------------------------------------------------------
def gln_act(y, gamma, beta, eps, kind, slope=0.0):
    """GlobLN on a 4-D map (per-utterance mean / biased variance over [CH, F, T], per-channel gain and bias) + activation."""
    y = y.double()
    mean = y.mean(dim=(1, 2, 3), keepdim=True)
    var = ((y - mean) ** 2).mean(dim=(1, 2, 3), keepdim=True)
    g, b = gamma.double().reshape(1, -1, 1, 1), beta.double().reshape(1, -1, 1, 1)
    return activation(g * (y - mean) / torch.sqrt(var + eps) + b, kind, slope)


def pad_column_correction(bias, f_out: int, ld: int, t: int):
    """What the pad columns of a GEMM over f_out * ld flattened frames add to its (sum, sum of squares): the taps are zero
    there, so every such output is its channel's bias."""
    pad = float(f_out * (ld - t))
    return float(bias.double().sum()) * pad, float((bias.double() ** 2).sum()) * pad


# ---- attentive statistics pooling with relative lengths ------------------------------------------------------------------
def valid_frames(lengths, t: int):
    """frame i of utterance n takes part iff float32(i) < float32(lengths[n]) * float32(t) -> counts [N] (a prefix)."""
    lim = lengths.to(torch.float32) * torch.tensor(float(t), dtype=torch.float32)
    return (torch.arange(t, dtype=torch.float32).reshape(1, -1) < lim.reshape(-1, 1)).sum(1)


def attn_pool(logits, x, lengths, eps):
    """-> (weights [N, C, T] (0 on masked frames), pooled [N, 2C] = cat(mean, std)), float64, row by row."""
    n, c, t = logits.shape
    cnt = valid_frames(lengths, t) if lengths is not None else torch.full((n,), t)
    w = torch.zeros(n, c, t, dtype=torch.float64)
    out = torch.zeros(n, 2 * c, dtype=torch.float64)
    for i in range(n):
        k = int(cnt[i])
        a = torch.softmax(logits[i, :, :k].double(), 1)
        w[i, :, :k] = a
        xv = x[i, :, :k].double()
        mean = (a * xv).sum(1)
        out[i, :c] = mean
        out[i, c:] = torch.sqrt(((a * (xv - mean.unsqueeze(1)) ** 2).sum(1)).clamp(min=eps))
    return w, out


# ---- streaming harness ---------------------------------------------------------------------------------------------------
def stream_windows(queue, chunk, hop: int):
    """queue [B, win] (the previous window), chunk [B, hops * hop] -> wins [hops, B, win]: the window slid by hop over
    queue[:, hop:] ++ chunk."""
    b, win = queue.shape
    sig = np.concatenate([queue[:, hop:], chunk], 1)
    hops = chunk.shape[1] // hop
    return np.stack([sig[:, i * hop:i * hop + win] for i in range(hops)], 0)


def stream_overlap(frames, tail, hop: int):
    """frames [hops, B, 2 hop], tail [B, hop] -> (blocks [B, hops * hop], new tail): block i = (previous frame's second
    half (the tail for i = 0) + frame i's first half) / 2."""
    blocks, prev = [], tail
    for f in frames:
        blocks.append((prev + f[:, :hop]) * 0.5)
        prev = f[:, hop:]
    return np.concatenate(blocks, 1), prev
