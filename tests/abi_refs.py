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


# ---- short-row GEMM kernels (conv1x1_small.hip): 1x1 convolution, FiLM, gates + cell, projection + LayerNorm -------------
def conv1x1_ref(x, w, bias=None, bias_n=None, res=None, pro=None):
    """y[n] = W a[n] + bias (+ bias_n[n]) (+ res[n]), a = the prologue of x [N, K, T] in the kernel's order (small_transform):
    ReLU-before -> norm -> PReLU -> tanh-after.  pro: dict of `pre_relu` (bool), `affine` = (gamma [K], beta [K]), `prelu` =
    slope, `post_tanh` (bool); `glob` = (gamma, beta, eps) takes the norm's place with the per-utterance mean / biased
    variance over [K, T] (the tiled kernel's global-norm prologue)."""
    pro = pro or {}
    a = x.double()
    if pro.get("pre_relu"):
        a = a.clamp(min=0)
    if pro.get("affine") is not None:
        g, b = pro["affine"]
        a = a * g.double().reshape(1, -1, 1) + b.double().reshape(1, -1, 1)
    if pro.get("glob") is not None:
        g, b, eps = pro["glob"]
        mean = a.mean(dim=(1, 2), keepdim=True)
        var = ((a - mean) ** 2).mean(dim=(1, 2), keepdim=True)
        a = (a - mean) / torch.sqrt(var + eps) * g.double().reshape(1, -1, 1) + b.double().reshape(1, -1, 1)
    if pro.get("prelu") is not None:
        a = torch.where(a >= 0, a, float(pro["prelu"]) * a)
    if pro.get("post_tanh"):
        a = torch.tanh(a)
    y = torch.matmul(w.double(), a)
    if bias is not None:
        y = y + bias.double().reshape(1, -1, 1)
    if bias_n is not None:
        y = y + bias_n.double().unsqueeze(2)
    if res is not None:
        y = y + res.double()
    return y


def film_conv_ref(x, w_scale, w_bias, res_scale=None, res_bias=None):
    """(Ws x + rs) * x + (Wb x + rb): x [N, C, T], Ws / Wb [C, C], rs / rb [N, C, T] or None."""
    x = x.double()
    scale, shift = torch.matmul(w_scale.double(), x), torch.matmul(w_bias.double(), x)
    if res_scale is not None:
        scale = scale + res_scale.double()
    if res_bias is not None:
        shift = shift + res_bias.double()
    return scale * x + shift


def gates_cell_ref(xh, w, bias, c):
    """gates = W [x; h] + b with rows gate-major (i, f, g, o, H rows each, nn.LSTM's order); c' = sig(f) c + sig(i) tanh(g),
    h' = sig(o) tanh(c').  xh [N, K, T], w [4H, K], bias [4H] or None, c [N, H, T] -> (c', h')."""
    a = torch.matmul(w.double(), xh.double())
    if bias is not None:
        a = a + bias.double().reshape(1, -1, 1)
    hid = w.shape[0] // 4
    gi, gf, gg, go = (a[:, g * hid:(g + 1) * hid] for g in range(4))
    c_new = torch.sigmoid(gf) * c.double() + torch.sigmoid(gi) * torch.tanh(gg)
    return c_new, torch.sigmoid(go) * torch.tanh(c_new)


def frame_layernorm(p, gamma, beta, eps):
    """LayerNorm of every frame of p [N, M, T] over its M channels, two-pass biased variance -> (y, variance [N, 1, T])."""
    mean = p.mean(1, keepdim=True)
    var = ((p - mean) ** 2).mean(1, keepdim=True)
    return (p - mean) / torch.sqrt(var + eps) * gamma.double().reshape(1, -1, 1) + beta.double().reshape(1, -1, 1), var


def proj_layernorm_ref(x, w, bias, gamma, beta, eps, res=None, res_inside=False, norm2=None, with_var=False):
    """y = res + LN(W x + b) or, res_inside, LN(W x + b + res); y2 = LN2(y) with norm2 = (gamma2, beta2, eps2), else None.
    with_var: also the smallest per-frame variance either norm divides by (the conditioning of the comparison)."""
    p = torch.matmul(w.double(), x.double())
    if bias is not None:
        p = p + bias.double().reshape(1, -1, 1)
    if res is not None and res_inside:
        p = p + res.double()
    y, var = frame_layernorm(p, gamma, beta, eps)
    if res is not None and not res_inside:
        y = y + res.double()
    y2, low = None, float(var.min())
    if norm2 is not None:
        y2, var2 = frame_layernorm(y, norm2[0], norm2[1], norm2[2])
        low = min(low, float(var2.min()))
    return (y, y2, low) if with_var else (y, y2)


def film_pack_weights(w_scale, w_bias):
    """[C, C] x 2 -> [2C, C] with rows (2c, 2c + 1) = (scale row c, bias row c): what ps_film_conv_f32 takes (then pack_wt)."""
    c = w_scale.shape[0]
    return torch.stack([w_scale, w_bias], 1).reshape(2 * c, -1)


def film_pack_rows(res_scale, res_bias):
    """[N, C, T] x 2 -> [N, 2C, T], rows paired like film_pack_weights."""
    n, c, t = res_scale.shape
    return torch.stack([res_scale, res_bias], 2).reshape(n, 2 * c, t)


def gate_unit_major(hid: int):
    """index [4H] taking gate-major rows (g H + u) to the unit-major order of ps_lstm_gates_cell_f32: row 4u + g."""
    return (torch.arange(4).reshape(1, 4) * hid + torch.arange(hid).reshape(hid, 1)).reshape(-1)
