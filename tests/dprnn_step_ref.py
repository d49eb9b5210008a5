"""A pure-torch reference of one causal DPRNN block advanced frame by frame (what ps_dprnn_block_step_f32 computes), written
with explicit loops: a frame counter, the intra reset at position 0 of a segment and a bank slot per position for the inter
state.  tests/test_streaming_dprnn.py checks it against nn.LSTM / nn.Linear / nn.LayerNorm on whole segments; the GPU kernel
test leans on it."""
import torch
import torch.nn as nn


def make_pass(c, h, seed, dtype=torch.float32):
    """(nn.LSTM(c, h), nn.Linear(h, c), nn.LayerNorm(c)) with every parameter random, the norm's affine part included."""
    g = torch.Generator().manual_seed(seed)
    mods = (nn.LSTM(c, h, num_layers=1, batch_first=True), nn.Linear(h, c), nn.LayerNorm(c))
    with torch.no_grad():
        for mod in mods:
            for p in mod.parameters():
                p.copy_(torch.rand(p.shape, generator=g) * 0.8 - 0.4)
        mods[2].weight.add_(1.0)
    return tuple(mod.to(dtype).eval() for mod in mods)


def _pass(mods, x, h, c):
    """One frame of one pass: x [B, C], (h, c) [B, H] -> (x + LN(P h' + b), h', c'), in float64."""
    lstm, proj, norm = mods
    f64 = lambda t: t.detach().double()  # noqa: E731
    hid = h.shape[1]
    gates = x @ f64(lstm.weight_ih_l0).t() + f64(lstm.bias_ih_l0) + h @ f64(lstm.weight_hh_l0).t() + f64(lstm.bias_hh_l0)
    i, f, g, o = (gates[:, j * hid:(j + 1) * hid] for j in range(4))
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    h = torch.sigmoid(o) * torch.tanh(c)
    v = h @ f64(proj.weight).t() + f64(proj.bias)
    mean = v.mean(dim=1, keepdim=True)
    var = ((v - mean) ** 2).mean(dim=1, keepdim=True)        # biased, as nn.LayerNorm
    return x + (v - mean) / torch.sqrt(var + norm.eps) * f64(norm.weight) + f64(norm.bias), h, c


def block_step(x, t0, seg, intra, inter, state):
    """x [k, B, C] float64: frames t0 .. t0 + k - 1 of B streams -> out [k, B, C].  state: dict(h_intra, c_intra [B, H],
    h_bank, c_bank [K, B, H]) float64, advanced in place.  Returns (out, the bank slots visited)."""
    out = torch.empty_like(x)
    visited = set()
    for f in range(x.shape[0]):
        p = (t0 + f) % seg
        if p == 0:                                           # the intra LSTM starts every segment from zero
            state["h_intra"].zero_()
            state["c_intra"].zero_()
        y, h, c = _pass(intra, x[f], state["h_intra"], state["c_intra"])
        state["h_intra"].copy_(h)
        state["c_intra"].copy_(c)
        o, h, c = _pass(inter, y, state["h_bank"][p], state["c_bank"][p])   # position p continues position p
        state["h_bank"][p] = h
        state["c_bank"][p] = c
        out[f] = o
        visited.add(p)
    return out, visited
