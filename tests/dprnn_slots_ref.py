"""A pure-torch reference of one causal DPRNN block advanced frame by frame in a slot session (what
ps_dprnn_block_step_slots_f32 computes), written with explicit loops over frames and columns on dprnn_step_ref._pass: a column
is live at frame g iff birth <= g < death, a live column sits at position (g - birth) % K of its own segment (the intra reset
and the bank slot follow that position), and a dead column reads nothing and changes nothing.
tests/test_streaming_dprnn_slots.py checks it against dprnn_step_ref.block_step; the GPU kernel test leans on it."""
import torch

from dprnn_step_ref import _pass


def block_step_slots(x, t0, seg, intra, inter, state, spans):
    """x [k, B, C] float64: frames t0 .. t0 + k - 1 of B columns (a dead frame may hold anything) -> out [k, B, C], NaN at
    dead frames.  state: dict(h_intra, c_intra [B, H], h_bank, c_bank [K, B, H]) float64, advanced in place for live frames
    only.  spans: per column (birth, death), absolute frame indices.  Returns (out, per column the set of bank slots
    visited)."""
    out = torch.full_like(x, float("nan"))
    visited = [set() for _ in spans]
    for f in range(x.shape[0]):
        g = t0 + f
        for b, (birth, death) in enumerate(spans):
            if not birth <= g < death:
                continue
            p = (g - birth) % seg
            col = slice(b, b + 1)
            h, c = state["h_intra"][col], state["c_intra"][col]
            if p == 0:                                       # the intra LSTM starts every segment of this column from zero
                h, c = torch.zeros_like(h), torch.zeros_like(c)
            y, h, c = _pass(intra, x[f, col], h, c)
            state["h_intra"][col] = h
            state["c_intra"][col] = c
            o, h, c = _pass(inter, y, state["h_bank"][p, col], state["c_bank"][p, col])   # position p continues position p
            state["h_bank"][p, col] = h
            state["c_bank"][p, col] = c
            out[f, col] = o
            visited[b].add(p)
    return out, visited
