"""A pure-torch reference of one causal SkiM block advanced frame by frame in a slot session (what
ps_skim_block_step_slots_f32 computes), written with explicit loops over frames and columns on skim_step_ref's pieces: a
column is live at frame g iff birth <= g < death, a live column's frame n = g - birth sits at position n % K of its own
segment n // K (the segment start -- zero or a bank slot -- and the MemLSTM hand-over follow that), and a dead column reads
nothing and changes nothing.  tests/test_streaming_skim_slots.py checks it against skim_step_ref.block_step; the GPU kernel
test leans on it."""
import torch

from skim_step_ref import _cell, _ln, _w


def block_step_slots(x, t0, seg, blk, state, spans, rs=None, rb=None, bank_in=None, bank_out=None):
    """x [k, B, C] float64: frames t0 .. t0 + k - 1 of B columns (a dead frame may hold anything) -> out [k, B, C], NaN at
    dead frames.  state, rs / rb, bank_in, bank_out as skim_step_ref.block_step takes them, advanced in place for live frames
    only.  spans: per column (birth, death), absolute frame indices.  Returns (out, per column the set of bank_in slots
    read, per column the set of bank_out slots written)."""
    out = torch.full_like(x, float("nan"))
    read, written = [set() for _ in spans], [set() for _ in spans]
    for f in range(x.shape[0]):
        g = t0 + f
        for b, (birth, death) in enumerate(spans):
            if not birth <= g < death:
                continue
            n = g - birth
            p, s = n % seg, n // seg
            col = slice(b, b + 1)
            if p == 0:
                if bank_in is None:
                    h, c = torch.zeros_like(state["seg_h"][col]), torch.zeros_like(state["seg_c"][col])
                else:
                    slot = s % bank_in[0].shape[0]
                    h, c = bank_in[0][slot, col].clone(), bank_in[1][slot, col].clone()
                    read[b].add(slot)
            else:
                h, c = state["seg_h"][col], state["seg_c"][col]
            v = x[f, col]
            if blk["film"] is not None:
                ws, wb, norm = blk["film"]
                u = _ln(v, norm)
                v = (u @ _w(ws, u).t() + rs[col]) * u + (u @ _w(wb, u).t() + rb[col])
            lstm, proj, norm = blk["seg"]
            h, c = _cell(lstm, v, h, c)
            state["seg_h"][col] = h
            state["seg_c"][col] = c
            out[f, col] = v + _ln(h @ _w(proj.weight, h).t() + _w(proj.bias, h), norm)
            if p == seg - 1 and blk["mem"] is not None:
                slot = (s + 1) % bank_out[0].shape[0]
                for key, val, dst in (("h", h, bank_out[0]), ("c", c, bank_out[1])):
                    lstm, proj, norm = blk["mem"][key]
                    zh, zc = _cell(lstm, val, state["mh_" + key][col], state["mc_" + key][col])
                    state["mh_" + key][col] = zh
                    state["mc_" + key][col] = zc
                    dst[slot, col] = val + _ln(zh @ _w(proj.weight, zh).t() + _w(proj.bias, zh), norm)
                written[b].add(slot)
    return out, read, written
