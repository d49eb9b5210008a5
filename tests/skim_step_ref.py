"""A pure-torch reference of one causal SkiM block advanced frame by frame (what ps_skim_block_step_f32 computes), written
with explicit loops: a frame counter, the segment start from zero or from a hand-over bank slot, FiLM on one frame, the
SegLSTM step, and at the last frame of a segment one MemLSTM step whose result goes to the next block's bank.  Also a chain
of such blocks.  tests/test_streaming_skim.py checks it against the reference project's own outputs and against torch's
modules on whole segments; the GPU kernel test leans on it."""
import torch
import torch.nn as nn

from dprnn_step_ref import make_pass


def slots_needed(k, seg):
    """Bank slots that always suffice for launches of up to k frames with segments of `seg` frames."""
    return (k - 1) // seg + 3


FILM_AMP = 0.4
#: the largest fan-in [x; h] at which make_pass's +-0.4 is tested on the DPRNN kernel (C, H) = (128, 64)
FAN_IN = 192


def _tamed(mods):
    """make_pass's modules with the LSTM's matrices scaled by sqrt(FAN_IN / fan-in) where the fan-in is larger: the gate
    pre-activations keep the spread they have at the DPRNN test's largest shape and do not saturate every gate."""
    lstm = mods[0]
    fan = lstm.input_size + lstm.hidden_size
    if fan > FAN_IN:
        with torch.no_grad():
            lstm.weight_ih_l0.mul_((FAN_IN / fan) ** 0.5)
            lstm.weight_hh_l0.mul_((FAN_IN / fan) ** 0.5)
    return mods


def make_block(c, h, seed, film=True, mem=True, dtype=torch.float32):
    """One block with every parameter random, scaled as dprnn_step_ref.make_pass scales them: dict(film = (Ws, Wb [C, C], the
    feature columns of cond_scale / cond_bias, nn.LayerNorm(C)) or None, seg = (nn.LSTM(c, h), nn.Linear(h, c),
    nn.LayerNorm(c)), mem = dict(h = (nn.LSTM(h, h), nn.Linear(h, h), nn.LayerNorm(h)), c = the same) or None)."""
    g = torch.Generator().manual_seed(seed)
    blk = dict(film=None, seg=_tamed(make_pass(c, h, seed * 7 + 1, dtype)), mem=None)
    if film:
        norm = nn.LayerNorm(c)
        with torch.no_grad():
            for p in norm.parameters():
                p.copy_(torch.rand(p.shape, generator=g) * 0.8 - 0.4)
            norm.weight.add_(1.0)
        amp = FILM_AMP / c ** 0.5
        blk["film"] = (((torch.rand(c, c, generator=g) * 2 - 1) * amp).to(dtype), ((torch.rand(c, c, generator=g) * 2 - 1) * amp).to(dtype),
                       norm.to(dtype).eval())
    if mem:
        blk["mem"] = dict(h=_tamed(make_pass(h, h, seed * 7 + 2, dtype)), c=_tamed(make_pass(h, h, seed * 7 + 3, dtype)))
    return blk


def block_of(masker, i):
    """Block i of a SkiM module (the reference's or this project's) in make_block's form; a block without fusion has
    film = None."""
    film = None
    if masker.embed_dim > 0 and masker.block_with_embed[i]:
        f = masker.seg_input_fusion[i]
        c = masker.input_size
        film = (f.cond_scale.weight.detach()[:, :c, 0], f.cond_bias.weight.detach()[:, :c, 0], f.norm)
    s = masker.seg_lstm[i]
    mem = None
    if i < masker.n_blocks - 1:
        m = masker.mem_lstm[i]
        mem = dict(h=(m.h_net, m.h_proj, m.h_norm), c=(m.c_net, m.c_proj, m.c_norm))
    return dict(film=film, seg=(s.lstm, s.proj, s.norm), mem=mem)


def embed_terms(masker, i, embed):
    """(rs, rb) [B, C] float64: what the embedding [B, E] adds to FiLM's scale and bias in block i (None, None without
    fusion); the masker's own L2 normalisation applied first."""
    if not (masker.embed_dim > 0 and masker.block_with_embed[i]):
        return None, None
    e = embed.detach().double()
    if masker.embed_norm:
        e = torch.nn.functional.normalize(e, dim=1)
    f = masker.seg_input_fusion[i]
    c = masker.input_size
    return e @ f.cond_scale.weight.detach().double()[:, c:, 0].t(), e @ f.cond_bias.weight.detach().double()[:, c:, 0].t()


def _w(t, like):
    """A parameter in the precision of the loop: that of its input (float64 for the reference; float32 to measure what
    plain fp32 arithmetic costs against it)."""
    return t.detach().to(like.dtype)


def _ln(v, norm):
    mean = v.mean(dim=1, keepdim=True)
    var = ((v - mean) ** 2).mean(dim=1, keepdim=True)        # biased, as nn.LayerNorm
    return (v - mean) / torch.sqrt(var + norm.eps) * _w(norm.weight, v) + _w(norm.bias, v)


def _cell(lstm, x, h, c):
    hid = h.shape[1]
    gates = x @ _w(lstm.weight_ih_l0, x).t() + _w(lstm.bias_ih_l0, x) + h @ _w(lstm.weight_hh_l0, x).t() + _w(lstm.bias_hh_l0, x)
    i, f, g, o = (gates[:, j * hid:(j + 1) * hid] for j in range(4))
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


def block_step(x, t0, seg, blk, state, rs=None, rb=None, bank_in=None, bank_out=None):
    """x [k, B, C] float64: frames t0 .. t0 + k - 1 of B streams -> out [k, B, C].  state: dict(seg_h, seg_c [B, H], and with a
    MemLSTM mh_h, mc_h, mh_c, mc_c [B, H]) float64, advanced in place.  (All of them float32: the same loop in fp32.)  bank_in = (init_h, init_c) [NS, B, H] or None (block
    0); bank_out the next block's, written at the end of a segment.  rs / rb [B, C] with FiLM.  Returns (out, the slots of
    bank_in read, the slots of bank_out written)."""
    out = torch.empty_like(x)
    read, written = set(), set()
    for f in range(x.shape[0]):
        g = t0 + f
        p, s = g % seg, g // seg
        if p == 0:
            if bank_in is None:
                h, c = torch.zeros_like(state["seg_h"]), torch.zeros_like(state["seg_c"])
            else:
                slot = s % bank_in[0].shape[0]
                h, c = bank_in[0][slot].clone(), bank_in[1][slot].clone()
                read.add(slot)
        else:
            h, c = state["seg_h"], state["seg_c"]
        v = x[f]
        if blk["film"] is not None:
            ws, wb, norm = blk["film"]
            u = _ln(v, norm)
            v = (u @ _w(ws, u).t() + rs) * u + (u @ _w(wb, u).t() + rb)
        lstm, proj, norm = blk["seg"]
        h, c = _cell(lstm, v, h, c)
        state["seg_h"].copy_(h)
        state["seg_c"].copy_(c)
        out[f] = v + _ln(h @ _w(proj.weight, h).t() + _w(proj.bias, h), norm)
        if p == seg - 1 and blk["mem"] is not None:
            slot = (s + 1) % bank_out[0].shape[0]
            for key, val, dst in (("h", h, bank_out[0]), ("c", c, bank_out[1])):
                lstm, proj, norm = blk["mem"][key]
                zh, zc = _cell(lstm, val, state["mh_" + key], state["mc_" + key])
                state["mh_" + key].copy_(zh)
                state["mc_" + key].copy_(zc)
                dst[slot] = val + _ln(zh @ _w(proj.weight, zh).t() + _w(proj.bias, zh), norm)
            written.add(slot)
    return out, read, written


def new_state(b, h, mem, fill=0.0):
    keys = ("seg_h", "seg_c") + (("mh_h", "mc_h", "mh_c", "mc_c") if mem else ())
    return {k: torch.full((b, h), fill, dtype=torch.float64) for k in keys}


class Chain:
    """The blocks of a masker (block_of each) as a session of B streams from frame 0: step(x [k, B, C]) -> [k, B, C]."""

    def __init__(self, blocks, seg, b, h, ns, terms=None):
        self.blocks, self.seg, self.t = blocks, seg, 0
        self.terms = terms or [(None, None)] * len(blocks)
        self.states = [new_state(b, h, blk["mem"] is not None) for blk in blocks]
        self.banks = [None] + [(torch.zeros(ns, b, h, dtype=torch.float64), torch.zeros(ns, b, h, dtype=torch.float64))
                               for _ in blocks[1:]]

    def step(self, x):
        for i, blk in enumerate(self.blocks):
            nxt = self.banks[i + 1] if i + 1 < len(self.blocks) else None
            x, _, _ = block_step(x, self.t, self.seg, blk, self.states[i], *self.terms[i], self.banks[i], nxt)
        self.t += x.shape[0]
        return x


def output_fc(masker, x):
    """x [T, B, C] float64 -> the masker's output_fc (PReLU, 1x1 convolution) [B, C_out, T]."""
    prelu, conv = masker.output_fc
    x = torch.where(x >= 0, x, _w(prelu.weight, x) * x)
    return (x @ _w(conv.weight, x)[:, :, 0].t() + _w(conv.bias, x)).permute(1, 2, 0)


# -------------------------------------------------------------------------------------------------------------------------
# the inputs of the kernel test (tests/test_streaming_skim_gpu.py), shared with the CPU test that measures what the same
# loop costs in plain fp32
# -------------------------------------------------------------------------------------------------------------------------
SHAPES = [(16, 8, 5), (5, 20, 10), (128, 64, 150), (128, 256, 150)]
STREAMS, HOPS, STARTS = (1, 3, 70), (1, 7, 16), ("0", "K-1", "3K+2")
#: variant -> (FiLM, incoming banks, MemLSTM and outgoing banks)
VARIANTS = {"first": (True, False, True), "middle": (True, True, True), "last": (True, True, False),
            "plain": (False, True, True)}


def kernel_cases():
    """The pruned cross product: per shape the nine (B, hops, start) of a Latin square -- every value of every axis, and with
    K = 5 the 16-hop launches that cross three segment ends -- with all four variants at the full-size shape and one
    variant, in turn, at the others."""
    out = []
    names = list(VARIANTS)
    for si, (c, h, k) in enumerate(SHAPES):
        for i, b in enumerate(STREAMS):
            for j, hops in enumerate(HOPS):
                start = STARTS[(i + j + si) % 3]
                for v in (names if (c, h) == (128, 256) else [names[(3 * i + j + si) % 4]]):
                    out.append((c, h, k, b, hops, start, v))
    return out


_BLOCKS = {}


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1


def kernel_case(c, h, k, b, hops, start, variant):
    """-> dict(blk, t0, ns, x [hops, B, C], state, rs, rb [B, C] or None, bank_in, bank_out ([NS, B, H] pairs or None)), all
    float64 and random: a missed reset or a wrong slot shows."""
    film, incoming, mem = VARIANTS[variant]
    key = (c, h, film, mem)
    if key not in _BLOCKS:
        _BLOCKS[key] = make_block(c, h, 17 * c + h, film, mem)
    t0 = {"0": 0, "K-1": k - 1, "3K+2": 3 * k + 2}[start]
    seed = 100000 * c + 1000 * b + 10 * hops + t0 + 7 * list(VARIANTS).index(variant)
    ns = slots_needed(16, k)
    state = new_state(b, h, mem)
    for n, name in enumerate(sorted(state)):
        state[name] = _rand((b, h), seed + 1 + n)
    pair = lambda s: (_rand((ns, b, h), s), _rand((ns, b, h), s + 1))  # noqa: E731
    return dict(blk=_BLOCKS[key], t0=t0, ns=ns, seg=k, x=_rand((hops, b, c), seed), state=state,
                rs=_rand((b, c), seed + 11) if film else None, rb=_rand((b, c), seed + 12) if film else None,
                bank_in=pair(seed + 13) if incoming else None, bank_out=pair(seed + 15) if mem else None)


def run_case(case, dtype=torch.float64):
    """The loop on a copy of the case in `dtype` -> dict(out, read, written, state, bank_out)."""
    to = lambda t: None if t is None else t.to(dtype).clone()  # noqa: E731
    state = {name: to(t) for name, t in case["state"].items()}
    bank_in = None if case["bank_in"] is None else tuple(to(t) for t in case["bank_in"])
    bank_out = None if case["bank_out"] is None else tuple(to(t) for t in case["bank_out"])
    out, read, written = block_step(to(case["x"]), case["t0"], case["seg"], case["blk"], state, to(case["rs"]), to(case["rb"]),
                                    bank_in, bank_out)
    return dict(out=out, read=read, written=written, state=state, bank_out=bank_out)
