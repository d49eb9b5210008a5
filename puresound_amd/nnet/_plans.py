"""Kernel-side parameter layouts ("plans") shared by the recurrent maskers.

A plan holds the packed / transposed fp32 copies of a module's parameters that the HIP kernels consume, keyed by a
fingerprint of the parameters so that load_state_dict / .to(device) / in-place edits invalidate it.  Plans hold
raw device pointers through the tensors they keep alive; they are never pickled.
"""
import contextlib
import os
from collections import namedtuple
from typing import Optional

import torch
import torch.nn as nn

from .. import hip

FUSE_PROJ_LN = os.environ.get("PS_FUSE_PROJ_LN", "1") == "1"   # 0: separate projection GEMM + LayerNorm kernels
FUSE_PROJ_LN_MAX_FRAMES = int(os.environ.get("PS_FUSE_PROJ_LN_MAX_FRAMES", "8192"))
FUSE_GEMM_LN = os.environ.get("PS_FUSE_GEMM_LN", "1") == "1"    # 0: projection GEMM and LayerNorm + skip as two launches
FMAJOR_LSTM = os.environ.get("PS_FMAJOR_LSTM", "1") == "1"      # 0: H = 128 recurrences stay on the channel-major kernels


# Arithmetic of the GEMMs a module builds (the LSTM input projections of the recurrent maskers: [4H*D x C] over every frame; the
# 1x1 convs of the TCN blocks): "fp32" = v_mfma_f32 on fp32 operands, "bf16x3" = fp32-accurate 3 x bf16 split, "bf16" = operands
# rounded to bf16 (what BASELINE.json names for its bf16 configurations), "fp16x2" (the default: two fp16 terms, three products;
# fp32-class results, 1e-6 against exact fp32 products on every preset measured, at 1.6-3.4 x the speed on the egs presets).
# fp16x2 needs the range of the GEMM's input per utterance: lstm_path takes it from the caller (`amax`: the partial maxima the
# projection + LayerNorm row kernel of the previous recurrence left behind) or measures it (hip.absmax, one pass over the rows:
# the first GEMM of a masker).  A per-module attribute `gemm_precision` (GemmPlanCache; no process-wide switch).
_PLANES = {"fp32": 0, "bf16": 1, "bf16x3": 3, "fp16x2": 2}


def tensor_signature(module: nn.Module) -> tuple:
    """Cheap fingerprint of every parameter / buffer: a changed value (in-place edit, load_state_dict, .to(device)) changes
    the version counter or the data pointer.  What a captured graph or a weight pack is checked against, by the streaming
    classes at every call: hence one walk over the module tree, not parameters() and then buffers()."""
    return tuple((t.data_ptr(), t._version) for m in module.modules() for tensors in (m._parameters, m._buffers)
                 for t in tensors.values() if t is not None)


def param_signature(module: nn.Module) -> tuple:
    """tensor_signature and the training switch: the key of a packed plan (PlanCache appends the device and the module's own
    switches)."""
    return tensor_signature(module) + (module.training,)


def _tensors_in(obj, seen: set, out: list) -> None:
    if torch.is_tensor(obj):
        if id(obj) not in seen:
            seen.add(id(obj))
            out.append(obj)
    elif isinstance(obj, dict):
        for v in obj.values():
            _tensors_in(v, seen, out)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _tensors_in(v, seen, out)


class PlanCache:
    """Mixin of every module under nnet/ that keeps something from call to call: packed weights ("plans": the kernel-side
    copies of its parameters, with the ctypes structs that point into them) and scratch.

    Plans: `self._plan_get(device, builder)` is builder(device) of the last call, as long as no parameter or buffer below the
    module, its training switch, the device or one of the module's own switches (`_plan_switches`) has changed; one plan per
    builder.  `prepare_plans(device)` builds or re-validates, on the current stream, every plan inference() reads.
    Scratch: `keep_scratch(name, lane, value)` / `scratch(name, lane)`, one entry per concurrent HIP stream of the caller.
    Neither is pickled or deep-copied (`__getstate__`), and `cached_tensors()` lists the tensors both keep alive."""

    _plans = None      # {builder's name: (key, plan)}
    _scratch = None    # {(name, lane): value}

    def _plan_switches(self) -> tuple:
        """The module's own switches that a plan depends on beside its parameters."""
        return ()

    def _plan_build(self, name: str, builder, device):
        return builder(device)

    def _plan_get(self, device, builder, key=None):
        """`key`: of a plan made of the children's plans (ConvTasNet's block array: their identities), which have validated
        their fingerprints already."""
        if key is None:
            key = param_signature(self) + (str(device),) + self._plan_switches()
        if self._plans is None:
            self._plans = {}
        name = builder.__name__
        kept = self._plans.get(name)
        if kept is None or kept[0] != key:
            self._plans[name] = kept = (key, self._plan_build(name, builder, device))
        return kept[1]

    def prepare_plans(self, device) -> None:
        self._plan_get(device, self._build)

    def scratch(self, name: str, lane: int = 0):
        return None if self._scratch is None else self._scratch.get((name, lane))

    def keep_scratch(self, name: str, lane: int, value):
        if self._scratch is None:
            self._scratch = {}
        self._scratch[name, lane] = value
        return value

    def kept_scratch(self) -> list:
        return [] if self._scratch is None else list(self._scratch.values())

    def cached_tensors(self) -> list:
        """Every tensor this module's plans and kept scratch hold (not its submodules')."""
        out = []
        _tensors_in([[plan for _, plan in (self._plans or {}).values()], self.kept_scratch()], set(), out)
        return out

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_plans", None)
        state.pop("_scratch", None)
        return state

    def set_gemm_precision(self, name: str):
        """"fp32" | "bf16x3" | "fp16x2" | "bf16" for this module and every module below it that has the choice (the TCN
        blocks' 1x1 convs, the recurrent maskers' LSTM input projections, attention layers, SingleRNN, the pooling).
        Assigning `m.gemm_precision` directly does the same for one module; either takes effect at the next call."""
        if name not in _PLANES:
            raise ValueError(f"gemm precision must be one of {sorted(_PLANES)}")
        for m in self.modules():
            if hasattr(m, "gemm_precision"):
                m.gemm_precision = name
        return self


@contextlib.contextmanager
def own_plans(mods: list, own: list):
    """Inside the block the plan-cached modules `mods` compute with the caller's own precision and plans, own[i] = {"gemm_precision":
    ..., "_plans": ...} of mods[i] (start: {"gemm_precision": "fp32"}); the modules' own are put back after it and what was built
    inside is kept in `own` for the next time.  How a path with exact fp32 products (the streamers, the ragged batches of the
    noise suppressors) leaves the model's plans, and so plain inference, untouched."""
    swap = ("gemm_precision", "_plans")
    saved = []
    for m, mine in zip(mods, own):
        saved.append({k: m.__dict__.pop(k) for k in swap if k in m.__dict__})
        m.__dict__.update(mine)
    try:
        yield
    finally:
        for i, m in enumerate(mods):
            own[i] = {k: m.__dict__.pop(k) for k in swap if k in m.__dict__}
            m.__dict__.update(saved[i])


class GemmPlanCache(PlanCache):
    """PlanCache of a module whose plans depend on `gemm_precision`."""

    gemm_precision = "fp16x2"

    def _plan_switches(self) -> tuple:
        return (self.gemm_precision,)


def _f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(dtype=torch.float32, device=device).contiguous()


def lstm_plan(lstm: nn.LSTM, device, gemm: str = "fp32") -> dict:
    """nn.LSTM(num_layers=1, batch_first=True): input projection rows stacked over directions (for one
    ps_conv1x1_f32), summed biases, W_hh transposed per direction."""
    if lstm.num_layers != 1 or not lstm.batch_first or lstm.proj_size != 0 or not lstm.bias:
        raise NotImplementedError("HIP LSTM: num_layers=1, batch_first=True, bias=True, no projection")
    dirs = 2 if lstm.bidirectional else 1
    hid = lstm.hidden_size
    wih, bias, whh = [], [], []
    for suf in ["", "_reverse"][:dirs]:
        wih.append(_f32(getattr(lstm, "weight_ih_l0" + suf), device))
        bias.append(_f32(getattr(lstm, "bias_ih_l0" + suf), device) + _f32(getattr(lstm, "bias_hh_l0" + suf), device))
        whh.append(_f32(getattr(lstm, "weight_hh_l0" + suf), device).t().contiguous())
    plan = dict(wih=hip.pack_wt(torch.cat(wih, 0)), wih_rows=torch.cat(wih, 0).contiguous(), bias=torch.cat(bias).contiguous(),
                whh_t=torch.stack(whh).contiguous(), H=hid, D=dirs, rows=dirs * 4 * hid, I=lstm.input_size,
                planes=_PLANES[gemm])
    if plan["planes"] == 0 and hid in (256, 192):
        # fp32 arithmetic: W_hh's image for ps_lstm_h256_f32, packed here so that a graph capture holds no packing
        plan["whh_h256_f32"] = hip.pack_whh_h256_f32(plan["whh_t"])
    return plan


def rnn_plan(rnn: nn.Module, device) -> dict:
    """nn.GRU / nn.RNN(tanh; num_layers=1, batch_first=True) for ps_rnn_f32: input projection rows stacked over directions,
    b_hh folded into the projection's bias except the GRU's n gate (its hidden bias sits inside the reset product: bhn)."""
    kind = "GRU" if isinstance(rnn, nn.GRU) else "RNN"
    if kind == "RNN" and getattr(rnn, "nonlinearity", "tanh") != "tanh":
        raise NotImplementedError("nn.RNN on HIP: tanh cells (the reference's SingleRNN builds no other)")
    if rnn.num_layers != 1 or not rnn.batch_first:
        raise NotImplementedError("HIP recurrences: one layer, batch_first")
    hid, ng = rnn.hidden_size, (3 if kind == "GRU" else 1)
    wih, bias, whh, bhn = [], [], [], []
    for suf in ([""] if not rnn.bidirectional else ["", "_reverse"]):
        b_hh = _f32(getattr(rnn, "bias_hh_l0" + suf), device)
        fold = b_hh.clone()
        if kind == "GRU":
            fold[2 * hid:] = 0.0
            bhn.append(b_hh[2 * hid:].clone())
        wih.append(_f32(getattr(rnn, "weight_ih_l0" + suf), device))
        bias.append(_f32(getattr(rnn, "bias_ih_l0" + suf), device) + fold)
        whh.append(_f32(getattr(rnn, "weight_hh_l0" + suf), device).t().contiguous())
    rows = torch.cat(wih, 0).contiguous()
    return dict(kind=kind, wih=hip.pack_wt(rows), rows=rows.shape[0], bias=torch.cat(bias).contiguous(),
                whh_t=torch.stack(whh).contiguous(), bhn=torch.stack(bhn).contiguous() if bhn else None, H=hid,
                D=2 if rnn.bidirectional else 1, I=rnn.input_size)


def linear_plan(lin: nn.Module, device) -> dict:
    """nn.Linear or nn.Conv1d(k=1)."""
    w = lin.weight
    if w.dim() == 3:
        w = w[:, :, 0]
    return dict(wt=hip.pack_wt(_f32(w, device)), bias=None if lin.bias is None else _f32(lin.bias, device),
                M=w.shape[0], K=w.shape[1], w_rows=_f32(w, device))


def layernorm_plan(ln: nn.Module, device) -> dict:
    """nn.LayerNorm(C) (weight/bias, eps) or ChanLN (gamma/beta, eps 1e-8)."""
    if isinstance(ln, nn.LayerNorm):
        if len(ln.normalized_shape) != 1 or ln.weight is None:
            raise NotImplementedError("HIP LayerNorm: one normalised dim with affine parameters")
        return dict(gamma=_f32(ln.weight, device), beta=_f32(ln.bias, device), eps=float(ln.eps))
    return dict(gamma=_f32(ln.gamma, device), beta=_f32(ln.beta, device), eps=float(ln.eps))


def packed(plan: dict, key, build, *args):
    """plan[key], made by build(*args) at the first call: a weight image that only some routes read."""
    image = plan.get(key)
    if image is None:
        image = plan[key] = build(*args)
    return image


def packed_ln_image(lin: dict):
    """linear_plan's 128 weight rows as the fp16x2 image hip.conv1x1_f16x2_ln reads: zero padded to 256 rows."""
    return packed(lin, "f16x2_ln", lambda w: hip.pack_wt_f16x2(torch.cat([w, torch.zeros_like(w)])), lin["w_rows"])


def _proj_norm(x, hseq, t, rnn, proj, norm, amax, skip=True):
    """x + LN(proj(h)) behind a recurrence (second half of lstm_path); skip=False: LN(proj(h)) alone."""
    res = x if skip else None
    n, _, ldt = x.shape
    dev = x.device
    # the fused projection + LayerNorm kernel is the short-row kernel (16-frame workgroups): on long rows (the 2-D
    # maps of DPCRN / DPARN: F * ld frames) the MFMA GEMM plus a LayerNorm pass is faster
    if proj["M"] <= 256 and FUSE_PROJ_LN and t <= FUSE_PROJ_LN_MAX_FRAMES:
        if amax is not None and rnn["planes"] == 2 and t >= 128:
            try:   # the row kernel hands the next GEMM its input range for free
                y, _, amax[0] = hip.proj_layernorm(hseq, t, proj["wt"], proj["bias"], proj["M"], norm["gamma"], norm["beta"],
                                                   norm["eps"], res, want_amax=True)
                return y
            except RuntimeError:
                amax[0] = None
        y, _ = hip.proj_layernorm(hseq, t, proj["wt"], proj["bias"], proj["M"], norm["gamma"], norm["beta"], norm["eps"], res)
        return y
    if (FUSE_GEMM_LN and rnn["planes"] == 2 and proj["M"] == 128 and proj["K"] % 32 == 0
            and hip.conv1x1_f16x2_ln_ok(n, proj["K"], 128, t)):
        # projection, LayerNorm and skip as ONE launch: the fp16x2 GEMM with the norm as its epilogue (|h| < 1 is its range)
        wf, we = packed_ln_image(proj)
        if amax is not None:   # the maxima of |y| ride along: the next recurrence's GEMM needs no pass of its own over y
            y, amax[0] = hip.conv1x1_f16x2_ln(hseq, t, wf, we, 128, proj["bias"], norm["gamma"], norm["beta"], norm["eps"], res,
                                              x_bound=1.0, want_amax=True)
            return y
        return hip.conv1x1_f16x2_ln(hseq, t, wf, we, 128, proj["bias"], norm["gamma"], norm["beta"], norm["eps"], res, x_bound=1.0)
    p = torch.empty(n, proj["M"], ldt, dtype=torch.float32, device=dev)
    if rnn["planes"] == 2 and proj["K"] >= 64:
        # the recurrence's arithmetic for its projection too: h is an LSTM output, |h| < 1 is its range
        wf, we = packed(proj, "f16x2", hip.pack_wt_f16x2, proj["w_rows"])
        hip.conv1x1_f16x2(hseq, t, wf, we, proj["M"], None, proj["bias"], out=p, x_bound=1.0)
    else:
        hip.conv1x1(hseq, t, proj["wt"], proj["M"], None, proj["bias"], out=p)
    return hip.chan_layernorm(p, t, norm["gamma"], norm["beta"], norm["eps"], res=res)


#: zeroed LSTM output rows a recurrence plan keeps per lane (_h_rows): one per (shape, geometry) lately seen, as long as
#: they stay under H_ROWS_BYTES together (the one in use is always kept: a full batch's rows alone are past a gigabyte)
H_ROWS_KEPT = 8
H_ROWS_BYTES = 256 << 20


def _h_rows(rnn: dict, x: torch.Tensor, t: int, q: int, q_stride: int, steps: int, step_stride: int, lane: int = 0,
            per_row: bool = False):
    """Output rows of a recurrence.  When the sequences do not cover the span of t frames (the 2-D maps of DPCRN / DPARN:
    F rows of ld frames, pad frames between them) the recurrence never writes the pad frames, and what follows it --
    projection, LayerNorm, the next GEMM's range maximum -- runs over the whole span: the rows then come from a zeroed
    buffer kept with the plan, so stale memory (a NaN, an Inf) cannot reach the maximum.

    One buffer per `lane` (the caller's concurrent HIP streams must not write the same rows), shape, device and sequence
    geometry (t, q, q_stride, steps, step_stride): rnn["h_rows"][lane][(shape, device, geometry)].  Whoever is handed a
    buffer -- an eager call or a captured graph, at any later time, in any order -- writes the frames of that one
    geometry into it and no others, so its pad frames are zero for as long as it lives and nothing ever has to clear it:
    the invariant rests on no host-side record that a graph replay would bypass.  (Two utterance lengths inside one row
    length share a shape and differ in their geometry: frames the longer call writes are pad frames of the shorter one.)
    A lane keeps its most recently used buffers, H_ROWS_KEPT at most and H_ROWS_BYTES together (the one in use always stays); an
    older one is dropped from the plan, never cleared or handed out again, so a captured graph that pinned it
    (graphs._cached_tensors) keeps it, with its pads, to itself, and an eager caller pays one fill per change of geometry.
    per_row: the walk of hip.lstm_rows, keyed apart from the plain walk of the same geometry.
    None = let the kernel wrapper allocate (every frame is written)."""
    if q * steps >= t:
        return None
    n, _, ldt = x.shape
    shape = (n, rnn["D"] * rnn["H"], ldt)
    key = (shape, str(x.device), (t, q, q_stride, steps, step_stride) + (("rows",) if per_row else ()))
    bufs = rnn.setdefault("h_rows", {}).setdefault(lane, {})
    buf = bufs.pop(key, None)
    if buf is None:
        size = 4 * n * shape[1] * ldt
        while bufs and (len(bufs) >= H_ROWS_KEPT or size + sum(4 * b.numel() for b in bufs.values()) > H_ROWS_BYTES):
            bufs.pop(next(iter(bufs)))
        buf = torch.zeros(shape, dtype=torch.float32, device=x.device)
    bufs[key] = buf       # (dicts keep insertion order: the most recently used buffer is the last)
    return buf


# What one LSTM pass runs (lstm_route).  gemm: the input projection's arithmetic, "fp32" | "bf16" | "f16x2"; planes: of "bf16", 1
# (operands rounded) or 3 (the fp32-accurate split), else 0; layout: of the gate pre-activations, "rows" (channel-major) |
# "fmajor" (frame-major); kernel: the recurrence, "generic" | "generic_f16x2" | "fmajor128" | "fmajor256" | "h256_f32".
Route = namedtuple("Route", "gemm planes layout kernel")


def lstm_route(rnn: dict, n: int, ldt: int, t: int, walk: tuple, carried: bool = False, state_shift: int = 0,
               standalone: bool = False) -> Route:
    """Which input-projection GEMM, in which layout, feeding which recurrence entry: the one place that chooses, for every
    LSTM pass of the models.  Launches nothing.  rnn: lstm_plan's scalars (planes, I, H, D, rows, whether it holds
    "whh_h256_f32"); n, ldt, t: the rows [N, C, ldt] with t valid frames; walk = (Q, q_stride, steps, step_stride); carried:
    the launch takes or returns states (h0, c0, want_state or state_out).  "h256_f32" stands under ps_lstm_h256_ok, which
    lstm_recurrence asks behind the GEMM's launch, where it has always been asked (refused: "generic").

    standalone: SingleRNN as a layer of its own (the speaker LSTM of tse_skim_v1), where no range is carried from pass to
    pass.  Its choice differs from the maskers' in four ways, kept as found because each changes bits (a later decision):
      1. H = 128 never takes the frame-major route (the maskers: in fp16x2 without carried states).
      2. FMAJOR_LSTM is not consulted: H = 256 / 192 in fp16x2 is frame-major whatever the switch says.
      3. fp16x2 off the frame-major routes runs the bf16x3 GEMM, which needs no range pass, and ps_lstm_f32 (the maskers:
         hip.absmax, the fp16x2 GEMM, ps_lstm_f16x2_f32).
      4. fp16x2 with I < 64 runs the fp32 GEMM and ps_lstm_f32 (the maskers: ps_lstm_f16x2_f32)."""
    planes, I, H, D = rnn["planes"], rnn["I"], rnn["H"], rnn["D"]
    gemm = ("bf16", planes) if planes and I >= 64 else ("fp32", 0)
    if planes == 2 and I >= 64:
        # H = 128 (the bottleneck LSTMs of DPCRN / DPARN): the 16-sequence recurrence that streams frame-major pre-activations
        if (not standalone and FMAJOR_LSTM and H == 128 and not carried and state_shift == 0
                and hip.lstm_fmajor_ok(n, ldt, H, D, *walk) and hip.conv1x1_f16x2_fmajor_ok(n, I, rnn["rows"], t, ldt)):
            return Route("f16x2", 0, "fmajor", "fmajor128")
        # H = 256 / 192 (SkiM's segment LSTMs, the speaker LSTM): W_hh streamed from L2 or resident in registers, states carried
        if ((standalone or FMAJOR_LSTM) and H in (256, 192) and hip.lstm_fmajor_h256_ok(n, ldt, D, *walk)
                and hip.conv1x1_f16x2_fmajor_ok(n, I, rnn["rows"], t, ldt)):
            return Route("f16x2", 0, "fmajor", "fmajor256")
        gemm = ("bf16", 3) if standalone else ("f16x2", 0)
    # fp32 arithmetic at H = 256 / 192 with enough sequences (hip.H256_F32_MIN_SEQS): W_hh streamed into exact fp32 MFMA
    if "whh_h256_f32" in rnn and hip.lstm_h256_f32_pays(H, D, n, walk[0]):
        return Route(*gemm, "rows", "h256_f32")
    return Route(*gemm, "rows", "generic_f16x2" if planes == 2 and not standalone else "generic")


def lstm_gates(x: torch.Tensor, t: int, rnn: dict, route: Route, x_amax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The input projection of every frame in route's arithmetic and layout -> gate pre-activations.  x_amax: the partial
    maxima of |x| for the fp16x2 GEMM (None: measured here)."""
    if route.gemm == "f16x2":
        wf, we = packed(rnn, "wih_f16x2", hip.pack_wt_f16x2, rnn["wih_rows"])
    if route.layout == "rows":
        gx = torch.empty(x.shape[0], rnn["rows"], x.shape[2], dtype=torch.float32, device=x.device)
    if route.gemm == "f16x2":
        x_amax = x_amax if x_amax is not None else hip.absmax(x, t)
        if route.layout == "fmajor":
            return hip.conv1x1_f16x2_fmajor(x, t, wf, we, rnn["rows"], rnn["bias"], x_amax=x_amax)
        hip.conv1x1_f16x2(x, t, wf, we, rnn["rows"], None, rnn["bias"], out=gx, x_amax=x_amax)
    elif route.gemm == "bf16":
        image = packed(rnn, ("wih_bf16", route.planes), hip.pack_wt_bf16, rnn["wih_rows"], route.planes)
        hip.conv1x1_bf16(x, t, image, rnn["rows"], None, rnn["bias"], out=gx)
    else:
        hip.conv1x1(x, t, rnn["wih"], rnn["rows"], None, rnn["bias"], out=gx)
    return gx


def lstm_recurrence(gx: torch.Tensor, x: torch.Tensor, t: int, rnn: dict, kernel: str, walk: tuple, h0=None, c0=None,
                    want_state: bool = False, state_shift: int = 0, state_out=None, lane: int = 0, steps_rows=None):
    """The recurrence entry `kernel` (Route.kernel) over lstm_gates' pre-activations -> (hout [N, D*H, ldt], final states or
    None); x: the pass's input rows (with the walk they decide where the output rows come from, see _h_rows).  steps_rows
    (int32 [N] on the device): a step count per utterance -- hip.lstm_rows whatever `kernel` says, channel-major
    pre-activations and no state_shift."""
    states = (h0, c0, want_state, state_shift, state_out)
    if steps_rows is not None:
        if gx.dim() != 3 or gx.shape[1] != rnn["rows"] or state_shift:
            raise RuntimeError("lstm_recurrence: a per-row step count takes channel-major pre-activations and no state_shift")
        return hip.lstm_rows(gx, rnn["whh_t"], rnn["H"], rnn["D"], *walk, steps_rows, h0, c0, want_state, state_out,
                             out=_h_rows(rnn, x, t, *walk, lane, per_row=True))
    if kernel == "fmajor256":
        image, scales = packed(rnn, "whh_h256", hip.pack_whh_h256, rnn["whh_t"])
    out = _h_rows(rnn, x, t, *walk, lane)
    if kernel == "fmajor256":
        return hip.lstm_fmajor_h256(gx, image, scales, rnn["D"], *walk, *states, out=out)
    if kernel == "fmajor128":
        return hip.lstm_fmajor(gx, rnn["whh_t"], rnn["H"], rnn["D"], *walk, out=out), None
    if kernel == "h256_f32" and hip.lstm_h256_f32_ok(
            x.shape[0], x.shape[2], rnn["H"], rnn["D"], *walk, state_shift=state_shift,
            ldq=min([s.shape[2] for s in (h0, c0) + tuple(state_out or ()) if s is not None], default=0)):
        return hip.lstm_h256_f32(gx, rnn["whh_h256_f32"], rnn["D"], *walk, *states, out=out)
    return hip.lstm(gx, rnn["whh_t"], rnn["H"], rnn["D"], *walk, *states, f16x2=kernel == "generic_f16x2", out=out)


def lstm_path(x: torch.Tensor, t: int, rnn: dict, proj: dict, norm: dict, q: int, q_stride: int, steps: int,
              step_stride: int, h0=None, c0=None, want_state: bool = False, state_shift: int = 0, state_out=None,
              amax: Optional[list] = None, skip: bool = True, lane: int = 0, steps_rows=None):
    """x + LN(proj(LSTM(x))) on padded [N,C,ldt] (dprnn.py:154-172, skim.py:215-227) -> (x', final states).
    `steps_rows`: lstm_recurrence's (a ragged batch; the caller's plans are exact fp32, whose pre-activations are channel-major).
    `amax`: a one-element list carried from recurrence to recurrence in the fp16x2 arithmetic -- on entry the partial maxima
    of |x| per utterance (or None: measured here), on return those of x' (None when the kernel that made x' has none).
    `lane`: which of the caller's concurrent HIP streams this is (selects the kept output rows, see _h_rows)."""
    x_amax = amax[0] if amax is not None else None
    if amax is not None:
        amax[0] = None
    walk = (q, q_stride, steps, step_stride)
    route = lstm_route(rnn, x.shape[0], x.shape[2], t, walk,
                       h0 is not None or c0 is not None or want_state or state_out is not None, state_shift)
    gx = lstm_gates(x, t, rnn, route, x_amax)
    hseq, state = lstm_recurrence(gx, x, t, rnn, route.kernel, walk, h0, c0, want_state, state_shift, state_out, lane,
                                  steps_rows)
    return _proj_norm(x, hseq, t, rnn, proj, norm, amax, skip), state
