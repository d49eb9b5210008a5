"""Streaming the causal time-domain Conv-TasNet (FreeEncDec + causal ConvTasNet, with or without a speaker branch: egs/tse
td_tse_conv_tasnet_v0_causal) on the HIP path, one hop at a time for B concurrent streams.

The model is exactly causal in time: a free encoder of `win`-sample frames every `hop` samples, TCN blocks whose depthwise
convolutions are padded on the left only, norms that act frame by frame (eval BatchNorm1d, a per-channel affine map; cLN, a
LayerNorm over the channels of one frame), a speaker embedding fixed for the whole session, and a transposed-convolution
decoder.  So the samples a stream returns, followed by flush(), equal `model.inference` on the whole signal: frame t covers
samples [t*hop, t*hop + win), and output samples [t*hop, (t+1)*hop) are final once frame t has been decoded.

Layout: the k frames of a chunk for the B streams are the N = k*B columns of the library's channel-major rows (column
f*B + b = frame f, stream b), so every 1x1 convolution is ps_conv1x1_f32 with N columns and every cLN ps_chan_layernorm_f32.
The speaker embedding enters as E extra rows of the residual-stream buffers, written once per session and chunk length,
which the embedding blocks' in_conv reads with its full [H x (C+E)] weight.  New kernels (csrc/tcn_step.hip) do what needs
earlier frames: ps_dwconv_step_f32 (the dilated causal depthwise convolution, history from a circular ring per block, indexed
by the device frame counter) and ps_free_decode_step_f32 (mask x features, the synthesis product and the overlap-add with a
per-stream tail); ps_stream_commit_frames_f32 moves the window queue and advances the counter by k.  No launch argument
depends on the frame index, so one captured graph per chunk length replays every chunk.

Arithmetic: exact fp32 products throughout, whatever the model's gemm_precision.  The streamer packs its own weights from
the parameters, so the model's own setting and plans are left as they were.  The embedding is computed once per stream by
the model's speaker branch (inference_tse_embedding), in the model's own arithmetic.

Slots (init_slots / open / end / close): a session of fixed capacity B whose columns begin and end streams of their own while
it runs.  Per slot the device holds a span (birth, death) of absolute frame indices; frame g of column b is live iff
birth[b] <= g < death[b].  ps_dwconv_step_slots_f32 reads a frame that is not live as 0 (the rule for g < 0, per column) and
ps_free_decode_step_slots_f32 adds nothing for it; everything else in a hop is column-wise, so dead columns compute values
nobody reads.  A slot's output is the offline output of its stream delayed by latency_samples, whatever the other slots do.
The session around the kernels (priming, step / step_chunk / flush, eager run or graph replay, the capture) and the slot
bookkeeping (open / end / close, the spans, the frame limit) are HopSession's: streaming/_session.py.  What follows from the
free encoder and decoder (their checks and packs, the front and back of a chunk, the flush) is FreeEncSession's:
streaming/_free.py; this file has the checks of the masker, its packs, rings and buffers, and the TCN blocks (`_masker`).
"""
from typing import Dict, List, Optional

import torch

from .. import hip
from .._abi import PS_NORM_AFFINE
from ..nnet.conv_tasnet import TCN, ConvTasNet
from ..nnet.lobe.norm import ChanLN, norm_plan
from ._free import FreeEncSession, check_back, check_front
# K_MAX: frames per launch at most, step_chunk splits longer chunks (the rings hold (P-1)*dilation + K_MAX frames);
# FRAME_LIMIT: where a session stops (HopSession._run), INT32_MAX: the death of a stream that has not ended
from ._session import FRAME_LIMIT, INT32_MAX, K_MAX, HopSession, check_on_device  # noqa: F401


def check_streamable(model) -> None:
    """Raise NotImplementedError naming the reason when `model` is not a configuration this streamer computes exactly."""
    name = "StreamingConvTasNet"
    check_front(model, name)
    m = model.masker
    if not isinstance(m, ConvTasNet):
        raise NotImplementedError(f"{name}: masker {type(m).__name__}: ConvTasNet only")
    if not m.causal:
        raise NotImplementedError(f"{name}: the ConvTasNet is not causal (causal=False: centred convolutions read future "
                                  f"frames)")
    if m.tcn_layer.lower() != "normal":
        raise NotImplementedError(f"{name}: tcn_layer {m.tcn_layer!r}: only the normal TCN block streams (not gated)")
    for what in ("tcn_norm", "dconv_norm"):
        if getattr(m, what) not in ("bN1d", "cLN"):
            raise NotImplementedError(f"{name}: {what} {getattr(m, what)!r}: bN1d (an affine map in eval mode) or cLN (a norm "
                                      f"over one frame's channels) only")
    if model.embedding_free_tse:
        raise NotImplementedError(f"{name}: embedding_free_tse (the enrolment seeds the masker) does not stream")
    if any(m.tcn_with_embed) and model.speaker_net is None:
        raise NotImplementedError(f"{name}: tcn_with_embed blocks without a speaker_net to compute the embedding")
    check_back(model, name)
    for blk in (b for stack in m.tcn_list for b in stack):
        dsc = blk.dconv[0]
        if any(a.weight.numel() != 1 for a in (blk.in_conv[2], dsc.depthwise[2], dsc.pointwise[2])):
            raise NotImplementedError(f"{name}: PReLU with per-channel slopes is not on the HIP path")
    check_on_device(model, name)


class StreamingConvTasNet(FreeEncSession):
    """Hop-by-hop inference of a causal Conv-TasNet separator / speaker extractor for B streams (see the module docstring).

    s = StreamingConvTasNet(model); s.init_streams(B, enroll); s.step(hop [B, hop]) -> [B, hop] or None while the first
    window fills; s.step_chunk([B, k*hop]) -> what k step() calls return, concatenated; s.flush() -> the last win - hop
    samples.

    Slots, for streams that begin and end on their own: s.init_slots(capacity); s.open(slot, enroll [L']); every
    s.step / s.step_chunk([capacity, k*hop]) -> [capacity, k*hop] from the first hop on (idle slots: constrain(0));
    s.end(slot, hops) when the stream has `hops` more hops of input; s.close(slot) -> the last win - hop samples, and the
    slot is idle again.  What a slot returned from open to close, then close's samples, is the offline output of its stream
    after latency_samples samples of constrain(0): slot_output_range(L, win, hop).
    """

    check_streamable = staticmethod(check_streamable)

    # -- weights ------------------------------------------------------------------------------------------------------
    def _build_packs(self, dev: torch.device) -> None:
        """Weights packed for the kernels (eval BatchNorm1d folded to scale / shift), held by the streamer: a captured
        graph keeps reading these tensors."""
        f32 = dict(dtype=torch.float32, device=dev)
        blocks = []
        for blk in self._blocks:
            dsc = blk.dconv[0]
            p = dict(E=blk.emb_dim, P=blk.kernel, dilation=blk.dilation,
                     in_wt=hip.pack_wt(blk.in_conv[0].weight.detach().to(**f32)[:, :, 0]),
                     dw_w=dsc.depthwise[0].weight.detach().to(**f32).contiguous(),
                     dw_b=dsc.depthwise[0].bias.detach().to(**f32).contiguous(),
                     pw_wt=hip.pack_wt(dsc.pointwise[0].weight.detach().to(**f32)),
                     pw_b=dsc.pointwise[0].bias.detach().to(**f32).contiguous(),
                     out_wt=hip.pack_wt(blk.out_conv.weight.detach().to(**f32)),
                     out_b=blk.out_conv.bias.detach().to(**f32).contiguous())
            for key, (norm, act) in (("in", blk.in_conv[1:3]), ("dw", dsc.depthwise[1:3]), ("pw", dsc.pointwise[1:3])):
                if isinstance(norm, ChanLN):
                    kind, g, b = "cln", norm.gamma.detach(), norm.beta.detach()
                else:
                    kind, g, b = norm_plan(norm)
                g, b = g.to(**f32).reshape(-1).contiguous(), b.to(**f32).reshape(-1).contiguous()
                slope = act.weight.detach().to(**f32).contiguous()
                pro = None if kind == "cln" else hip.make_prologue(PS_NORM_AFFINE, True, None, 0.0, 1e-8, g, b, slope)
                p[key] = (kind, g, b, slope, pro)
            blocks.append(p)
        self._packs = dict(self._free_packs(dev), blocks=blocks)

    # -- session ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def init_streams(self, streams: int = 1, enroll: Optional[torch.Tensor] = None, use_graph: bool = True) -> None:
        """Start `streams` new streams (every state zeroed).  enroll [streams, L'] on the model's device: the enrolment of
        each stream, required iff the model has a speaker_net; its embedding is computed here, once."""
        b = self._at_least_one(streams, "init_streams: streams")
        model, m = self.model, self.model.masker
        if (enroll is not None) != (model.speaker_net is not None):
            raise ValueError("StreamingConvTasNet.init_streams: an enrolment [streams, L'] is required iff the model has a "
                             "speaker_net")
        dev = next(model.parameters()).device
        self._emb = None
        if enroll is not None:
            self._check_enrolments(enroll, b)
            if any(m.tcn_with_embed):
                dvec = model.inference_tse_embedding(enroll)[..., 0].float().contiguous()   # [B, E]
                self._emb = hip.l2_normalize(dvec) if m.embed_norm else dvec
        self._new_session(b, dev, use_graph)

    def _new_session(self, b: int, dev: torch.device, use_graph: bool) -> None:
        """Zeroed state of b columns (self._emb is set by the caller)."""
        m = self.model.masker
        self._begin(b, dev, use_graph)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        self._blocks: List[TCN] = [blk for stack in m.tcn_list for blk in stack]
        # one circular ring of activated depthwise inputs per block: (P-1)*dilation frames of history plus a chunk
        self._rings = [z((blk.kernel - 1) * blk.dilation + K_MAX, blk.hid_channels, b) for blk in self._blocks]
        self._bufs: Dict[int, dict] = {}

    @torch.no_grad()
    def init_slots(self, capacity: int, use_graph: bool = True) -> None:
        """Start a slot session of `capacity` columns, every slot idle (every state zeroed); open() starts a stream."""
        b = self._at_least_one(capacity, "init_slots: capacity")
        model, m = self.model, self.model.masker
        dev = next(model.parameters()).device
        self._emb = None
        if model.speaker_net is not None and any(m.tcn_with_embed):
            self._emb = torch.zeros(b, m.embed_dim, dtype=torch.float32, device=dev)
        self._new_session(b, dev, use_graph)
        self._make_slots()

    def _enrolment_rule(self) -> tuple:
        has = self.model.speaker_net is not None
        return has, f"iff the model has a speaker_net (this one has {'one: pass enroll' if has else 'none: pass no enroll'})"

    def _open_slot(self, slot: int, enroll: Optional[torch.Tensor]) -> None:
        """The slot's embedding, computed here, once (the rings need no reset: a dead frame's ring slot is never read)."""
        model, m = self.model, self.model.masker
        if self._emb is not None:
            dvec = model.inference_tse_embedding(enroll)[..., 0].float().contiguous()   # [1, E]
            dvec = (hip.l2_normalize(dvec) if m.embed_norm else dvec)[0]
            self._emb[slot] = dvec
            c = m.input_dim
            for bufs in self._bufs.values():           # (chunk lengths created later read self._emb)
                for r in bufs["res"]:
                    r[0, c:, slot:bufs["n"]:self.streams] = dvec[:, None]

    def _state(self) -> List[torch.Tensor]:
        return [self._queue, self._tail, self._counter] + self._rings

    # -- one chunk ----------------------------------------------------------------------------------------------------
    def _buffers(self, hops: int) -> dict:
        """Activation buffers of a `hops`-frame chunk: [1, rows, ld] over N = hops * B columns.  The residual-stream buffers
        carry the embedding rows (column f*B + b = stream b's embedding), written here once per session and chunk length."""
        if hops not in self._bufs:
            m, b = self.model.masker, self.streams
            n = hops * b
            ld = hip.padded_frames(n)
            c, h = m.input_dim, m.tcn_dim
            e = m.embed_dim if self._emb is not None else 0
            z = lambda rows: torch.zeros(1, rows, ld, dtype=torch.float32, device=self.device)  # noqa: E731
            res = [z(c + e) for _ in range(3)]     # features (kept for the decoder), then two alternating block outputs
            if e:
                rows = self._emb.t().repeat(1, hops)   # [E, N]
                for r in res:
                    r[0, c:, :n] = rows
            self._bufs[hops] = dict(n=n, ld=ld, res=res, feats=res[0][:, :c], y1=z(h), a1=z(h), y2=z(h), a2=z(h), y3=z(h),
                                    a3=z(h))
        return self._bufs[hops]

    def _block(self, i: int, p: dict, x: torch.Tensor, out: torch.Tensor, bufs: dict, hops: int) -> None:
        """TCN block i on the chunk: x [1, C(+E), ld] -> out[:, :C]; the depthwise convolution reads / feeds ring i."""
        n, c = bufs["n"], self.model.masker.input_dim
        h = self._blocks[i].hid_channels

        def settle(y, key, a):
            """-> (tensor, prologue) the next stage consumes for the norm + PReLU that follow `y`."""
            kind, g, b, slope, pro = p[key]
            if kind == "cln":
                return hip.chan_layernorm(y, n, g, b, 1e-8, slope=slope, out=a), None
            return y, pro

        y1, _ = hip.conv1x1(x[:, :c + p["E"]], n, p["in_wt"], h, out=bufs["y1"])
        src, pro = settle(y1, "in", bufs["a1"])
        y2 = hip.dwconv_step(src, self._rings[i], self._counter, p["dw_w"], p["dw_b"], p["dilation"], self.streams, hops, pro,
                             out=bufs["y2"], span=self._span)
        src, pro = settle(y2, "dw", bufs["a2"])
        y3, _ = hip.conv1x1(src, n, p["pw_wt"], h, pro, p["pw_b"], out=bufs["y3"])
        src, pro = settle(y3, "pw", bufs["a3"])
        hip.conv1x1(src, n, p["out_wt"], c, pro, p["out_b"], res=x[:, :c], out=out[:, :c])

    def _masker(self, hops: int, bufs: dict, feats: torch.Tensor) -> torch.Tensor:
        """The TCN blocks on the residual stream, alternating between two buffers -> the last block's output."""
        x, x0, x1 = bufs["res"]
        for i, p in enumerate(self._packs["blocks"]):
            y = x0 if i % 2 == 0 else x1
            self._block(i, p, x, y, bufs, hops)
            x = y
        return x[:, :feats.shape[1]]
