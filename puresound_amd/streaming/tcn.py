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
"""
from typing import Dict, List, Optional

import torch

from .. import hip
from .._abi import PS_NORM_AFFINE
from ..nnet.base_nn import _MASK_ACTS, SoTaskWrapModule
from ..nnet.conv_tasnet import TCN, ConvTasNet
from ..nnet.lobe.encoder import FreeEncDec
from ..nnet.lobe.norm import ChanLN, norm_plan
from .spectral import StreamingSeparator

#: frames per launch at most: step_chunk splits longer chunks (the rings hold (P-1)*dilation + K_MAX frames)
K_MAX = 16


def check_streamable(model) -> None:
    """Raise NotImplementedError naming the reason when `model` is not a configuration this streamer computes exactly."""
    name = "StreamingConvTasNet"
    if not isinstance(model, SoTaskWrapModule):
        raise NotImplementedError(f"{name}: a SoTaskWrapModule (got {type(model).__name__})")
    if not isinstance(model.encoder, FreeEncDec):
        raise NotImplementedError(f"{name}: encoder {type(model.encoder).__name__}: only the free encoder (FreeEncDec) streams "
                                  f"here; conv-STFT models stream through StreamingSeparator")
    win, hop = model.encoder.win_length, model.encoder.hop_length
    if win % hop:
        raise NotImplementedError(f"{name}: win = {win} is not a multiple of hop = {hop}")
    if win % 4 or win > 256:
        raise NotImplementedError(f"{name}: win = {win}: a multiple of 4 up to 256 (the window queue moves in float4 "
                                  f"columns, the decoder keeps a window per stream in LDS)")
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
    pair = (model.mask_type.lower(), model.f_type.lower())
    if pair != ("real", "real"):
        raise NotImplementedError(f"{name}: mask pairing {pair}: the free encoder uses (real, real) only")
    if model.mask_constraint.lower() not in _MASK_ACTS:
        raise NotImplementedError(f"{name}: mask_constraint {model.mask_constraint!r}")
    if model.output_constraint.lower() not in ("linear", "sigmoid"):
        raise NotImplementedError(f"{name}: output_constraint {model.output_constraint!r}: linear or sigmoid")
    for blk in (b for stack in m.tcn_list for b in stack):
        dsc = blk.dconv[0]
        if any(a.weight.numel() != 1 for a in (blk.in_conv[2], dsc.depthwise[2], dsc.pointwise[2])):
            raise NotImplementedError(f"{name}: PReLU with per-channel slopes is not on the HIP path")
    devs = {t.device.type for t in list(model.parameters()) + list(model.buffers())}
    if devs != {"cuda"}:
        raise NotImplementedError(f"{name}: the model's tensors are on {sorted(devs)}; streaming runs on a ROCm device only "
                                  f"(move the model with .to(device))")


class StreamingConvTasNet:
    """Hop-by-hop inference of a causal Conv-TasNet separator / speaker extractor for B streams (see the module docstring).

    s = StreamingConvTasNet(model); s.init_streams(B, enroll); s.step(hop [B, hop]) -> [B, hop] or None while the first
    window fills; s.step_chunk([B, k*hop]) -> what k step() calls return, concatenated; s.flush() -> the last win - hop
    samples.
    """

    def __init__(self, model: SoTaskWrapModule):
        check_streamable(model)
        if model.training:
            raise RuntimeError("StreamingConvTasNet: the model is in training mode -- call .eval()")
        self.model = model
        enc = model.encoder
        self.win_length, self.hop_length = int(enc.win_length), int(enc.hop_length)
        self.n_fft = self.win_length       # (the analysis window, under the name the shared helpers read)
        self.prime_hops = self.win_length // self.hop_length - 1
        self._mask_act = model.mask_constraint.lower()
        self._out_mode = model.output_constraint.lower()
        self.streams = None
        self._drop_weights()

    @property
    def latency_samples(self) -> int:
        """Samples between a sample entering and its value leaving: the analysis window minus one hop."""
        return self.win_length - self.hop_length

    output_length = staticmethod(StreamingSeparator.output_length)

    # -- weights ------------------------------------------------------------------------------------------------------
    _signature = StreamingSeparator._signature
    _check_parameters = StreamingSeparator._check_parameters

    def _drop_weights(self) -> None:
        """Forget graphs and weight packs (they are rebuilt from the current parameters on next use)."""
        self._graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self._packs = None
        self._sig = self._signature()

    def _build_packs(self, dev: torch.device) -> None:
        """Weights packed for the kernels (eval BatchNorm1d folded to scale / shift), held by the streamer: a captured
        graph keeps reading these tensors."""
        f32 = dict(dtype=torch.float32, device=dev)
        enc = self.model.encoder
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
        self._packs = dict(enc_wt=hip.pack_wt(enc.encoder.weight.detach().to(**f32)[:, 0, :]),
                           dec_w=enc.decoder.weight.detach().to(**f32).contiguous(), blocks=blocks)

    # -- session ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def init_streams(self, streams: int = 1, enroll: Optional[torch.Tensor] = None, use_graph: bool = True) -> None:
        """Start `streams` new streams (every state zeroed).  enroll [streams, L'] on the model's device: the enrolment of
        each stream, required iff the model has a speaker_net; its embedding is computed here, once."""
        if int(streams) < 1:
            raise ValueError("init_streams: streams >= 1")
        model, m = self.model, self.model.masker
        if (enroll is not None) != (model.speaker_net is not None):
            raise ValueError("StreamingConvTasNet.init_streams: an enrolment [streams, L'] is required iff the model has a "
                             "speaker_net")
        self._check_parameters()
        self._graphs = {}
        dev = next(model.parameters()).device
        b = int(streams)
        self._emb = None
        if enroll is not None:
            hip.require_device(enroll, "StreamingConvTasNet.init_streams")
            if enroll.dim() != 2 or enroll.shape[0] != b:
                raise ValueError(f"StreamingConvTasNet.init_streams: enroll must be [{b}, L'], got {tuple(enroll.shape)}")
            if any(m.tcn_with_embed):
                dvec = model.inference_tse_embedding(enroll)[..., 0].float().contiguous()   # [B, E]
                self._emb = hip.l2_normalize(dvec) if m.embed_norm else dvec
        self.streams, self.device, self._use_graph = b, dev, bool(use_graph)
        self._hops = 0
        self.frames = 0
        self._finished = False
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        self._blocks: List[TCN] = [blk for stack in m.tcn_list for blk in stack]
        # one circular ring of activated depthwise inputs per block: (P-1)*dilation frames of history plus a chunk
        self._rings = [z((blk.kernel - 1) * blk.dilation + K_MAX, blk.hid_channels, b) for blk in self._blocks]
        self._queue = z(b, self.win_length)
        self._tail = z(b, self.win_length - self.hop_length)
        self._counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self._io: Dict[int, tuple] = {}
        self._bufs: Dict[int, dict] = {}

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
            self._bufs[hops] = dict(n=n, ld=ld, res=res, y1=z(h), a1=z(h), y2=z(h), a2=z(h), y3=z(h), a3=z(h))
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
                             out=bufs["y2"])
        src, pro = settle(y2, "dw", bufs["a2"])
        y3, _ = hip.conv1x1(src, n, p["pw_wt"], h, pro, p["pw_b"], out=bufs["y3"])
        src, pro = settle(y3, "pw", bufs["a3"])
        hip.conv1x1(src, n, p["out_wt"], c, pro, p["out_b"], res=x[:, :c], out=out[:, :c])

    def _body(self, hops: int) -> None:
        """`hops` frames of every stream: input _io[hops][0] [B, hops*hop] -> output _io[hops][1] [B, hops*hop]."""
        chunk, out, wins = self._io[hops]
        hop, win, pk = self.hop_length, self.win_length, self._packs
        bufs = self._buffers(hops)
        c, n = self.model.masker.input_dim, bufs["n"]
        feats, x0, x1 = bufs["res"]
        hip.stream_windows(self._queue, chunk, wins, hop)
        frames, _ = hip.frame(wins.view(1, -1), win, win)               # [1, win, ld]: column f*B + b
        hip.conv1x1(frames, n, pk["enc_wt"], c, out=feats[:, :c])
        if self.model.encoder.output_active:
            hip.activation_(feats[:, :c], "relu", None, n)
        x = feats
        for i, p in enumerate(pk["blocks"]):
            y = x0 if i % 2 == 0 else x1
            self._block(i, p, x, y, bufs, hops)
            x = y
        hip.free_decode_step(feats[:, :c], x[:, :c], pk["dec_w"], self._tail, out, hop, hops, self._mask_act, self._out_mode)
        hip.stream_commit_frames(hip.commit_table([(wins[hops - 1], self._queue)]), self._counter, hops, self.device)

    def _run_piece(self, piece: torch.Tensor) -> torch.Tensor:
        """At most K_MAX whole hops past the priming -> their output samples [B, hops*hop] (graph replay or eager)."""
        hops = piece.shape[1] // self.hop_length
        if hops not in self._io:
            z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.device)  # noqa: E731
            self._io[hops] = (z(self.streams, piece.shape[1]), z(self.streams, piece.shape[1]),
                              z(hops, self.streams * self.win_length))
        self._io[hops][0].copy_(piece)
        if not self._use_graph:
            self._body(hops)
        else:
            g = self._graphs.get(hops)
            if g is None:
                g = self._capture(hops)
            g.replay()
        self._hops += hops
        self.frames += hops
        return self._io[hops][1].clone()

    def _run(self, chunk: torch.Tensor) -> torch.Tensor:
        """Whole hops past the priming -> their output samples, in pieces of at most K_MAX hops."""
        self._check_parameters()
        if self._packs is None:
            self._build_packs(self.device)
        step = K_MAX * self.hop_length
        outs = [self._run_piece(chunk[:, i:i + step]) for i in range(0, chunk.shape[1], step)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)

    def _capture(self, hops: int) -> torch.cuda.CUDAGraph:
        """Warm up once eagerly on a side stream (allocates what the launches need), put the state back, capture."""
        state = self._state()
        saved = [t.clone() for t in state]
        dev = self.device
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            self._body(hops)
        torch.cuda.current_stream(dev).wait_stream(s)
        for t, v in zip(state, saved):
            t.copy_(v)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._body(hops)
        self._graphs[hops] = g
        return g

    _prime = StreamingSeparator._prime

    def _check_input(self, x: torch.Tensor, what: str) -> int:
        if self.streams is None:
            raise RuntimeError(f"StreamingConvTasNet.{what}: call init_streams() first")
        if self._finished:
            raise RuntimeError(f"StreamingConvTasNet.{what}: the streams were flushed; call init_streams() for new ones")
        hip.require_device(x, f"StreamingConvTasNet.{what}")
        if x.dim() != 2 or x.shape[0] != self.streams or x.shape[1] % self.hop_length:
            raise ValueError(f"StreamingConvTasNet.{what}: expected [{self.streams}, k * {self.hop_length}] samples, "
                             f"got {tuple(x.shape)}")
        return x.shape[1] // self.hop_length

    @torch.no_grad()
    def step(self, hop: torch.Tensor) -> Optional[torch.Tensor]:
        """hop [B, hop_length] new samples per stream -> [B, hop_length] output samples, or None while the first analysis
        window fills (the first win / hop - 1 hops)."""
        if self._check_input(hop, "step") != 1:
            raise ValueError(f"StreamingConvTasNet.step: one hop of {self.hop_length} samples per stream")
        if self._hops < self.prime_hops:
            self._prime(hop)
            return None
        return self._run(hop)

    @torch.no_grad()
    def step_chunk(self, chunk: torch.Tensor) -> torch.Tensor:
        """chunk [B, k*hop_length] -> what k step() calls return, concatenated ([B, 0] when every hop only primes)."""
        k = self._check_input(chunk, "step_chunk")
        i = 0
        while i < k and self._hops < self.prime_hops:
            self._prime(chunk[:, i * self.hop_length:(i + 1) * self.hop_length])
            i += 1
        if i == k:
            return chunk.new_zeros(self.streams, 0)
        return self._run(chunk[:, i * self.hop_length:])

    @torch.no_grad()
    def flush(self) -> torch.Tensor:
        """The last win - hop_length samples of every stream ([B, win - hop_length]); the streams are then finished."""
        if self.streams is None or self._finished:
            raise RuntimeError("StreamingConvTasNet.flush: no open streams")
        if self.frames == 0:
            raise RuntimeError(f"StreamingConvTasNet.flush: no complete frame yet (a stream needs {self.win_length} samples)")
        self._check_parameters()
        if self._packs is None:
            self._build_packs(self.device)
        out = torch.empty(self.streams, self.win_length - self.hop_length, dtype=torch.float32, device=self.device)
        hip.free_decode_step(None, None, self._packs["dec_w"], self._tail, out, self.hop_length, out_mode=self._out_mode,
                             flush=True)
        self._finished = True
        return out
