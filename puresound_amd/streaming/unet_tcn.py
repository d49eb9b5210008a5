"""Streaming the causal conv-STFT U-Net with a gated-TCN bottleneck and a speaker branch (egs/tse tse_unet_tcn_v0_causal:
ConvEncDec 512 / 128 + UnetTcn with eval bN2d, causal GatedTCN blocks with bN1d, a 192-dim embedding) on the HIP path, one
hop at a time for B concurrent streams.

The model is causal with a fixed delay.  Down convolutions are padded on the left only, the gated blocks' dense dilated
convolutions likewise, every norm is an affine map in eval mode and the embedding is fixed for the session.  With
transpose_delay=True each of the n transposed convolutions (2 frames in time) trims its FIRST output frame, not its last:
frame t of its output reads frames t and t + 1 of its input, one frame of lookahead per layer.  So mask frame t is final once
frame t + D has come in, D = n (6 at the preset: "Lookahead(samples): 1152" = 384 of the STFT window + 6 x 128), and the
samples a stream returns, followed by flush(), equal `model.inference(x, enroll)` on the whole signal, D hops later than a
delay-free model would return them.  transpose_delay=False is the same class with D = 0.

Layout and front end are StreamingSeparator's (spectral.py): the B streams are the frame axis of the library's channel-major
rows, analysis / mask / synthesis / overlap-add are ps_stream_windows_f32, ps_frame_f32, the STFT GEMMs, ps_real_mask_f32 and
ps_istft_step_f32, the down path is ps_conv2d_step_f32 with shift rings.  The bottleneck is per block ps_conv1x1_f32
(in_conv), ps_gated_tcn_step_f32 (both dense dilated convolutions from one pass over the taps, the norms, the gate; history
from a circular ring per block indexed by the device frame counter; the embedding as per-tap constants `emb_taps`, computed
once per session, that count only for taps whose frame is >= 0 -- offline the embedding rows are zero-padded with the other
channels) and ps_conv1x1_f32 (out_conv + residual).

The up path needs no kernel of its own, only a schedule.  At hop s layer j (0-based) computes
    act(bias + W0 . in<s> + W1 . in<s-1>),   in = cat(x_j, skip_j),
which is frame s - j - 1 of its offline output: x_0<s> is the TCN's frame s, x_j<s> is layer j-1's result of this hop, and
skip_j<s> is frame s - j of down layer n-1-j, read from that tensor's ring of j + 1 frames: slot R - j is passed to
ps_conv2d_step_f32 as the "current" tensor and the ring shortened to R - j slots as its history.  The features the mask
multiplies come from a ring of D frames in the same way.  The first D computed frames emit nothing (HopSession's mute
hops); the frames a layer computes for s - j - 1 < 0 are the offline trimmed frames, and they only ever feed other trimmed
frames.  flush() runs D more hops on the host: at flush hop i layers j < i are skipped (their last frame is out), layer i
reads an all-zero "current" input (offline, frame T of its input is the transposed convolution's own zero, not a computed
frame) and layers j > i run as usual; then the overlap-add tail is flushed.

Two device counters: `_counter` counts computed frames and indexes the TCN rings; `_synth` counts synthesised frames
(computed - D) and is the frame index of ps_istft_step_f32.  No launch argument depends on either, so one captured graph per
chunk length replays every chunk (the D mute hops of a session run eagerly).

Arithmetic: exact fp32 products throughout, whatever the model's gemm_precision.  The streamer packs its own weights, so the
model's own setting and plans are left as they were.  The embedding is computed once per stream by the model's speaker
branch (inference_tse_embedding) in the model's own arithmetic, l2-normalised when embed_norm; a deployment may cache it and
pass `embed=`.

Slots (init_slots / open / end / close, HopSession's): streams that join and leave a running session.  One rule, and no new
state: frame g of a tensor is read as an exact 0 for stream b unless birth_b <= g < death_b, and up layer j runs j frames
behind the hop.  The kernels are the *_slots_f32 variants (ps_conv2d_step_slots_f32, ps_gated_tcn_step_slots_f32,
ps_istft_step_slots_f32) with the session's span [B, 2] and one counter: the down path and the TCN launch with shift 0, up
layer j with shift j (its "current" tensors are frame counter - j), the synthesis with shift D.  What the block session
does on the host falls out of the rule per stream: a slot's frames before its birth are the offline zero padding and trimmed
frames; at the i-th hop after its death layers j < i see only dead frames (skipped), layer i reads a dead (zero) current
frame and layers j > i run as usual -- the flush schedule -- while its neighbours go on streaming.  So a slot session has
no priming, no mute hops, no flushing pass and no second counter, one commit per hop, and step() returns [capacity, hop]
from the first hop on; a slot's last D frames leave in the D hops after its last input hop, then close() flushes its tail.
open() writes the slot's column of every emb_taps in place (computed over MIN_GEMM_COLUMNS columns: the bits of a
one-stream session) and clears no ring: dead frames are never read, whatever they hold.  A slot's samples are the bits of the
block session of its stream at the session's width: the 1x1 convolutions run over `capacity` columns, as init_streams(B)
runs them over B, and ps_conv1x1_f32 has one kernel up to 16 columns and other orders of summation beyond, so up to a capacity
of 16 a slot equals an init_streams(1, ...) session of its stream and in a wider session its row of init_streams(capacity).
"""
from typing import List, Optional

import torch
import torch.nn as nn

from .. import hip
from .._abi import PS_NORM_AFFINE
from ..nnet.base_nn import _MASK_ACTS, SoTaskWrapModule
from ..nnet.conv_tasnet import GatedTCN
from ..nnet.lobe.encoder import ConvEncDec
from ..nnet.lobe.norm import norm_plan
from ..nnet.unet import UnetTcn
from ._session import HopSession, check_on_device
from .dprnn import MIN_GEMM_COLUMNS

NAME = "StreamingUnetTcn"


def _ring_pairs(m: UnetTcn) -> int:
    """Ring pairs one hop commits: every tensor a convolution reads at earlier frames (a skip also at its layer's shift), the
    delayed features, the window queue."""
    n = m.n_cnn
    delayed = bool(m.transpose_delay) and m.t_kernel > 1
    hist = {}
    for i in range(n):
        src = "in" if i == 0 else f"d{i - 1}"
        hist[src] = max(hist.get(src, 0), (m.kernel[i][1] - 1) * m.dilation[i][1])
    for j, i in enumerate(reversed(range(n))):
        back = (m.t_kernel - 1) * m.dilation[i][1]
        src = "mid" if j == 0 else f"u{j - 1}"
        hist[src] = max(hist.get(src, 0), back)
        hist[f"d{i}"] = max(hist.get(f"d{i}", 0), back + (j if delayed else 0))
    return sum(h > 0 for h in hist.values()) + (1 if delayed else 0) + 1


def check_streamable(model) -> None:
    """Raise NotImplementedError naming the reason when `model` is not a configuration this streamer computes exactly."""
    if not isinstance(model, SoTaskWrapModule):
        raise NotImplementedError(f"{NAME}: a SoTaskWrapModule (got {type(model).__name__})")
    if not isinstance(model.encoder, ConvEncDec):
        raise NotImplementedError(f"{NAME}: encoder {type(model.encoder).__name__}: only the conv-STFT encoder (ConvEncDec) "
                                  f"streams here; free-encoder models stream through StreamingConvTasNet")
    stft = model.encoder.encoder
    if stft.n_fft % stft.stride:
        raise NotImplementedError(f"{NAME}: n_fft = {stft.n_fft} is not a multiple of hop = {stft.stride}")
    if not hasattr(stft, "kernel_sin_inv"):
        raise NotImplementedError(f"{NAME}: the encoder has no iSTFT (iSTFT=False)")
    m = model.masker
    if type(m) is not UnetTcn:
        raise NotImplementedError(f"{NAME}: masker {type(m).__name__}: UnetTcn only (DPCRN / DPARN stream through "
                                  f"StreamingSeparator)")
    if not m.causal:
        raise NotImplementedError(f"{NAME}: the TCN is not causal (causal=False: centred convolutions read future frames)")
    if m.tcn_layer.lower() != "gated":
        raise NotImplementedError(f"{NAME}: tcn_layer {m.tcn_layer!r}: only the gated block streams here")
    if m.tcn_use_film:
        raise NotImplementedError(f"{NAME}: tcn_use_film=True: FiLM conditioning of the gated blocks does not stream (the "
                                  f"embedding is concatenated in every causal preset)")
    if m.tcn_norm != "bN1d":
        raise NotImplementedError(f"{NAME}: tcn_norm {m.tcn_norm!r}: only bN1d (an affine map in eval mode) is causal frame "
                                  f"by frame")
    if m.norm_type.lower() != "bn2d":
        raise NotImplementedError(f"{NAME}: norm_type {m.norm_type!r}: only bN2d (an affine map in eval mode) is causal frame "
                                  f"by frame")
    if m.skip_conv:
        raise NotImplementedError(f"{NAME}: skip_conv=True")
    if any(d != 0 for d in m.delay):
        raise NotImplementedError(f"{NAME}: delay {tuple(m.delay)}: a delayed down convolution is a lookahead this streamer "
                                  f"does not schedule")
    if any(st != 1 for _, st in m.stride):
        raise NotImplementedError(f"{NAME}: stride_t must be 1")
    for (kf, kt), (df, dt) in zip(m.kernel, m.dilation):
        if (kt - 1) * (dt - 1):
            raise NotImplementedError(f"{NAME}: a down convolution with kernel_t = {kt}, dilation_t = {dt} pads {kt - 1} "
                                      f"frames on the left and reads {(kt - 1) * (dt - 1)} future frames (not causal)")
    if m.transpose_delay and m.t_kernel > 1 and (m.t_kernel != 2 or any(dt != 1 for _, dt in m.dilation)):
        raise NotImplementedError(f"{NAME}: transpose_delay=True with transpose_t_size = {m.t_kernel}, dilation_t = "
                                  f"{tuple(dt for _, dt in m.dilation)}: the delayed schedule is one frame per layer "
                                  f"(transpose_t_size 2, dilation_t 1)")
    pair = (model.mask_type.lower(), model.f_type.lower())
    if pair != ("real", "real"):
        raise NotImplementedError(f"{NAME}: mask pairing {pair}: (real, real) only")
    if model.mask_constraint.lower() not in _MASK_ACTS:
        raise NotImplementedError(f"{NAME}: mask_constraint {model.mask_constraint!r}")
    if model.output_constraint.lower() not in ("linear", "sigmoid"):
        raise NotImplementedError(f"{NAME}: output_constraint {model.output_constraint!r}: linear or sigmoid")
    if model.embedding_free_tse:
        raise NotImplementedError(f"{NAME}: embedding_free_tse (the enrolment seeds the masker) does not stream")
    if any(m.tcn_with_embed) and m.embed_dim > 0 and model.speaker_net is None:
        raise NotImplementedError(f"{NAME}: tcn_with_embed blocks without a speaker_net to compute the embedding")
    if m.activation_type.lower() not in ("prelu", "relu"):
        raise NotImplementedError(f"{NAME}: activation {m.activation_type!r}: PReLU or ReLU")
    acts = [mod for seq in list(m.cnn_down) + list(m.cnn_up) for mod in seq]
    acts += [blk.left_conv[2] for stack in m.tcn_list for blk in stack] + [blk.right_conv[2] for stack in m.tcn_list for blk in stack]
    if any(isinstance(a, nn.PReLU) and a.weight.numel() != 1 for a in acts):
        raise NotImplementedError(f"{NAME}: PReLU with per-channel slopes is not on the HIP path")
    ch0 = 2 if m.input_type.lower() == "ri" else 1
    bins = stft.freq_bins if stft.freq_bins is not None else stft.wcos.shape[0]
    rows = 2 * (bins - (1 if model.drop_first_bin else 0))
    if ch0 * m.num_freq != rows or m.channels[0] != ch0:
        raise NotImplementedError(f"{NAME}: the masker reads {ch0} x {m.num_freq} rows, the encoder gives {rows}")
    if _ring_pairs(m) > hip._abi.PS_MAX_RING_PAIRS:
        raise NotImplementedError(f"{NAME}: {_ring_pairs(m)} ring pairs per hop, more than one commit launch takes "
                                  f"({hip._abi.PS_MAX_RING_PAIRS})")
    check_on_device(model, NAME)


class StreamingUnetTcn(HopSession):
    """Hop-by-hop inference of the causal U-Net + gated-TCN speaker extractor for B streams (see the module docstring).

    s = StreamingUnetTcn(model); s.init_streams(B, enroll=e [B, L']) or s.init_streams(B, embed=d [B, E]);
    s.step(hop [B, hop]) -> [B, hop], or None for the first prime_hops hops (the analysis window fills, then the model's
    delay_frames pass); s.step_chunk([B, k*hop]) -> what k step() calls return, concatenated; s.flush() -> the last
    latency_samples samples.

    Streams that join and leave: s.init_slots(capacity); s.open(slot, enroll=e [L']) or s.open(slot, embed=d [E]);
    s.step / s.step_chunk([capacity, k*hop]) -> [capacity, k*hop] from the first hop on (an idle slot: constrain(0));
    s.end(slot, hops) when the stream has `hops` more hops of input, delay_frames more hops of the session (they carry the
    stream's last frames out; its input in them is ignored), then s.close(slot) -> the last window - hop samples.
    """

    _flushing = False    # True inside flush(): the first layer _up_path runs reads an all-zero current frame

    def __init__(self, model: SoTaskWrapModule):
        check_streamable(model)
        stft, m = model.encoder.encoder, model.masker
        delay = m.n_cnn if (m.transpose_delay and m.t_kernel > 1) else 0
        super().__init__(model, stft.n_fft, stft.stride, delay_frames=delay)
        self.n_fft = self.window

    # -- weights ------------------------------------------------------------------------------------------------------
    def _build_packs(self, dev: torch.device) -> None:
        """Conv weights (eval BatchNorm folded), the gated blocks' two dense weights in GEMM layout and the STFT tables, held
        by the streamer: a captured graph keeps reading these tensors."""
        model, m = self.model, self.model.masker
        stft = model.encoder.encoder
        f32 = dict(dtype=torch.float32, device=dev)
        wt_a, rows = stft._analysis_plan(model.drop_first_bin)
        wt_s, window = stft._synthesis_plan(model.drop_first_bin)
        p = m._build_unet(dev)
        blocks = []
        for blk in (b for stack in m.tcn_list for b in stack):
            h = blk.hid_channels
            w_right = blk.right_conv[0].weight.detach().to(**f32)                  # [H, H + E, P]
            q = dict(P=blk.kernel, dilation=blk.dilation, H=h, E=blk.emb_dim,
                     in_wt=hip.pack_wt(blk.in_conv.weight.detach().to(**f32)),
                     wl=hip.pack_wt(GatedTCN._unfolded(blk.left_conv[0].weight.detach().to(**f32))),
                     wr=hip.pack_wt(GatedTCN._unfolded(w_right[:, :h, :].contiguous())),
                     emb_w=[w_right[:, h:, j].contiguous() for j in range(blk.kernel)] if blk.emb_dim > 0 else None,
                     out_wt=hip.pack_wt(blk.out_conv.weight.detach().to(**f32)))
            for side, seq in (("left", blk.left_conv), ("right", blk.right_conv)):
                kind, g, b = norm_plan(seq[1])
                assert kind == PS_NORM_AFFINE
                q[side] = (g.to(**f32).contiguous(), b.to(**f32).contiguous(), seq[2].weight.detach().to(**f32).contiguous())
                q["pro_" + side] = hip.make_prologue(PS_NORM_AFFINE, True, None, 0.0, 1e-8, *q[side])
            blocks.append(q)
        self._packs = dict(wt_a=wt_a, rows=rows, wt_s=wt_s, window=window, down=p["down"], up=p["up"], blocks=blocks)
        if getattr(self, "_emb_taps", None) is not None and self._slots is not None:
            for slot, emb in enumerate(self._slot_embeds):     # a running slot session: every open slot's column, in place
                if emb is not None:
                    self._write_taps(slot, emb)
        elif getattr(self, "_emb_taps", None) is not None:     # a running session: its constants are those of the old weights
            self._emb_taps = [self._tap_constants(q, self._emb, self.streams) if (q["E"] > 0 and self._emb is not None) else None
                              for q in blocks]

    # -- session ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def init_streams(self, streams: int = 1, enroll: Optional[torch.Tensor] = None, embed: Optional[torch.Tensor] = None,
                     use_graph: bool = True) -> None:
        """Start `streams` new streams (every state zeroed).  A model with a speaker_net takes exactly one of enroll
        [streams, L'] (through model.inference_tse_embedding, here, once) and embed [streams, E] or [streams, E, 1] (what
        that call returns; a deployment caches it), on the model's device; a model without one takes neither."""
        name = f"{NAME}.init_streams"
        if int(streams) < 1:
            raise ValueError("init_streams: streams >= 1")
        model, m = self.model, self.model.masker
        b = int(streams)
        dev = next(model.parameters()).device
        takes = model.speaker_net is not None
        if takes and (enroll is None) == (embed is None):
            raise ValueError(f"{name}: the model has a speaker_net: pass exactly one of enroll [streams, L'] and embed "
                             f"[streams, {m.embed_dim}]")
        if not takes and (enroll is not None or embed is not None):
            raise ValueError(f"{name}: the model has no speaker_net: pass neither enroll nor embed")
        if enroll is not None:
            hip.require_device(enroll, name)
            if enroll.dim() != 2 or enroll.shape[0] != b:
                raise ValueError(f"{name}: enroll must be [{b}, L'], got {tuple(enroll.shape)}")
            embed = model.inference_tse_embedding(enroll)
        emb = None
        if embed is not None:
            hip.require_device(embed, name)
            if embed.dim() == 3 and embed.shape[2] == 1:               # (as inference_tse_embedding returns it)
                embed = embed[:, :, 0]
            if tuple(embed.shape) != (b, m.embed_dim) or embed.device != dev:
                raise ValueError(f"{name}: embed must be [{b}, {m.embed_dim}] on {dev}, got {tuple(embed.shape)} on "
                                 f"{embed.device}")
            if any(m.tcn_with_embed) and m.embed_dim > 0:
                emb = embed.detach().float().contiguous()
                emb = hip.l2_normalize(emb) if m.embed_norm else emb
        self._emb_taps = None
        self._begin(b, dev, use_graph)
        self._ready()
        self._allocate(b, dev, emb)

    @torch.no_grad()
    def init_slots(self, capacity: int, use_graph: bool = True) -> None:
        """Start a slot session of `capacity` columns, every slot idle (every state and every tap constant zeroed); open()
        starts a stream."""
        if int(capacity) < 1:
            raise ValueError("init_slots: capacity >= 1")
        b, dev = int(capacity), next(self.model.parameters()).device
        self._emb_taps = None
        self._begin(b, dev, use_graph)
        self._make_slots()
        self._ready()
        self._slot_embeds = [None] * b                   # per slot the (normalised) embedding [1, E] its stream was opened with
        self._allocate(b, dev, None)

    def _enrolment_rule(self) -> tuple:
        e = self.model.masker.embed_dim
        if self.model.speaker_net is not None:
            return True, f"the model has a speaker_net: pass exactly one of enroll [L'] and embed [{e}]"
        return False, "the model has no speaker_net: pass neither enroll nor embed"

    @torch.no_grad()
    def open(self, slot: int, enroll: Optional[torch.Tensor] = None, embed: Optional[torch.Tensor] = None) -> None:
        """Start a stream in the idle slot `slot`: its first input hop is the first hop of the next step / step_chunk call.
        A model with a speaker_net takes exactly one of enroll [L'] or [1, L'] (through model.inference_tse_embedding, here,
        once) and embed [E], [1, E] or [1, E, 1] (what that call returns; a deployment caches it), on the session's device; a
        model without one takes neither.  No synchronisation, no captured graph is touched, no ring is cleared."""
        name = f"{type(self).__name__}.open"
        slot = self._slot(slot, "open", idle=True)
        required, why = self._enrolment_rule()
        if (enroll is not None) + (embed is not None) != int(required):
            raise ValueError(f"{name}: {why}")
        if enroll is not None:
            enroll = self._one_enrolment(enroll, name)
        if embed is not None:
            e = self.model.masker.embed_dim
            hip.require_device(embed, name)
            if embed.device != self.device:
                raise RuntimeError(f"{name}: the embedding is on {embed.device}, the session on {self.device}; move it with "
                                   f".to({str(self.device)!r})")
            if tuple(embed.shape) not in ((e,), (1, e), (1, e, 1)):
                raise ValueError(f"{name}: embed must be [{e}], [1, {e}] or [1, {e}, 1] (one stream), got {tuple(embed.shape)}")
            embed = embed.reshape(1, e)
        self._start_slot(slot, (enroll, embed), name)

    def _open_slot(self, slot: int, seed: tuple) -> None:
        """The new stream's tap constants into column `slot` of every block's emb_taps (computed here, once, as init_streams
        does for one stream).  Nothing is cleared: what the slot's predecessor left in the rings are dead frames."""
        m = self.model.masker
        enroll, embed = seed
        if enroll is not None:
            embed = self.model.inference_tse_embedding(enroll)[:, :, 0]
        self._ready()
        self._slot_embeds[slot] = None
        if embed is not None and any(m.tcn_with_embed) and m.embed_dim > 0:
            emb = embed.detach().float().contiguous()
            self._slot_embeds[slot] = hip.l2_normalize(emb) if m.embed_norm else emb.clone()
            self._write_taps(slot, self._slot_embeds[slot])

    def _write_taps(self, slot: int, emb: torch.Tensor) -> None:
        """Column `slot` of every block's emb_taps <- the constants of emb [1, E], the bits of a session of that one stream;
        in place: a captured graph keeps reading these tensors."""
        for q, taps in zip(self._packs["blocks"], self._emb_taps):
            if taps is not None:
                taps[:, :, slot] = self._tap_constants(q, emb, 1)[:, :, 0]

    def _allocate(self, b: int, dev: torch.device, emb: Optional[torch.Tensor]) -> None:
        """Geometry of every convolution (unet.py:219-281), the frame buffers, the rings and the embedding's tap constants."""
        m, pk = self.model.masker, self._packs
        n, D = m.n_cnn, self.delay_frames
        self._ldb = ldb = hip.padded_frames(b)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        ch0 = 2 if m.input_type.lower() == "ri" else 1
        shapes = {"in": (m.channels[0], m.num_freq)}
        self._down, self._up = [], []
        f = m.num_freq
        for i in range(n):
            (kf, kt), (sf, _), (df, dt) = m.kernel[i], m.stride[i], m.dilation[i]
            pf = kf // 2
            f_out = (f + 2 * pf - df * (kf - 1) - 1) // sf + 1
            self._down.append(dict(src="in" if i == 0 else f"d{i - 1}", f_out=f_out, kf=kf, kt=kt, sf=sf, df=df, dt=dt, pf=pf))
            f = f_out
            shapes[f"d{i}"] = (m.channels[i + 1], f)
        shapes["mid"] = shapes[f"d{n - 1}"]
        x = "mid"
        for j, i in enumerate(reversed(range(n))):
            (kf, _), (sf, _), (df, dt) = m.kernel[i], m.stride[i], m.dilation[i]
            pf = kf // 2
            op = sf - kf + 2 * pf
            f_out = (shapes[x][1] - 1) * sf - 2 * pf + df * (kf - 1) + op + 1
            # shift: how many frames behind the hop this layer's input runs (one per layer above it when transpose_delay)
            self._up.append(dict(src=x, skip=f"d{i}", f_out=f_out, kf=kf, kt=m.t_kernel, sf=sf, df=df, dt=dt, pf=pf,
                                 shift=j if D else 0))
            if j < n - 1:
                x = f"u{j}"
                shapes[x] = (m.channels[i], f_out)
        if (self._up[-1]["f_out"], pk["up"][-1]["M"]) != (m.num_freq, ch0):
            raise NotImplementedError(f"{NAME}: the decoder does not return the encoder's frequency rows")
        if shapes["mid"][0] * shapes["mid"][1] != m.temporal_input_dim:
            raise NotImplementedError(f"{NAME}: the bottleneck has {shapes['mid']} rows, the TCN takes {m.temporal_input_dim}")
        # history each tensor must keep: the most any convolution reading it needs (a skip also its layer's shift)
        hist = {k: 0 for k in shapes}
        for c in self._down:
            hist[c["src"]] = max(hist[c["src"]], (c["kt"] - 1) * c["dt"])
        for c in self._up:
            hist[c["src"]] = max(hist[c["src"]], (c["kt"] - 1) * c["dt"])
            hist[c["skip"]] = max(hist[c["skip"]], (c["kt"] - 1) * c["dt"] + c["shift"])
        self._in_shape = (1,) + shapes["in"] + (ldb,)
        self._mid_shape = (1,) + shapes["mid"] + (ldb,)
        self._cur = {k: z(1, ch, fr, ldb) for k, (ch, fr) in shapes.items() if k[0] == "d"}
        self._rings = {k: (z(r, *shapes[k], ldb) if r > 0 else None) for k, r in hist.items()}
        self._upout = [z(1, pk["up"][j]["M"], c["f_out"], ldb) for j, c in enumerate(self._up)]
        for j in range(n - 1):
            self._cur[f"u{j}"] = self._upout[j]
        # the features of the last D frames, for the mask of frame s - D
        self._feats = z(1, pk["rows"], ldb)
        self._feat_ring = z(D, pk["rows"], ldb) if D else None
        # the bottleneck: in_conv output, the gate's output, two alternating residual-stream buffers, a ring per block
        c_tcn, h = m.temporal_input_dim, m.tcn_dim
        self._y1, self._g, self._xbuf = z(1, h, ldb), z(1, h, ldb), [z(1, c_tcn, ldb), z(1, c_tcn, ldb)]
        self._tcn_rings = [z((q["P"] - 1) * q["dilation"] + 1, q["H"], b) for q in pk["blocks"]]
        self._emb = emb
        if self._slots is not None:     # (the launches read these tensors for as long as the session lasts: open() writes a column)
            self._emb_taps = [z(q["P"], q["H"], b) if q["E"] > 0 else None for q in pk["blocks"]]
        else:
            self._emb_taps = [self._tap_constants(q, emb, b) if (q["E"] > 0 and emb is not None) else None
                              for q in pk["blocks"]]
            if any(q["E"] > 0 for q in pk["blocks"]) and emb is None:
                raise ValueError(f"{NAME}.init_streams: the TCN has embedding blocks but no embedding was given")
        self._synth = torch.zeros(1, dtype=torch.int32, device=dev)

    def _tap_constants(self, q: dict, emb: torch.Tensor, b: int) -> torch.Tensor:
        """emb_taps [P, H, B] of one block: tap j of the right convolution applied to the embedding of every stream
        (ps_conv1x1_f32 over the streams as columns, at least MIN_GEMM_COLUMNS of them, so a stream's constants do not depend
        on B)."""
        cols = max(b, MIN_GEMM_COLUMNS)
        rows = torch.zeros(1, q["E"], hip.padded_frames(cols), dtype=torch.float32, device=self.device)
        rows[0, :, :b] = emb.t()
        taps = torch.empty(q["P"], q["H"], b, dtype=torch.float32, device=self.device)
        for j, w in enumerate(q["emb_w"]):
            out, _ = hip.conv1x1(rows, cols, hip.pack_wt(w), q["H"])
            taps[j] = out[0, :, :b]
        return taps

    def _state(self) -> List[torch.Tensor]:
        return ([self._queue, self._tail, self._counter, self._synth] + [r for r in self._rings.values() if r is not None]
                + ([self._feat_ring] if self._feat_ring is not None else []) + self._tcn_rings)

    # -- one hop ------------------------------------------------------------------------------------------------------
    def _down_tcn(self, feats: torch.Tensor) -> dict:
        """[1, rows, ldB] features of frame s -> {tensor name: this frame} with the down stack's outputs and the TCN's."""
        b, pk = self.streams, self._packs
        live = self._live(0)
        cur = dict(self._cur)
        cur["in"] = feats.view(self._in_shape)
        for i, (c, lay) in enumerate(zip(self._down, pk["down"])):
            hip.conv2d_step(cur[c["src"]], self._rings[c["src"]], None, None, lay["wt"], lay["bias"], lay["M"], b, c["f_out"],
                            c["kf"], c["kt"], c["sf"], c["df"], c["dt"], c["pf"], False, lay["act"], lay["slope"],
                            out=cur[f"d{i}"], **live)
        x = cur[f"d{len(self._down) - 1}"].view(1, -1, self._ldb)
        for i, q in enumerate(pk["blocks"]):
            hip.conv1x1(x, b, q["in_wt"], q["H"], out=self._y1)
            hip.gated_tcn_step(self._y1, self._tcn_rings[i], self._counter, q["wl"], q["wr"], q["P"], q["dilation"], b, 1,
                               q["pro_left"], q["pro_right"], self._emb_taps[i], out=self._g, span=self._span)
            y = self._xbuf[i % 2]
            hip.conv1x1(self._g, b, q["out_wt"], x.shape[1], res=x, out=y)
            x = y
        cur["mid"] = x.view(self._mid_shape)
        return cur

    def _up_path(self, cur: dict, first: int = 0) -> torch.Tensor:
        """The transposed convolutions from layer `first` on -> the mask [1, rows, ldB] of frame s - D.  first > 0 (flush):
        the layers before it are done, and layer `first` reads an all-zero current frame."""
        b, pk = self.streams, self._packs
        for j, (c, lay) in enumerate(zip(self._up, pk["up"])):
            if j < first:
                continue
            x1, r1 = cur[c["src"]], self._rings[c["src"]]
            ring = self._rings[c["skip"]]
            sh = c["shift"]
            if sh:   # the skip's frame s - shift is ring slot R - shift; the slots before it are its history
                x2, r2 = ring[ring.shape[0] - sh:ring.shape[0] - sh + 1], ring[:ring.shape[0] - sh]
            else:
                x2, r2 = cur[c["skip"]], ring
            if self._flushing and j == first:
                x1, x2 = torch.zeros_like(x1), torch.zeros_like(x2)
            hip.conv2d_step(x1, r1, x2, r2, lay["wt"], lay["bias"], lay["M"], b, c["f_out"], c["kf"], c["kt"], c["sf"], c["df"],
                            c["dt"], c["pf"], True, lay["act"], lay["slope"], out=self._upout[j], **self._live(sh))
        return self._upout[-1].view(1, -1, self._ldb)

    def _live(self, shift: int) -> dict:
        """What a slot session adds to a ps_conv2d_step launch whose current tensors run `shift` frames behind the hop."""
        return {} if self._span is None else dict(counter=self._counter, span=self._span, shift=shift)

    def _synthesise(self, mask: torch.Tensor, out: torch.Tensor) -> None:
        """mask of frame s - D x the features of that frame -> its hop of samples (the iSTFT's frame index is _synth; in a
        slot session counter - D - the slot's birth)."""
        b, pk = self.streams, self._packs
        feats = self._feat_ring[0:1] if self._feat_ring is not None else self._feats
        enh = hip.real_mask(feats, mask, self._mask_act)
        syn, _ = hip.conv1x1(enh, b, pk["wt_s"], self.n_fft,
                             out=torch.empty(1, self.n_fft, self._ldb, dtype=torch.float32, device=self.device))
        if self._span is not None:
            hip.istft_step(syn, pk["window"], self._tail, out, self._counter, self.hop_length, self._out_mode, span=self._span,
                           shift=self.delay_frames)
        else:
            hip.istft_step(syn, pk["window"], self._tail, out, self._synth, self.hop_length, self._out_mode)

    def _pairs(self, cur: dict) -> list:
        pairs = [(cur[k], r) for k, r in self._rings.items() if r is not None]
        if self._feat_ring is not None:
            pairs.append((self._feats, self._feat_ring))
        return pairs

    def _body(self, hops: int) -> None:
        """`hops` hops of every stream: input _io[hops][0] [B, hops*hop] -> output _io[hops][1] [B, hops*hop] (self._mute:
        frames inside the model's delay -- no synthesis, the tail and _synth stay as they are)."""
        chunk, out, wins = self._io[hops]
        b, hop, pk = self.streams, self.hop_length, self._packs
        hip.stream_windows(self._queue, chunk, wins, hop)
        for i in range(hops):
            frames, _ = hip.frame(wins[i:i + 1], self.n_fft, self.n_fft)               # [1, n_fft, ldB]: streams = frames
            hip.conv1x1(frames, b, pk["wt_a"], pk["rows"], out=self._feats)
            cur = self._down_tcn(self._feats)
            mask = self._up_path(cur)
            queue = [(wins[i], self._queue)]
            if self._span is not None:     # a slot session: every hop synthesises, one commit, one counter
                self._synthesise(mask, out[:, i * hop:(i + 1) * hop])
                hip.stream_commit(hip.commit_table(self._pairs(cur) + queue), self._counter, self.device)
            elif self._mute:
                hip.stream_commit(hip.commit_table(self._pairs(cur) + queue), self._counter, self.device)
            else:
                self._synthesise(mask, out[:, i * hop:(i + 1) * hop])
                hip.stream_commit(hip.commit_table(self._pairs(cur)), self._counter, self.device)
                hip.stream_commit(hip.commit_table(queue), self._synth, self.device)

    def _flush_into(self, out: torch.Tensor) -> None:
        """The frames still inside the up path (D more hops, without input), then the overlap-add tail."""
        D, hop = self.delay_frames, self.hop_length
        held = min(self.frames, D)
        cur = dict(self._cur)      # (the rings keep shifting; what the down path and the TCN left here is never read again)
        cur["in"] = self._feats.view(self._in_shape)
        cur["mid"] = self._xbuf[(len(self._packs["blocks"]) - 1) % 2].view(self._mid_shape)
        self._flushing = True
        try:
            for i in range(D):
                mask = self._up_path(cur, first=i)
                e = i - (D - held)            # this hop synthesises frame frames + i - D: the e-th of the held ones
                if e >= 0:
                    self._synthesise(mask, out[:, e * hop:(e + 1) * hop])
                    hip.stream_commit(hip.commit_table(self._pairs(cur)), self._synth, self.device)
                else:
                    hip.stream_commit(hip.commit_table(self._pairs(cur)), None, self.device)
        finally:
            self._flushing = False
        hip.istft_step(None, self._packs["window"], self._tail, out[:, held * hop:], self._synth, hop, self._out_mode,
                       flush=True)

    def _flush_slot(self, out: torch.Tensor, slot: int) -> None:
        """close(): the tail of one slot, with the window sum of its own frames (B = 1 on its tail row and span row)."""
        hip.istft_step(None, self._packs["window"], self._tail[slot:slot + 1], out, self._counter, self.hop_length,
                       self._out_mode, flush=True, span=self._span[slot:slot + 1], shift=self.delay_frames)
