"""Streaming the causal conv-STFT U-Net maskers (DPCRN / DPARN: egs/ns ns_dpcrn_v0_causal, ns_dparn_v0_causal) on the HIP
path, one hop at a time for B concurrent streams.

The models are exactly causal in time (down convolutions padded (kt-1, 0), transposed convolutions trimmed at the end,
unidirectional inter LSTM, eval BatchNorm2d, intra passes within one frame, an STFT that does not pad the signal), so the
samples a stream returns, followed by flush(), equal `model.inference` on the whole signal: output samples
[t*hop, t*hop + hop) are final once frame t has been synthesised.

Layout: as StreamingSkiM, the B streams are the frame axis of the library's channel-major rows, so one hop of an offline
[N, CH, F, ld] activation is [1, CH, F, ldB], ldB = padded_frames(B), and most of the frame's work is the offline code with
t = B: the analysis / synthesis GEMMs of ConvSTFT, the intra LSTM / attention passes of the bottleneck blocks, the inter
LSTM with one step per sequence and carried states, the mask kernels.  New kernels (csrc/stream_step.hip) do what needs the
previous frames: ps_conv2d_step_f32 (a causal convolution frame, history from per-source rings), ps_istft_step_f32 (the
overlap-add with the offline window sum, edge frames included) and ps_stream_commit_f32 (rings, carried states and the window
queue advance by one frame, the device frame counter by one).  No launch argument depends on the frame index, so one captured
graph replays every hop; `step_chunk` captures one graph per chunk length.

Arithmetic: exact fp32 products throughout, whatever the model's gemm_precision.  The streamer keeps its own fp32 kernel
plans and swaps them into the masker's modules only while it builds or runs a hop, so the model's own setting and plans
are left as they were.
The session around the kernels (priming, step / step_chunk / flush, eager run or graph replay, the capture) is HopSession's:
streaming/_session.py.

Slots (init_slots / open / end / close, HopSession's): streams that join and leave a running session, with StreamingUnetTcn's
one rule and no new state: frame g of a tensor is read as an exact 0 for stream b unless birth_b <= g < death_b.  The down
path, the up path and the synthesis are the *_slots_f32 kernels (ps_conv2d_step_slots_f32, ps_istft_step_slots_f32) with the
session's span [B, 2], the one counter and shift 0: the model has no delay, a stream's last frame leaves with its last input
hop and close() may follow it directly.  The one tensor that remembers earlier frames outside a ring is the carried state of
the inter LSTM: the state a stream reads at frame t is "the tensor at frame t - 1", so ps_state_gate_slots_f32 (one launch at
the top of each hop, shift 1, all four states of both blocks) stores zeros into the columns whose frame t - 1 is dead -- zeros
at a stream's birth, as offline, and through the n_fft / hop - 1 hops between open() and the birth, in which the LSTM steps
on dead frames (a convolution of zeros plus its bias is not zero).  The gate is on the read side, not in the commit: the
commit advances the counter from one thread while its other workgroups copy, so nothing in that launch may read it.  So a
slot session has no priming and no flushing pass, open() clears nothing on the device but the slot's window queue and tail
row, and step() returns [capacity, hop] from the first hop on.  The intra passes work inside one frame of one stream and
need nothing.  A slot's samples are the bits of row `slot` of an init_streams(capacity) session fed its stream from frame
0: the reused GEMM and recurrence kernels pick their tiling from the column count, so the identity holds at the session's
width.
"""
import contextlib
from typing import List

import torch

from .. import hip
from ..nnet._plans import PlanCache, own_plans
from ..nnet.base_nn import _MASK_ACTS, SoTaskWrapModule
from ..nnet.dparn import DPARN
from ..nnet.dpcrn import DPCRN
from ..nnet.lobe.encoder import ConvEncDec
from ._session import HopSession, check_on_device


def check_streamable(model) -> None:
    """Raise NotImplementedError naming the reason when `model` is not a configuration this streamer computes exactly."""
    if not isinstance(model, SoTaskWrapModule):
        raise NotImplementedError(f"StreamingSeparator: a SoTaskWrapModule (got {type(model).__name__})")
    if not isinstance(model.encoder, ConvEncDec):
        raise NotImplementedError(f"StreamingSeparator: encoder {type(model.encoder).__name__}: only the conv-STFT encoder "
                                  f"(ConvEncDec) streams")
    stft = model.encoder.encoder
    if stft.n_fft % stft.stride:
        raise NotImplementedError(f"StreamingSeparator: n_fft = {stft.n_fft} is not a multiple of hop = {stft.stride}")
    if not hasattr(stft, "kernel_sin_inv"):
        raise NotImplementedError("StreamingSeparator: the encoder has no iSTFT (iSTFT=False)")
    if model.speaker_net is not None or model.embedding_free_tse:
        raise NotImplementedError("StreamingSeparator: no speaker_net / enrolment (target speech extraction does not stream)")
    pair = (model.mask_type.lower(), model.f_type.lower())
    if pair not in (("complex", "complex"), ("real", "real")):
        raise NotImplementedError(f"StreamingSeparator: mask pairing {pair}: (complex, complex) or (real, real) only")
    if model.mask_constraint.lower() not in _MASK_ACTS:
        raise NotImplementedError(f"StreamingSeparator: mask_constraint {model.mask_constraint!r}")
    if model.output_constraint.lower() not in ("linear", "sigmoid"):
        raise NotImplementedError(f"StreamingSeparator: output_constraint {model.output_constraint!r}: linear or sigmoid")
    m = model.masker
    if type(m) not in (DPCRN, DPARN):
        raise NotImplementedError(f"StreamingSeparator: masker {type(m).__name__}: DPCRN or DPARN only")
    if m.norm_type.lower() != "bn2d":
        raise NotImplementedError(f"StreamingSeparator: norm_type {m.norm_type!r}: only bN2d (an affine map in eval mode) is "
                                  f"causal frame by frame")
    if getattr(m, "spectral_compress", False) or m.multi_output != 1:
        raise NotImplementedError("StreamingSeparator: spectral_compress / multi_output maskers")
    if m.transpose_delay:
        raise NotImplementedError("StreamingSeparator: transpose_delay=True is a lookahead model (not causal)")
    if m.skip_conv:
        raise NotImplementedError("StreamingSeparator: skip_conv=True")
    if any(d != 0 for d in m.delay):
        raise NotImplementedError(f"StreamingSeparator: delay {tuple(m.delay)}: a delay is a lookahead (not causal)")
    if any(st != 1 for _, st in m.stride):
        raise NotImplementedError("StreamingSeparator: stride_t must be 1")
    for (kf, kt), (df, dt) in zip(m.kernel, m.dilation):
        if (kt - 1) * (dt - 1):
            raise NotImplementedError(f"StreamingSeparator: a down convolution with kernel_t = {kt}, dilation_t = {dt} pads "
                                      f"{kt - 1} frames on the left and reads {(kt - 1) * (dt - 1)} future frames (not causal)")
    if m.activation_type.lower() not in ("prelu", "relu"):
        raise NotImplementedError(f"StreamingSeparator: activation {m.activation_type!r}: PReLU or ReLU")
    ch0 = 2 if m.input_type.lower() == "ri" else 1
    bins = stft.freq_bins if stft.freq_bins is not None else stft.wcos.shape[0]
    rows = 2 * (bins - (1 if model.drop_first_bin else 0))
    if ch0 * m.num_freq != rows or m.channels[0] != ch0:
        raise NotImplementedError(f"StreamingSeparator: the masker reads {ch0} x {m.num_freq} rows, the encoder gives {rows}")
    check_on_device(model, "StreamingSeparator")


class StreamingSeparator(HopSession):
    """Hop-by-hop inference of a causal DPCRN / DPARN noise suppressor for B streams (see the module docstring).

    s = StreamingSeparator(model); s.init_streams(B); s.step(hop [B, hop]) -> [B, hop] or None while the analysis window
    fills; s.step_chunk([B, k*hop]) -> what k step() calls return, concatenated; s.flush() -> the last n_fft - hop samples.

    Streams that join and leave: s.init_slots(capacity); s.open(slot); s.step / s.step_chunk([capacity, k*hop]) ->
    [capacity, k*hop] from the first hop on (an idle slot: constrain(0), whatever its input row holds); s.end(slot, hops)
    when the stream has `hops` more hops of input; s.close(slot) -> the last n_fft - hop samples.
    """

    def __init__(self, model: SoTaskWrapModule):
        check_streamable(model)
        stft = model.encoder.encoder
        self._plan_mods = [m for m in model.masker.modules() if isinstance(m, PlanCache)]
        super().__init__(model, stft.n_fft, stft.stride)
        self.n_fft = self.window
        self._pairing = model.mask_type.lower()

    # -- weights ------------------------------------------------------------------------------------------------------
    def _drop_weights(self) -> None:
        """Forget graphs, fp32 plans and weight packs (they are rebuilt from the current parameters on next use)."""
        super()._drop_weights()
        self._own = [{"gemm_precision": "fp32"} for _ in self._plan_mods]

    def _around_body(self):
        return self._fp32_plans()

    @contextlib.contextmanager
    def _fp32_plans(self):
        """The masker's plan-cached modules compute with the streamer's own exact-fp32 plans inside this block; their own
        precision and plans are put back after it."""
        with own_plans(self._plan_mods, self._own):
            yield

    def _build_packs(self, dev: torch.device) -> None:
        """Conv weights (eval BatchNorm2d folded, packed for the GEMM kernels) and the STFT tables, held by the streamer:
        a captured graph keeps reading these tensors."""
        model, m = self.model, self.model.masker
        stft = model.encoder.encoder
        wt_a, rows = stft._analysis_plan(model.drop_first_bin)
        wt_s, window = stft._synthesis_plan(model.drop_first_bin)
        p = m._build_unet(dev)
        self._packs = dict(wt_a=wt_a, rows=rows, wt_s=wt_s, window=window, down=p["down"], up=p["up"])

    # -- session ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def init_streams(self, streams: int = 1, use_graph: bool = True) -> None:
        """Start `streams` new streams (every state zeroed)."""
        if int(streams) < 1:
            raise ValueError("init_streams: streams >= 1")
        dev = next(self.model.parameters()).device
        b = int(streams)
        self._begin(b, dev, use_graph)
        self._allocate(b, dev)

    @torch.no_grad()
    def init_slots(self, capacity: int, use_graph: bool = True) -> None:
        """Start a slot session of `capacity` columns, every slot idle (every state zeroed); open() starts a stream."""
        if int(capacity) < 1:
            raise ValueError("init_slots: capacity >= 1")
        b, dev = int(capacity), next(self.model.parameters()).device
        self._begin(b, dev, use_graph)
        self._make_slots()
        self._ready()
        self._allocate(b, dev)

    def _enrolment_rule(self) -> tuple:
        return False, "iff the model has a speaker_net (a noise suppressor has none: pass no enroll)"

    def _open_slot(self, slot: int, seed) -> None:
        """Nothing is reset or cleared: what the slot's predecessor left in the rings and the carried states are dead frames,
        which the kernels read as zeros through the span."""
        self._ready()

    def _allocate(self, b: int, dev: torch.device) -> None:
        """Geometry of every convolution (unet.py:219-281), the frame buffers, the rings and the carried LSTM states."""
        m = self.model.masker
        self._ldb = ldb = hip.padded_frames(b)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        n = m.n_cnn
        ch0 = 2 if m.input_type.lower() == "ri" else 1
        # geometry of every convolution (unet.py:219-281) and the frame shape of every tensor a convolution reads
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
            f_in = shapes[x][1]
            f_out = (f_in - 1) * sf - 2 * pf + df * (kf - 1) + op + 1
            self._up.append(dict(src=x, skip=f"d{i}", f_out=f_out, kf=kf, kt=m.t_kernel, sf=sf, df=df, dt=dt, pf=pf))
            if j < n - 1:
                x = f"u{j}"
                shapes[x] = (m.channels[i], f_out)
        if (self._up[-1]["f_out"], ch0 * m.multi_output) != (m.num_freq, ch0):
            raise NotImplementedError("StreamingSeparator: the decoder does not return the encoder's frequency rows")
        # history each tensor must keep: the most any convolution reading it needs
        hist = {k: 0 for k in shapes}
        for c in self._down:
            hist[c["src"]] = max(hist[c["src"]], (c["kt"] - 1) * c["dt"])
        for c in self._up:
            for k in (c["src"], c["skip"]):
                hist[k] = max(hist[k], (c["kt"] - 1) * c["dt"])
        # persistent frame buffers (zeroed: their pad frames stay zero) and the rings behind them
        self._in_shape = (1,) + shapes["in"] + (ldb,)
        self._cur = {k: z(1, ch, fr, ldb) for k, (ch, fr) in shapes.items() if k[0] == "d"}
        self._rings = {k: (z(r, *shapes[k], ldb) if r > 0 else None) for k, r in hist.items()}
        self._upout = [z(1, m.channels[i] if j < n - 1 else ch0, c["f_out"], ldb)
                       for j, (i, c) in enumerate(zip(reversed(range(n)), self._up))]
        for j in range(n - 1):
            self._cur[f"u{j}"] = self._upout[j]
        blocks = [m.dprnn_block1, m.dprnn_block2]
        hid = [blk.inter_rnn.rnn.hidden_size for blk in blocks]
        fb = shapes["mid"][1]
        self._lstm = [tuple(z(1, h, fb * ldb) for _ in range(4)) for h in hid]   # h0, c0, h', c'
        if sum(r is not None for r in self._rings.values()) + 2 * len(blocks) + 1 > hip._abi.PS_MAX_RING_PAIRS:
            raise NotImplementedError("StreamingSeparator: more history buffers than one commit launch takes")

    def _state(self) -> List[torch.Tensor]:
        return ([self._queue, self._tail, self._counter] + [r for r in self._rings.values() if r is not None]
                + [t for s in self._lstm for t in s])

    # -- one hop ------------------------------------------------------------------------------------------------------
    def _masker_step(self, feats: torch.Tensor) -> tuple:
        """[1, rows, ldB] features -> ([1, rows, ldB] mask, {tensor name: this frame}) through the U-Net and the two
        bottleneck blocks."""
        m, b, pk = self.model.masker, self.streams, self._packs
        # a slot session: every tensor of this hop is frame counter - 0, a tap reads it through the span
        live = {} if self._span is None else dict(counter=self._counter, span=self._span, shift=0)
        cur = dict(self._cur)
        cur["in"] = feats.view(self._in_shape)
        for i, (c, lay) in enumerate(zip(self._down, pk["down"])):
            hip.conv2d_step(cur[c["src"]], self._rings[c["src"]], None, None, lay["wt"], lay["bias"], lay["M"], b, c["f_out"],
                            c["kf"], c["kt"], c["sf"], c["df"], c["dt"], c["pf"], False, lay["act"], lay["slope"],
                            out=cur[f"d{i}"], **live)
        y = cur[f"d{m.n_cnn - 1}"]
        for blk, (h0, c0, h1, c1) in zip((m.dprnn_block1, m.dprnn_block2), self._lstm):
            y = blk.forward_step(y, b, h0, c0, (h1, c1))
        cur["mid"] = y
        for j, (c, lay) in enumerate(zip(self._up, pk["up"])):
            hip.conv2d_step(cur[c["src"]], self._rings[c["src"]], cur[c["skip"]], self._rings[c["skip"]], lay["wt"],
                            lay["bias"], lay["M"], b, c["f_out"], c["kf"], c["kt"], c["sf"], c["df"], c["dt"], c["pf"], True,
                            lay["act"], lay["slope"], out=self._upout[j], **live)
        return self._upout[-1].view(1, -1, self._ldb), cur

    def _body(self, hops: int) -> None:
        """`hops` hops of every stream: input _io[hops][0] [B, hops*hop] -> output _io[hops][1] [B, hops*hop]."""
        chunk, out, wins = self._io[hops]
        b, hop, pk = self.streams, self.hop_length, self._packs
        hip.stream_windows(self._queue, chunk, wins, hop)
        for i in range(hops):
            frames, _ = hip.frame(wins[i:i + 1], self.n_fft, self.n_fft)               # [1, n_fft, ldB]: streams = frames
            feats, _ = hip.conv1x1(frames, b, pk["wt_a"], pk["rows"],
                                   out=torch.empty(1, pk["rows"], self._ldb, dtype=torch.float32, device=self.device))
            if self._span is not None:     # the carried states are frame counter - 1: zeros where that frame is dead
                hip.state_gate([t for h0, c0, _, _ in self._lstm for t in (h0, c0)], self._counter, self._span, b, shift=1)
            mask, cur = self._masker_step(feats)
            enh = (hip.complex_mask(feats, mask, self._mask_act) if self._pairing == "complex"
                   else hip.real_mask(feats, mask, self._mask_act))
            syn, _ = hip.conv1x1(enh, b, pk["wt_s"], self.n_fft,
                                 out=torch.empty(1, self.n_fft, self._ldb, dtype=torch.float32, device=self.device))
            if self._span is not None:
                hip.istft_step(syn, pk["window"], self._tail, out[:, i * hop:(i + 1) * hop], self._counter, hop,
                               self._out_mode, span=self._span, shift=0)
            else:
                hip.istft_step(syn, pk["window"], self._tail, out[:, i * hop:(i + 1) * hop], self._counter, hop,
                               self._out_mode)
            pairs = [(cur[k], r) for k, r in self._rings.items() if r is not None]
            pairs += [(h1, h0) for h0, _, h1, _ in self._lstm] + [(c1, c0) for _, c0, _, c1 in self._lstm]
            if i == hops - 1:
                pairs.append((wins[i], self._queue))
            hip.stream_commit(hip.commit_table(pairs), self._counter, self.device)

    def _flush_into(self, out: torch.Tensor) -> None:
        hip.istft_step(None, self._packs["window"], self._tail, out, self._counter, self.hop_length, self._out_mode, flush=True)

    def _flush_slot(self, out: torch.Tensor, slot: int) -> None:
        """close(): the tail of one slot, with the window sum of its own frames (B = 1 on its tail row and span row)."""
        hip.istft_step(None, self._packs["window"], self._tail[slot:slot + 1], out, self._counter, self.hop_length,
                       self._out_mode, flush=True, span=self._span[slot:slot + 1], shift=0)
