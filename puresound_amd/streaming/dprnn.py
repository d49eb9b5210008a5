"""Streaming the causal time-domain DPRNN speaker extractor (FreeEncDec + DPRNN(causal=True), with or without
embedding_free_tse: egs/tse veve_dprnn_v0_causal) on the HIP path, one hop at a time for B concurrent streams.

The model is exactly causal in time.  A segment is K = seg_size consecutive frames (seg_overlap=False).  With causal=True both
LSTMs of a block run forward only: the intra LSTM walks the K frames of a segment from a zero state, and the inter LSTM at
position p = g % K of frame g continues from the state it left at position p of the previous segment -- for the first
segment from zero, or, with embedding_free_tse, from the state the enrolment pass ended in at that position.  LayerNorm acts
on one frame, and the zero padding to whole segments lies after the last frame.  So frame g needs frames <= g only, and the
samples a stream returns, followed by flush(), equal `model.inference(noisy, enroll)`, win - hop samples late.

Layout as tcn.py: the k frames of a chunk for the B streams are the N = k*B columns of the library's channel-major rows
(column f*B + b = frame f, stream b).  Every dependency of a block is per stream, so one launch of ps_dprnn_block_step_f32
(csrc/dprnn_step.hip) runs a whole block on a whole chunk: a workgroup owns 16 stream columns and walks their frames in order.
Per block the device holds the intra state (h, c) [H, ldB] and two banks [K, H, ldB], slot p = the inter state at position p.
A chunk is: stream_windows, frame, the encoder's conv1x1 (+ ReLU), n_blocks block launches, output_fc (a conv1x1 with a PReLU
prologue), free_decode_step (two launches) and stream_commit_frames -- n_blocks + 7 or 8 launches whatever its length.  No
launch argument depends on the frame index, so one captured graph per chunk length replays every chunk.

Arithmetic: exact fp32 products throughout, whatever the model's gemm_precision; every sum of a stream's column has one fixed
order (the two 1x1 convolutions always take ps_conv1x1_f32's tiled kernel: MIN_GEMM_COLUMNS), so a stream's output does not depend on B, on its neighbours or on how its hops are split into calls.  The streamer
packs its own weights from the parameters; the model's own setting and plans are left as they were.  The enrolment states are
computed once per session by the model's own offline pieces, in the model's own arithmetic.  The session around the kernels
(priming, step / step_chunk / flush, eager run or graph replay, the capture) is HopSession's: streaming/_session.py; the
encoder, output_fc, decoder and commit of a chunk, their checks and packs are RecurrentFreeSession's: streaming/_free.py.

Slots (init_slots / open / end / close; the bookkeeping is HopSession's): a session of fixed capacity B whose columns begin
and end streams of their own while it runs.  Per slot the device holds a span (birth, death) of absolute frame indices; frame
g of column b is live iff birth[b] <= g < death[b].  The segment position is part of the recurrence, so a stream that joins
at an arbitrary frame has a phase of its own: ps_dprnn_block_step_slots_f32 puts frame g of column b at position
(g - birth[b]) % K -- its frame n at n % K, whatever the session's counter says -- resets the intra state and picks the bank
slot by it, reads a dead frame's input as 0 and stores no state for it; ps_free_decode_step_slots_f32 adds nothing for a dead
frame.  open() zeroes the slot's queue, tail and intra states and sets all K bank slots of its column (zero, or the states
its enrolment ends in), so nothing of the slot's predecessor is left.  What a slot returned from open to close, followed by
close()'s samples, is `model.inference(x, enroll)` of its own stream after latency_samples samples of constrain(0), whatever
the other slots do; every sum has one fixed order per column, so it is bit-identical to a block session of that stream.
"""
from typing import List, Optional

import torch

from .. import hip
from ..nnet.dprnn import DPRNN
# MIN_GEMM_COLUMNS: the fewest columns a 1x1 convolution of this streamer runs on (unet_tcn.py and callers take it from here)
from ._free import MIN_GEMM_COLUMNS, RecurrentFreeSession, check_front, check_recurrent  # noqa: F401
# K_MAX: frames per launch at most, step_chunk splits longer chunks; FRAME_LIMIT: where a session stops (the device frame
# counter is an int32, and a launch reads up to K_MAX frames past it); INT32_MAX: the death of a stream that has not ended
from ._session import FRAME_LIMIT, INT32_MAX, K_MAX, HopSession, check_on_device  # noqa: F401


def check_streamable(model) -> None:
    """Raise NotImplementedError naming the reason when `model` is not a configuration this streamer computes exactly."""
    name = "StreamingDPRNN"
    check_front(model, name)
    m = model.masker
    if not isinstance(m, DPRNN):
        raise NotImplementedError(f"{name}: masker {type(m).__name__}: DPRNN only (ConvTasNet streams through "
                                  f"StreamingConvTasNet)")
    if m.bi_direct:
        raise NotImplementedError(f"{name}: the DPRNN is not causal (causal=False: bidirectional LSTMs read future frames)")
    if m.seg_overlap:
        raise NotImplementedError(f"{name}: seg_overlap=True (half-overlapped segments) does not stream here")
    if m.embed_dim != 0 or any(f is not None for f in m.input_film):
        raise NotImplementedError(f"{name}: FiLM-conditioned blocks (embed_dim = {m.embed_dim}) are out of scope")
    if model.speaker_net is not None:
        raise NotImplementedError(f"{name}: a speaker_net (an embedding-conditioned DPRNN) is out of scope; the enrolment "
                                  f"enters through embedding_free_tse only")
    if bool(model.embedding_free_tse) != bool(m.embedding_free_tse):
        raise NotImplementedError(f"{name}: embedding_free_tse differs between the wrapper ({model.embedding_free_tse}) and "
                                  f"the masker ({m.embedding_free_tse})")
    check_recurrent(model, name, "DPRNN", hip.dprnn_block_step_ok, "ps_dprnn_block_step_f32",
                    "(2 C + 6 H) * 64 bytes of LDS, 64 KiB at most")
    check_on_device(model, name)


class StreamingDPRNN(RecurrentFreeSession):
    """Hop-by-hop inference of a causal DPRNN separator / enrolment-seeded speaker extractor for B streams (see the module
    docstring).

    s = StreamingDPRNN(model); s.init_streams(B, enroll); s.step(hop [B, hop]) -> [B, hop] or None while the first window
    fills; s.step_chunk([B, k*hop]) -> what k step() calls return, concatenated; s.flush() -> the last win - hop samples.

    Slots, for streams that begin and end on their own: s.init_slots(capacity); s.open(slot, enroll [L']); every
    s.step / s.step_chunk([capacity, k*hop]) -> [capacity, k*hop] from the first hop on (idle slots: constrain(0));
    s.end(slot, hops) when the stream has `hops` more hops of input; s.close(slot) -> the last win - hop samples, and the
    slot is idle again.  What a slot returned from open to close, then close's samples, is model.inference(x, enroll) of its
    own stream after latency_samples samples of constrain(0) (slot_output_range(L, win, hop)), whatever the other slots do,
    and bit-identical to a block session of that stream.
    """

    check_streamable = staticmethod(check_streamable)

    # -- weights ------------------------------------------------------------------------------------------------------
    def _build_packs(self, dev: torch.device) -> None:
        """fp32 weights packed for the kernels, held by the streamer: a captured graph keeps reading these tensors."""
        m = self.model.masker
        blocks = [(hip.pack_dprnn_pass(m.intra_rnn[i], m.intra_proj[i], m.intra_norm[i], dev),
                   hip.pack_dprnn_pass(m.inter_rnn[i], m.inter_proj[i], m.inter_norm[i], dev)) for i in range(m.n_blocks)]
        self._packs = dict(self._free_packs(dev), blocks=blocks)

    # -- session ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def init_streams(self, streams: int = 1, enroll: Optional[torch.Tensor] = None, use_graph: bool = True) -> None:
        """Start `streams` new streams.  enroll [streams, L'] on the model's device: the enrolment of each stream, required iff
        the model is embedding_free_tse; the inter-LSTM states its pass ends in are computed here, once, and seed the banks.
        Every other state is zeroed."""
        b = self._at_least_one(streams, "init_streams: streams")
        model, m = self.model, self.model.masker
        if (enroll is not None) != bool(model.embedding_free_tse):
            raise ValueError("StreamingDPRNN.init_streams: an enrolment [streams, L'] is required iff the model is "
                             "embedding_free_tse")
        dev = next(model.parameters()).device
        seeds = None
        if enroll is not None:
            self._check_enrolments(enroll, b)
            seeds = self._seeds(enroll)
        self._new_session(b, dev, use_graph)
        if seeds is not None:
            self._seed_banks(slice(0, b), seeds)

    def _seeds(self, enroll: torch.Tensor) -> list:
        """The final inter-LSTM states of the enrolment pass, by the model's own offline pieces: per block (h, c)
        [B, H, ldq], [b, :, p] = position p of stream b."""
        model, m = self.model, self.model.masker
        feats, te = model.encoder.encode_padded(enroll.contiguous(), m.padded_frames_needed)
        return m.hidden_states_padded(feats, te)

    def _seed_banks(self, cols: slice, seeds: list) -> None:
        """All K slots of the columns `cols` of every block's banks <- the seeds of as many streams."""
        k = self.model.masker.seg_size
        for bank, seed in zip(self._banks, seeds):
            for dst, src in zip(bank, seed):
                dst[:, :, cols] = src[:, :, :k].float().permute(2, 1, 0)

    def _new_session(self, b: int, dev: torch.device, use_graph: bool) -> None:
        """Zeroed state of b columns."""
        m = self.model.masker
        self._begin(b, dev, use_graph)
        k, h, ldb = m.seg_size, m.hidden_size, hip.padded_frames(b)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        self._intra = [(z(h, ldb), z(h, ldb)) for _ in range(m.n_blocks)]
        self._banks = [(z(k, h, ldb), z(k, h, ldb)) for _ in range(m.n_blocks)]
        self._bufs = {}

    @torch.no_grad()
    def init_slots(self, capacity: int, use_graph: bool = True) -> None:
        """Start a slot session of `capacity` columns, every slot idle (every state zeroed); open() starts a stream."""
        self._new_session(self._at_least_one(capacity, "init_slots: capacity"), next(self.model.parameters()).device, use_graph)
        self._make_slots()

    def _enrolment_rule(self) -> tuple:
        tse = bool(self.model.embedding_free_tse)
        return tse, ("iff the model is embedding_free_tse (this one " +
                     ("is: pass enroll)" if tse else "is not: pass no enroll)"))

    def _open_slot(self, slot: int, enroll: Optional[torch.Tensor]) -> None:
        """Nothing of the slot's predecessor stays: the intra (h, c) of every block zeroed, all K bank slots of the column
        zeroed or, with an enrolment, set to the inter states its pass ends in (computed here, once, as init_streams does)."""
        seeds = self._seeds(enroll) if enroll is not None else None
        for h, c in self._intra:
            h[:, slot].zero_()
            c[:, slot].zero_()
        if seeds is None:
            for h, c in self._banks:
                h[:, :, slot].zero_()
                c[:, :, slot].zero_()
        else:
            self._seed_banks(slice(slot, slot + 1), seeds)

    def _state(self) -> List[torch.Tensor]:
        return [self._queue, self._tail, self._counter] + [t for pair in self._intra + self._banks for t in pair]

    # -- one chunk ----------------------------------------------------------------------------------------------------
    def _masker(self, hops: int, bufs: dict, feats: torch.Tensor) -> torch.Tensor:
        """The blocks, one launch each, alternating between two buffers, then output_fc."""
        x = feats
        for i, (intra, inter) in enumerate(self._packs["blocks"]):
            y = bufs["x0"] if i % 2 == 0 else bufs["x1"]
            hip.dprnn_block_step(x, self._counter, intra, inter, *self._intra[i], *self._banks[i], self.streams, hops, out=y,
                                 span=self._span)
            x = y
        return self._mask_head(x, bufs)
