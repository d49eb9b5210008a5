"""Streaming the causal time-domain SkiM speaker extractors (FreeEncDec + SkiM(causal=True) with FiLM conditioning: egs/tse
tse_skim_v0_causal, tse_skim_v1_causal, tse_skim_v2_causal, tse_skim_v0_causal_vad) on the HIP path, one hop at a time for B
concurrent streams.

The model is exactly causal in time.  A segment is K = seg_size consecutive frames (seg_overlap=False).  With causal=True every
SegLSTM runs forward only; block 0 starts every segment from zero, and block i + 1 starts segment s from what MemLSTM i made of
block i's final state of segment s - 1 (the shift in MemLSTM.forward; segment 0 starts from zero).  LayerNorm and FiLM act on
one frame, and the zero padding to whole segments lies after the last frame.  So frame g needs frames <= g only, and the
samples a stream returns, followed by flush(), equal `model.inference(noisy[b:b+1], enroll[b:b+1])` of that stream, win - hop
samples late.

Of that stream ALONE: on a batch the offline model is not a function of one utterance.  The reference shifts the MemLSTM's
result along the flattened (utterance, segment) axis (skim.py:102-109), so utterance n > 0 of a batch starts its first
segment, in every block but the first, from the state utterance n - 1 reached at the end of its LAST (zero padded) segment;
the offline path here reproduces that.  A stream cannot depend on its neighbour's future, and does not here: row 0 of
`model.inference(batch)` is what stream 0 returns, every other stream returns what the model gives for it as a batch of one.

Layout as dprnn.py: the k frames of a chunk for the B streams are the N = k*B columns of the library's channel-major rows
(column f*B + b = frame f, stream b).  Every dependency of a block is per stream, so one launch of ps_skim_block_step_f32
(csrc/skim_step.hip) runs a whole block on a whole chunk: a workgroup owns 16 stream columns and walks their frames in order.
Per block the device holds the running SegLSTM state (h, c) [H, ldB], the carried states of its MemLSTM's two nets, the
embedding's share of FiLM's scale and bias [C, ldB] (computed once per session) and, for every block but the first, two banks
[NS, H, ldB] of incoming hand-overs: block i writes slot (s + 1) % NS at the end of segment s, block i + 1 reads slot s % NS at
the start of segment s.  A chunk is: stream_windows, frame, the encoder's conv1x1 (+ ReLU), n_blocks block launches, output_fc
(a conv1x1 with a PReLU prologue), free_decode_step (two launches) and stream_commit_frames -- n_blocks + 7 or 8 launches
whatever its length.  No launch argument depends on the frame index, so one captured graph per chunk length replays every
chunk.

Arithmetic: exact fp32 products throughout, whatever the model's gemm_precision; every sum of a stream's column has one fixed
order (the 1x1 convolutions always take ps_conv1x1_f32's tiled kernel: MIN_GEMM_COLUMNS), so a stream's output does not depend
on B, on its neighbours or on how its hops are split into calls.  The streamer packs its own weights from the parameters; the
model's own setting and plans are left as they were.  The session around the kernels (priming, step / step_chunk / flush,
eager run or graph replay, the capture) is HopSession's: streaming/_session.py; the encoder, output_fc, decoder and commit of
a chunk, their checks and packs are RecurrentFreeSession's: streaming/_free.py.

Slots (init_slots / open / end / close; the bookkeeping is HopSession's): a session of fixed capacity B whose columns begin
and end streams of their own while it runs.  Per slot the device holds a span (birth, death) of absolute frame indices; frame
g of column b is live iff birth[b] <= g < death[b].  The segment grid is part of the recurrence, so a stream that joins at an
arbitrary frame counts its segments from its own birth: ps_skim_block_step_slots_f32 puts frame g of column b at position
(g - birth[b]) % K of segment (g - birth[b]) // K -- its frame n where a session of its own would have it -- and takes the
segment start (zero, or the bank slot) and the MemLSTM hand-over per column by that; a dead frame reads its input as 0 and
stores no state and no bank slot; ps_free_decode_step_slots_f32 adds nothing for a dead frame.  open() zeroes the slot's
queue, tail, SegLSTM and MemLSTM states and all NS slots of its column of every bank, and writes the FiLM terms of the new
stream's embedding into its column (computed as a session of one stream computes them), so nothing of the slot's predecessor
is left.  What a slot returned from open to close, followed by close()'s samples, is `model.inference(x[None], enroll[None])`
of its own stream after latency_samples samples of constrain(0), whatever the other slots do; every sum has one fixed order
per column, so it is bit-identical to an init_streams(1, ...) session of that stream.  A tile of 16 slots pays the hand-over
at every frame at which any of its slots ends a segment: DESIGN 4.11 has what staggered births cost, measured.
"""
from typing import List, Optional

import torch

from .. import hip
from ..nnet.lobe.trivial import FiLM, Gate
from ..nnet.skim import SkiM
from ._free import MIN_GEMM_COLUMNS, RecurrentFreeSession, check_front, check_recurrent
from ._session import FRAME_LIMIT, INT32_MAX, K_MAX, HopSession, check_on_device  # noqa: F401


def check_streamable(model) -> None:
    """Raise NotImplementedError naming the reason when `model` is not a configuration this streamer computes exactly."""
    name = "StreamingSkiMExtractor"
    check_front(model, name)
    m = model.masker
    if not isinstance(m, SkiM):
        raise NotImplementedError(f"{name}: masker {type(m).__name__}: SkiM only (DPRNN streams through StreamingDPRNN, "
                                  f"ConvTasNet through StreamingConvTasNet)")
    fusions = list(m.seg_input_fusion) if m.embed_dim > 0 else []
    if any(isinstance(f, Gate) for f in fusions):
        raise NotImplementedError(f"{name}: Gate fusion is out of scope; FiLM-conditioned blocks stream here")
    if not m.causal:
        raise NotImplementedError(f"{name}: the SkiM is not causal (causal=False: bidirectional LSTMs read future frames)")
    if m.seg_overlap:
        raise NotImplementedError(f"{name}: seg_overlap=True (half-overlapped segments) does not stream here")
    if model.embedding_free_tse:
        raise NotImplementedError(f"{name}: embedding_free_tse is the DPRNN's way of enrolment (StreamingDPRNN); a SkiM takes "
                                  f"an embedding")
    if m.embed_dim > 0 and model.speaker_net is None:
        raise NotImplementedError(f"{name}: embed_dim = {m.embed_dim} but the model has no speaker_net: model.inference can "
                                  f"hand this masker no embedding, so there is no output to reproduce")
    if m.seg_size < 1:
        raise NotImplementedError(f"{name}: seg_size = {m.seg_size}")
    for i, f in enumerate(fusions):
        if f is not None and not (isinstance(f, FiLM) and f.inp_norm):
            raise NotImplementedError(f"{name}: block {i}: fusion {type(f).__name__}: FiLM with its input norm, or none")
    check_recurrent(model, name, "SkiM", hip.skim_block_step_ok, "ps_skim_block_step_f32",
                    "(2 max(C, H) + 2 H + max(4 H, 2 C)) * 64 bytes of LDS, 160 KiB at most")
    check_on_device(model, name)


class StreamingSkiMExtractor(RecurrentFreeSession):
    """Hop-by-hop inference of a causal SkiM speaker extractor (or plain SkiM separator) for B streams (see the module
    docstring).

    s = StreamingSkiMExtractor(model); s.init_streams(B, enroll=e) or s.init_streams(B, embed=d);
    s.step(hop [B, hop]) -> [B, hop] or None while the first window fills; s.step_chunk([B, k*hop]) -> what k step() calls
    return, concatenated; s.flush() -> the last win - hop samples.

    Slots, for streams that begin and end on their own: s.init_slots(capacity); s.open(slot, enroll=e [L']) or
    s.open(slot, embed=d [E]); every s.step / s.step_chunk([capacity, k*hop]) -> [capacity, k*hop] from the first hop on
    (idle slots: constrain(0)); s.end(slot, hops) when the stream has `hops` more hops of input; s.close(slot) -> the last
    win - hop samples, and the slot is idle again.  What a slot returned from open to close, then close's samples, is
    model.inference(x[None], enroll[None]) of its own stream after latency_samples samples of constrain(0)
    (slot_output_range(L, win, hop)), whatever the other slots do, and bit-identical to an init_streams(1, ...) session of
    that stream.
    """

    check_streamable = staticmethod(check_streamable)

    # -- weights ------------------------------------------------------------------------------------------------------
    def _build_packs(self, dev: torch.device) -> None:
        """fp32 weights packed for the kernels, held by the streamer: a captured graph keeps reading these tensors."""
        m = self.model.masker
        self._packs = dict(self._free_packs(dev), blocks=[hip.pack_skim_block(m, i, dev) for i in range(m.n_blocks)])
        if self._slots is not None:                                # (changed weights in a session: FiLM's terms follow them;
            for slot, embed in enumerate(self._slot_embeds):       # a slot session's, in place, for the slots that are open)
                if embed is not None and self._slots[slot] is not None:
                    self._write_terms(slot, embed)
        elif self.streams is not None:
            self._terms = self._film_terms()

    # -- session ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def init_streams(self, streams: int = 1, enroll: Optional[torch.Tensor] = None, embed: Optional[torch.Tensor] = None,
                     use_graph: bool = True) -> None:
        """Start `streams` new streams.  A masker with embed_dim > 0 takes exactly one of enroll [streams, L'] (through
        model.inference_tse_embedding, once) and embed [streams, E] (what that call returns; a deployment caches it), on the
        model's device; a masker without takes neither.  The masker's own L2 normalisation is applied here, and what the
        embedding adds to every FiLM's scale and bias is computed here, once.  Every other state is zeroed."""
        name = "StreamingSkiMExtractor.init_streams"
        b = self._at_least_one(streams, "init_streams: streams")
        model, m = self.model, self.model.masker
        if m.embed_dim > 0 and (enroll is None) == (embed is None):
            raise ValueError(f"{name}: the masker takes an embedding (embed_dim = {m.embed_dim}): pass exactly one of enroll "
                             f"[streams, L'] and embed [streams, {m.embed_dim}]")
        if m.embed_dim == 0 and (enroll is not None or embed is not None):
            raise ValueError(f"{name}: the masker takes no embedding (embed_dim = 0): pass neither enroll nor embed")
        dev = next(model.parameters()).device
        if enroll is not None:
            self._check_enrolments(enroll, b)
            embed = model.inference_tse_embedding(enroll)
        if embed is not None:
            hip.require_device(embed, name)
            if embed.dim() == 3 and embed.shape[2] == 1:           # (as inference_tse_embedding returns it)
                embed = embed[:, :, 0]
            if tuple(embed.shape) != (b, m.embed_dim) or embed.device != dev:
                raise ValueError(f"{name}: embed must be [{b}, {m.embed_dim}] on {dev}, got {tuple(embed.shape)} on "
                                 f"{embed.device}")
        self._begin(b, dev, use_graph)
        h, ldb = m.hidden_size, hip.padded_frames(max(b, MIN_GEMM_COLUMNS))
        self._embed, self._ldb = embed, ldb
        self._packs = None                                         # (rebuilt with this session's terms on first use)
        ns = hip.skim_bank_slots(K_MAX, m.seg_size)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        self._seg = [(z(h, ldb), z(h, ldb)) for _ in range(m.n_blocks)]
        self._mem = [tuple(z(h, ldb) for _ in range(4)) for _ in range(m.n_blocks - 1)]
        self._banks = [(z(ns, h, ldb), z(ns, h, ldb)) for _ in range(m.n_blocks - 1)]
        self._bufs = {}
        self._ready()

    @torch.no_grad()
    def init_slots(self, capacity: int, use_graph: bool = True) -> None:
        """Start a slot session of `capacity` columns, every slot idle (every state and every FiLM term zeroed); open() starts
        a stream."""
        m = self.model.masker
        b, dev = self._at_least_one(capacity, "init_slots: capacity"), next(self.model.parameters()).device
        self._begin(b, dev, use_graph)
        self._make_slots()
        h, c, ldb = m.hidden_size, m.input_size, hip.padded_frames(max(b, MIN_GEMM_COLUMNS))
        self._embed, self._ldb = None, ldb
        self._slot_embeds = [None] * b                             # per slot the embedding [1, E] its stream was opened with
        ns = hip.skim_bank_slots(K_MAX, m.seg_size)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        self._seg = [(z(h, ldb), z(h, ldb)) for _ in range(m.n_blocks)]
        self._mem = [tuple(z(h, ldb) for _ in range(4)) for _ in range(m.n_blocks - 1)]
        self._banks = [(z(ns, h, ldb), z(ns, h, ldb)) for _ in range(m.n_blocks - 1)]
        # (the launches read these tensors for as long as the session lasts: open() writes a column of them)
        self._terms = [(z(c, ldb), z(c, ldb)) if m.embed_dim > 0 and m.block_with_embed[i] else None for i in range(m.n_blocks)]
        self._bufs = {}

    def _enrolment_rule(self) -> tuple:
        e = self.model.masker.embed_dim
        if e > 0:
            return True, (f"the masker takes an embedding (embed_dim = {e}): pass exactly one of enroll [L'] and embed [{e}]")
        return False, "the masker takes no embedding (embed_dim = 0): pass neither enroll nor embed"

    def _slot(self, slot: int, what: str, idle: bool) -> int:
        """(a block session answers the slot calls with the NotImplementedError -- a RuntimeError, as the siblings raise --
        and the words it has always had for them: its streams are not slots)"""
        if self.streams is not None and self._slots is None:
            raise NotImplementedError(f"{type(self).__name__}.{what}: an init_streams() session has no slot sessions: its "
                                      f"streams start together and end together in flush(); call init_slots() for slots that "
                                      f"open and close on their own")
        return super()._slot(slot, what, idle)

    @torch.no_grad()
    def open(self, slot: int, enroll: Optional[torch.Tensor] = None, embed: Optional[torch.Tensor] = None) -> None:
        """Start a stream in the idle slot `slot`: its first input hop is the first hop of the next step / step_chunk call.
        A masker with embed_dim > 0 takes exactly one of enroll [L'] or [1, L'] (through model.inference_tse_embedding, here,
        once) and embed [E], [1, E] or [1, E, 1] (what that call returns; a deployment caches it), on the session's device; a
        masker without takes neither.  No synchronisation, no captured graph is touched."""
        name = f"{type(self).__name__}.open"
        slot = self._slot(slot, "open", idle=True)
        required, why = self._enrolment_rule()
        given = (enroll is not None) + (embed is not None)
        if given != int(required):
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
        """Nothing of the slot's predecessor stays: the column zeroed in every block's (seg_h, seg_c), MemLSTM states and all
        NS slots of both banks, and the new stream's FiLM terms written into it (computed here, once, as init_streams does
        for one stream)."""
        enroll, embed = seed
        if enroll is not None:
            embed = self.model.inference_tse_embedding(enroll)[:, :, 0]
        self._ready()
        for group in self._seg + self._mem:
            for t in group:
                t[:, slot].zero_()
        for bank in self._banks:
            for t in bank:
                t[:, :, slot].zero_()
        self._slot_embeds[slot] = None if embed is None else embed.detach().to(torch.float32).clone()
        if embed is not None:
            self._write_terms(slot, self._slot_embeds[slot])

    def _write_terms(self, slot: int, embed: torch.Tensor) -> None:
        """Column `slot` of every block's (rs, rb) <- the terms of embed [1, E], the bits of a session of that one stream."""
        one = self._terms_of(embed, hip.padded_frames(MIN_GEMM_COLUMNS))
        for dst, src in zip(self._terms, one):
            if dst is not None:
                dst[0][:, slot] = src[0][:, 0]
                dst[1][:, slot] = src[1][:, 0]

    def _film_terms(self) -> list:
        """Per block with FiLM (rs, rb) [C, ldb]: the embedding columns of cond_scale / cond_bias applied to the (normalised)
        embedding of every stream.  Both sums run as ps_conv1x1_f32 over the streams as columns, at least MIN_GEMM_COLUMNS of
        them, so a stream's terms do not depend on B."""
        if self._embed is None:
            return [None] * self.model.masker.n_blocks
        return self._terms_of(self._embed, self._ldb)

    def _terms_of(self, embed: torch.Tensor, ldb: int) -> list:
        """_film_terms for embed [b, E] in rows of ldb columns."""
        m = self.model.masker
        b, e = embed.shape
        c, cols = m.input_size, max(b, MIN_GEMM_COLUMNS)
        rows = torch.zeros(1, e, ldb, dtype=torch.float32, device=self.device)
        rows[0, :, :b] = embed.t()
        if m.embed_norm:                                           # F.normalize: e / max(|e|, 1e-12)
            ones = hip.pack_wt(torch.ones(1, e, dtype=torch.float32, device=self.device))
            sq, _ = hip.conv1x1(rows * rows, cols, ones, 1)
            rows = rows / sq.sqrt().clamp_min(1e-12)
        terms = []
        for pk in self._packs["blocks"]:
            if pk["film"] is None:
                terms.append(None)
                continue
            both, _ = hip.conv1x1(rows, cols, hip.pack_wt(pk["film"]["embed_wt"]), 2 * c)
            terms.append((both[0, :c], both[0, c:]))
        return terms

    def _state(self) -> List[torch.Tensor]:
        return [self._queue, self._tail, self._counter] + [t for group in self._seg + self._mem + self._banks for t in group]

    # -- one chunk ----------------------------------------------------------------------------------------------------
    def _masker(self, hops: int, bufs: dict, feats: torch.Tensor) -> torch.Tensor:
        """The blocks, one launch each, alternating between two buffers, then output_fc."""
        m = self.model.masker
        x = feats
        last = m.n_blocks - 1
        for i, block in enumerate(self._packs["blocks"]):
            y = bufs["x0"] if i % 2 == 0 else bufs["x1"]
            hip.skim_block_step(x, self._counter, block, self._seg[i], m.seg_size, self.streams, hops, y, terms=self._terms[i],
                                bank_in=self._banks[i - 1] if i > 0 else None, mem_state=self._mem[i] if i < last else None,
                                bank_out=self._banks[i] if i < last else None, span=self._span)
            x = y
        return self._mask_head(x, bufs)
