"""The session mechanics the hop-by-hop streamers share (spectral.py, unet_tcn.py; tcn.py, dprnn.py and skim.py through
FreeEncSession, _free.py): B streams fed whole hops, a priming phase while the first analysis window fills, then chunks of
hops through the subclass's kernels -- eagerly, or as one captured graph per number of hops in a launch -- and a flush of the
overlap-add tail.

A streamer provides: `_build_packs(device)` (sets self._packs from the current parameters), `_state()` (every tensor a body
run advances), `_body(hops)` (the launches of `hops` hops: self._io[hops] = (input [B, hops*hop], output [B, hops*hop],
windows [hops, B*window])), `_flush_into(out)`; it may set `max_hops` and override `_around_body`.  Its init_streams checks
its own arguments, calls `_begin` and allocates what `_state` returns; `_queue` [B, window], `_tail` [B, window - hop] and
`_counter` (int32 [1], the device frame counter) are allocated here.  Every session, block or slot, stops at FRAME_LIMIT frames
(`_run`): below it no kernel sees a frame index past INT32_MAX, and a kernel must not form a larger quantity from it in an int
(the sample index t * hop does not fit: ps_istft_step_f32 indexes its window without it).

A model delay (unet_tcn.py): a streamer whose model looks `delay_frames` = D frames ahead passes D to the constructor.  Its
first D computed frames run the body with `self._mute` set -- always eagerly -- and emit nothing: the body advances the model
state and leaves the overlap-add tail, the window sum and its synthesis counter as they were.  So prime_hops and
latency_samples grow by D hops, and flush() first lets the streamer run the hops that are still inside the model (the
streamer's `_flush_into(out)` fills min(frames, D) * hop + window - hop samples).  D = 0: nothing of this happens.

Slots (all five streamers): a session of fixed capacity whose columns begin and end streams of their own while it runs.  The
model-independent half lives here: the device span [B, 2] of (birth, death) frame indices and the host record per slot, the
slot checks, open / end / close, the hops each slot was fed, the frame limit, and the rules that a slot session has no
priming phase and no flush().  A streamer with slots calls `_begin` and then `_make_slots` in its init_slots, passes
`self._span` to its kernels in `_body`, and provides `_enrolment_rule()` (whether open() takes an enrolment, and the words
that say why), `_open_slot(slot, enroll)` (reset or seed the slot's model state) and a `_flush_into(out, tail)` that takes
the tail rows to flush.  A streamer whose open() takes other arguments (skim.py: an enrolment or its embedding) overrides
open(), checks them and ends in `_start_slot`.

Slots and a model delay (unet_tcn.py): a slot is born at its first full window, counter + window / hop - 1 -- the model's
delay is not part of the birth, the model's state is live from that frame on -- and a slot session has no mute hops: the
streamer's kernels read every tensor with the shift of its layer, so a frame is live or dead by its own index.  The D hops
of the session after a slot's last input hop carry its last frames out (the slot's input in those hops is ignored);
close() before they were stepped raises, as does close() without an earlier end(): end(slot, 0), D hops, close(slot).  The
tail is flushed per slot through `_flush_slot(out, slot)`, by default `_flush_into(out, tail row)`.  spectral.py is the same
rule with delay_frames = 0; its carried LSTM states are read through the span too (ps_state_gate_slots_f32).
"""
import contextlib
from typing import Dict, List, Optional

import torch

from .. import hip
from ..graphs import _cached_tensors, capture
from ..nnet._plans import tensor_signature


#: frames per launch at most of the streamers that split a chunk into pieces (tcn.py, dprnn.py)
K_MAX = 16
INT32_MAX = 2 ** 31 - 1
#: a session stops here: the device frame counter is an int32, and a launch reads up to K_MAX frames past it
FRAME_LIMIT = INT32_MAX - K_MAX


def check_on_device(model, name: str) -> None:
    """The last check of a check_streamable: every parameter and buffer of the model lives on a ROCm device."""
    devs = {t.device.type for t in list(model.parameters()) + list(model.buffers())}
    if devs != {"cuda"}:
        raise NotImplementedError(f"{name}: the model's tensors are on {sorted(devs)}; streaming runs on a ROCm device only "
                                  f"(move the model with .to(device))")


class HopSession:
    #: hops per launch at most: longer chunks run in pieces (None: a chunk is one launch, whatever its length)
    max_hops: Optional[int] = None
    _how_to_start = "call init_streams() first"

    def __init__(self, model, window: int, hop: int, delay_frames: int = 0):
        if model.training:
            raise RuntimeError(f"{type(self).__name__}: the model is in training mode -- call .eval()")
        self.model = model
        self.window, self.hop_length = int(window), int(hop)
        self.delay_frames = int(delay_frames)
        self._fill_hops = self.window // self.hop_length - 1      # hops that only fill the first analysis window
        self.prime_hops = self._fill_hops + self.delay_frames     # hops for which step() returns None
        self._mute = False
        self._mask_act = model.mask_constraint.lower()
        self._out_mode = model.output_constraint.lower()
        self.streams = None
        self._span = self._slots = None
        self._drop_weights()

    @property
    def latency_samples(self) -> int:
        """Samples between a sample entering and its value leaving: the analysis window minus one hop, plus the model's
        delay_frames hops."""
        return self.window - self.hop_length + self.delay_frames * self.hop_length

    @staticmethod
    def output_length(samples: int, n_fft: int, hop: int, delay_frames: int = 0) -> Dict[str, int]:
        """Length bookkeeping of a stream of `samples` = k * hop input samples: priming hops, the T frames computed, samples
        the steps emit, samples flush() returns (their sum is the offline output length (T - 1) * hop + n_fft,
        T = (samples - n_fft) // hop + 1).  delay_frames = D: the first D frames emit nothing, and flush() returns them."""
        if samples % hop or n_fft % hop or samples < n_fft or delay_frames < 0:
            raise ValueError("output_length: whole hops, n_fft a multiple of hop, at least one window, delay_frames >= 0")
        fill = n_fft // hop - 1
        frames = samples // hop - fill
        held = min(frames, delay_frames)
        return dict(prime_hops=fill + delay_frames, frames=frames, emitted=(frames - held) * hop,
                    flushed=n_fft - hop + held * hop)

    # -- weights ------------------------------------------------------------------------------------------------------
    def _drop_weights(self) -> None:
        """Forget graphs and weight packs (they are rebuilt from the current parameters on next use)."""
        self._graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self._pinned: Dict[int, list] = {}
        self._packs = None
        self._sig = tensor_signature(self.model)

    def _check_parameters(self) -> None:
        if tensor_signature(self.model) != self._sig:
            self._drop_weights()

    def _ready(self) -> None:
        """Before anything reads the packs: they are those of the current parameters."""
        self._check_parameters()
        if self._packs is None:
            self._build_packs(self.device)

    # -- session ------------------------------------------------------------------------------------------------------
    def _begin(self, streams: int, device: torch.device, use_graph: bool) -> None:
        """A new session of `streams` columns: counters at zero, no graph, window queue and overlap-add tail zeroed."""
        self._check_parameters()
        self._graphs, self._pinned = {}, {}
        self.streams, self.device, self._use_graph = int(streams), device, bool(use_graph)
        self._hops = 0           # hops taken in, priming included
        self.frames = 0          # hops past the priming: frames computed
        self._finished = False
        self._queue = torch.zeros(self.streams, self.window, dtype=torch.float32, device=device)
        self._tail = torch.zeros(self.streams, self.window - self.hop_length, dtype=torch.float32, device=device)
        self._counter = torch.zeros(1, dtype=torch.int32, device=device)
        self._io: Dict[int, tuple] = {}
        self._span = None        # int32 [B, 2] (birth, death) in a slot session
        self._slots = None       # per slot None (idle) or dict(hops fed, total hops once end() was called)

    def _make_slots(self) -> None:
        """After _begin: the session is a slot session, every slot idle."""
        self._span = torch.zeros(self.streams, 2, dtype=torch.int32, device=self.device)
        self._slots = [None] * self.streams

    def _around_body(self):
        """A context manager that encloses every run of _body (eager, warm-up and capture; never a replay)."""
        return contextlib.nullcontext()

    def _io_for(self, hops: int) -> tuple:
        """The static (input, output, windows) buffers of a `hops`-hop launch."""
        if hops not in self._io:
            z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.device)  # noqa: E731
            self._io[hops] = (z(self.streams, hops * self.hop_length), z(self.streams, hops * self.hop_length),
                              z(hops, self.streams * self.window))
        return self._io[hops]

    def _prime(self, hop_in: torch.Tensor) -> None:
        """A hop that only fills the analysis window: the queue slides, no model state moves."""
        chunk, _, wins = self._io_for(1)
        chunk.copy_(hop_in)
        hip.stream_windows(self._queue, chunk, wins, self.hop_length)
        self._queue.copy_(wins.view(self.streams, self.window))
        self._hops += 1

    def _priming(self) -> bool:
        """(a slot session has no priming phase: a slot's first prime_hops frames are dead by its span)"""
        return self._slots is None and self._hops < self._fill_hops

    def _run_piece(self, piece: torch.Tensor, mute: bool = False) -> Optional[torch.Tensor]:
        """Whole hops of one launch -> their output samples [B, hops*hop] (graph replay or eager); mute: frames inside the
        model's delay, run eagerly with self._mute set -> None."""
        hops = piece.shape[1] // self.hop_length
        chunk, out, _ = self._io_for(hops)
        chunk.copy_(piece)
        if mute or not self._use_graph:
            self._mute = mute
            try:
                with self._around_body():
                    self._body(hops)
            finally:
                self._mute = False
        else:
            g = self._graphs.get(hops)
            if g is None:
                g = self._capture(hops)
            g.replay()
        self._hops += hops
        self.frames += hops
        return None if mute else out.clone()

    def _run(self, chunk: torch.Tensor) -> torch.Tensor:
        """Whole hops past the priming -> their output samples, in pieces of at most max_hops hops.  The frame limit of every
        session before the chunk (nothing has moved when it raises); in a slot session the hops each slot's stream was fed
        after it.  `frames` is the device frame counter of every streamer, and a second counter a streamer keeps runs behind
        it (unet_tcn.py: _synth = frames - delay_frames), so the one bound covers both."""
        k = chunk.shape[1] // self.hop_length
        if self.frames + k > FRAME_LIMIT:
            way_out = ("close the streams and call init_slots()" if self._slots is not None
                       else "flush the streams and call init_streams()")
            raise RuntimeError(f"{type(self).__name__}: {self.frames} + {k} frames pass this session's limit of {FRAME_LIMIT} "
                               f"(2**31 - 1 - K_MAX: the device frame counter is an int32); {way_out} for a new session")
        self._ready()
        step = self.max_hops * self.hop_length if self.max_hops else chunk.shape[1]
        # frames inside the model's delay (a slot session has none: a slot's frames are live or dead by its span)
        quiet = 0 if self._slots is not None else min(k, max(self.delay_frames - self.frames, 0)) * self.hop_length
        for i in range(0, quiet, step):
            self._run_piece(chunk[:, i:min(i + step, quiet)], mute=True)
        outs = [self._run_piece(chunk[:, i:i + step]) for i in range(quiet, chunk.shape[1], step)]
        if not outs:
            return chunk.new_zeros(self.streams, 0)
        for st in self._slots or ():
            if st is not None:
                fed = k if st["total"] is None else min(k, st["total"] - st["hops"])
                st["hops"] += fed
                st["drained"] = min(st["drained"] + k - fed, self.delay_frames)   # hops past the stream's last input hop
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)

    def _capture(self, hops: int) -> torch.cuda.CUDAGraph:
        """Warm up once eagerly on a side stream (allocates what the launches need), put the state back, capture.  The body
        reads the streamer's own packs, buffers and state, which live as long as the session's graphs do; what it reads of
        the model's plan caches besides (inside _around_body: the plans that are in place while the body runs) is pinned
        with the graph, and dropped with it -- the model may replace a cache entry for another caller at any time."""
        with self._around_body():
            g, _ = capture(lambda: self._body(hops), self.device, self._state())
            self._pinned[hops] = _cached_tensors(self.model)
        self._graphs[hops] = g
        return g

    def _check_input(self, x: torch.Tensor, what: str) -> int:
        name = f"{type(self).__name__}.{what}"
        if self.streams is None:
            raise RuntimeError(f"{name}: {self._how_to_start}")
        if self._finished:
            raise RuntimeError(f"{name}: the streams were flushed; call init_streams() for new ones")
        hip.require_device(x, name)
        if x.dim() != 2 or x.shape[0] != self.streams or x.shape[1] % self.hop_length:
            raise ValueError(f"{name}: expected [{self.streams}, k * {self.hop_length}] samples, got {tuple(x.shape)}")
        return x.shape[1] // self.hop_length

    @torch.no_grad()
    def step(self, hop: torch.Tensor) -> Optional[torch.Tensor]:
        """hop [B, hop_length] new samples per stream -> [B, hop_length] output samples, or None while the first analysis
        window fills and the model's delay passes (the first prime_hops = window / hop - 1 + delay_frames hops)."""
        if self._check_input(hop, "step") != 1:
            raise ValueError(f"{type(self).__name__}.step: one hop of {self.hop_length} samples per stream")
        if self._priming():
            self._prime(hop)
            return None
        out = self._run(hop)
        return out if out.shape[1] else None

    @torch.no_grad()
    def step_chunk(self, chunk: torch.Tensor) -> torch.Tensor:
        """chunk [B, k*hop_length] -> what k step() calls return, concatenated ([B, 0] when every hop only primes)."""
        k = self._check_input(chunk, "step_chunk")
        i = 0
        while i < k and self._priming():
            self._prime(chunk[:, i * self.hop_length:(i + 1) * self.hop_length])
            i += 1
        if i == k:
            return chunk.new_zeros(self.streams, 0)
        return self._run(chunk[:, i * self.hop_length:])

    @torch.no_grad()
    def flush(self) -> torch.Tensor:
        """The last latency_samples samples of every stream ([B, window - hop_length + delay_frames * hop_length]; a stream of
        T < delay_frames frames has T hops in place of the delay's); the streams are then finished."""
        name = f"{type(self).__name__}.flush"
        if self._slots is not None:
            raise RuntimeError(f"{name}: a slot session ends its streams one by one: close(slot) returns a slot's last samples")
        if self.streams is None or self._finished:
            raise RuntimeError(f"{name}: no open streams")
        if self.frames == 0:
            raise RuntimeError(f"{name}: no complete frame yet (a stream needs {self.window} samples)")
        self._ready()
        held = min(self.frames, self.delay_frames) * self.hop_length
        out = torch.empty(self.streams, held + self.window - self.hop_length, dtype=torch.float32, device=self.device)
        self._flush_into(out)
        self._finished = True
        return out

    # -- slots --------------------------------------------------------------------------------------------------------
    @staticmethod
    def slot_output_range(samples: int, win: int, hop: int, delay_frames: int = 0) -> range:
        """The indices of y that hold model.inference(x, e) for a stream x of `samples` = k * hop samples in a slot, y = every
        output of the slot from open() on ‖ close(): the offline output (`samples` samples) after the latency,
        win - hop + delay_frames * hop samples."""
        HopSession.output_length(samples, win, hop, delay_frames)      # (the argument checks)
        lat = win - hop + delay_frames * hop
        return range(lat, lat + samples)

    @property
    def active(self) -> List[int]:
        """The slots that carry a stream (opened and not yet closed)."""
        return [] if self._slots is None else [i for i, st in enumerate(self._slots) if st is not None]

    def _slot(self, slot: int, what: str, idle: bool) -> int:
        """Check that `slot` names a slot of this slot session that is idle / carries a stream -> its index."""
        name = f"{type(self).__name__}.{what}"
        if not hasattr(self, "init_slots"):
            raise NotImplementedError(f"{name}: {type(self).__name__} has no slot sessions: its streams start together in "
                                      f"init_streams() and end together in flush()")
        if self.streams is None or self._slots is None:
            raise RuntimeError(f"{name}: not a slot session; call init_slots() (an init_streams() session starts and ends "
                               f"all its streams at once, with flush())")
        if not isinstance(slot, int) or isinstance(slot, bool) or not 0 <= slot < self.streams:
            raise IndexError(f"{name}: slot {slot!r} is out of range; this session has slots 0 .. {self.streams - 1}")
        if idle and self._slots[slot] is not None:
            raise RuntimeError(f"{name}: slot {slot} carries a stream; close({slot}) it first, or take one of the idle slots "
                               f"{[i for i, st in enumerate(self._slots) if st is None]}")
        if not idle and self._slots[slot] is None:
            raise RuntimeError(f"{name}: slot {slot} is idle; open({slot}) starts a stream in it")
        return slot

    @torch.no_grad()
    def open(self, slot: int, enroll: Optional[torch.Tensor] = None) -> None:
        """Start a stream in the idle slot `slot`: its first input hop is the first hop of the next step / step_chunk call.
        enroll [L'] or [1, L'] on the model's device, where the streamer's model takes one; what it seeds is computed here,
        once.  No synchronisation, no captured graph is touched."""
        name = f"{type(self).__name__}.open"
        slot = self._slot(slot, "open", idle=True)
        required, why = self._enrolment_rule()
        if (enroll is not None) != required:
            raise ValueError(f"{name}: an enrolment [L'] is required {why}")
        if enroll is not None:
            enroll = self._one_enrolment(enroll, name)
        self._start_slot(slot, enroll, name)

    def _one_enrolment(self, enroll: torch.Tensor, name: str) -> torch.Tensor:
        """open()'s checks of an enrolment -> [1, L']."""
        hip.require_device(enroll, name)
        if enroll.device != self.device:
            raise RuntimeError(f"{name}: the enrolment is on {enroll.device}, the session on {self.device}; move it with "
                               f".to({str(self.device)!r})")
        enroll = enroll[None] if enroll.dim() == 1 else enroll
        if enroll.dim() != 2 or enroll.shape[0] != 1:
            raise ValueError(f"{name}: enroll must be [L'] or [1, L'] (one stream), got {tuple(enroll.shape)}")
        return enroll

    def _start_slot(self, slot: int, seed, name: str) -> None:
        """The rest of open() once its arguments are checked; `seed` is what the streamer's _open_slot takes."""
        if self.frames + self.prime_hops > FRAME_LIMIT:
            raise RuntimeError(f"{name}: the session is at its limit of {FRAME_LIMIT} frames (an int32 frame counter); close "
                               f"the streams and call init_slots() for a new session")
        self._check_parameters()
        self._open_slot(slot, seed)
        self._queue[slot].zero_()
        self._tail[slot].zero_()
        # frames counter .. counter + window / hop - 2 see a partly filled window: dead.  (device-side add: no read-back)
        self._span[slot, 0:1] = self._counter + self._fill_hops
        self._span[slot, 1:2] = INT32_MAX
        self._slots[slot] = dict(hops=0, total=None, drained=0)

    def _flush_slot(self, out: torch.Tensor, slot: int) -> None:
        """close()'s flush of one slot's tail row -> out [1, window - hop] (a streamer whose flush reads the slot's span
        overrides this)."""
        self._flush_into(out, self._tail[slot:slot + 1])

    def _needs(self, st: dict, more: int, what: str, slot: int) -> None:
        """flush()'s rule per slot: a stream that ends after fewer than window samples has no frame."""
        need = self.window // self.hop_length
        if st["hops"] + more < need:
            raise RuntimeError(f"{type(self).__name__}.{what}: the stream in slot {slot} would end after "
                               f"{(st['hops'] + more) * self.hop_length} samples, and a stream needs {self.window} (no "
                               f"complete frame yet): step {need - st['hops'] - more} more hops of it first")

    @torch.no_grad()
    def end(self, slot: int, hops: int) -> None:
        """The stream in `slot` has `hops` >= 0 more hops of input: frames after them are dead, whatever the caller pads the
        rest of a chunk with, and the slot's later output hops drain its overlap-add tail."""
        name = f"{type(self).__name__}.end"
        slot = self._slot(slot, "end", idle=False)
        st = self._slots[slot]
        if not isinstance(hops, int) or hops < 0:
            raise ValueError(f"{name}: hops = {hops!r}: the whole hops of input still to come, >= 0")
        if st["total"] is not None:
            raise RuntimeError(f"{name}: slot {slot} was ended already ({st['total'] - st['hops']} hops to go); close({slot}) "
                               f"frees it")
        self._needs(st, hops, "end", slot)
        self._span[slot, 1:2] = self._counter + hops
        st["total"] = st["hops"] + hops

    @torch.no_grad()
    def close(self, slot: int) -> torch.Tensor:
        """-> [window - hop]: what is left of the slot's overlap-add tail, through the output constraint; the slot is idle
        again.  Without an earlier end() the stream ends now.  (The slot's model state stays as it is: nothing reads or
        writes it while the slot is idle, and open() resets it.)"""
        slot = self._slot(slot, "close", idle=False)
        st = self._slots[slot]
        D = self.delay_frames
        if st["total"] is None:
            if D:
                raise RuntimeError(f"{type(self).__name__}.close: the model holds the last {D} frames of the stream in slot "
                                   f"{slot}: call end({slot}, 0), step {D} more hops of the session (they carry those frames "
                                   f"out; the slot's input in them is ignored), then close({slot})")
            self._needs(st, 0, "close", slot)
        elif st["hops"] < st["total"]:
            raise RuntimeError(f"{type(self).__name__}.close: end({slot}, ..) announced {st['total'] - st['hops']} more hops "
                               f"of input; step them first")
        elif st["drained"] < D:
            raise RuntimeError(f"{type(self).__name__}.close: the model still holds {D - st['drained']} frames of the stream "
                               f"in slot {slot}: step {D - st['drained']} more hops of the session first (the slot's input in "
                               f"them is ignored)")
        self._ready()
        if st["total"] is None:
            self.end(slot, 0)
        out = torch.empty(1, self.window - self.hop_length, dtype=torch.float32, device=self.device)
        self._flush_slot(out, slot)
        self._tail[slot].zero_()
        self._span[slot].zero_()
        self._slots[slot] = None
        return out[0]
