"""The session mechanics the hop-by-hop streamers share (spectral.py, tcn.py): B streams fed whole hops, a priming phase
while the first analysis window fills, then chunks of hops through the subclass's kernels -- eagerly, or as one captured
graph per number of hops in a launch -- and a flush of the overlap-add tail.

A streamer provides: `_build_packs(device)` (sets self._packs from the current parameters), `_state()` (every tensor a body
run advances), `_body(hops)` (the launches of `hops` hops: self._io[hops] = (input [B, hops*hop], output [B, hops*hop],
windows [hops, B*window])), `_flush_into(out)`; it may set `max_hops` and override `_around_body`.  Its init_streams checks
its own arguments, calls `_begin` and allocates what `_state` returns; `_queue` [B, window], `_tail` [B, window - hop] and
`_counter` (int32 [1], the device frame counter) are allocated here.
"""
import contextlib
from typing import Dict, Optional

import torch

from .. import hip
from ..graphs import capture
from ..nnet._plans import tensor_signature


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

    def __init__(self, model, window: int, hop: int):
        if model.training:
            raise RuntimeError(f"{type(self).__name__}: the model is in training mode -- call .eval()")
        self.model = model
        self.window, self.hop_length = int(window), int(hop)
        self.prime_hops = self.window // self.hop_length - 1
        self._mask_act = model.mask_constraint.lower()
        self._out_mode = model.output_constraint.lower()
        self.streams = None
        self._drop_weights()

    @property
    def latency_samples(self) -> int:
        """Samples between a sample entering and its value leaving: the analysis window minus one hop."""
        return self.window - self.hop_length

    @staticmethod
    def output_length(samples: int, n_fft: int, hop: int) -> Dict[str, int]:
        """Length bookkeeping of a stream of `samples` = k * hop input samples: priming hops, samples the steps emit, samples
        flush() returns (their sum is the offline output length (T - 1) * hop + n_fft, T = (samples - n_fft) // hop + 1)."""
        if samples % hop or n_fft % hop or samples < n_fft:
            raise ValueError("output_length: whole hops, n_fft a multiple of hop, at least one window")
        prime = n_fft // hop - 1
        frames = samples // hop - prime
        return dict(prime_hops=prime, frames=frames, emitted=frames * hop, flushed=n_fft - hop)

    # -- weights ------------------------------------------------------------------------------------------------------
    def _drop_weights(self) -> None:
        """Forget graphs and weight packs (they are rebuilt from the current parameters on next use)."""
        self._graphs: Dict[int, torch.cuda.CUDAGraph] = {}
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
        self._graphs = {}
        self.streams, self.device, self._use_graph = int(streams), device, bool(use_graph)
        self._hops = 0           # hops taken in, priming included
        self.frames = 0          # hops past the priming: frames computed
        self._finished = False
        self._queue = torch.zeros(self.streams, self.window, dtype=torch.float32, device=device)
        self._tail = torch.zeros(self.streams, self.window - self.hop_length, dtype=torch.float32, device=device)
        self._counter = torch.zeros(1, dtype=torch.int32, device=device)
        self._io: Dict[int, tuple] = {}

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
        return self._hops < self.prime_hops

    def _run_piece(self, piece: torch.Tensor) -> torch.Tensor:
        """Whole hops of one launch -> their output samples [B, hops*hop] (graph replay or eager)."""
        hops = piece.shape[1] // self.hop_length
        chunk, out, _ = self._io_for(hops)
        chunk.copy_(piece)
        if not self._use_graph:
            with self._around_body():
                self._body(hops)
        else:
            g = self._graphs.get(hops)
            if g is None:
                g = self._capture(hops)
            g.replay()
        self._hops += hops
        self.frames += hops
        return out.clone()

    def _run(self, chunk: torch.Tensor) -> torch.Tensor:
        """Whole hops past the priming -> their output samples, in pieces of at most max_hops hops."""
        self._ready()
        step = self.max_hops * self.hop_length if self.max_hops else chunk.shape[1]
        outs = [self._run_piece(chunk[:, i:i + step]) for i in range(0, chunk.shape[1], step)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)

    def _capture(self, hops: int) -> torch.cuda.CUDAGraph:
        """Warm up once eagerly on a side stream (allocates what the launches need), put the state back, capture."""
        with self._around_body():
            g, _ = capture(lambda: self._body(hops), self.device, self._state())
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
        window fills (the first window / hop - 1 hops)."""
        if self._check_input(hop, "step") != 1:
            raise ValueError(f"{type(self).__name__}.step: one hop of {self.hop_length} samples per stream")
        if self._priming():
            self._prime(hop)
            return None
        return self._run(hop)

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
        """The last window - hop_length samples of every stream ([B, window - hop_length]); the streams are then finished."""
        name = f"{type(self).__name__}.flush"
        if self.streams is None or self._finished:
            raise RuntimeError(f"{name}: no open streams")
        if self.frames == 0:
            raise RuntimeError(f"{name}: no complete frame yet (a stream needs {self.window} samples)")
        self._ready()
        out = torch.empty(self.streams, self.window - self.hop_length, dtype=torch.float32, device=self.device)
        self._flush_into(out)
        self._finished = True
        return out
