"""What follows from a FreeEncDec encoder and decoder around a masker, once for the streamers of the time-domain models
(tcn.py, dprnn.py, skim.py): the checks of the wrapper, encoder and window (`check_front`), of the mask pairing and the
constraints (`check_back`) and of a recurrent masker's mask head, channels, kernel and mode (`check_recurrent`); and
FreeEncSession, a HopSession whose chunk is stream_windows, frame, the encoder's conv1x1 (+ ReLU), the streamer's
`_masker(hops, bufs, feats) -> mask`, free_decode_step and stream_commit_frames.  A streamer provides `check_streamable`
(as a static method, too), `_masker`, `_buffers(hops)` (a dict with `n` = hops * B and `feats` [1, C, ld]) and its
`_build_packs` on top of `_free_packs`; RecurrentFreeSession has the buffers, the output_fc pack and the mask head of a
masker that ends in output_fc = (PReLU, 1x1 convolution)."""
from typing import Optional

import torch

from .. import hip
from ..nnet.base_nn import _MASK_ACTS, SoTaskWrapModule
from ..nnet.lobe.encoder import FreeEncDec
from ._session import K_MAX, HopSession

#: the 1x1 convolutions of dprnn.py and skim.py always run on at least this many columns (the rows are at least 128 wide; the
#: columns past the chunk hold values nobody reads): ps_conv1x1_f32 has another kernel, with another order of summation, for
#: 64 columns or fewer, and a stream's bits must not depend on how many columns share its launch
MIN_GEMM_COLUMNS = 65


def check_front(model, name: str) -> None:
    """The first checks of a check_streamable: the wrapper, the free encoder, its window."""
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


def check_back(model, name: str) -> None:
    """The checks behind the masker's own: the mask pairing and the two constraints."""
    pair = (model.mask_type.lower(), model.f_type.lower())
    if pair != ("real", "real"):
        raise NotImplementedError(f"{name}: mask pairing {pair}: the free encoder uses (real, real) only")
    if model.mask_constraint.lower() not in _MASK_ACTS:
        raise NotImplementedError(f"{name}: mask_constraint {model.mask_constraint!r}")
    if model.output_constraint.lower() not in ("linear", "sigmoid"):
        raise NotImplementedError(f"{name}: output_constraint {model.output_constraint!r}: linear or sigmoid")


def check_recurrent(model, name: str, masker: str, step_ok, entry: str, lds: str) -> None:
    """check_back for a `masker` (its name in words) that ends in output_fc and runs a block as one launch of `entry`
    (`step_ok(C, H, K)`: whether it has a kernel, `lds`: what one needs): the PReLU slope in front, then a mask per encoder
    channel, the kernel and the mode."""
    m = model.masker
    if m.output_fc[0].weight.numel() != 1:
        raise NotImplementedError(f"{name}: PReLU with per-channel slopes is not on the HIP path")
    check_back(model, name)
    c = model.encoder.encoder.weight.shape[0]
    if m.input_size != c or m.output_fc[1].out_channels != c:
        raise NotImplementedError(f"{name}: shapes: the encoder has {c} channels, the {masker} takes {m.input_size} and returns "
                                  f"{m.output_fc[1].out_channels}; a mask per encoder channel is needed")
    if not step_ok(m.input_size, m.hidden_size, m.seg_size):
        raise NotImplementedError(f"{name}: shapes: {entry} has no kernel for (C, H, K) = ({m.input_size}, "
                                  f"{m.hidden_size}, {m.seg_size}): a tile of 16 streams needs {lds}")
    if model.training:
        raise NotImplementedError(f"{name}: the model is in training mode -- call .eval()")


class FreeEncSession(HopSession):
    max_hops = K_MAX
    _how_to_start = "call init_streams() first (or init_slots())"
    #: the encoder's conv1x1 runs on at least this many columns
    _gemm_columns = 1

    def __init__(self, model: SoTaskWrapModule):
        self.check_streamable(model)
        super().__init__(model, model.encoder.win_length, model.encoder.hop_length)
        self.win_length = self.window

    def _free_packs(self, dev: torch.device) -> dict:
        """The encoder's and the decoder's weights, fp32, packed for the kernels."""
        f32 = dict(dtype=torch.float32, device=dev)
        enc = self.model.encoder
        return dict(enc_wt=hip.pack_wt(enc.encoder.weight.detach().to(**f32)[:, 0, :]),
                    dec_w=enc.decoder.weight.detach().to(**f32).contiguous())

    @staticmethod
    def _at_least_one(count: int, what: str) -> int:
        """The streams of init_streams / the capacity of init_slots."""
        if int(count) < 1:
            raise ValueError(f"{what} >= 1")
        return int(count)

    def _check_enrolments(self, enroll: torch.Tensor, b: int) -> None:
        """init_streams' checks of the enrolments of b streams."""
        name = f"{type(self).__name__}.init_streams"
        hip.require_device(enroll, name)
        if enroll.dim() != 2 or enroll.shape[0] != b:
            raise ValueError(f"{name}: enroll must be [{b}, L'], got {tuple(enroll.shape)}")

    def _body(self, hops: int) -> None:
        """`hops` frames of every stream: input _io[hops][0] [B, hops*hop] -> output _io[hops][1] [B, hops*hop]."""
        chunk, out, wins = self._io[hops]
        hop, win, pk = self.hop_length, self.win_length, self._packs
        bufs = self._buffers(hops)
        n, feats = bufs["n"], bufs["feats"]
        hip.stream_windows(self._queue, chunk, wins, hop)
        frames, _ = hip.frame(wins.view(1, -1), win, win)               # [1, win, ld]: column f*B + b
        hip.conv1x1(frames, max(n, self._gemm_columns), pk["enc_wt"], feats.shape[1], out=feats)
        if self.model.encoder.output_active:
            hip.activation_(feats, "relu", None, n)
        mask = self._masker(hops, bufs, feats)
        hip.free_decode_step(feats, mask, pk["dec_w"], self._tail, out, hop, hops, self._mask_act, self._out_mode,
                             span=self._span, counter=self._counter if self._span is not None else None)
        hip.stream_commit_frames(hip.commit_table([(wins[hops - 1], self._queue)]), self._counter, hops, self.device)

    def _flush_into(self, out: torch.Tensor, tail: Optional[torch.Tensor] = None) -> None:
        hip.free_decode_step(None, None, self._packs["dec_w"], self._tail if tail is None else tail, out, self.hop_length,
                             out_mode=self._out_mode, flush=True)


class RecurrentFreeSession(FreeEncSession):
    """A masker of C = input_size channels that ends in output_fc; every 1x1 convolution on MIN_GEMM_COLUMNS at least."""
    _gemm_columns = MIN_GEMM_COLUMNS

    def _free_packs(self, dev: torch.device) -> dict:
        fc = self.model.masker.output_fc
        f32 = dict(dtype=torch.float32, device=dev)
        slope = fc[0].weight.detach().to(**f32).contiguous()
        return dict(super()._free_packs(dev), out_wt=hip.pack_wt(fc[1].weight.detach().to(**f32)),
                    out_b=fc[1].bias.detach().to(**f32).contiguous(), out_slope=slope,
                    out_pro=hip.make_prologue(0, True, None, 0.0, 0.0, None, None, slope))

    def _buffers(self, hops: int) -> dict:
        """Activation buffers of a `hops`-frame chunk: [1, C, ld] over N = hops * B columns."""
        if hops not in self._bufs:
            n = hops * self.streams
            ld = hip.padded_frames(max(n, MIN_GEMM_COLUMNS))
            c = self.model.masker.input_size
            z = lambda: torch.zeros(1, c, ld, dtype=torch.float32, device=self.device)  # noqa: E731
            self._bufs[hops] = dict(n=n, feats=z(), x0=z(), x1=z(), mask=z())
        return self._bufs[hops]

    def _mask_head(self, x: torch.Tensor, bufs: dict) -> torch.Tensor:
        """output_fc on the last block's output -> the mask."""
        pk = self._packs
        hip.conv1x1(x, max(bufs["n"], MIN_GEMM_COLUMNS), pk["out_wt"], x.shape[1], pk["out_pro"], pk["out_b"], out=bufs["mask"])
        return bufs["mask"]
