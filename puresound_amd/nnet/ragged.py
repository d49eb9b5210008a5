"""Batches of utterances of unequal length through SoTaskWrapModule.inference(noisy, enroll, lengths, enroll_lengths): the
host side -- what a call is refused for, and the per-row limits the kernels of csrc/ragged.hip read.

Row n of noisy [N, L] is an utterance of lengths[n] samples followed by junk; the result's row n is, on its first
(T_n - 1) * hop + win samples (T_n = (lengths[n] - win) // hop + 1), what inference(noisy[n:n+1, :lengths[n]]) returns for
that utterance alone, and exact 0.0 behind them.  Everything here runs on the host, before any launch, and is shared by the
HIP path (base_nn.py) and the CPU path (cpu_path.py), which loops over the rows and so defines the semantics without a GPU.

Covered: FreeEncDec encoder, the normal-TCN ConvTasNet masker on the fused driver (no cLN), and for `enroll_lengths` a
speaker net of plain TCN blocks -> AttentiveStatisticsPooling -> k=1 projection(s) (td_tse_conv_tasnet_v0[_causal]).  On
the HIP path also the noise suppressors of egs/ns: the conv-STFT encoder (ConvEncDec, Complex output, (complex, complex)
masks) in front of a DPCRN or DPARN with bN2d norms on the implicit-GEMM convolution, either transpose_delay, any delay,
no enrolment (ns_dpcrn_v0[_causal], ns_dparn_v0[_causal]); the CPU path has no stock-ATen DPCRN / DPARN and keeps refusing
them.  On the HIP path also FreeEncDec + SkiM without segment overlap, causal or not, FiLM fusion or no embedding, with the
plain-TCN speaker net above or SingleRNN(LSTM) -> AttentiveStatisticsPooling -> k=1 projection(s) (tse_skim_v0[_causal],
tse_skim_v0_causal_vad, tse_skim_v1_causal); the CPU path has no SkiM.  Everything else raises NotImplementedError.
Scoring such a batch: SoTaskWrapModule.inference_scored_ragged (base_nn.py), whose model refusals are check_model's and whose length values -- like the `lengths` of the scores in nnet/loss/ -- go through
host_lengths."""
from typing import List, NamedTuple, Optional, Sequence

import torch
import torch.nn as nn


def host_lengths(name: str, values, n: int, upper: Optional[int], win: Optional[int], who: str = "inference") -> List[int]:
    """`values` (a sequence of N Python ints or a CPU integer tensor [N]) -> the list, validated against the row length
    `upper` (None: there are no rows) and the encoder's window (None: the values of a score, which need one sample).  `who`
    names the caller in the messages: the scores of nnet/loss/ validate their `lengths` here too."""
    if torch.is_tensor(values):
        if values.is_cuda or values.is_floating_point() or values.dtype == torch.bool or values.dim() != 1:
            raise ValueError(f"{who}: {name} must be a sequence of ints or a CPU integer tensor [N] "
                             f"(got {values.dtype} {tuple(values.shape)} on {values.device})")
        values = values.tolist()
    else:
        values = list(values)
        if not all(isinstance(v, int) and not isinstance(v, bool) for v in values):
            raise ValueError(f"{who}: {name} must hold Python ints")
    if len(values) != n:
        raise ValueError(f"{who}: {name} holds {len(values)} values for a batch of {n} rows")
    for i, v in enumerate(values):
        if upper is not None and v > upper:
            raise ValueError(f"{who}: {name}[{i}] = {v} exceeds the row length {upper}")
        if win is None:
            if v < 1:
                raise ValueError(f"{who}: {name}[{i}] = {v} must be at least 1")
        elif v < win:  # (the wording of free_encode for an utterance shorter than one frame)
            raise RuntimeError(f"{who}: {name}[{i}]: input length {v} is shorter than the window {win}")
    return values


def frames(length: int, win: int, hop: int) -> int:
    return (length - win) // hop + 1


def _plain_speaker_net(net) -> bool:
    """plain TCN blocks on the fused driver -> AttentiveStatisticsPooling -> Conv1d(k=1, bias=False) projection(s)"""
    from .conv_tasnet import TCN
    from .lobe.pooling import AttentiveStatisticsPooling
    if not isinstance(net, (nn.ModuleList, nn.Sequential)):
        return False
    layers = list(net)
    i = 0
    while i < len(layers) and isinstance(layers[i], TCN) and layers[i].emb_dim == 0 and layers[i].fused_norms():
        i += 1
    if i == 0 or i >= len(layers) - 1 or not isinstance(layers[i], AttentiveStatisticsPooling):
        return False
    return all(isinstance(m, nn.Conv1d) and m.kernel_size == (1,) and m.bias is None for m in layers[i + 1:])


def _lstm_speaker_net(net) -> bool:
    """SingleRNN(LSTM) -> AttentiveStatisticsPooling -> Conv1d(k=1, bias=False) projection(s) (tse_skim_v1_causal)"""
    from .lobe.pooling import AttentiveStatisticsPooling
    from .lobe.rnn import SingleRNN
    if not isinstance(net, (nn.ModuleList, nn.Sequential)):
        return False
    layers = list(net)
    if len(layers) < 3 or not isinstance(layers[0], SingleRNN) or layers[0].rnn_type != "LSTM":
        return False
    if not isinstance(layers[1], AttentiveStatisticsPooling):
        return False
    return all(isinstance(m, nn.Conv1d) and m.kernel_size == (1,) and m.bias is None for m in layers[2:])


def skim(w) -> bool:
    """Whether `w` is of the FreeEncDec + SkiM family (check_model's third branch; _ragged_forward's)."""
    from .lobe.encoder import FreeEncDec
    from .skim import SkiM
    return isinstance(w.encoder, FreeEncDec) and isinstance(w.masker, SkiM)


def _check_skim(w, enroll: Optional[torch.Tensor], hip_path: bool, who: str) -> None:
    """FreeEncDec + SkiM: frames meet in the segment LSTMs (inside one segment: no limit needed once the features are zero
    behind T_n), in the Mem-LSTM over a row's segments and in a recurrent speaker net over the enrolment's frames, which
    have a per-row form on the HIP path (ps_lstm_rows_f32; the causal hand-over is shifted inside each row)."""
    from .lobe.encoder import FreeEncDec
    from .lobe.rnn import SingleRNN
    from .lobe.trivial import Gate, SpecAugment
    m = w.masker
    if not hip_path:
        raise NotImplementedError(f"{who}: SkiM behind the FreeEncDec encoder is covered on the HIP path only (the CPU path has "
                                  f"no stock-ATen SkiM)")
    if m.seg_overlap:
        raise NotImplementedError(f"{who}: SkiM with seg_overlap=True is not covered (the split's padding differs per row)")
    if any(isinstance(f, Gate) for f in getattr(m, "seg_input_fusion", [])):
        raise NotImplementedError(f"{who}: SkiM with Gate fusion is not covered (FiLM fusion or no embedding)")
    if w.embedding_free_tse:
        raise NotImplementedError(f"{who}: embedding_free_tse is not covered")
    if w.check_mask_pairing(w.mask_type, w.f_type) != "real":
        raise NotImplementedError(f"{who}: FreeEncDec encoder with (real, real) masks")
    if enroll is not None:
        if w.speaker_net is None:
            raise NotImplementedError(f"{who}: an enrolment needs a speaker_net")
        enc = w.encoder_spk if w.encoder_spk is not None else w.encoder
        layers = list(w.speaker_net) if isinstance(w.speaker_net, (nn.ModuleList, nn.Sequential)) else []
        if any(isinstance(lay, SpecAugment) for lay in layers):
            raise NotImplementedError(f"{who}: a speaker net with a SpecAugment layer is not covered (its random draws have no "
                                      f"per-row meaning)")
        if not isinstance(enc, FreeEncDec):
            raise NotImplementedError(f"{who}: with an enrolment in front of SkiM, a FreeEncDec enrolment encoder only (got "
                                      f"{type(enc).__name__})")
        if any(isinstance(lay, SingleRNN) and lay.rnn_type != "LSTM" for lay in layers):
            raise NotImplementedError(f"{who}: a SingleRNN speaker net that is not an LSTM is not covered (the per-row "
                                      f"recurrence is the LSTM's)")
        if not (_plain_speaker_net(w.speaker_net) or _lstm_speaker_net(w.speaker_net)):
            raise NotImplementedError(f"{who}: with an enrolment in front of SkiM, a speaker net of plain TCN blocks or "
                                      f"SingleRNN(LSTM) -> AttentiveStatisticsPooling -> k=1 projection(s) only")


def spectral(w) -> bool:
    """Whether `w` is of the conv-STFT family (check_model's second branch; _ragged_forward's)."""
    from .lobe.encoder import ConvEncDec
    return isinstance(w.encoder, ConvEncDec)


def _check_spectral(w, enroll: Optional[torch.Tensor], hip_path: bool, who: str) -> None:
    """The conv-STFT encoder in front of a DPCRN / DPARN: frames meet in the time taps of the 2-D convolutions and in the
    iSTFT's overlap-add, which have a per-row form on the HIP path (ps_conv2d_ragged_f32, ps_istft_ola_ragged_f32)."""
    from .conv_tasnet import ConvTasNet
    from .dparn import DPARN
    from .dpcrn import DPCRN
    m = w.masker
    if isinstance(m, ConvTasNet):
        raise NotImplementedError(f"{who}: an STFT encoder in front of a ConvTasNet is not covered (FreeEncDec + ConvTasNet, or "
                                  f"ConvEncDec + DPCRN / DPARN)")
    if type(m) not in (DPCRN, DPARN):
        raise NotImplementedError(f"{who}: behind the STFT encoder a DPCRN or DPARN masker only (got {type(m).__name__}; Unet, "
                                  f"UnetTcn, DPARN_Mout, DPRNN and SkiM have no per-row frame limit)")
    if not hip_path:
        raise NotImplementedError(f"{who}: {type(m).__name__} behind the STFT encoder is covered on the HIP path only (the CPU "
                                  f"path has no stock-ATen {type(m).__name__})")
    stft = w.encoder.encoder
    if stft.output_format != "Complex" or not hasattr(stft, "kernel_sin_inv"):
        raise NotImplementedError(f"{who}: the STFT encoder's Complex output with its iSTFT only")
    if w.check_mask_pairing(w.mask_type, w.f_type) != "complex":
        raise NotImplementedError(f"{who}: STFT encoder with (complex, complex) masks only (got ({w.mask_type}, {w.f_type}))")
    if getattr(m, "spectral_compress", False) or m.multi_output != 1:
        raise NotImplementedError(f"{who}: spectral_compress / multi_output maskers are not covered")
    reason = m.per_row_refusal()
    if reason:
        raise NotImplementedError(f"{who}: {type(m).__name__}: {reason}")
    if w.embedding_free_tse:
        raise NotImplementedError(f"{who}: embedding_free_tse is not covered")
    if enroll is not None:
        raise NotImplementedError(f"{who}: an enrolment is not covered behind the STFT encoder")


def check_model(w, enroll: Optional[torch.Tensor], enroll_lengths, hip_path: bool = False) -> None:
    """What the lengths path does not cover: raised before any launch, each with its reason.  hip_path: the call is on device
    tensors (the noise suppressors behind the STFT encoder have no CPU form)."""
    from .conv_tasnet import ConvTasNet
    from .lobe.encoder import FreeEncDec
    if enroll_lengths is not None and enroll is None:
        raise ValueError("inference: enroll_lengths was given without enroll")
    who = "inference with lengths"
    if spectral(w):
        return _check_spectral(w, enroll, hip_path, who)
    if skim(w):
        return _check_skim(w, enroll, hip_path, who)
    if not isinstance(w.encoder, FreeEncDec):
        raise NotImplementedError(f"{who}: the FreeEncDec encoder, or the conv-STFT encoder in front of a DPCRN / DPARN "
                                  f"(got {type(w.encoder).__name__})")
    if not isinstance(w.masker, ConvTasNet):
        raise NotImplementedError(f"{who}: behind the FreeEncDec encoder the Conv-TasNet or SkiM masker only (got "
                                  f"{type(w.masker).__name__}; the DPRNN and U-Net maskers have no per-row frame limit there)")
    if w.masker.tcn_layer.lower() != "normal":
        raise NotImplementedError(f'{who}: tcn_layer="{w.masker.tcn_layer}" is not covered (normal TCN blocks only)')
    if not all(m.fused_norms() for stack in w.masker.tcn_list for m in stack):
        raise NotImplementedError(f"{who}: a TCN stack with a cLN runs stage by stage, not on the fused driver, and is not covered")
    if w.embedding_free_tse:
        raise NotImplementedError(f"{who}: embedding_free_tse is not covered")
    if w.check_mask_pairing(w.mask_type, w.f_type) != "real":
        raise NotImplementedError(f"{who}: FreeEncDec encoder with (real, real) masks")
    if enroll is not None:
        if w.speaker_net is None:
            raise NotImplementedError(f"{who}: an enrolment needs a speaker_net")
        enc = w.encoder_spk if w.encoder_spk is not None else w.encoder
        if not isinstance(enc, FreeEncDec) or not _plain_speaker_net(w.speaker_net):
            raise NotImplementedError(f"{who}: with an enrolment, a FreeEncDec enrolment encoder and a speaker net of plain TCN "
                                      f"blocks -> AttentiveStatisticsPooling -> k=1 projection(s) only")


class Plan(NamedTuple):
    """The host side of one ragged call."""
    lengths: List[int]
    t_rows: List[int]            # T_n
    out_lengths: List[int]       # (T_n - 1) * hop + win
    enroll_lengths: Optional[List[int]]
    enroll_t_rows: Optional[List[int]]
    enroll_frames: int           # T' of the enrolment rows (0 without one)
    seg_rows: Optional[List[int]] = None   # SkiM: S_n = T_n // K + 1 segments per row


def plan(w, noisy: torch.Tensor, enroll: Optional[torch.Tensor], lengths, enroll_lengths,
         hip_path: Optional[bool] = None) -> Plan:
    """Refusals first, then the limits: everything a ragged call needs from the host.  hip_path: see check_model (None: whether
    `noisy` is a device tensor)."""
    check_model(w, enroll, enroll_lengths, noisy.device.type != "cpu" if hip_path is None else hip_path)
    if noisy.dim() != 2:
        raise ValueError(f"inference with lengths: noisy must be [N, L] (got {tuple(noisy.shape)})")
    n, length = noisy.shape
    win, hop = w.encoder.win_length, w.encoder.hop_length
    if enroll is not None and (enroll.dim() != 2 or enroll.shape[0] != n):
        raise RuntimeError("inference: noisy and enroll must have the same batch size")
    lens = host_lengths("lengths", [length] * n if lengths is None else lengths, n, length, win)
    t_rows = [frames(v, win, hop) for v in lens]
    e_lens = e_rows = None
    e_frames = 0
    if enroll is not None:
        enc = w.encoder_spk if w.encoder_spk is not None else w.encoder
        e_len = enroll.shape[1]
        e_lens = host_lengths("enroll_lengths", [e_len] * n if enroll_lengths is None else enroll_lengths, n, e_len,
                              enc.win_length)
        e_rows = [frames(v, enc.win_length, enc.hop_length) for v in e_lens]
        e_frames = frames(e_len, enc.win_length, enc.hop_length)
    seg_rows = [t // w.masker.seg_size + 1 for t in t_rows] if skim(w) else None
    return Plan(lens, t_rows, [(t - 1) * hop + win for t in t_rows], e_lens, e_rows, e_frames, seg_rows)


def relative_lengths(t_rows: Sequence[int], t: int) -> List[float]:
    """What AttentiveStatisticsPooling takes as `lengths` for T'_n of T' frames: (T'_n - 0.5) / T'.  The kernel keeps frame f
    iff float(f) < lengths[n] * float(T'); T'_n / T' can round across T'_n, the half-frame offset cannot."""
    return [(v - 0.5) / t for v in t_rows]
