"""Spectral scores of the reference's loss/stft_loss.py, forward only (evaluation of enhanced speech; the inference stack
has no autograd): `stft` (puresound/nnet/loss/stft_loss.py:8-24), `SpectralConvergengeLoss` (:27-42),
`LogSTFTMagnitudeLoss` (:45-60), `STFTLoss` (:63-92), `MultiResolutionSTFTLoss` (:95-141), `over_suppression_loss`
(:144-153), with the reference's names, constructor orders and defaults.

With x / y the clamped magnitudes sqrt(clamp(re^2 + im^2, min=1e-7)) of estimate / reference, every score is algebra on
four sums over frames and bins, which `STFTLoss.moments` returns per utterance in fp64:
  S0 = sum (y-x)^2   S1 = sum y^2   S2 = sum |log y - log x|   S3 = sum relu(y^p - x^p)^2
  sc = sqrt(sum_n S0) / sqrt(sum_n S1)      mag = sum_n S2 / (N frames bins)      ov = sum_n S3 / (N frames bins)
(the reductions run over the whole batch, as in the reference).

CPU tensors: stock ATen (`torch.stft(..., return_complex=True)` and elementwise ops); this defines the semantics.  On a ROCm
device: hip.frame_reflect -> hip.conv1x1 against the windowed Fourier basis (exact fp32 products, the window's support
only) -> hip.spec_pair_moments; estimate and reference share each launch as rows n and N + n.  The scores are formed from
the sums on the device, without a host sync.

Rows of unequal length (`lengths=`, not in the reference: N host ints): row n's sums are those of its first lengths[n]
samples alone -- T_n = hip.stft_frames(lengths[n], fft_size, hop) frames, reflect-padded at the row's own end, whatever the
row holds behind them -- and the batch values are the same formulas over the elements that exist:
  sc = sqrt(sum_n S0) / sqrt(sum_n S1)      mag = sum_n S2 / (bins sum_n T_n)      ov = sum_n S3 / (bins sum_n T_n)
CPU tensors: each row alone through the path above.  Device: hip.frame_reflect_rows -> hip.conv1x1 over all T columns (those
behind T_n are zeros) -> hip.spec_pair_moments_rows, the lengths and the T_n of every resolution in one int32 copy.
"""
import math

import torch
import torch.nn as nn

from ... import hip
from .._plans import PlanCache

CLAMP = 1e-7


def _check_pair(who: str, x: torch.Tensor, y: torch.Tensor) -> None:
    if x.dim() != 2 or y.dim() != 2:
        raise RuntimeError(f"{who}: need input shape as (batch, length) (got {tuple(x.shape)} and {tuple(y.shape)})")
    if x.shape != y.shape or x.device != y.device:
        raise RuntimeError(f"{who}: estimate and reference must have one shape on one device (got {tuple(x.shape)} on "
                           f"{x.device} and {tuple(y.shape)} on {y.device})")


def _check_resolution(who: str, length: int, fft_size: int, hop_size: int, win_length: int, window: torch.Tensor) -> None:
    if win_length > fft_size:
        raise RuntimeError(f"{who}: win_length {win_length} exceeds fft_size {fft_size}")
    if window.dim() != 1 or window.shape[0] != win_length:
        raise RuntimeError(f"{who}: the window must hold win_length = {win_length} samples (got {tuple(window.shape)})")
    if hop_size < 1:
        raise RuntimeError(f"{who}: hop_size must be positive (got {hop_size})")
    if length <= fft_size // 2:
        raise RuntimeError(f"{who}: reflect padding needs more than fft_size // 2 samples: length {length} with "
                           f"fft_size {fft_size}")


def _host_rows(who: str, n: int, length: int, lengths, fft_sizes) -> list:
    """Per-row `lengths` of a batch [N, L] (N Python ints or a CPU integer tensor [N]; host values) -> the list, validated
    against the row length and against every resolution of the call: reflect padding at a row's own end needs
    lengths[n] > fft_size // 2."""
    from ..ragged import host_lengths
    lens = host_lengths("lengths", lengths, n, length, None, who=who)
    for fft_size in fft_sizes:
        for i, v in enumerate(lens):
            if v <= fft_size // 2:
                raise RuntimeError(f"{who}: reflect padding needs more than fft_size // 2 samples: lengths[{i}] = {v} with "
                                   f"fft_size {fft_size}")
    return lens


def limit_rows(lens, resolutions) -> list:
    """The host integers a device call with per-row lengths reads, [1 + R][N]: the lengths, then per resolution
    (fft_size, hop_size) the frame counts T_n.  A caller with limits of its own (inference_scored_ragged) appends them to its
    one copy (hip.row_limits) and hands the device rows back as `limits`."""
    return [list(lens)] + [[hip.stft_frames(v, f, h) for v in lens] for f, h in resolutions]


def check_rows(who: str, loss, n: int, length: int, lengths) -> list:
    """What `loss` (an STFTLoss or a MultiResolutionSTFTLoss) would refuse signals [N, length] with per-row `lengths` for,
    raised here: a caller that launches before it scores (inference_scored_ragged) asks first.  -> [(fft_size, hop_size)] per
    resolution."""
    parts = list(loss.stft_losses) if isinstance(loss, MultiResolutionSTFTLoss) else [loss]
    for f in parts:
        _check_resolution(who, length, f.fft_size, f.shift_size, f.win_length, f.window)
    _host_rows(who, n, length, lengths, [f.fft_size for f in parts])
    return [(f.fft_size, f.shift_size) for f in parts]


def fourier_basis(window: torch.Tensor, fft_size: int) -> torch.Tensor:
    """fp32 [2 * bins, win]: rows m < bins are w[k] cos(2 pi m (k + off) / fft_size), rows bins + m the same with sin,
    off = (fft_size - win) // 2 (torch.stft's centred, zero-padded window); built in fp64 on the host, the angle reduced
    mod fft_size in integers.  (The sign of the imaginary part does not matter to a magnitude.)"""
    w = window.detach().to(device="cpu", dtype=torch.float64)
    win, bins = w.shape[0], fft_size // 2 + 1
    k = torch.arange(win, dtype=torch.int64) + (fft_size - win) // 2
    ang = (torch.arange(bins, dtype=torch.int64)[:, None] * k[None, :] % fft_size).double() * (2.0 * math.pi / fft_size)
    return torch.cat([torch.cos(ang) * w, torch.sin(ang) * w]).float()


def _packed_basis(window: torch.Tensor, fft_size: int, device) -> torch.Tensor:
    return hip.pack_wt(fourier_basis(window, fft_size).to(device))


# Kept scratch of the device path, one flat buffer per (device, stream) that every resolution carves its frames and its
# spectrogram from: [2N][win][ldt] + [2N][2 bins][ldt] floats, grown to the largest resolution seen.  Nothing is read from it
# that the same call did not write.  It belongs to no module, because the resolutions of a MultiResolutionSTFTLoss and
# over_suppression_loss, a function, share it: release_scratch() frees it.  Callers that share a stream share the buffer, as
# they share the stream's order.
_WORK = {}
# over_suppression_loss has no module to keep its basis: (device, fft_size, win_length) -> packed basis of the Hann window
_OV_BASIS = {}


def release_scratch() -> None:
    """Drop the kept scratch of the device path and over_suppression_loss's packed bases (every device, every stream); the next
    call allocates and packs again.  The caller orders this behind the scores still in flight."""
    _WORK.clear()
    _OV_BASIS.clear()


def kept_tensors() -> list:
    """What this file keeps alive outside the modules' plan caches."""
    return list(_WORK.values()) + list(_OV_BASIS.values())


def _work(device: torch.device, floats: int) -> torch.Tensor:
    key = (device, torch.cuda.current_stream(device).cuda_stream)   # (a tensor's device: it carries its index)
    buf = _WORK.get(key)
    if buf is None or buf.numel() < floats:
        _WORK.pop(key, None)
        buf = _WORK[key] = torch.empty(floats, dtype=torch.float32, device=device)
    return buf


def _device_moments(x: torch.Tensor, y: torch.Tensor, fft_size: int, hop_size: int, win_length: int, wt: torch.Tensor,
                    p: float, want_mag: bool = False, limits=None):
    """-> (fp64 sums [N, 4], T, magnitudes [2N, bins, ldt] or None) on the HIP path.  limits: (lengths, T_n) as int32 [N] on
    the device -- row n is framed as an utterance of lengths[n] samples on its own and summed over its T_n frames; the product
    in between runs over all T columns, those behind T_n being the zeros the framing wrote."""
    hip.require_device(x, "stft_loss")
    hip.require_device(y, "stft_loss")
    n, length = x.shape
    bins, t = fft_size // 2 + 1, hip.stft_frames(length, fft_size, hop_size)
    ldt = hip.padded_frames(t)
    f_floats, s_floats = 2 * n * win_length * ldt, 2 * n * 2 * bins * ldt
    buf = _work(x.device, f_floats + s_floats)
    frames = buf[:f_floats].view(2 * n, win_length, ldt)
    spec = buf[f_floats:f_floats + s_floats].view(2 * n, 2 * bins, ldt)
    if limits is not None:
        hip.frame_reflect_rows(x, y, limits[0], fft_size, win_length, hop_size, out=frames)
        hip.conv1x1(frames, t, wt, 2 * bins, out=spec)
        return hip.spec_pair_moments_rows(spec, bins, t, limits[1], p), t, None
    hip.frame_reflect(x, y, fft_size, win_length, hop_size, out=frames)
    hip.conv1x1(frames, t, wt, 2 * bins, out=spec)
    mag = torch.empty(2 * n, bins, ldt, dtype=torch.float32, device=x.device) if want_mag else None
    return hip.spec_pair_moments(spec, bins, t, p, mag), t, mag


def _cpu_magnitudes(x: torch.Tensor, fft_size: int, hop_size: int, win_length: int, window: torch.Tensor) -> torch.Tensor:
    spec = torch.stft(x, fft_size, hop_size, win_length, window.to(device=x.device, dtype=x.dtype), return_complex=True)
    return torch.sqrt(torch.clamp(spec.real ** 2 + spec.imag ** 2, min=CLAMP)).transpose(2, 1)


def _cpu_moments(x_mag: torch.Tensor, y_mag: torch.Tensor, p: float) -> torch.Tensor:
    x, y = x_mag.double(), y_mag.double()
    over = torch.relu(y.pow(p) - x.pow(p))
    return torch.stack([((y - x) ** 2).sum((1, 2)), (y * y).sum((1, 2)), (y.log() - x.log()).abs().sum((1, 2)),
                        (over * over).sum((1, 2))], dim=-1)


def _moments(who: str, x: torch.Tensor, y: torch.Tensor, fft_size: int, hop_size: int, win_length: int,
             window: torch.Tensor, p: float, packed, lengths=None, limits=None):
    """-> (fp64 sums [N, 4], elements of the batch's spectrograms).  packed: () -> the packed basis on x's device.
    lengths: row n's sums are those of x[n:n+1, :lengths[n]], y[n:n+1, :lengths[n]] alone -- T_n = stft_frames(lengths[n]) frames,
    reflect-padded at the row's own end -- and the elements are bins * sum_n T_n.  CPU tensors take each row alone through
    torch.stft; on a device the lengths and the T_n go there in one int32 copy, unless the caller hands them in as `limits` =
    (lengths, T_n), int32 [N] each."""
    _check_pair(who, x, y)
    _check_resolution(who, x.shape[1], fft_size, hop_size, win_length, window)
    bins = fft_size // 2 + 1
    if lengths is None:
        if x.device.type == "cpu":
            x_mag = _cpu_magnitudes(x, fft_size, hop_size, win_length, window)
            y_mag = _cpu_magnitudes(y, fft_size, hop_size, win_length, window)
            return _cpu_moments(x_mag, y_mag, p), x.shape[0] * x_mag.shape[1] * bins
        m, t, _ = _device_moments(x, y, fft_size, hop_size, win_length, packed(), p)
        return m, x.shape[0] * t * bins
    lens = _host_rows(who, x.shape[0], x.shape[1], lengths, [fft_size])
    rows = limit_rows(lens, [(fft_size, hop_size)])
    count = bins * sum(rows[1])
    if x.device.type == "cpu":
        return torch.cat([_cpu_moments(_cpu_magnitudes(x[n:n + 1, :v], fft_size, hop_size, win_length, window),
                                       _cpu_magnitudes(y[n:n + 1, :v], fft_size, hop_size, win_length, window), p)
                          for n, v in enumerate(lens)]), count
    if limits is None:
        limits = hip.row_limits(who, rows, x.device)
    m, _, _ = _device_moments(x, y, fft_size, hop_size, win_length, packed(), p, limits=limits)
    return m, count


def _sc_mag(m: torch.Tensor, count: int):
    """fp64 (spectral convergence, log-magnitude distance) of a batch from its sums [N, 4] over `count` elements"""
    return torch.sqrt(m[:, 0].sum()) / torch.sqrt(m[:, 1].sum()), m[:, 2].sum() / count


@torch.no_grad()
def stft(x: torch.Tensor, fft_size: int, hop_size: int, win_length: int, window: torch.Tensor) -> torch.Tensor:
    """x [B, L] -> clamped magnitudes [B, frames, fft_size // 2 + 1] (stft_loss.py:8-24; torch.stft's rules: center=True,
    reflect padding, the window zero-padded to fft_size and centred).  On a ROCm device the basis is built from `window` at
    every call: STFTLoss keeps its own."""
    if x.dim() != 2:
        raise RuntimeError(f"stft: need input shape as (batch, length) (got {tuple(x.shape)})")
    _check_resolution("stft", x.shape[1], fft_size, hop_size, win_length, window)
    if x.device.type == "cpu":
        return _cpu_magnitudes(x, fft_size, hop_size, win_length, window)
    return _device_magnitudes(x, fft_size, hop_size, win_length, _packed_basis(window, fft_size, x.device))


def _device_magnitudes(x: torch.Tensor, fft_size: int, hop_size: int, win_length: int, wt: torch.Tensor) -> torch.Tensor:
    # (the pair kernel on (x, x): the magnitudes of the first half of the rows)
    _, t, mag = _device_moments(x, x, fft_size, hop_size, win_length, wt, 0.5, want_mag=True)
    return mag[:x.shape[0], :, :t].transpose(2, 1)


class SpectralConvergengeLoss(nn.Module):
    """stft_loss.py:27-42: ||y_mag - x_mag||_F / ||y_mag||_F over the whole batch (plain torch ops)."""

    @torch.no_grad()
    def forward(self, x_mag: torch.Tensor, y_mag: torch.Tensor) -> torch.Tensor:
        return torch.norm(y_mag - x_mag, p="fro") / torch.norm(y_mag, p="fro")


class LogSTFTMagnitudeLoss(nn.Module):
    """stft_loss.py:45-60: mean |log y_mag - log x_mag| (plain torch ops)."""

    @torch.no_grad()
    def forward(self, x_mag: torch.Tensor, y_mag: torch.Tensor) -> torch.Tensor:
        return torch.nn.functional.l1_loss(torch.log(y_mag), torch.log(x_mag))


class STFTLoss(PlanCache, nn.Module):
    """stft_loss.py:63-92: same constructor, buffer and forward value (sc_loss, mag_loss).  The window buffer may stay on
    the CPU while the signals are on a device (the recipes build the loss inside a closure and never move it): the packed
    basis follows the signals' device and is rebuilt when the buffer changes."""

    def __init__(self, fft_size: int = 1024, shift_size: int = 120, win_length: int = 600, window: str = "hann_window"):
        super().__init__()
        self.fft_size = fft_size
        self.shift_size = shift_size
        self.win_length = win_length
        self.register_buffer("window", getattr(torch, window)(win_length))
        self.spectral_convergenge_loss = SpectralConvergengeLoss()
        self.log_stft_magnitude_loss = LogSTFTMagnitudeLoss()

    def _build(self, device):
        return _packed_basis(self.window, self.fft_size, device)

    @torch.no_grad()
    def magnitudes(self, x: torch.Tensor) -> torch.Tensor:
        """stft(x, ...) of this resolution with the kept basis."""
        if x.dim() != 2:
            raise RuntimeError(f"STFTLoss: need input shape as (batch, length) (got {tuple(x.shape)})")
        _check_resolution("STFTLoss", x.shape[1], self.fft_size, self.shift_size, self.win_length, self.window)
        if x.device.type == "cpu":
            return _cpu_magnitudes(x, self.fft_size, self.shift_size, self.win_length, self.window)
        return _device_magnitudes(x, self.fft_size, self.shift_size, self.win_length, self._plan_get(x.device, self._build))

    def _sums(self, x: torch.Tensor, y: torch.Tensor, p: float = 0.5, lengths=None, limits=None):
        return _moments("STFTLoss", x, y, self.fft_size, self.shift_size, self.win_length, self.window, p,
                        lambda: self._plan_get(x.device, self._build), lengths, limits)

    @torch.no_grad()
    def moments(self, x: torch.Tensor, y: torch.Tensor, p: float = 0.5, lengths=None) -> torch.Tensor:
        """Not in the reference: x (estimate), y (reference) [N, L] -> fp64 [N, 4] = (S0, S1, S2, S3) of this resolution, on
        the signals' device.  lengths (N Python ints or a CPU integer tensor [N], each in (fft_size // 2, L]): row n's sums
        are those of x[n:n+1, :lengths[n]], y[n:n+1, :lengths[n]] alone, whatever the rows hold behind them; with
        frame_counts(lengths) a caller forms per-utterance scores from them."""
        return self._sums(x, y, p, lengths)[0]

    def frame_counts(self, lengths) -> list:
        """Not in the reference: T_n = frames of an utterance of lengths[n] samples at this resolution (its spectrogram holds
        T_n * (fft_size // 2 + 1) elements)."""
        return [hip.stft_frames(int(v), self.fft_size, self.shift_size) for v in lengths]

    @torch.no_grad()
    def forward(self, x: torch.Tensor, y: torch.Tensor, lengths=None, limits=None):
        """lengths: the reference's formulas over the elements that exist -- sc = sqrt(sum_n S0) / sqrt(sum_n S1),
        mag = sum_n S2 / (bins * sum_n T_n) with row n's sums those of its first lengths[n] samples alone.  limits: the device
        rows of limit_rows(lengths, ...) from a caller that copied them already."""
        sc, mag = _sc_mag(*self._sums(x, y, 0.5, lengths, limits))
        return sc.float(), mag.float()


class MultiResolutionSTFTLoss(nn.Module):
    """stft_loss.py:95-141: factor_sc * mean_r(sc_r) + factor_mag * mean_r(mag_r)."""

    def __init__(self, fft_sizes=[1024, 2048, 512], hop_sizes=[120, 240, 50], win_lengths=[600, 1200, 240],
                 window: str = "hann_window", factor_sc: float = 0.1, factor_mag: float = 0.1):
        super().__init__()
        assert len(fft_sizes) == len(hop_sizes) == len(win_lengths)
        self.stft_losses = nn.ModuleList()
        for fs, ss, wl in zip(fft_sizes, hop_sizes, win_lengths):
            self.stft_losses += [STFTLoss(fs, ss, wl, window)]
        self.factor_sc = factor_sc
        self.factor_mag = factor_mag

    @torch.no_grad()
    def resolutions(self) -> list:
        """(fft_size, hop_size) per resolution: what limit_rows takes"""
        return [(f.fft_size, f.shift_size) for f in self.stft_losses]

    @torch.no_grad()
    def forward(self, x: torch.Tensor, y: torch.Tensor, lengths=None, limits=None) -> torch.Tensor:
        """lengths / limits: as STFTLoss.forward's, per resolution; the lengths and every resolution's T_n go to the device in
        one copy (limits: int32 [1 + R, N], the device rows of limit_rows(lengths, self.resolutions()))."""
        _check_pair("MultiResolutionSTFTLoss", x, y)
        for f in self.stft_losses:   # every refusal before the first launch
            _check_resolution("MultiResolutionSTFTLoss", x.shape[1], f.fft_size, f.shift_size, f.win_length, f.window)
        per_res = [None] * len(self.stft_losses)
        if lengths is not None:
            lengths = _host_rows("MultiResolutionSTFTLoss", x.shape[0], x.shape[1], lengths,
                                 [f.fft_size for f in self.stft_losses])
            if x.device.type != "cpu":
                if limits is None:
                    limits = hip.row_limits("MultiResolutionSTFTLoss", limit_rows(lengths, self.resolutions()), x.device)
                per_res = [(limits[0], limits[1 + i]) for i in range(len(self.stft_losses))]
        sc_loss, mag_loss = 0.0, 0.0
        for f, lim in zip(self.stft_losses, per_res):
            sc, mag = _sc_mag(*f._sums(x, y, 0.5, lengths, lim))
            sc_loss = sc_loss + sc
            mag_loss = mag_loss + mag
        count = len(self.stft_losses)
        return (self.factor_sc * (sc_loss / count) + self.factor_mag * (mag_loss / count)).float()


def _over_suppression(who: str, enh: torch.Tensor, ref: torch.Tensor, p: float, fft_size: int, hop_size: int, win_length: int,
                      lengths) -> torch.Tensor:
    window = torch.hann_window(win_length)

    def packed():
        key = (enh.device, fft_size, win_length)   # (a tensor's device: it carries its index)
        if key not in _OV_BASIS:
            _OV_BASIS[key] = _packed_basis(window, fft_size, enh.device)
        return _OV_BASIS[key]

    m, count = _moments(who, enh, ref, fft_size, hop_size, win_length, window, p, packed, lengths)
    return (m[:, 3].sum() / count).float()


@torch.no_grad()
def over_suppression_loss(enh: torch.Tensor, ref: torch.Tensor, p: float = 0.5, fft_size: int = 512, hop_size: int = 128,
                          win_length: int = 512) -> torch.Tensor:
    """stft_loss.py:144-153: mean(relu(ref_mag^p - enh_mag^p)^2) with a Hann window."""
    return _over_suppression("over_suppression_loss", enh, ref, p, fft_size, hop_size, win_length, None)


@torch.no_grad()
def over_suppression_loss_ragged(enh: torch.Tensor, ref: torch.Tensor, lengths, p: float = 0.5, fft_size: int = 512,
                                 hop_size: int = 128, win_length: int = 512) -> torch.Tensor:
    """Not in the reference: over_suppression_loss of rows of unequal length -- the mean over the elements that exist,
    sum_n S3 / (bins * sum_n T_n), with row n's sum that of its first lengths[n] samples alone (STFTLoss.moments).  A function
    of its own: over_suppression_loss keeps the reference's signature, which the recipes' closures rely on."""
    return _over_suppression("over_suppression_loss_ragged", enh, ref, p, fft_size, hop_size, win_length, lengths)
