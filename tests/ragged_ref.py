"""Float64 references and the shared batch of the ragged-batch tests (test_ragged_batch.py, test_ragged_batch_gpu.py).

Kernel level: plain torch in float64 for what csrc/ragged.hip computes -- the statistics of the valid frames as the mean and
rstd a consumer derives from the scaled partials (load_norm_scalars, ps_common.h), the depthwise convolution with a per-row
frame limit behind the three prologue kinds, the zeroed tail.

End to end: a batch of cfg2_short utterances of edge_length_cases' lengths, row n followed by junk, and per row the float64
oracle of the utterance alone (edge_length_cases.problem: computed once, shared, never written to)."""
import functools

import torch

import edge_length_cases as E
from detweights import det_wave

NONE, GLOBAL, AFFINE = 0, 1, 2
EPS = 1e-8

# T_n of the end-to-end batches.  The row limits bracket the 128-frame row granule and the 256-frame GEMM tile, one and two
# frames, and the full row.
CFG2_T = (301, 1, 2, 127, 129, 257)
CFG3_T = (301, 2, 129)
CFG3_ENROL_T = (186, 1, 129)
JUNK_GAIN = 20.0   # the junk behind an utterance: 20 x the signal's amplitude


# ---- kernel level ----------------------------------------------------------------------------------------------------------------
def valid_mask(t_rows, t):
    """[N, 1, T] bool: frame f of row n is valid"""
    return (torch.arange(t)[None, :] < torch.as_tensor(t_rows)[:, None])[:, None, :]


def stats_ref(y, t_rows):
    """y [N, R, T] -> (mean [N], rstd [N]) over r < R, f < t_rows[n], in float64 (biased variance, eps 1e-8)"""
    y = y.double()
    m = valid_mask(t_rows, y.shape[-1])
    cnt = torch.as_tensor(t_rows, dtype=torch.float64) * y.shape[1]
    mean = torch.where(m, y, 0.0).sum((1, 2)) / cnt
    var = torch.where(m, (y - mean[:, None, None]) ** 2, 0.0).sum((1, 2)) / cnt
    return mean, 1.0 / torch.sqrt(var + EPS)


def consumer_scalars(stats, count_full):
    """What load_norm_scalars makes of partials [N, parts, 2] under a launch-wide count: (mean [N], rstd [N]) in float64"""
    tot = stats.double().sum(1)
    mean = tot[:, 0] / count_full
    var = (tot[:, 1] / count_full - mean * mean).clamp_min(0.0)
    return mean, 1.0 / torch.sqrt(var + EPS)


def prologue_ref(x, kind, t_rows, gamma, beta, slope):
    """a = PReLU(norm(x)) in float64; GLOBAL takes each row's statistics over its valid frames"""
    a = x.double()
    if kind == GLOBAL:
        mean, rstd = stats_ref(x, t_rows)
        a = (a - mean[:, None, None]) * rstd[:, None, None]
    if kind != NONE:
        a = a * gamma.double()[None, :, None] + beta.double()[None, :, None]
    return torch.where(a >= 0, a, a * float(slope))


def dwconv_ragged_ref(x, t_rows, w, b, dilation, left, kind, gamma, beta, slope):
    """x [N, H, T] (junk behind each row's end), w [H, 1, P] -> y [N, H, T] float64: the depthwise convolution of each row's
    valid frames alone (zero padding outside them), 0 behind them"""
    n, h, t = x.shape
    p = w.shape[-1]
    m = valid_mask(t_rows, t)
    clean = torch.where(m, x.double(), 0.0)              # junk may be NaN: a select
    a = torch.where(m, prologue_ref(clean, kind, t_rows, gamma, beta, slope), 0.0)
    right = (p - 1) * dilation - left
    ap = torch.nn.functional.pad(a, (left, right))
    y = b.double()[None, :, None].expand(n, h, t).clone()
    for j in range(p):
        y = y + w.double()[None, :, 0, j, None] * ap[..., j * dilation:j * dilation + t]
    return torch.where(m, y, 0.0)


def zero_tail_ref(x, limits):
    """x [N, R, ld] -> a copy with 0 at columns >= limits[n]"""
    return torch.where(valid_mask(limits, x.shape[-1]), x, 0.0)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def lengths_of(name, frames):
    return [E.length_of(name, t) for t in frames]


@functools.lru_cache(maxsize=None)
def batch(name, frames, enrol_frames=None, junk="noise"):
    """-> (noisy [N, L], lengths, enroll [N, L'] or None, enroll_lengths or None, refs): row n of noisy is utterance n of
    edge_length_cases (the row-th utterance of its seeded batch, lengths_of(frames)[n] samples) followed by junk -- uniform
    noise at JUNK_GAIN x the signal's amplitude, or NaN; refs[n] [1, (T_n - 1) * hop + win] is the float64 oracle of the
    utterance alone."""
    lens = lengths_of(name, frames)
    e_lens = None if enrol_frames is None else lengths_of(name, enrol_frames)
    fill = (lambda seed, n, l: det_wave(seed, n, l) * (E.AMP * JUNK_GAIN)) if junk == "noise" else \
        (lambda seed, n, l: torch.full((n, l), float("nan")))
    noisy = fill(7001, len(lens), max(lens))
    enroll = None if e_lens is None else fill(7002, len(lens), max(e_lens))
    refs = []
    for n, length in enumerate(lens):
        kw = {} if e_lens is None else dict(enrol_length=e_lens[n])
        x, e, ref = E.problem(name, length, 1, row=n, **kw)
        noisy[n, :length] = x[0]
        if e is not None:
            enroll[n, :e_lens[n]] = e[0]
        refs.append(ref)
    return noisy, lens, enroll, e_lens, refs
