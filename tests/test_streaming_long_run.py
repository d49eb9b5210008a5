"""What ps_istft_step_f32 got wrong at large frame counters, shown without the kernel: the index arithmetic of its non-slot
branch before the fix (`base = t * hop`, `g = base + j`, `t_hi`, `t_lo`, `window[g - u * hop]`, all `int`) restated in numpy
int32 next to the same lines in int64 and next to the index the kernel uses now (`window[j + d * hop]`, which never forms
`t * hop`).  The GPU side is tests/test_streaming_long_run_gpu.py."""
import numpy as np
import pytest

SHAPES = [(64, 16), (48, 48), (512, 128), (32, 8)]          # (n_fft, hop); 48: not a power of two, no overlap
FRAME_LIMIT = 2 ** 31 - 1 - 16


def _tdiv(a, b):
    """C's integer division (it truncates; numpy's floors)."""
    return np.fix(a.astype(np.float64) / b.astype(np.float64)).astype(a.dtype)


def _old_window_indices(t, j, n_fft, hop, flush, itype):
    """The window indices the old lines visit for sample j of the launch at frame counter t, in the order they visit them,
    every quantity an `itype` as the kernel's were `int` (int32 wraps as the device's does)."""
    t, j, n_fft, hop, one = (np.array([v], dtype=itype) for v in (t, j, n_fft, hop, 1))
    with np.errstate(over="ignore"):
        base = t * hop
        t_last = t - one if flush else t
        g = base + j
        t_hi = np.minimum(_tdiv(g, hop), t_last)
        t_lo = np.zeros_like(g) if int((g - n_fft + one)[0]) <= 0 else _tdiv(g - n_fft + one + hop - one, hop)
        return [int((g - np.array([u], dtype=itype) * hop)[0]) for u in range(int(t_lo[0]), int(t_hi[0]) + 1)]


def _new_window_indices(t, j, n_fft, hop, flush):
    """The kernel's lines now: frames t - d, d_first >= d >= d_last, at window index j + d * hop."""
    d_first = min((n_fft - 1 - j) // hop, t)
    return [j + d * hop for d in range(d_first, (1 if flush else 0) - 1, -1)]


def _window_sum(indices, window):
    assert all(0 <= i < window.shape[0] for i in indices), f"window index out of [0, {window.shape[0]}): {indices}"
    return float(sum(window[i] ** 2 for i in indices))


def _full_sum(j, n_fft, hop, flush, window):
    """fp64 sum of w^2 over every frame that covers the sample (the stream is long past its first frames)."""
    return float(sum(window[i] ** 2 for i in range(j + (hop if flush else 0), n_fft, hop)))


def _samples(n_fft, hop, flush):
    emit = n_fft - hop if flush else hop
    return sorted({j for j in (0, 1, hop // 2, hop - 1, hop, emit - 1) if 0 <= j < emit})


def _check_above(itype):
    """From t = 2^31 / hop on, every sample still gets the whole window-square sum, from window entries inside the window."""
    for n_fft, hop in SHAPES:
        window = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
        first = -(-2 ** 31 // hop)                                    # the first t with t * hop >= 2^31
        wrap = -(-2 ** 32 // hop)
        for t in (first, first + 1, 2 ** 31 // hop + 3, wrap - 1, wrap, wrap + 2, FRAME_LIMIT - 1, FRAME_LIMIT):
            for flush in (False, True):
                for j in _samples(n_fft, hop, flush):
                    got = _window_sum(_old_window_indices(t, j, n_fft, hop, flush, itype), window)
                    assert got == pytest.approx(_full_sum(j, n_fft, hop, flush, window), rel=1e-12, abs=1e-300), \
                        (n_fft, hop, t, flush, j)


def test_old_index_arithmetic_is_right_in_int64_and_wrong_in_int32_from_2_31_samples_on():
    _check_above(np.int64)
    with pytest.raises(AssertionError):
        _check_above(np.int32)


def test_int32_and_int64_agree_below_2_31_samples_and_the_new_index_is_theirs():
    """Below t = 2^31 / hop the old lines were right, first frames included, and the new index visits the same window
    entries in the same order (so the fp32 sum keeps its bits); above, the new index is what int64 gives."""
    for n_fft, hop in SHAPES:
        edge = 2 ** 31 // hop
        below = list(range(0, n_fft // hop + 2)) + [1000, edge // 2] + list(range(edge - n_fft // hop - 1, edge))
        below = [t for t in below if t * hop + max(hop, n_fft - hop) <= 2 ** 31]     # (a flush reaches n_fft - hop samples on)
        above = [edge + 1, 2 ** 32 // hop - 1, -(-2 ** 32 // hop), FRAME_LIMIT]
        for t in below + above:
            for flush in (False, True):
                for j in _samples(n_fft, hop, flush):
                    wide = _old_window_indices(t, j, n_fft, hop, flush, np.int64)
                    assert _new_window_indices(t, j, n_fft, hop, flush) == wide, (n_fft, hop, t, flush, j)
                    assert all(0 <= i < n_fft for i in wide)
                    if t in below:
                        assert _old_window_indices(t, j, n_fft, hop, flush, np.int32) == wide, (n_fft, hop, t, flush, j)


def test_what_the_old_lines_did_past_the_edge():
    """The two failures by name: no frame at all once t * hop has passed 2^31 (an empty sum, so the division was skipped),
    and at t = 2^32 / hop - 1 (hop a power of two) a read in front of the window."""
    n_fft, hop = 512, 128
    for j in (0, 1, hop - 1):
        assert _old_window_indices(2 ** 31 // hop, j, n_fft, hop, False, np.int32) == []
        assert len(_old_window_indices(2 ** 31 // hop, j, n_fft, hop, False, np.int64)) == n_fft // hop
    t = 2 ** 32 // hop - 1
    assert _old_window_indices(t, 1, n_fft, hop, False, np.int32) == [1 - hop]
    assert _old_window_indices(t, hop - 1, n_fft, hop, False, np.int32) == [-1]
    assert min(_new_window_indices(t, 1, n_fft, hop, False)) == 1
