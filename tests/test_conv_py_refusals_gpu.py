"""The depthwise-conv, encoder / decoder, conv2d and iSTFT wrappers of hip.py refuse, with a RuntimeError and before any
launch, every operand that would reach a kernel as a wild pointer: one on the CPU, in half precision (fp32 for the fp16x2
weight image) or non-contiguous.  Nothing here launches a kernel (the module is imported as `front`, so the ledger of
tests/test_abi_coverage.py does not count these calls as tests of the entries).  Smallest valid shapes: N = 1, four
channels, ld = 128."""
import pytest
import torch

from puresound_amd import hip as front

pytestmark = pytest.mark.gpu

LD, SENTINEL = 128, 7.0
GEOMETRY = (4, 3, 1, 1, 1, 1, 1, 0, False)   # f_out, kf, kt, stride_f, dil_f, dil_t, pad_f, pad_t, transposed


def _z(*shape, device="cuda", dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device=device)


def _bad(kind, *shape, dtype=torch.float32):
    """A tensor of `shape` that is on the CPU, of the other precision, or every second element of a wider one."""
    if kind == "cpu":
        return _z(*shape, device="cpu", dtype=dtype)
    if kind == "dtype":
        return _z(*shape, dtype=torch.float16 if dtype == torch.float32 else torch.float32)
    return _z(*shape[:-1], 2 * shape[-1], dtype=dtype)[..., ::2]


X4 = lambda: _z(1, 4, 4, LD)                                                   # noqa: E731
WT = lambda: _z(1, 16, 256)                                                    # noqa: E731  (pack_wt of [4, 12])
IMG = lambda: _z(1, 1, 2, 2, 4, 16, 8, dtype=torch.float16)                    # noqa: E731  (pack_conv2d_f16x2 of [4, 12])
# operand -> call(out, bad): `bad` builds the operand under test from a shape
CASES = {
    "free_encode:w": lambda out, bad: front.free_encode(_z(1, 64), bad(4, 1, 32), 16),
    "free_decode:w": lambda out, bad: front.free_decode(_z(1, 4, LD), 2, bad(4, 1, 32), 16, out=out),
    "free_decode:mask": lambda out, bad: front.free_decode(_z(1, 4, LD), 2, _z(4, 1, 32), 16, bad(1, 4, LD), out=out),
    "free_decode_moments:mask": lambda out, bad: front.free_decode_moments(_z(1, 4, LD), 2, _z(4, 1, 32), 16, _z(1, 48),
                                                                           bad(1, 4, LD), out=out),
    "dwconv:w": lambda out, bad: front.dwconv(_z(1, 4, LD), 100, bad(4, 1, 3), _z(4), 1, 1),
    "dwconv:b": lambda out, bad: front.dwconv(_z(1, 4, LD), 100, _z(4, 1, 3), bad(4), 1, 1),
    "unfold2d:x2": lambda out, bad: front.unfold2d(X4(), bad(1, 4, 4, LD), 100, *GEOMETRY),
    "conv2d:x2": lambda out, bad: front.conv2d(X4(), bad(1, 4, 4, LD), WT(), None, 4, 100, *GEOMETRY),
    "conv2d:wt": lambda out, bad: front.conv2d(X4(), None, bad(1, 16, 256), None, 4, 100, *GEOMETRY),
    "conv2d:bias": lambda out, bad: front.conv2d(X4(), None, WT(), bad(4), 4, 100, *GEOMETRY),
    "conv2d:slope": lambda out, bad: front.conv2d(X4(), None, WT(), None, 4, 100, *GEOMETRY, "prelu", bad(2)),
    "conv2d_stats:x2": lambda out, bad: front.conv2d_stats(X4(), bad(1, 4, 4, LD), WT(), None, 4, 100, *GEOMETRY),
    "conv2d_stats:wt": lambda out, bad: front.conv2d_stats(X4(), None, bad(1, 16, 256), None, 4, 100, *GEOMETRY),
    "conv2d_stats:bias": lambda out, bad: front.conv2d_stats(X4(), None, WT(), bad(4), 4, 100, *GEOMETRY),
    "conv2d_f16x2:x2": lambda out, bad: front.conv2d_f16x2(X4(), bad(1, 4, 4, LD), IMG(), 0, None, 4, 100, *GEOMETRY),
    "conv2d_f16x2:wimg": lambda out, bad: front.conv2d_f16x2(X4(), None, bad(1, 1, 2, 2, 4, 16, 8, dtype=torch.float16), 0, None,
                                                             4, 100, *GEOMETRY),
    "conv2d_f16x2:bias": lambda out, bad: front.conv2d_f16x2(X4(), None, IMG(), 0, bad(4), 4, 100, *GEOMETRY),
    "conv2d_f16x2:slope": lambda out, bad: front.conv2d_f16x2(X4(), None, IMG(), 0, None, 4, 100, *GEOMETRY, "prelu",
                                                              bad(2)),
    "istft_ola:window": lambda out, bad: front.istft_ola(_z(1, 32, LD), 2, bad(32), 16),
}


@pytest.mark.parametrize("kind", ["cpu", "dtype", "strided"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_wild_pointers_are_refused_before_any_launch(case, kind):
    out = torch.full((1, 48), SENTINEL, device="cuda")   # (T - 1) * hop + win of the decoder cases
    with pytest.raises(RuntimeError, match=rf"^{case.split(':')[0]}: "):   # (hip.py's, not the library's)
        CASES[case](out, lambda *shape, **kw: _bad(kind, *shape, **kw))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
