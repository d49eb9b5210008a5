"""The recurrence wrappers of hip.py refuse, with a RuntimeError and before any launch, every tensor that would reach a
kernel as a wild pointer: one on the CPU, of another dtype, non-contiguous, or an `out` of the wrong shape.  Nothing here
launches a recurrence (the module is imported as `front`, so the ledger of tests/test_abi_coverage.py does not count these
calls as tests of the entries).  Smallest shapes: N = 1, H = 64 (128 frame-major, 256 for h256), Q = 4, steps = 4, ldt = 128."""
import pytest
import torch

from puresound_amd import hip as front

pytestmark = pytest.mark.gpu

LDT, WALK = 128, (4, 4, 4, 1)   # Q, q_stride, steps, step_stride
SENTINEL = 7.0


def _z(*shape, device="cuda", dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device=device)


def _image(**kw):
    return _z(1, 8, 8, 2, 4, 2, 64, 8, dtype=torch.float16, **kw)


def _lstm(out, **kw):
    whh_t = kw.pop("whh_t", None)
    return front.lstm(_z(1, 256, LDT), _z(1, 64, 256) if whh_t is None else whh_t, 64, 1, *WALK, out=out, **kw)


def _h256(out, image=None, **kw):
    return front.lstm_fmajor_h256(_z(1, LDT, 1024), _image() if image is None else image, [1.0], 1, *WALK, out=out, **kw)


STATE = lambda **kw: _z(1, 64, LDT, **kw)   # noqa: E731
CASES = {
    "lstm_h0_on_the_cpu": lambda out: _lstm(out, h0=STATE(device="cpu")),
    "lstm_c0_in_fp16": lambda out: _lstm(out, c0=STATE(dtype=torch.float16)),
    "lstm_whh_t_not_contiguous": lambda out: _lstm(out, whh_t=_z(1, 256, 64).transpose(1, 2)),
    "lstm_whh_t_on_the_cpu": lambda out: _lstm(out, whh_t=_z(1, 64, 256, device="cpu")),
    "lstm_state_out_on_the_cpu": lambda out: _lstm(out, state_out=(STATE(device="cpu"), STATE(device="cpu"))),
    "lstm_state_out_of_another_shape": lambda out: _lstm(out, state_out=(_z(1, 32, LDT), _z(1, 32, LDT))),
    "lstm_gx_not_contiguous": lambda out: front.lstm(_z(1, LDT, 256).transpose(1, 2), _z(1, 64, 256), 64, 1, *WALK, out=out),
    "rnn_whh_t_on_the_cpu": lambda out: front.rnn(_z(1, 64, LDT), _z(1, 64, 64, device="cpu"), "RNN", 64, 1, *WALK),
    "rnn_bhn_in_fp16": lambda out: front.rnn(_z(1, 192, LDT), _z(1, 64, 192), "GRU", 64, 1, *WALK,
                                             bhn=_z(1, 64, dtype=torch.float16)),
    "rnn_h0_on_the_cpu": lambda out: front.rnn(_z(1, 64, LDT), _z(1, 64, 64), "RNN", 64, 1, *WALK, h0=STATE(device="cpu")),
    "lstm_fmajor_whh_t_on_the_cpu": lambda out: front.lstm_fmajor(_z(1, LDT, 512), _z(1, 128, 512, device="cpu"), 128, 1, *WALK),
    "h256_out_of_the_wrong_shape": lambda out: _h256(out[:, :, :64].contiguous()),
    "h256_out_not_contiguous": lambda out: _h256(_z(1, LDT, 256).transpose(1, 2)),
    "h256_image_not_contiguous": lambda out: _h256(out, image=_z(1, 8, 8, 2, 4, 2, 8, 64, dtype=torch.float16).transpose(-1, -2)),
    "h256_image_on_the_cpu": lambda out: _h256(out, image=_image(device="cpu")),
    "h256_h0_on_the_cpu": lambda out: _h256(out, h0=_z(1, 256, LDT, device="cpu")),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_wild_pointers_are_refused_before_any_launch(case):
    out = torch.full((1, 256 if case.startswith("h256") else 64, LDT), SENTINEL, device="cuda")
    front._COOP_LAST[0] = None
    with pytest.raises(RuntimeError, match=r"^(lstm|rnn|lstm_fmajor|lstm_fmajor_h256): "):   # (hip.py's, not the library's)
        CASES[case](out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and front._COOP_LAST[0] is None
