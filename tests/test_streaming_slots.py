"""Slot sessions of StreamingConvTasNet (puresound_amd/streaming/tcn.py) without a GPU: the ABI of the two slot kernels and the
host-only length bookkeeping."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ps_dwconv_step_slots_f32", "ps_free_decode_step_slots_f32")


def _header():
    with open(os.path.join(ROOT, "include", "puresound_hip.h")) as f:
        return f.read()


def test_slot_entry_points_are_bound_and_declared():
    from puresound_amd import _abi
    header = _header()
    for name in NEW:
        assert name in _abi.SIGNATURES, name
        assert re.search(r"^int %s\(" % name, header, re.M), f"{name} is not declared in the header"
    # one more argument than the entry point each one is the sibling of: the span (the decoder: no flush, but the counter)
    n = lambda name: len(_abi.SIGNATURES[name][1])  # noqa: E731
    assert n("ps_dwconv_step_slots_f32") == n("ps_dwconv_step_f32") + 1
    assert n("ps_free_decode_step_slots_f32") == n("ps_free_decode_step_f32") + 1


def test_additions_keep_the_abi_number():
    from puresound_amd import _abi
    assert _abi.ABI_VERSION == 24
    header = _header()
    assert re.search(r"^#define PS_ABI_VERSION 24$", header, re.M)
    above = header[:header.index("#define PS_ABI_VERSION")][-400:].lower()
    assert "adds" in above and "keeps the number" in above, "the header says when the number moves"


def test_slot_kernels_are_in_the_source_as_compile_time_variants():
    with open(os.path.join(ROOT, "puresound_amd", "csrc", "tcn_step.hip")) as f:
        src = f.read()
    for name in NEW:
        assert re.search(r'extern "C" int %s\(' % name, src), name
    assert len(re.findall(r"^template <bool SLOTS", src, re.M)) == 2      # the depthwise body, the synthesis kernel
    assert "if constexpr (SLOTS)" in src


@pytest.mark.parametrize("win,hop", [(32, 16), (16, 8), (16, 16), (64, 16), (256, 4)])
@pytest.mark.parametrize("extra_hops", [0, 1, 7, 500])
def test_slot_output_range_is_the_offline_output_after_the_latency(win, hop, extra_hops):
    from puresound_amd.streaming import StreamingConvTasNet as S
    samples = win + extra_hops * hop
    r = S.slot_output_range(samples, win, hop)
    n = S.output_length(samples, win, hop)
    frames = (samples - win) // hop + 1
    assert r.start == win - hop                                   # latency_samples
    assert len(r) == n["emitted"] + n["flushed"] == (frames - 1) * hop + win
    # y = one output hop per input hop from open() on, then close(): win - hop more samples
    assert r.stop == samples + (win - hop)
    assert n["prime_hops"] * hop == r.start                       # the dead frames' output hops, exactly


def test_slot_output_range_refuses_what_output_length_refuses():
    from puresound_amd.streaming import StreamingConvTasNet as S
    for bad in ((31, 32, 16), (16, 32, 16), (64, 32, 12)):
        with pytest.raises(ValueError):
            S.slot_output_range(*bad)


def test_frame_limit_leaves_room_for_one_launch():
    from puresound_amd.streaming import tcn
    assert tcn.FRAME_LIMIT == 2 ** 31 - 1 - tcn.K_MAX
    assert tcn.INT32_MAX == 2 ** 31 - 1
