"""Slot sessions of StreamingUnetTcn (puresound_amd/streaming/unet_tcn.py) without a GPU: the ABI of the three slot kernels,
the span rule in fp64 (tests/unet_tcn_slots_ref.py) against each stream's offline result on its own, and the host-only length
bookkeeping with a model delay."""
import os
import re

import pytest
import torch

import gated_tcn_step_ref as G
import unet_delay_ref as UD
import unet_tcn_slots_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {  # entry: (its sibling, arguments more than the sibling, source file)
    "ps_conv2d_step_slots_f32": ("ps_conv2d_step_f32", 3, "stream_step.hip"),          # counter, span, shift
    "ps_istft_step_slots_f32": ("ps_istft_step_f32", 2, "stream_step.hip"),            # span, shift
    "ps_gated_tcn_step_slots_f32": ("ps_gated_tcn_step_f32", 1, "gated_tcn_step.hip"),  # span
}
# three streams: births 0 / 4 / 9, lengths 7 / 2 / 11 -- one shorter than the delay D = 3; dead frames hold 1e6
BIRTHS, LENGTHS, D, DEAD = (0, 4, 9), (7, 2, 11), 3, 1e6
SPAN = torch.tensor([[b, b + n] for b, n in zip(BIRTHS, LENGTHS)])
HOPS = max(b + n for b, n in zip(BIRTHS, LENGTHS)) + D + 6


def _read(*rel):
    with open(os.path.join(ROOT, *rel)) as f:
        return f.read()


def _args(decl):
    return [a.strip() for a in decl.split(",")]


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_slot_entry_points_are_declared_bound_and_defined():
    from puresound_amd import _abi
    header = re.sub(r"/\*.*?\*/", "", _read("include", "puresound_hip.h"), flags=re.S)
    for name, (sibling, more, src) in NEW.items():
        assert name in _abi.SIGNATURES, name
        decl = {n: re.search(r"^int %s\((.*?)\);" % n, header, re.M | re.S) for n in (name, sibling)}
        assert decl[name], f"{name} is not declared in the header"
        assert re.search(r'extern "C" int %s\(' % name, _read("puresound_amd", "csrc", src)), name
        assert len(_abi.SIGNATURES[name][1]) == len(_abi.SIGNATURES[sibling][1]) + more
        assert len(_args(decl[name].group(1))) == len(_args(decl[sibling].group(1))) + more == len(_abi.SIGNATURES[name][1])


def test_each_signature_is_its_siblings_plus_the_stated_arguments():
    header = re.sub(r"/\*.*?\*/", "", _read("include", "puresound_hip.h"), flags=re.S)
    norm = lambda n: [re.sub(r"\s+", " ", a) for a in _args(re.search(r"^int %s\((.*?)\);" % n, header, re.M | re.S).group(1))]  # noqa: E731
    conv, conv_s = norm("ps_conv2d_step_f32"), norm("ps_conv2d_step_slots_f32")
    assert conv_s == conv[:-1] + ["const int* counter", "const int* span", "int shift"] + conv[-1:]
    ist, ist_s = norm("ps_istft_step_f32"), norm("ps_istft_step_slots_f32")
    i = ist.index("const int* counter") + 1
    assert ist_s == ist[:i] + ["const int* span", "int shift"] + ist[i:]
    gat, gat_s = norm("ps_gated_tcn_step_f32"), norm("ps_gated_tcn_step_slots_f32")
    i = gat.index("const int* counter") + 1
    assert gat_s == gat[:i] + ["const int* span"] + gat[i:]


def test_additions_keep_the_abi_number():
    from puresound_amd import _abi
    assert _abi.ABI_VERSION == 24
    assert re.search(r"^#define PS_ABI_VERSION 24$", _read("include", "puresound_hip.h"), re.M)


def test_slot_kernels_are_compile_time_variants():
    """template <..., bool SLOTS, typename... Extra> kernels with `if constexpr (SLOTS)`, as csrc/tcn_step.hip: the slot
    arguments are a trailing pack, so the instantiation without a span keeps its kernel arguments (and its code)."""
    step, gated = _read("puresound_amd", "csrc", "stream_step.hip"), _read("puresound_amd", "csrc", "gated_tcn_step.hip")
    pat = r"^template <(?:int \w+, )*bool SLOTS, typename\.\.\. Extra>\n__global__"
    assert len(re.findall(pat, step, re.M)) == 2                       # the convolution, the iSTFT
    assert len(re.findall(pat, gated, re.M)) == 1
    for src, kernels in ((step, ("conv2d_step_kernel<16, 256, false>", "conv2d_step_kernel<16, 256, true, Conv2dStepSlots>",
                                 "istft_step_kernel<false>", "istft_step_kernel<true, IstftStepSlots>")),
                         (gated, ("gated_tcn_step_kernel<16, false>", "gated_tcn_step_kernel<16, true, const int*>"))):
        assert "if constexpr (SLOTS)" in src and "static_assert(sizeof...(Extra) == (SLOTS ? 1 : 0)" in src
        for k in kernels:
            assert k in src, k
    assert "conv2d_step_kernel(Conv2dStepArgs a, Extra... extra)" in step
    assert "gated_tcn_step_kernel(GatedStepArgs a, Extra... extra)" in gated


def test_wrappers_pick_the_entry_by_span():
    hip_py = _read("puresound_amd", "hip.py")
    for wrapper, entry in (("conv2d_step", "ps_conv2d_step_slots_f32"), ("istft_step", "ps_istft_step_slots_f32"),
                           ("gated_tcn_step", "ps_gated_tcn_step_slots_f32")):
        body = hip_py[hip_py.index(f"def {wrapper}("):]
        body = body[:body.index("\ndef ", 1)]
        assert "span: Optional[torch.Tensor] = None" in body and f"lib().{entry}(" in body, wrapper
    for doc in ("INTEGRATION.md",):
        for name in NEW:
            assert name in _read(doc), (doc, name)


# ---- the span rule in fp64 ------------------------------------------------------------------------------------------------
def _session_tensor(streams, shape, gen):
    """[B, *shape, HOPS] holding DEAD everywhere but stream b's own frames at births[b] .. births[b] + lengths[b]."""
    x = torch.full((len(BIRTHS), *shape, HOPS), DEAD, dtype=torch.float64)
    own = []
    for b, (birth, n) in enumerate(zip(BIRTHS, LENGTHS)):
        own.append(torch.rand(*shape, n, generator=gen, dtype=torch.float64) * 2 - 1)
        x[b, ..., birth:birth + n] = own[-1]
    return x, own


def test_up_path_under_the_span_rule_is_each_streams_offline_decoder():
    gen = torch.Generator().manual_seed(3)
    ch, f = 3, 6
    layers = UD.make_decoder(D, ch, seed=5)
    x, x_own = _session_tensor(3, (ch, f), gen)
    skips, skips_own = zip(*[_session_tensor(3, (ch, f), gen) for _ in range(D)])
    got = R.up_path_slots(x, list(skips), layers, SPAN, HOPS)          # hop s holds frame s - D
    for b, (birth, n) in enumerate(zip(BIRTHS, LENGTHS)):
        want = UD.offline(x_own[b][None], [s[b][None] for s in skips_own], layers)[0]
        mine = got[b, ..., birth + D:birth + D + n]
        assert float((mine - want).abs().max()) <= 1e-14 * max(1.0, float(want.abs().max())), b
        assert float(got[b].abs().max()) < 1e3, b                       # no dead frame reached any output of this stream


def test_gated_block_under_the_span_rule_is_each_streams_offline_block():
    gen = torch.Generator().manual_seed(4)
    h, e, p = 5, 3, 3
    for dilation in (1, 2, 4):
        blk = G.make_block(h, e, p, dilation, seed=dilation)
        emb = torch.rand(3, e, generator=gen, dtype=torch.float64) * 2 - 1
        y, y_own = _session_tensor(3, (h,), gen)                        # [B, H, HOPS]
        y = y.permute(2, 1, 0).contiguous()                             # [HOPS, H, B]
        for k in (1, 3, 16):
            ring = torch.full(((p - 1) * dilation + k, h, 3), DEAD, dtype=torch.float64)     # nothing clears the ring
            got = torch.cat([R.block_step_slots(y[t0:t0 + k], t0, blk, ring, SPAN, emb) for t0 in range(0, HOPS, k)])
            for b, (birth, n) in enumerate(zip(BIRTHS, LENGTHS)):
                want = G.offline(y_own[b][None], blk, emb[b:b + 1])[0]  # [H, n]
                assert float((got[birth:birth + n, :, b].t() - want).abs().max()) <= 1e-13, (dilation, k, b)
        # the streams moved to frame 0 are what an entry without a span takes (the GPU test's comparison)
        aligned = R.align(y, SPAN)
        alone = G.block_step(aligned, 0, blk, torch.zeros(HOPS + (p - 1) * dilation, h, 3, dtype=torch.float64), emb)
        for b, (birth, n) in enumerate(zip(BIRTHS, LENGTHS)):
            assert float((alone[:n, :, b] - got[birth:birth + n, :, b]).abs().max()) <= 1e-13


@pytest.mark.parametrize("out_mode", ["linear", "none"])
@pytest.mark.parametrize("n_fft,hop", [(16, 4), (12, 12), (8, 4)])
def test_window_sum_rule_is_each_streams_overlap_add(n_fft, hop, out_mode):
    gen = torch.Generator().manual_seed(n_fft + hop)
    window = torch.hann_window(n_fft, dtype=torch.float64)
    frames, own = _session_tensor(3, (n_fft,), gen)                     # [B, n_fft, HOPS]; a frame arrives D hops late
    frames = torch.roll(frames, D, dims=-1).permute(2, 0, 1).contiguous()
    out, tails = R.istft_slots(frames, window, SPAN, D, hop, out_mode)
    keep = n_fft - hop
    for b, (birth, n) in enumerate(zip(BIRTHS, LENGTHS)):
        want = R.ola_alone(own[b].t(), window, hop, out_mode)
        first = (birth + D) * hop
        assert float(out[b, :first].abs().max()) == 0.0                 # before the stream: constrain(0)
        # the steps, then the tail drained by later steps, equal the offline signal (n hops + n_fft - hop samples) ...
        assert float((out[b, first:first + want.shape[0]] - want).abs().max()) <= 1e-13, b
        assert float(out[b, first + want.shape[0]:].abs().max()) == 0.0
        # ... and so does a flush right after the last frame, or any number of hops later
        for late in range(0, keep // hop + 2 if keep else 0):
            t = birth + n + D + late
            rest = R.istft_flush_slots(tails[t, b], window, SPAN[b], t, D, hop, out_mode)
            full = torch.cat([want[(n + late) * hop:], torch.zeros(late * hop, dtype=torch.float64)])[:keep]
            assert float((rest - full).abs().max()) <= 1e-13, (b, late)


# ---- the bookkeeping ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delay", [0, 3, 6])
@pytest.mark.parametrize("win,hop", [(512, 128), (64, 16), (16, 16)])
@pytest.mark.parametrize("extra_hops", [0, 1, 7])
def test_slot_output_range_with_a_model_delay(win, hop, extra_hops, delay):
    from puresound_amd.streaming import StreamingUnetTcn as S
    samples = win + extra_hops * hop
    r = S.slot_output_range(samples, win, hop, delay_frames=delay)
    lat = win - hop + delay * hop
    assert (r.start, len(r)) == (lat, samples)
    # y = one output hop per input hop and per drain hop from open() on, then close(): exactly the range's end
    assert r.stop == samples + delay * hop + (win - hop)
    if delay == 0:
        assert r == S.slot_output_range(samples, win, hop) == range(win - hop, win - hop + samples)
    with pytest.raises(ValueError):
        S.slot_output_range(samples + 1, win, hop, delay_frames=delay)
    with pytest.raises(ValueError):
        S.slot_output_range(samples, win, hop, delay_frames=-1)


def test_streamer_has_the_slot_calls_and_says_so():
    from puresound_amd.streaming import StreamingUnetTcn as S
    for name in ("init_slots", "open", "end", "close", "_flush_slot", "_open_slot", "_enrolment_rule"):
        assert callable(getattr(S, name)), name
    for doc in ("README.md", "DESIGN.md"):
        assert "No join / leave slots yet" not in _read(doc) and "Join / leave slots are not built" not in _read(doc), doc
