"""Batches of utterances of unequal length through the egs/ns noise suppressors (conv-STFT encoder + DPCRN / DPARN), without a
GPU: what the host side accepts for the HIP path and what it refuses, each before any library call; the two C entries'
declarations; and the condition that keeps the GPU test (test_ragged_ns_gpu.py) honest -- on its batch, zero-padding a short
row changes the float64 oracle's answer by far more than any bound in use, at the utterance's end for every model and, for the
lookahead presets, already in the hops in front of the last window."""
import os
import re

import pytest
import torch

import cases
import edge_length_cases as E
import ragged_ns_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def PA():
    import puresound_amd.nnet as PA
    return PA


@pytest.fixture
def no_library(monkeypatch):
    """any call into the HIP library fails the test"""
    from puresound_amd import _abi, hip

    def lib():
        raise AssertionError("the HIP library was called")
    monkeypatch.setattr(_abi, "lib", lib)
    monkeypatch.setattr(hip, "lib", lib)


def _wrap(PA, masker, **kw):
    args = dict(mask_constraint="linear", f_type="Complex", mask_type="Complex", drop_first_bin=True)
    args.update(kw)
    return PA.SoTaskWrapModule(encoder=cases.build_encoder(PA.NS, dict(kind="stft", n_fft=512, hop=128)), masker=masker,
                               verbose=False, **args).eval()


# ---- the plan: accepted for the HIP path, without a device -----------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_the_host_side_accepts_the_four_models_for_the_hip_path(PA, no_library, name):
    from puresound_amd.nnet import ragged
    model = C.build(PA.NS, name).eval()
    noisy = torch.zeros(2, 4000)
    ragged.check_model(model, None, None, hip_path=True)
    rp = ragged.plan(model, noisy, None, [4000, 2000], None, hip_path=True)
    assert rp.t_rows == [28, 12] and rp.out_lengths == [3968, 1920] and rp.lengths == [4000, 2000]
    assert rp.enroll_lengths is None and rp.enroll_t_rows is None and rp.enroll_frames == 0
    assert model.output_lengths([4000, 2000]) == [3968, 1920]
    # any delay, either transpose_delay
    kw = dict(C.spec(name)["masker"]["kw"], delay=(1, 0, 1, 0, 0), kernel_t=(3, 2, 3, 2, 2))
    ragged.check_model(_wrap(PA, getattr(PA, C.spec(name)["masker"]["cls"])(**kw)), None, None, hip_path=True)
    # the length values are validated as for every other model
    with pytest.raises(RuntimeError, match="input length 511 is shorter than the window 512"):
        ragged.plan(model, noisy, None, [4000, 511], None, hip_path=True)
    with pytest.raises(ValueError, match="exceeds the row length 4000"):
        ragged.plan(model, noisy, None, [4001, 600], None, hip_path=True)


@pytest.mark.parametrize("name", C.NAMES)
def test_cpu_tensors_keep_their_refusal(PA, no_library, name):
    """the CPU path has no stock-ATen DPCRN / DPARN: refused before any work, and the default of plan() follows the tensor"""
    from puresound_amd.nnet import ragged
    model = C.build(PA.NS, name).eval()
    with pytest.raises(NotImplementedError, match="inference with lengths.*HIP path only"):
        model.inference(torch.zeros(2, 4000), lengths=[4000, 2000])
    with pytest.raises(NotImplementedError, match="HIP path only"):
        ragged.plan(model, torch.zeros(2, 4000), None, [4000, 2000], None)
    with pytest.raises(NotImplementedError, match="HIP path only"):
        model.inference_scored_ragged(torch.zeros(2, 4000), torch.zeros(2, 4000), lengths=[4000, 2000])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_what_the_hip_path_does_not_cover_is_refused_before_any_library_call(PA, no_library):
    from puresound_amd.nnet import ragged
    noisy, lens = torch.zeros(2, 4000), [4000, 2000]
    dpcrn = dict(C.spec("ns_dpcrn_short")["masker"]["kw"])
    dparn = dict(C.spec("ns_dparn_short")["masker"]["kw"])

    def refused(model, text, enroll=None):
        with pytest.raises(NotImplementedError, match=text):
            ragged.plan(model, noisy, enroll, lens, None, hip_path=True)
        with pytest.raises(NotImplementedError, match="inference with lengths"):
            ragged.check_model(model, enroll, None, hip_path=True)

    refused(_wrap(PA, PA.Unet()), "DPCRN or DPARN masker only \\(got Unet")
    refused(cases.build(PA.NS, "tse_unet_tcn_causal_short").eval(), "got UnetTcn")
    refused(_wrap(PA, PA.DPARN_Mout(**{k: v for k, v in dparn.items() if k != "nhead"})), "got DPARN_Mout")
    refused(_wrap(PA, PA.DPCRN(**dict(dpcrn, norm_type="gLN"))), 'norm_type="gLN".*statistics of a gLN span the frames')
    refused(_wrap(PA, PA.DPARN(**dict(dparn, norm_type="gLN"))), 'norm_type="gLN"')
    refused(_wrap(PA, PA.DPCRN(**dict(dpcrn, skip_conv=True))), "skip_conv=True is not covered")
    refused(_wrap(PA, PA.DPCRN(**dict(dpcrn, channels=(1, 32, 32, 32, 64, 512)))), "Cin\\*kf\\*kt = 6144 is off the implicit-GEMM")
    refused(_wrap(PA, PA.DPCRN(**dpcrn), f_type="real", mask_type="real"), "\\(complex, complex\\) masks only")
    refused(cases.build(PA.NS, "cfg1_short").eval(), "STFT encoder in front of a ConvTasNet")
    refused(C.build(PA.NS, "ns_dpcrn_short").eval(), "an enrolment is not covered", enroll=torch.zeros(2, 3000))
    refused(_wrap(PA, PA.DPCRN(**dict(dpcrn, spectral_compress=True))), "spectral_compress")
    # SiMoTaskWrapModule refuses lengths whatever it wraps
    simo = PA.SiMoTaskWrapModule(encoder=cases.build_encoder(PA.NS, dict(kind="stft", n_fft=512, hop=128)),
                                 masker=PA.DPARN_Mout(**{k: v for k, v in dparn.items() if k != "nhead"}), verbose=False,
                                 f_type="Complex", mask_type="Complex", drop_first_bin=True).eval()
    with pytest.raises(NotImplementedError, match="SiMoTaskWrapModule"):
        simo.inference(noisy, lengths=lens)


def test_the_unet_refuses_a_per_row_limit_it_cannot_honour(PA, no_library):
    """Unet._down / _up themselves, for a caller that skipped check_model: never a silent run over whole rows"""
    dpcrn = dict(C.spec("ns_dpcrn_short")["masker"]["kw"])
    assert PA.DPCRN(**dpcrn).per_row_refusal() is None
    assert PA.DPCRN(**dict(dpcrn, transpose_delay=True, delay=(1, 0, 0, 0, 0), kernel_t=(3, 2, 2, 2, 2))).per_row_refusal() is None
    assert "skip_conv" in PA.DPCRN(**dict(dpcrn, skip_conv=True)).per_row_refusal()
    assert "gLN" in PA.DPCRN(**dict(dpcrn, norm_type="gLN")).per_row_refusal()


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_two_entries_are_declared_and_the_abi_number_stays():
    from puresound_amd import _abi
    header = open(f"{ROOT}/include/puresound_hip.h").read()
    assert _abi.ABI_VERSION == 24 and re.search(r"^#define PS_ABI_VERSION 24$", header, flags=re.M)
    for name, sibling, more in (("ps_conv2d_ragged_f32", "ps_conv2d_f32", 0), ("ps_istft_ola_ragged_f32", "ps_istft_ola_f32", 1)):
        assert name in _abi.SIGNATURES
        decl = re.search(rf"^int {name}\(([^;]*)\);", header, flags=re.M | re.S)
        assert decl, name
        args = [a.strip() for a in decl.group(1).split(",")]
        assert len(args) == len(_abi.SIGNATURES[name][1]) == len(_abi.SIGNATURES[sibling][1]) + more
        assert "const int* t_rows" in args and args[-1] == "void* stream"
    # t_rows stands where T_in stood
    conv = re.search(r"^int ps_conv2d_f32\(([^;]*)\);", header, flags=re.M | re.S).group(1)
    ragged = re.search(r"^int ps_conv2d_ragged_f32\(([^;]*)\);", header, flags=re.M | re.S).group(1)
    assert re.sub(r"\s+", " ", conv).replace("int T_in,", "const int* t_rows,") == re.sub(r"\s+", " ", ragged)
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = open(f"{ROOT}/{doc}").read()
        assert "ps_conv2d_ragged_f32" in text and "ps_istft_ola_ragged_f32" in text, doc


# ---- the float64 oracle: zero-padding is wrong on the GPU tests' batch -------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_zero_padding_a_short_row_is_wrong_on_the_gpu_tests_batch(name):
    """The oracle on the zero-padded batch against the oracle on each utterance alone.  Every shorter row: weighted_rel_max >=
    0.05 (frames that straddle the utterance's end enter the overlap-add and its window sum).  transpose_delay=True, T_n >= 2:
    already >= 0.04 in the 5 hops in front of the last window (each of the six up layers reads one frame ahead).  Everything in
    front of that zone -- for the causal models the zone too -- agrees to 1e-12: the models are causal in time."""
    padded = C.oracle(name, C.batch("zero"))
    outs = C.out_lengths()
    assert padded.shape == (len(C.FRAMES), max(outs))
    for n, t in enumerate(C.FRAMES):
        _, ref = C.alone(name, n)
        assert ref.shape == (1, outs[n])
        share = E.clamped_share(C.BASE[name], ref.numpy())
        whole = E.weighted_rel_max(padded[n:n + 1, :outs[n]].numpy(), ref.numpy(), t)
        before, zone, behind = C.weighted_parts(padded[n, :outs[n]].numpy(), ref[0].numpy(), t)
        print(f"{name} row {n} (T = {t}): padded against alone, weighted {whole:.3e}; before the zone {before:.2e}, in it "
              f"{zone:.3e}, behind it {behind:.3e}; clamped share {share:.1e}")
        assert share <= E.CLAMP_CAP
        assert before <= 1e-12
        if t == max(C.FRAMES):
            assert whole <= 1e-12
            continue
        assert whole >= 0.05
        if name in C.LOOKAHEAD:
            if t >= 2:
                assert zone >= 0.04
        else:
            assert zone <= 1e-12
