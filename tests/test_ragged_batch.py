"""Batches of utterances of unequal length, without a GPU: SoTaskWrapModule.inference(noisy, enroll, lengths, enroll_lengths)
on CPU tensors (nnet/cpu_path.py loops over the rows: the definition of the semantics), output_lengths, every refusal before a
library call, and the condition that keeps the GPU test (test_ragged_batch_gpu.py) honest: on its batch, zero-padding a short
row changes the float64 oracle's answer by far more than any bound in use, so a path that merely padded would fail there."""
import pytest
import torch
import torch.nn as nn

import cases
import edge_length_cases as E
import ragged_ref as R
from oracle import separator_oracle as O

NAME = "cfg2_short"


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


def _cpu_model(PA, name):
    model = cases.build(PA.NS, name).eval()
    model.load_state_dict(E.weights(name)[0])
    return model


def _small(PA, **masker_kw):
    """FreeEncDec(win 16, hop 8, 24) + a two-block ConvTasNet -> a wrapper the refusal tests vary"""
    kw = dict(tcn_kernel=3, tcn_dim=12, repeat_tcn=1, tcn_dilated_basic=2, per_tcn_stack=2, tcn_with_embed=[0, 0])
    kw.update(masker_kw)
    wrap = {k: kw.pop(k) for k in ("speaker_net", "embedding_free_tse") if k in kw}
    enc = PA.FreeEncDec(win_length=16, hop_length=8, laten_length=24)
    return PA.SoTaskWrapModule(encoder=enc, masker=PA.ConvTasNet(24, kw.pop("embed_dim", 0), False, **kw), verbose=False,
                               **wrap).eval()


def test_cpu_inference_with_lengths_is_the_rows_one_by_one(PA):
    model = _cpu_model(PA, NAME)
    noisy, lens, _, _, _ = R.batch(NAME, R.CFG2_T)
    out = model.inference(noisy, lengths=lens)      # (TypeError before this feature)
    win, hop = E.win_hop(NAME)
    assert out.dtype == torch.float32 and out.shape == (len(lens), (max(R.CFG2_T) - 1) * hop + win)
    valid = model.output_lengths(lens)
    assert valid == [E.out_length(NAME, t) for t in R.CFG2_T]
    for n, length in enumerate(lens):
        alone = model.inference(noisy[n:n + 1, :length])
        assert alone.shape == (1, valid[n])
        assert torch.equal(out[n, :valid[n]], alone[0]), n
        assert float(out[n, valid[n]:].abs().max() if valid[n] < out.shape[1] else 0.0) == 0.0, n
    # the same lengths as a CPU integer tensor; and the junk does not matter
    assert torch.equal(model.inference(noisy, lengths=torch.tensor(lens)), out)
    nan_batch = R.batch(NAME, R.CFG2_T, junk="nan")[0]
    assert torch.equal(model.inference(nan_batch, lengths=lens), out)


def test_sigmoid_output_is_zero_behind_the_utterance(PA):
    model = cases.build(PA.NS, "tiny_free").eval()      # mask and output constraint "sigmoid": sigmoid(0) = 0.5 otherwise
    noisy = E.det_wave(5, 3, 400) * 0.1
    out = model.inference(noisy, lengths=[400, 16, 215])
    assert model.output_lengths([400, 16, 215]) == [400, 16, 208]
    assert float(out[1, 16:].abs().max()) == 0.0 and float(out[2, 208:].abs().max()) == 0.0
    assert float(out[1, :16].min()) > 0.0 and torch.equal(out[2:3, :208], model.inference(noisy[2:3, :215]))


def test_output_lengths(PA):
    model = _small(PA)
    assert model.output_lengths([16, 23, 24, 100]) == [16, 16, 24, 96]
    assert model.output_lengths(torch.tensor([16, 31])) == [16, 24]
    with pytest.raises(RuntimeError, match="shorter than the window"):
        model.output_lengths([15])


def test_zero_padding_a_short_row_is_wrong_on_the_gpu_tests_batch():
    """The float64 oracle on the zero-padded batch against the oracle on each utterance alone: rel_max >= 1e-2 on every
    short row (the global norms' statistics and the depthwise taps see the padding)."""
    noisy, lens, _, _, refs = R.batch(NAME, R.CFG2_T)
    padded = torch.zeros_like(noisy, dtype=torch.float64)
    for n, length in enumerate(lens):
        padded[n, :length] = noisy[n, :length].double()
    with torch.no_grad():
        out = O.inference(padded, E.weights(NAME)[1], cases.oracle_cfg(NAME))
    short = [n for n, t in enumerate(R.CFG2_T) if t < max(R.CFG2_T)]
    assert len(short) == len(R.CFG2_T) - 1
    for n in short:
        valid = refs[n].shape[-1]
        err = E.errors(NAME, out[n:n + 1, :valid].numpy(), refs[n].numpy())["rel_max"]
        print(f"row {n} (T = {R.CFG2_T[n]}): zero-padded against alone, rel_max {err:.3e}")
        assert err >= 1e-2, (n, err)
    full = R.CFG2_T.index(max(R.CFG2_T))
    assert E.errors(NAME, out[full:full + 1].numpy(), refs[full].numpy())["rel_max"] < 1e-9


# ---- refusals: each before any library call --------------------------------------------------------------------------------------
def test_length_values_are_refused(PA, no_library):
    model = _small(PA)
    noisy = torch.zeros(3, 200)
    for bad, exc, text in (([200, 100], ValueError, "2 values for a batch of 3"),
                           ([200, 201, 100], ValueError, "exceeds the row length 200"),
                           (torch.tensor([200, 100, 201]), ValueError, "exceeds the row length"),
                           ([200, 100.0, 50], ValueError, "Python ints"),
                           (torch.tensor([200.0, 100.0, 50.0]), ValueError, "integer tensor"),
                           ([200, 15, 100], RuntimeError, "input length 15 is shorter than the window 16")):
        with pytest.raises(exc, match=text):
            model.inference(noisy, lengths=bad)
    with pytest.raises(ValueError, match="enroll_lengths was given without enroll"):
        model.inference(noisy, lengths=[200, 100, 50], enroll_lengths=[100, 100, 100])
    with pytest.raises(ValueError, match="enroll_lengths was given without enroll"):
        model.inference(noisy, enroll_lengths=[100, 100, 100])


@pytest.mark.parametrize("name", ["cfg1_short", "cfg4_short", "cfg4_tse_short", "tse_skim_causal_short",
                                  "tse_unet_tcn_causal_short", "ns_dpcrn_short"])
def test_presets_outside_the_conv_tasnet_family_are_refused(PA, no_library, name):
    """an STFT encoder; DPRNN (also embedding-free TSE), SkiM and Unet-family maskers"""
    model = cases.build(PA.NS, name).eval()
    with pytest.raises(NotImplementedError, match="inference with lengths"):
        model.inference(torch.zeros(2, 4000), lengths=[4000, 2000])


def test_uncovered_conv_tasnet_variants_are_refused(PA, no_library):
    noisy, lens = torch.zeros(2, 200), [200, 100]
    with pytest.raises(NotImplementedError, match='tcn_layer="gated"'):
        _small(PA, tcn_layer="gated").inference(noisy, lengths=lens)
    with pytest.raises(NotImplementedError, match="cLN"):
        _small(PA, tcn_norm="cLN").inference(noisy, lengths=lens)
    with pytest.raises(NotImplementedError, match="cLN"):
        _small(PA, dconv_norm="cLN").inference(noisy, lengths=lens)
    with pytest.raises(NotImplementedError, match="embedding_free_tse"):
        _small(PA, embedding_free_tse=True).inference(noisy, lengths=lens)
    with pytest.raises(NotImplementedError, match="inference_scored"):
        _small(PA).inference_scored(noisy, torch.zeros(2, 200), lengths=lens)
    simo = cases.build(PA.NS, "simo_free").eval()
    with pytest.raises(NotImplementedError, match="SiMoTaskWrapModule"):
        simo.inference(noisy, lengths=lens)


def test_enrolment_lengths_need_the_plain_speaker_net(PA, no_library):
    noisy, enroll, lens = torch.zeros(2, 200), torch.zeros(2, 160), [200, 100]
    rnn_net = cases.build_speaker_net(PA.NS, dict(block="rnn", C=24, H=8, att=8, E=6, bidirectional=True))
    model = _small(PA, speaker_net=rnn_net, embed_dim=6, tcn_with_embed=[1, 0])
    with pytest.raises(NotImplementedError, match="plain TCN"):
        model.inference(noisy, enroll, lengths=lens, enroll_lengths=[160, 80])
    gated = nn.ModuleList([PA.GatedTCN(24, 12, 3, 1), PA.AttentiveStatisticsPooling(24, 8), nn.Conv1d(48, 6, 1, bias=False)])
    with pytest.raises(NotImplementedError, match="plain TCN"):
        _small(PA, speaker_net=gated, embed_dim=6, tcn_with_embed=[1, 0]).inference(noisy, enroll, lengths=lens,
                                                                                   enroll_lengths=[160, 80])
    with pytest.raises(NotImplementedError, match="needs a speaker_net"):
        _small(PA).inference(noisy, enroll, lengths=lens, enroll_lengths=[160, 80])
    # the covered shape passes the checks: its enrolment's lengths are validated next
    plain = nn.ModuleList([PA.TCN(24, 12, 3, 1), PA.TCN(24, 12, 3, 2), PA.AttentiveStatisticsPooling(24, 8),
                           nn.Conv1d(48, 6, 1, bias=False)])
    with pytest.raises(ValueError, match=r"enroll_lengths\[1\] = 161 exceeds the row length 160"):
        _small(PA, speaker_net=plain, embed_dim=6, tcn_with_embed=[1, 0]).inference(noisy, enroll, lengths=lens,
                                                                                   enroll_lengths=[160, 161])


# ---- the C entries refuse on the host, before any launch (the library loads without a GPU) ----------------------------------------
def test_ragged_entries_refuse_bad_arguments_on_the_host():
    import ctypes as C
    from puresound_amd import _abi
    lib = _abi.lib()
    buf = C.create_string_buffer(1 << 16)
    base = (C.addressof(buf) + 255) // 256 * 256     # aligned host memory that nothing dereferences: every call is refused
    x, y, lim, ws = base, base + 4096, base + 8192, base + 16384

    def refused(rc, text):
        assert rc != 0 and text in lib.ps_last_error().decode(), (rc, lib.ps_last_error())
    refused(lib.ps_ragged_stats_f32(None, lim, y, 2, 16, 100, 128, 4, 1600.0, None), "null pointer")
    refused(lib.ps_ragged_stats_f32(x, lim, y, 2, 16, 100, 100, 4, 1600.0, None), "ldt=100 must be a multiple of 128")
    refused(lib.ps_ragged_stats_f32(x, lim, y, 2, 16, 100, 128, 0, 1600.0, None), "parts > 0")
    refused(lib.ps_ragged_stats_f32(x, lim, y, 2, 16, 100, 128, 4, 0.0, None), "count_full > 0")
    refused(lib.ps_zero_tail_f32(x, None, 2, 16, 128, None), "null pointer")
    refused(lib.ps_zero_tail_f32(x, lim, 70000, 16, 128, None), "N=70000")
    def with_args(entry, **defaults):
        """-> call(**changed): `entry` with its arguments in the order given here, some of them replaced"""
        return lambda **changed: entry(*{**defaults, **changed}.values())

    dw = with_args(lib.ps_dwconv_ragged_f32, x=x, w=lim, b=None, y=y, t_rows=lim, N=2, H=16, T=100, ldt=128, P=3, dilation=1,
                   left=1, pro=None, ostats=None, count_full=1600.0, stream=None)
    refused(dw(t_rows=None), "null pointer")
    refused(dw(P=9), "bad argument")
    refused(dw(left=3), "left=3 exceeds the receptive field")
    refused(dw(dilation=600, left=600), "halo")
    refused(dw(y=x), "must not alias")
    refused(dw(ldt=96), "ldt=96 must be a multiple of 128")
    refused(dw(ostats=y, count_full=0.0), "count_full > 0")
    blocks = (_abi.TcnBlock * 1)()
    b = blocks[0]
    b.C, b.H, b.P, b.dilation = 8, 4, 3, 1
    b.in_norm = b.dw_norm = b.pw_norm = _abi.PS_NORM_GLOBAL
    need = lib.ps_conv_tasnet_workspace_bytes(2, 8, 4, 100)
    call = with_args(lib.ps_conv_tasnet_ragged_f32, blocks=blocks, n_blocks=1, x_in=x, x_out=y, dvec=None, embed_norm=0, N=2,
                     T=100, ldt=128, t_rows=lim, workspace=ws, workspace_bytes=need, stream=None)
    assert need <= (1 << 16) - 16384 - 256
    refused(call(), "lacks the fp32 weights")            # (every other rule is met: this is the last check)
    refused(call(x_out=x), "x_in must not alias x_out")
    refused(call(ldt=256), "ldt=256 must be ps_padded_frames")
    refused(call(workspace_bytes=need - 1), "workspace too small")
    refused(call(t_rows=None), "t_rows is NULL")
    b.causal = 1
    refused(call(), "global norms conflict with causal=1")


# ---- the float64 references of the GPU tests, against torch's own operators on each row cut out ------------------------------------
def test_kernel_references_agree_with_torch_on_each_row_alone():
    from abi_refs import rand
    t_rows, h, t, p = (40, 1, 2, 17), 6, 40, 3
    x = rand((len(t_rows), h, t), 1) + 0.5
    for n, tn in enumerate(t_rows):
        x[n, :, tn:] = float("nan")
    w, b = rand((h, 1, p), 2), rand((h,), 3)
    gamma, beta, slope = rand((h,), 4) + 1.5, rand((h,), 5), torch.tensor([0.25])
    for kind in (R.GLOBAL, R.AFFINE, R.NONE):
        for dilation, left in ((1, 1), (4, 8), (4, 0)):
            y = R.dwconv_ragged_ref(x, t_rows, w, b, dilation, left, kind, gamma, beta, slope)
            for n, tn in enumerate(t_rows):
                row = x[n:n + 1, :, :tn].double()
                if kind == R.GLOBAL:
                    row = (row - row.mean()) / torch.sqrt(row.var(unbiased=False) + R.EPS)
                if kind != R.NONE:
                    row = row * gamma.double()[None, :, None] + beta.double()[None, :, None]
                row = torch.nn.functional.prelu(row, slope.double())
                row = torch.nn.functional.pad(row, (left, (p - 1) * dilation - left))
                alone = torch.nn.functional.conv1d(row, w.double(), b.double(), dilation=dilation, groups=h)
                assert torch.allclose(y[n:n + 1, :, :tn], alone, rtol=1e-12, atol=1e-12), (kind, dilation, left, n)
                assert float(y[n, :, tn:].abs().max() if tn < t else 0.0) == 0.0
    # partials scaled by count_full / (R * T_n), read back as the consumer reads them under count_full
    clean = torch.where(R.valid_mask(t_rows, t), x.double(), 0.0)
    scale = (h * t) / (h * torch.tensor(t_rows, dtype=torch.float64))
    stats = torch.stack([clean.sum((1, 2)) * scale, (clean ** 2).sum((1, 2)) * scale], -1)[:, None, :]
    mean, rstd = R.consumer_scalars(stats, float(h * t))
    mean_ref, rstd_ref = R.stats_ref(clean, t_rows)
    assert torch.allclose(mean, mean_ref, rtol=1e-12) and torch.allclose(rstd, rstd_ref, rtol=1e-9)
    assert torch.equal(R.zero_tail_ref(torch.ones(2, 1, 5), (0, 3))[:, 0], torch.tensor([[0.] * 5, [1., 1., 1., 0., 0.]]))
