"""The float64 references of test_abi_kernels_gpu.py (tests/abi_refs.py) against independent formulations -- torch.nn modules
in double, F.conv2d / F.conv_transpose2d, the offline oracle path -- so the reference side of the GPU parity tests is proven
on a machine without a GPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import abi_refs as R
from conftest import rel_max
from oracle import dualpath_oracle as DP
from oracle import separator_oracle as O


@pytest.mark.parametrize("kind,hid,bi", [("GRU", 1, False), ("GRU", 20, True), ("RNN", 33, True), ("GRU", 64, False),
                                         ("RNN", 5, False)])
def test_rnn_gate_fold_and_recurrence(kind, hid, bi):
    """gx + bhn built from a module's weights (b_ih + b_hh folded for r, z; b_in only for n; b_hn apart) and walked step by
    step give nn.GRU / nn.RNN, with an initial state, both directions."""
    torch.manual_seed(3)
    c, b, steps = 7, 5, 23
    mod = (torch.nn.GRU if kind == "GRU" else torch.nn.RNN)(c, hid, batch_first=True, bidirectional=bi).double()
    x = R.rand((b, steps, c), 11).double()
    h0 = R.rand((2 if bi else 1, b, hid), 12, -0.5, 0.5).double()
    ref, hn = mod(x, h0)
    w_ih, bias, whh_t, bhn = R.rnn_fold(mod)
    assert (bhn is None) == (kind == "RNN")
    out, last = R.rnn_from_gx(x @ w_ih.t() + bias, whh_t, bhn, h0)
    assert rel_max(out.detach().numpy(), ref.detach().numpy()) < 1e-12
    assert rel_max(last.detach().numpy(), hn.detach().numpy()) < 1e-12
    if kind == "GRU":   # the fold matters: b_hn inside the projection bias instead is a different function
        wrong, _ = R.rnn_from_gx(x @ w_ih.t() + bias + torch.cat([torch.zeros(2 * hid).double(), bhn[0]] * bhn.shape[0]),
                                 whh_t, torch.zeros_like(bhn), h0)
        assert rel_max(wrong.detach().numpy(), ref.detach().numpy()) > 1e-4


GEOMETRIES = [  # kf, kt, sf, df, dt, pf, pt, transposed
    (5, 2, 2, 1, 1, 2, 1, False), (1, 9, 1, 1, 1, 0, 7, False), (3, 3, 1, 2, 2, 2, 4, False), (5, 1, 4, 1, 1, 2, 0, False),
    (5, 2, 2, 1, 1, 2, 1, True), (3, 2, 1, 1, 1, 1, 0, True), (5, 3, 4, 1, 1, 2, 2, True), (3, 2, 2, 2, 3, 1, 3, True),
    (1, 2, 1, 1, 1, 0, 0, True)]


# (a geometry without an output row at some F is not a case: kf = 3, df = 2, pf = 2 on one input row has one, the rest too)
CONV_CASES = [(g, f, t) for g in GEOMETRIES for f, t in ((1, 1), (2, 5), (11, 19))
              if R.conv2d_out_rows(f, g[0], g[2], g[3], g[5], g[7]) >= 1]


@pytest.mark.parametrize("geom,f_in,t", CONV_CASES)
def test_conv2d_tap_reference(geom, f_in, t):
    """the tap-definition gather against nn.ZeroPad2d + F.conv2d and F.conv_transpose2d + the time trim"""
    kf, kt, sf, df, dt, pf, pt, transposed = geom
    n, c, m = 2, 3, 4
    f_out = R.conv2d_out_rows(f_in, kf, sf, df, pf, transposed)
    x, b = R.rand((n, c, f_in, t), 21).double(), R.rand((m,), 23).double()
    if not transposed:
        w = R.rand((m, c, kf, kt), 22).double()
        right = dt * (kt - 1) - pt
        ref = F.conv2d(F.pad(x, (pt, right, pf, pf)), w, b, stride=(sf, 1), dilation=(df, dt))
        w2 = w.reshape(m, -1)
    else:
        w = R.rand((c, m, kf, kt), 22).double()
        full = F.conv_transpose2d(x, w, b, stride=(sf, 1), padding=(pf, 0), output_padding=(sf - kf + 2 * pf, 0),
                                  dilation=(df, dt))
        ref = full[..., pt:pt + t]
        w2 = w.permute(1, 0, 2, 3).reshape(m, -1)
    assert ref.shape == (n, m, f_out, t)
    got = R.conv2d_taps(x, w2, b, t, f_out, kf, kt, sf, df, dt, pf, pt, transposed)
    assert rel_max(got.numpy(), ref.numpy()) < 1e-12
    if transposed:   # the untrimmed form a gLN decoder layer asks for: T = T_in + dt (kt - 1) frames, pt = 0
        ext = dt * (kt - 1)
        got = R.conv2d_taps(x, w2, b, t + ext, f_out, kf, kt, sf, df, dt, pf, 0, True)
        assert rel_max(got.numpy(), full.numpy()) < 1e-12


@pytest.mark.parametrize("kind", R.ACT_KINDS)
def test_gln_reference_and_pad_column_correction(kind):
    """gln_act against the oracle's GlobLN and torch's activations; the pad-column correction takes exactly the bias-only
    columns out of a GEMM's statistics over f_out * ld frames."""
    n, ch, f, t, ld = 2, 5, 3, 37, 128
    y = R.rand((n, ch, f, t), 31).double() + 100.0
    gamma, beta = R.rand((ch,), 32).double() + 1.5, R.rand((ch,), 33).double()
    want = O.glob_ln(y.reshape(n, ch, f * t), gamma.reshape(1, -1, 1), beta.reshape(1, -1, 1), 1e-8).reshape(n, ch, f, t)
    act = {"none": lambda v: v, "relu": torch.relu, "prelu": lambda v: F.prelu(v, torch.tensor([0.25]).double()),
           "mish": F.mish, "sigmoid": torch.sigmoid, "tanh": torch.tanh}[kind]
    assert rel_max(R.gln_act(y, gamma, beta, 1e-8, kind, 0.25).numpy(), act(want).numpy()) < 1e-9
    bias = R.rand((ch,), 34).double() * 3.0
    full = bias.reshape(1, -1, 1, 1).expand(n, ch, f, ld).clone()      # pad columns of the GEMM output: the bias alone
    full[..., :t] = y
    cs, cq = R.pad_column_correction(bias, f, ld, t)
    np.testing.assert_allclose(full.sum((1, 2, 3)).numpy() - cs, y.sum((1, 2, 3)).numpy(), rtol=1e-12)
    np.testing.assert_allclose((full ** 2).sum((1, 2, 3)).numpy() - cq, (y ** 2).sum((1, 2, 3)).numpy(), rtol=1e-12)


def test_mish_reference_is_finite_at_large_arguments():
    x = torch.tensor([-100.0, -30.0, 0.0, 30.0, 100.0]).double()
    got = R.activation(x, "mish")
    assert torch.isfinite(got).all()
    assert rel_max(got.numpy(), F.mish(x).numpy()) < 1e-12


@pytest.mark.parametrize("rel", [1.0, 0.5, 1.0 / 77, 1.5])
def test_masked_softmax_reference(rel):
    """row-by-row pooling against length_to_mask + masked_fill(-inf) + softmax on the whole tensor"""
    n, c, t = 3, 4, 77
    logits, x = R.rand((n, c, t), 41, -3, 3), R.rand((n, c, t), 42)
    lengths = torch.tensor([rel, 1.0, rel])
    mask = torch.arange(t).reshape(1, 1, -1) < (lengths * t).reshape(-1, 1, 1)
    a = torch.softmax(logits.double().masked_fill(~mask, float("-inf")), 2)
    mean = (a * x.double()).sum(2)
    std = torch.sqrt((a * (x.double() - mean.unsqueeze(2)) ** 2).sum(2).clamp(1e-12))
    w, out = R.attn_pool(logits, x, lengths, 1e-12)
    assert rel_max(w.numpy(), a.numpy()) < 1e-12
    assert rel_max(out.numpy(), torch.cat((mean, std), 1).numpy()) < 1e-12
    k = int(R.valid_frames(lengths, t)[0])
    assert k == min(t, math.ceil(rel * t - 1e-4)) and (w[0, :, k:] == 0).all()   # frames i < rel * t


@pytest.mark.parametrize("win,hop,hops", [(16, 8, 5), (8, 8, 3), (24, 8, 4), (2, 1, 7)])
def test_stream_window_and_overlap_references(win, hop, hops):
    """the chunked harness against the offline path: framing of the whole signal (oracle frame()) and the hop-by-hop averaging
    overlap-add of the demo harness (oracle overlap_add_mean)"""
    b = 3
    queue, chunk = R.rand((b, win), 51).numpy(), R.rand((b, hops * hop), 52).numpy()
    wins = R.stream_windows(queue, chunk, hop)
    sig = torch.tensor(np.concatenate([queue[:, hop:], chunk], 1))
    assert np.array_equal(wins, O.frame(sig, win, hop).permute(1, 0, 2).numpy())
    if win != 2 * hop:
        return
    frames, tail = R.rand((hops, b, win), 53).double().numpy(), R.rand((b, hop), 54).double().numpy()
    blocks, new_tail = R.stream_overlap(frames, tail, hop)
    run = torch.tensor(tail)                      # the running output of the hop-by-hop harness, the old tail first
    for f in frames:
        run = DP.overlap_add_mean(run, torch.tensor(f), hop)
    assert rel_max(blocks, run[:, :hops * hop].numpy()) < 1e-15
    assert np.array_equal(new_tail, frames[-1][:, hop:])
