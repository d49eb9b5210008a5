"""The float64 references of test_abi_kernels_gpu.py (tests/abi_refs.py) against independent formulations -- torch.nn modules
in double, F.conv2d / F.conv_transpose2d, the offline oracle path -- so the reference side of the GPU parity tests is proven
on a machine without a GPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import abi_refs as R
import short_row_cases as SR
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


# ---- the short-row GEMM kernels' references (test_short_row_kernels_gpu.py) -------------------------------------------------
@pytest.mark.parametrize("pname", list(SR.PROLOGUES))
def test_conv1x1_reference(pname):
    """conv1x1_ref against F.conv1d behind torch's own activations, in the prologue order ReLU -> affine -> PReLU -> tanh"""
    n, k, m, t = 3, 33, 17, 21
    d = SR.build_conv1x1((n, k, m, t, True, True, True, pname))
    pre_relu, affine, prelu, post_tanh = SR.PROLOGUES[pname]
    a = d["x"].double()
    if pre_relu:
        a = F.relu(a)
    if affine:
        a = a * d["gamma"].double().reshape(1, -1, 1) + d["beta"].double().reshape(1, -1, 1)
    if prelu:
        a = F.prelu(a, d["slope"].double())
    if post_tanh:
        a = torch.tanh(a)
    want = F.conv1d(a, d["w"].double().unsqueeze(2), d["bias"].double()) + d["bias_n"].double().unsqueeze(2) + d["res"].double()
    assert rel_max(d["ref"].numpy(), want.numpy()) < 1e-12
    if pname == "all":   # the order matters: the affine step behind the PReLU is another function
        swapped = F.prelu(F.relu(d["x"].double()), d["slope"].double()) * d["gamma"].double().reshape(1, -1, 1) \
            + d["beta"].double().reshape(1, -1, 1)
        other = F.conv1d(torch.tanh(swapped), d["w"].double().unsqueeze(2), d["bias"].double())
        assert rel_max((other + d["bias_n"].double().unsqueeze(2) + d["res"].double()).numpy(), want.numpy()) > 1e-3
    # the global-norm slot: the oracle's GlobLN
    g = SR.build_conv1x1((n, k, m, t, True, False, False, "prelu"), glob=True)
    a = F.prelu(O.glob_ln(g["x"].double(), g["gamma"].double(), g["beta"].double(), 1e-8), g["slope"].double())
    assert rel_max(g["ref"].numpy(), F.conv1d(a, g["w"].double().unsqueeze(2), g["bias"].double()).numpy()) < 1e-12


@pytest.mark.parametrize("has_res", [False, True])
def test_film_conv_reference(has_res):
    d = SR.build_film((3, 12, 19, has_res))
    x = d["x"].double()
    scale, shift = F.conv1d(x, d["ws"].double().unsqueeze(2)), F.conv1d(x, d["wb"].double().unsqueeze(2))
    if has_res:
        scale, shift = scale + d["rs"].double(), shift + d["rb"].double()
    assert rel_max(d["ref"].numpy(), (scale * x + shift).numpy()) < 1e-12


@pytest.mark.parametrize("k,hid", [(5, 3), (20, 8), (9, 1)])
def test_gates_cell_reference(k, hid):
    """gates_cell_ref against nn.LSTMCell, one step per frame column: xh = [x; h], W = [W_ih | W_hh], b = b_ih + b_hh"""
    torch.manual_seed(5)
    n, t = 3, 7
    d = SR.build_gates((n, k, hid, t, 0, True))
    cell = torch.nn.LSTMCell(k - hid, hid).double()
    w = torch.cat([cell.weight_ih, cell.weight_hh], 1).detach()
    bias = (cell.bias_ih + cell.bias_hh).detach()
    c_new, h_new = R.gates_cell_ref(d["xh"], w, bias, d["c"])
    for i in range(t):
        xh = d["xh"][:, :, i].double()
        h_want, c_want = cell(xh[:, :k - hid], (xh[:, k - hid:], d["c"][:, :, i].double()))
        assert rel_max(c_new[:, :, i].numpy(), c_want.detach().numpy()) < 1e-12
        assert rel_max(h_new[:, :, i].numpy(), h_want.detach().numpy()) < 1e-12


@pytest.mark.parametrize("has_bias,has_res,res_inside,has_norm2", [(True, True, False, True), (False, True, True, True),
                                                                   (True, False, False, False), (False, False, True, True)])
def test_proj_layernorm_reference(has_bias, has_res, res_inside, has_norm2):
    n, k, m, t = 3, 20, 37, 23
    d = SR.build_pln((n, k, m, t, has_bias, has_res, res_inside, has_norm2, False))
    p = F.conv1d(d["x"].double(), d["w"].double().unsqueeze(2), None if d["bias"] is None else d["bias"].double())
    if has_res and res_inside:
        p = p + d["res"].double()
    y = F.layer_norm(p.transpose(1, 2), (m,), d["gamma"].double(), d["beta"].double(), 1e-5).transpose(1, 2)
    if has_res and not res_inside:
        y = y + d["res"].double()
    assert rel_max(d["y_ref"].numpy(), y.numpy()) < 1e-12
    if has_norm2:
        g2, b2, e2 = d["norm2"]
        y2 = F.layer_norm(y.transpose(1, 2), (m,), g2.double(), b2.double(), e2).transpose(1, 2)
        assert rel_max(d["y2_ref"].numpy(), y2.numpy()) < 1e-12
    else:
        assert d["y2_ref"] is None


@pytest.mark.parametrize("c", [1, 2, 7])
def test_short_row_packing_helpers_permute_the_rows(c):
    """pair-interleaved FiLM weights / residual rows and unit-major gate rows: every source row once, at the documented place"""
    n, t = 2, 5
    ws, wb = R.rand((c, c + 1), 71), R.rand((c, c + 1), 72)
    pairs = R.film_pack_weights(ws, wb)
    assert pairs.shape == (2 * c, c + 1)
    assert torch.equal(pairs[0::2], ws) and torch.equal(pairs[1::2], wb)
    rs, rb = R.rand((n, c, t), 73), R.rand((n, c, t), 74)
    rows = R.film_pack_rows(rs, rb)
    assert rows.shape == (n, 2 * c, t)
    assert torch.equal(rows[:, 0::2], rs) and torch.equal(rows[:, 1::2], rb)
    order = R.gate_unit_major(c)
    assert sorted(order.tolist()) == list(range(4 * c))
    for u in range(c):
        for g in range(4):
            assert int(order[4 * u + g]) == g * c + u


def test_short_row_case_tables_cover_every_branch():
    """Every listed value appears, every named combination is there, no case twice."""
    for cases_ in (SR.CONV_CASES, SR.FILM_CASES, SR.GATES_CASES, SR.PLN_CASES, SR.AMAX_CASES):
        assert len(set(cases_)) == len(cases_) and 36 <= len(cases_) <= 60, len(cases_)
    col = lambda cases_, i: {c[i] for c in cases_}  # noqa: E731
    conv = SR.CONV_CASES
    assert col(conv, 0) == set(SR.CONV_N) and col(conv, 1) == set(SR.CONV_K) and col(conv, 2) == set(SR.CONV_M)
    assert col(conv, 3) == set(SR.CONV_T) and col(conv, 7) == set(SR.PROLOGUES)
    for i in (4, 5, 6):
        assert col(conv, i) == {False, True}
    # every instantiation <NCB, TR>, each also behind the second weight panel (M > 256)
    for m_min in (1, 257):
        assert {(SR.conv_ncb(c[3]), c[7] != "none") for c in conv if c[2] >= m_min} == {(ncb, tr) for ncb in (1, 2, 4)
                                                                                       for tr in (False, True)}
    assert any(c[1] == 272 and c[2] == 260 for c in conv)        # three K trips into the second panel
    assert {c[7] for c in conv if c[5]} >= {"none", "all"}        # bias_n on both instantiation families
    film = SR.FILM_CASES
    assert col(film, 0) == set(SR.FUSED_N) and col(film, 1) == set(SR.FILM_C) and col(film, 2) == set(SR.FUSED_T)
    assert col(film, 3) == {False, True}
    assert any(c[0] > 1 and c[1] == 130 and c[2] > 64 and c[3] for c in film)   # N > 1, M = 260, blockIdx.z > 0, residual
    gates = SR.GATES_CASES
    assert col(gates, 0) == set(SR.FUSED_N) and col(gates, 3) == set(SR.FUSED_T)
    assert col(gates, 1) == {5, 20, 132} and col(gates, 2) == {1, 3, 8, 64, 65}
    assert any(c[0] > 1 and c[2] == 65 and c[3] > 64 for c in gates) and any(c[4] for c in gates)
    assert col(gates, 5) == {False, True} and {SR.conv_ncb(c[3]) for c in gates if not c[5]} == {1, 2, 4}   # bias_units NULL
    pln = SR.PLN_CASES
    assert col(pln, 0) >= set(SR.PLN_N) and col(pln, 1) == set(SR.PLN_K) and col(pln, 2) == set(SR.PLN_M)
    assert col(pln, 3) >= set(SR.PLN_T)
    for i in (4, 5, 6, 7, 8):
        assert col(pln, i) == {False, True}
    assert {SR.pln_kernel(c[0], c[2], c[3]) for c in pln} == {"<8,8>", "<8>", "<16>"}
    for n, t, kern in ((4, 256, "<8,8>"), (5, 208, "<8>")):      # 64 | 65 workgroups, kept on this kernel by the second norm
        hits = [c for c in pln if (c[0], c[3]) == (n, t)]
        assert len(hits) == 2 and all(c[7] and c[2] <= 128 and SR.pln_kernel(c[0], c[2], c[3]) == kern for c in hits)
    assert 4 * ((256 + 15) // 16) == 64 and 5 * ((208 + 15) // 16) == 65
    assert any(not c[4] and not c[5] and c[7] for c in pln) and any(c[5] and c[6] and c[7] for c in pln)
    # rows off the 16-frame kernel's conditions would leave it: T >= 128 needs the second norm, the copy or M % 4 != 0
    assert all(c[3] < 128 or c[7] or c[8] or c[2] % 4 for c in pln)
    assert all(c[3] >= 128 and c[2] % 4 == 0 for c in SR.AMAX_CASES)


@pytest.mark.parametrize("case", SR.PLN_CASES + SR.AMAX_CASES, ids=str)
def test_short_row_layernorm_cases_are_well_conditioned(case):
    """the comparison with fp64 is meaningful only where no frame's variance over its channels is near zero"""
    d = SR.build_amax(case) if len(case) == 6 else SR.build_pln(case)
    if case[2] == 1:   # one channel: the deviation is exactly zero in any arithmetic, y = beta (+ res)
        assert d["min_var"] == 0.0
        return
    assert d["min_var"] > 1e-3, d["min_var"]
