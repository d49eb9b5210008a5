"""Direct parity tests of the launching C-ABI entries that the model-level goldens reach only at one small shape: each test
calls the wrapper in puresound_amd/hip.py (so the call goes through the C ABI) at the entry's edge shapes and compares with a
plain float64 reference (tests/abi_refs.py, proven without a GPU by test_abi_references.py).

House rules: seeded Philox inputs, NaN in the caching allocator, NaN written into the pad columns of every padded input whose
pads the entry promises not to read, exact zeros asserted in the pad columns an entry promises to clear, one
pytest.raises(RuntimeError) per documented refusal that can be reached without touching memory.

Tolerances by class (the project's own): torch.equal for data movement, rel_max < 1e-6 for one-product elementwise results,
< 2e-5 where a sum of products, a normalisation or a transcendental is involved."""
import numpy as np
import pytest
import torch

import abi_refs as R
from abi_refs import rand as _rand
from conftest import rel_max
from puresound_amd import _abi

pytestmark = pytest.mark.gpu
EXACT1, FP32 = 1e-6, 2e-5
NAN = float("nan")
# torch's own fp32 CPU nn.GRU / nn.RNN against float64 on the 200-step inputs below (H in {1 .. 256}, both directions):
# rel_max 3.0e-7 (GRU), 4.6e-7 (RNN).  The HIP kernel gets 4 x that (summation order, tanhf / expf), floor 2e-5: the floor.
RNN_TOL = max(4 * 4.6e-7, 2e-5)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def H():
    from puresound_amd import hip
    hip.lib()
    return hip


@pytest.fixture(autouse=True)
def _nan_in_the_allocator_cache(dev):
    """NaN-filled blocks in torch's caching allocator: `torch.empty` scratch and outputs start as NaN, not as zeros."""
    junk = [torch.full((1 << 22,), NAN, device=dev) for _ in range(16)]
    junk += [torch.full((n,), NAN, device=dev) for n in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20)]
    del junk
    yield


def _pad(H, dev, x, t=None, fill=NAN):
    """compact [..., T] -> padded rows on the device with `fill` in the pad columns"""
    t = x.shape[-1] if t is None else t
    p = H.pad_rows(x.float().to(dev))
    p[..., t:] = fill
    return p


def _pad4(H, dev, x, min_frames=0):
    n, c, f, t = x.shape
    p = H.pad_rows(x.float().reshape(n, c * f, t).to(dev), min_frames)
    p[..., t:] = NAN
    return p.view(n, c, f, -1)


def _err(got, ref):
    return rel_max(got.detach().cpu().double().numpy(), ref.detach().double().numpy())


# ------------------------------------------------------------------------------------------------
# ps_rnn_f32: GRU and Elman cells
# ------------------------------------------------------------------------------------------------
RNN_CASES = [  # H, D, Q, N, layout, steps
    (1, 1, 1, 1, "intra", 1), (20, 2, 5, 3, "inter", 37), (64, 1, 4, 1, "row", 37), (100, 2, 7, 3, "intra", 200),
    (256, 1, 5, 1, "inter", 200), (256, 2, 4, 3, "row", 1), (20, 1, 7, 1, "intra", 37), (64, 2, 1, 3, "inter", 200),
    (1, 2, 7, 1, "row", 200), (100, 1, 4, 3, "inter", 1)]


@pytest.mark.parametrize("kind", ["GRU", "RNN"])
@pytest.mark.parametrize("hid,d,q,n,layout,steps", RNN_CASES)
def test_rnn(H, dev, kind, hid, d, q, n, layout, steps):
    """Full and ragged last workgroups (4 sequences each), both directions, the three frame layouts of the LSTM tests, initial
    and final states; reference nn.GRU / nn.RNN in float64, gx and bhn folded from the module's weights by the test."""
    c = 6
    torch.manual_seed(100 + hid)
    mod = (torch.nn.GRU if kind == "GRU" else torch.nn.RNN)(c, hid, batch_first=True, bidirectional=d == 2).double()
    w_ih, bias, whh_t, bhn = R.rnn_fold(mod)
    seqs = _rand((n, q, steps, c), 71).double()
    h0 = _rand((d, n * q, hid), 72, -0.5, 0.5).double()
    with torch.no_grad():
        ref, hn = mod(seqs.reshape(n * q, steps, c), h0)
        ref0, _ = mod(seqs.reshape(n * q, steps, c))
    ld = _abi.padded_frames(steps)
    q_stride, step_stride = {"intra": (steps, 1), "inter": (1, q), "row": (ld, 1)}[layout]
    idx = (torch.arange(q).reshape(-1, 1) * q_stride + torch.arange(steps).reshape(1, -1) * step_stride).reshape(-1)
    ldt = _abi.padded_frames(int(idx.max()) + 1)
    g = w_ih.shape[0]
    gx = torch.full((n, g, ldt), NAN)                      # frames no sequence owns hold NaN: they are never read
    gx[:, :, idx] = (seqs @ w_ih.t() + bias).permute(0, 3, 1, 2).reshape(n, g, q * steps).float()
    state = _pad(H, dev, h0.reshape(d, n, q, hid).permute(1, 0, 3, 2).reshape(n, d * hid, q))
    args = (gx.to(dev), whh_t.float().to(dev), kind, hid, d, q, q_stride, steps, step_stride,
            None if bhn is None else bhn.float().to(dev))
    hout, hl = H.rnn(*args, h0=state, want_state=True)
    hout0 = H.rnn(*args)
    torch.cuda.synchronize()
    back = lambda v: v[:, :, idx].cpu().reshape(n, d * hid, q, steps).permute(0, 2, 3, 1).reshape(n * q, steps, d * hid)  # noqa: E731
    e = (_err(back(hout), ref), _err(back(hout0), ref0),
         _err(hl[..., :q].reshape(n, d, hid, q).permute(1, 0, 3, 2).reshape(d, n * q, hid), hn))
    print("rnn", kind, hid, d, q, n, layout, steps, e)
    assert max(e) < RNN_TOL, e
    assert hl.shape[-1] == state.shape[-1]


def test_rnn_refusals(H, dev):
    gx, w = torch.zeros(1, 3 * 8, 128, device=dev), torch.zeros(1, 8, 24, device=dev)
    with pytest.raises(RuntimeError):                       # the GRU needs bhn
        H.rnn(gx, w, "GRU", 8, 1, 1, 1, 4, 1, None)
    with pytest.raises(RuntimeError):                       # H = 257: unsupported hidden size
        H.rnn(torch.zeros(1, 257, 128, device=dev), torch.zeros(1, 257, 257, device=dev), "RNN", 257, 1, 1, 1, 4, 1)
    with pytest.raises(RuntimeError):                       # a frame outside the row
        H.rnn(gx, w, "GRU", 8, 1, 2, 100, 40, 1, torch.zeros(1, 8, device=dev))
    with pytest.raises(RuntimeError):                       # mismatched shapes
        H.rnn(gx, torch.zeros(1, 8, 8, device=dev), "GRU", 8, 1, 1, 1, 4, 1, torch.zeros(1, 8, device=dev))
    with pytest.raises(RuntimeError):                       # a state row shorter than Q
        H.rnn(torch.zeros(1, 8, 256, device=dev), torch.zeros(1, 8, 8, device=dev), "RNN", 8, 1, 200, 1, 1, 1,
              h0=torch.zeros(1, 8, 128, device=dev))


# ------------------------------------------------------------------------------------------------
# ps_conv2d_f32 / ps_conv2d_stats_f32 / ps_conv2d_f16x2_f32
# ------------------------------------------------------------------------------------------------
# (kf, kt, stride_f, dil_f, dil_t, pad_f, pad_t, transposed) the presets of tests/golden/cases.py can emit.  Down layers
# (nnet/unet.py:224-233: pad_f = kf // 2, pad_t = kt - delay - 1), with nnet/dpcrn.py and nnet/dparn.py building their stacks
# through the same Unet._down / _up:
PRESET_DOWN = [
    (5, 2, 2, 1, 1, 2, 1, False), (3, 2, 2, 1, 1, 1, 1, False), (3, 2, 1, 1, 1, 1, 1, False),   # cases.py:73-77, 337-350
    (5, 3, 2, 1, 1, 2, 1, False),                                                               # cases.py:311-313 (delay 1)
    (5, 1, 4, 1, 1, 2, 0, False),                                                               # cases.py:316, 498-500
    (1, 5, 1, 1, 1, 0, 4, False), (1, 9, 1, 1, 1, 0, 7, False), (1, 1, 1, 1, 1, 0, 0, False)]   # cases.py:498-500 (delay 1 at 9)
# Up layers (nnet/unet.py:255-280: kt = transpose_t_size, pad_t = its trim shift with transpose_delay, else 0; a gLN layer runs
# untrimmed: T = T_in + dil_t (kt - 1) with pad_t = 0, written below as pad_t = -1):
PRESET_UP = [
    (5, 2, 2, 1, 1, 2, 0, True), (5, 2, 2, 1, 1, 2, 1, True), (3, 2, 2, 1, 1, 1, 0, True), (3, 2, 1, 1, 1, 1, 1, True),
    (5, 3, 4, 1, 1, 2, 0, True), (3, 3, 1, 1, 1, 1, 0, True), (1, 2, 1, 1, 1, 0, 0, True), (5, 2, 4, 1, 1, 2, 0, True),
    (5, 2, 2, 1, 1, 2, -1, True), (3, 2, 1, 1, 1, 1, -1, True)]
OFF_PRESET = [(3, 3, 1, 2, 2, 2, 4, False), (3, 2, 2, 2, 3, 1, 3, True)]      # dilated in both axes
F_EDGES, T_EDGES = (1, 2, 11, 257), (1, 127, 128, 129, 1025)


def _conv_cases():
    out = []
    for g in (PRESET_DOWN[0], PRESET_UP[1], OFF_PRESET[0], OFF_PRESET[1]):    # the edge sweeps, two sources
        out += [(g, f, 129, 3, 2) for f in F_EDGES] + [(g, 11, t, 3, 2) for t in T_EDGES if t != 129]
    for i, g in enumerate(PRESET_DOWN + PRESET_UP):                            # every preset tuple, edges in rotation
        out.append((g, F_EDGES[i % 4], T_EDGES[(i * 2 + 1) % 5], 3 + i % 3, 0 if i % 2 else 2))
    return [c for c in out if R.conv2d_out_rows(c[1], c[0][0], c[0][2], c[0][3], c[0][5], c[0][7]) >= 1]


@pytest.mark.parametrize("geom,f_in,t_in,c1,c2", _conv_cases())
def test_conv2d_family(H, dev, geom, f_in, t_in, c1, c2):
    """conv2d_lds_kernel (M = 6), conv2d_rows_kernel (M = 2), conv2d_f16x2_kernel and the statistics epilogue at every preset
    geometry and two dilated ones, F and T at the tile edges (T = 1025: nine 128-frame tiles), one source and two."""
    kf, kt, sf, df, dt, pf, pt, transposed = geom
    n, m = (1 if f_in * t_in > 100000 else 2), 6
    t = t_in
    if pt < 0:                                                 # the untrimmed decoder form
        t, pt = t_in + dt * (kt - 1), 0
    f_out = R.conv2d_out_rows(f_in, kf, sf, df, pf, transposed)
    x1 = _rand((n, c1, f_in, t_in), 81)
    x2 = _rand((n, c2, f_in, t_in), 82) if c2 else None
    x = torch.cat([x1, x2], 1) if c2 else x1
    w2, b, slope = _rand((m, (c1 + c2) * kf * kt), 83, -0.3, 0.3), _rand((m,), 84), torch.tensor([0.2])
    pre = R.conv2d_taps(x, w2, b, t, f_out, kf, kt, sf, df, dt, pf, pt, transposed)
    ref = R.activation(pre, "prelu", 0.2)
    d1, d2 = _pad4(H, dev, x1, t), (None if x2 is None else _pad4(H, dev, x2, t))
    bd, sd = b.to(dev), slope.to(dev)
    tail = (t, f_out, kf, kt, sf, df, dt, pf, pt, transposed)
    y6 = H.conv2d(d1, d2, H.pack_wt(w2.to(dev)), bd, m, *tail, "prelu", sd, t_in=t_in)
    y2 = H.conv2d(d1, d2, H.pack_wt(w2[:2].contiguous().to(dev)), bd[:2].contiguous(), 2, *tail, "prelu", sd, t_in=t_in)
    ys, stats = H.conv2d_stats(d1, d2, H.pack_wt(w2.to(dev)), bd, m, *tail, t_in=t_in)
    y0 = H.conv2d(d1, d2, H.pack_wt(w2.to(dev)), bd, m, *tail, "none", None, t_in=t_in)
    img, w_exp = H.pack_conv2d_f16x2(w2.to(dev))
    yh = H.conv2d_f16x2(d1, d2, img, w_exp, bd, m, *tail, "prelu", sd, t_in=t_in)
    yhs, hstats = H.conv2d_f16x2(d1, d2, img, w_exp, bd, m, *tail, t_in=t_in, want_stats=True)
    torch.cuda.synchronize()
    e = (_err(y6[..., :t], ref), _err(y2[..., :t], ref[:, :2]), _err(yh[..., :t], ref), _err(yhs[..., :t], pre))
    print("conv2d", geom, f_in, t_in, c1, c2, e)
    assert max(e) < FP32, e
    assert torch.equal(ys, y0)                                 # the statistics epilogue changes no output bit
    for y in (y6, y2, ys, yh, yhs):
        assert y.shape[2] == f_out and (y.shape[-1] == t or float(y[..., t:].abs().max()) == 0.0)
    for st in (stats, hstats):
        tot = st.sum(1).cpu().numpy()
        np.testing.assert_allclose(tot[:, 0], pre.sum((1, 2, 3)).numpy(), rtol=1e-5, atol=1e-3)
        np.testing.assert_allclose(tot[:, 1], (pre ** 2).sum((1, 2, 3)).numpy(), rtol=1e-5)


def test_conv2d_refusals(H, dev):
    x = torch.zeros(1, 2, 4, 128, device=dev)
    wt, b = H.pack_wt(torch.zeros(3, 12, device=dev)), torch.zeros(3, device=dev)
    ok = (3, 100, 4, 3, 2, 1, 1, 1, 1, 1, False)
    H.conv2d(x, None, wt, b, *ok, "relu", None)
    with pytest.raises(RuntimeError):                       # PReLU without a slope
        H.conv2d(x, None, wt, b, *ok, "prelu", None)
    with pytest.raises(RuntimeError):                       # more frames than the row holds
        H.conv2d(x, None, wt, b, 3, 129, *ok[2:], "relu", None)
    with pytest.raises(RuntimeError):                       # zero stride
        H.conv2d_stats(x, None, wt, b, 3, 100, 4, 3, 2, 0, 1, 1, 1, 1, False)
    with pytest.raises(RuntimeError):                       # sources that disagree in F
        H.conv2d(x, torch.zeros(1, 2, 5, 128, device=dev), wt, b, *ok, "relu", None)
    with pytest.raises(RuntimeError):                       # rows that are no multiple of 128 frames
        H.conv2d(torch.zeros(1, 2, 4, 64, device=dev), None, wt, b, 3, 50, *ok[2:], "relu", None)
    with pytest.raises(RuntimeError):                       # K = 1366 * 3 = 4098 > 4096: the unfold path's job
        H.conv2d(torch.zeros(1, 1366, 1, 128, device=dev), None, wt, b, 3, 100, 1, 3, 1, 1, 1, 1, 1, 0, False, "relu", None)
    img, w_exp = H.pack_conv2d_f16x2(torch.ones(3, 12, device=dev))
    with pytest.raises(RuntimeError):
        H.conv2d_f16x2(x, None, img, w_exp, b, *ok, "prelu", None)


# ------------------------------------------------------------------------------------------------
# ps_row_stats_f64 / ps_conv2d_stats_f32 / conv1x1 statistics -> ps_norm_activation_f32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ch,f,t", [(2, 3, 5, 1), (1, 8, 300, 127), (2, 4, 7, 128), (2, 5, 3, 129), (1, 2, 600, 1025),
                                      (1, 1, 1, 1025), (2, 1, 1, 1)])
def test_row_stats_then_norm_activation(H, dev, n, ch, f, t):
    """GlobLN on its own over a 4-D map with a large mean (cancellation in E[x^2] - mean^2 would show), all six activations,
    NaN in the input's pad columns, exact zeros in the output's."""
    x = _rand((n, ch, f, t), 91) + 100.0
    gamma, beta, slope = _rand((ch,), 92) + 1.5, _rand((ch,), 93), torch.tensor([0.25])
    gd, bd, sd = gamma.to(dev), beta.to(dev), slope.to(dev)
    for kind in R.ACT_KINDS:
        xd = _pad4(H, dev, x)
        stats = H.row_stats(xd.view(n, ch * f, -1), t)
        pro = H.make_prologue(_abi.PS_NORM_GLOBAL, False, stats, float(ch * f * t), 1e-8, gd, bd, None)
        y = H.norm_activation_(xd, t, pro, 0.0, 0.0, kind, sd if kind == "prelu" else None)
        torch.cuda.synchronize()
        tot = stats.sum(1).cpu().numpy()
        np.testing.assert_allclose(tot[:, 0], x.double().sum((1, 2, 3)).numpy(), rtol=1e-9)
        np.testing.assert_allclose(tot[:, 1], (x.double() ** 2).sum((1, 2, 3)).numpy(), rtol=1e-9)
        ref = R.gln_act(x, gamma, beta, 1e-8, kind, 0.25)
        e = _err(y[..., :t], ref)
        print("row_stats + norm_activation", (n, ch, f, t), kind, e)
        assert e < FP32, (kind, e)
        assert y.shape[-1] == t or float(y[..., t:].abs().max()) == 0.0


@pytest.mark.parametrize("t", [1, 127, 129, 1025])
@pytest.mark.parametrize("kind", ["prelu", "tanh"])
def test_conv_statistics_then_norm_activation(H, dev, t, kind):
    """The two ways Unet feeds a gLN: conv2d_stats with no correction (Unet._gln_act) and unfold2d + conv1x1(want_stats) over
    f_out * ld frames with the pad-column correction of Unet._gemm_act; |bias| ~ 3, so a missing or doubled correction moves
    the result far past the tolerance.  Reference: float64 gLN over the valid frames only."""
    n, c, m, f_in = 2, 3, 5, 11
    kf, kt, sf, df, dt, pf, pt, transposed = 5, 2, 2, 1, 1, 2, 1, False
    f_out = R.conv2d_out_rows(f_in, kf, sf, df, pf, transposed)
    x = _rand((n, c, f_in, t), 101)
    w2, b = _rand((m, c * kf * kt), 102, -0.3, 0.3), torch.tensor([3.0, -2.5, 3.5, 2.0, -3.0])
    gamma, beta, slope = _rand((m,), 103) + 1.5, _rand((m,), 104), torch.tensor([0.25])
    gd, bd, sd = gamma.to(dev), beta.to(dev), (slope.to(dev) if kind == "prelu" else None)
    ref = R.gln_act(R.conv2d_taps(x, w2, b, t, f_out, kf, kt, sf, df, dt, pf, pt, transposed), gamma, beta, 1e-8, kind, 0.25)
    xd, wt = _pad4(H, dev, x), H.pack_wt(w2.to(dev))
    ld = xd.shape[-1]
    count = float(m * f_out * t)
    # (b) the implicit GEMM: statistics over the valid frames only
    y, stats = H.conv2d_stats(xd, None, wt, b.to(dev), m, t, f_out, kf, kt, sf, df, dt, pf, pt, transposed)
    pro = H.make_prologue(_abi.PS_NORM_GLOBAL, False, stats, count, 1e-8, gd, bd, None)
    y = H.norm_activation_(y, t, pro, 0.0, 0.0, kind, sd)
    # (c) the tap matrix and the plain GEMM: statistics over all f_out * ld frames, the pad columns' share taken out
    taps = H.unfold2d(xd, None, t, f_out, kf, kt, sf, df, dt, pf, pt, transposed)
    z, zst = H.conv1x1(taps, f_out * ld, wt, m, None, b.to(dev), want_stats=True,
                       out=torch.empty(n, m, f_out * ld, dtype=torch.float32, device=dev))
    cs, cq = R.pad_column_correction(b, f_out, ld, t)
    pro2 = H.make_prologue(_abi.PS_NORM_GLOBAL, False, zst, count, 1e-8, gd, bd, None)
    z = H.norm_activation_(z.view(n, m, f_out, ld), t, pro2, cs, cq, kind, sd)
    torch.cuda.synchronize()
    e = (_err(y[..., :t], ref), _err(z[..., :t], ref))
    print("conv stats + norm_activation", t, kind, e)
    assert max(e) < FP32, e
    assert float(y[..., t:].abs().max()) == 0.0 and float(z[..., t:].abs().max()) == 0.0


def test_norm_activation_affine_and_refusals(H, dev):
    n, ch, f, t = 2, 5, 7, 129
    x = _rand((n, ch, f, t), 111)
    scale, shift = _rand((ch,), 112) + 1.5, _rand((ch,), 113)
    sc_d, sh_d = scale.to(dev), shift.to(dev)                  # (a prologue holds raw pointers: the tensors must outlive it)
    pro = H.make_prologue(_abi.PS_NORM_AFFINE, False, None, 0.0, 0.0, sc_d, sh_d, None)
    y = H.norm_activation_(_pad4(H, dev, x), t, pro, 0.0, 0.0, "mish", None)
    ref = R.activation(x.double() * scale.double().reshape(1, -1, 1, 1) + shift.double().reshape(1, -1, 1, 1), "mish")
    assert _err(y[..., :t], ref) < FP32
    assert float(y[..., t:].abs().max()) == 0.0
    xd = torch.zeros(n, ch, f, 256, device=dev)
    with pytest.raises(RuntimeError):                       # PReLU without a slope
        H.norm_activation_(xd, t, pro, 0.0, 0.0, "prelu", None)
    with pytest.raises(RuntimeError):                       # a global norm without statistics
        H.norm_activation_(xd, t, H.make_prologue(_abi.PS_NORM_GLOBAL, False, None, 10.0, 1e-8, sc_d, sh_d), 0.0, 0.0, "relu", None)
    with pytest.raises(RuntimeError):                       # no norm at all
        H.norm_activation_(xd, t, H.make_prologue(_abi.PS_NORM_NONE), 0.0, 0.0, "relu", None)
    with pytest.raises(RuntimeError):                       # ld % 4
        H.norm_activation_(torch.zeros(n, ch, f, 130, device=dev), t, pro, 0.0, 0.0, "relu", None)
    with pytest.raises(RuntimeError):                       # more frames than the row holds
        H.row_stats(torch.zeros(2, 3, 128, device=dev), 129)


# ------------------------------------------------------------------------------------------------
# ps_activation_f32, ps_add_f32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,t", [(7, 1), (5, 127), (3, 128), (9, 129), (2, 1025), (65535 + 3, 100)])
def test_activation(H, dev, rows, t):
    """kinds 0-5, arguments up to +-100 (mish and sigmoid stay finite), rows = 65 535 + 3 (the chunked launch), pads cleared"""
    x = _rand((rows, t), 121, -4.0, 4.0)
    x.view(-1)[::7] *= 25.0
    x[-1, -1], x[0, 0] = 100.0, -100.0
    slope = torch.tensor([0.25])
    for kind in R.ACT_KINDS:
        y = H.activation_(_pad(H, dev, x), kind, slope.to(dev) if kind == "prelu" else None, t)
        torch.cuda.synchronize()
        ref = R.activation(x, kind, 0.25)
        assert torch.isfinite(y).all(), kind
        if kind in ("none", "relu"):
            assert torch.equal(y[..., :t].cpu(), ref.float()), kind
        else:
            assert _err(y[..., :t], ref) < (EXACT1 if kind == "prelu" else FP32), kind
        assert float(y[..., t:].abs().sum()) == 0.0, kind
    with pytest.raises(RuntimeError):
        H.activation_(torch.zeros(2, 128, device=dev), "prelu", None, 100)
    with pytest.raises(RuntimeError):
        H.activation_(torch.zeros(2, 130, device=dev), "relu", None, 100)
    with pytest.raises(RuntimeError):
        H.activation_(torch.zeros(2, 128, device=dev), "relu", None, 129)


@pytest.mark.parametrize("count", [4, 1020, (1 << 20) + 4])
def test_add(H, dev, count):
    a, b = _rand((count,), 131), _rand((count,), 132, -3.0, 3.0)
    got = H.add_(a.to(dev), b.to(dev))
    assert torch.equal(got.cpu(), (a.double() + b.double()).float())
    with pytest.raises(RuntimeError):                       # count % 4
        H.add_(torch.zeros(6, device=dev), torch.zeros(6, device=dev))
    with pytest.raises(RuntimeError):
        H.add_(torch.zeros(8, device=dev), torch.zeros(4, device=dev))


# ------------------------------------------------------------------------------------------------
# GatedTCN and SkiM glue: ps_unfold_taps(_out)_f32, ps_gated_product_f32, ps_lstm_cell_f32, ps_film_apply_f32
# ------------------------------------------------------------------------------------------------
T_ROWS = (1, 127, 128, 129, 4001)


def _unfold_ref(x, t_out, taps, dil, left, scale, shift, embed):
    n, k, t = x.shape
    e = 0 if embed is None else embed.shape[1]
    xs = x if scale is None else x * scale.reshape(n, k, 1) + shift.reshape(n, k, 1)
    full = xs if embed is None else torch.cat([xs, embed.reshape(n, e, 1).expand(n, e, t)], 1)
    out = torch.zeros(n, taps, k + e, t_out)
    for j in range(taps):
        for tt in range(t_out):
            src = tt + j * dil - left
            if 0 <= src < t:
                out[:, j, :, tt] = full[:, :, src]
    return out.reshape(n, taps * (k + e), t_out)


@pytest.mark.parametrize("t", T_ROWS)
@pytest.mark.parametrize("taps,dil,left,extra,film,emb", [(3, 2, 2, 0, False, 0), (3, 4, 8, 8, True, 5), (2, 1, 1, 0, True, 0),
                                                          (5, 3, 6, 12, False, 3)])
def test_unfold_taps(H, dev, t, taps, dil, left, extra, film, emb):
    """tap-shifted copies with zero padding, FiLM before the padding, embedding rows, t_out != t; pure data movement (the
    affine is one fused multiply-add at most: compared at the one-product tolerance)"""
    n, k = 2, 7
    x = _rand((n, k, t), 141)
    scale, shift = (_rand((n, k), 142) + 1.5, _rand((n, k), 143)) if film else (None, None)
    embed = _rand((n, emb), 144) if emb else None
    t_out = t + extra
    xd = _pad(H, dev, x, fill=NAN) if t_out == t else H.pad_rows(x.to(dev), t_out)
    if t_out != t:
        xd[..., t:] = NAN
    dv = lambda v: None if v is None else v.to(dev)  # noqa: E731
    y = H.unfold_taps(xd, t, taps, dil, left, dv(scale), dv(shift), dv(embed), t_out=None if t_out == t else t_out)
    torch.cuda.synchronize()
    ref = _unfold_ref(x.double(), t_out, taps, dil, left, None if scale is None else scale.double(),
                      None if shift is None else shift.double(), None if embed is None else embed.double())
    got = y[..., :t_out].cpu()
    if film:
        assert _err(got, ref) < EXACT1
    else:
        assert torch.equal(got, ref.float())


def test_unfold_taps_refusals(H, dev):
    x = torch.zeros(1, 3, 128, device=dev)
    with pytest.raises(RuntimeError):                       # a scale without a shift
        H.unfold_taps(x, 100, 3, 1, 1, torch.zeros(1, 3, device=dev), None)
    with pytest.raises(RuntimeError):                       # t_out beyond the row
        H.unfold_taps(x, 100, 3, 1, 1, t_out=129)
    with pytest.raises(RuntimeError):                       # t_out < t
        H.unfold_taps(x, 100, 3, 1, 1, t_out=50)
    with pytest.raises(RuntimeError):                       # dilation 0
        H.unfold_taps(x, 100, 3, 0, 1)


def _gate_side(H, dev, norm, x, t, seed):
    """-> (prologue, keep-alive tensors, float64 reference of PReLU(norm(x)))"""
    n, h, _ = x.shape
    gamma, beta, slope = _rand((h,), seed) + 1.5, _rand((h,), seed + 1), torch.tensor([0.3])
    xd = x.double()
    if norm == _abi.PS_NORM_NONE:
        keep = (slope.to(dev),)
        return H.make_prologue(norm, True, slope=keep[0]), keep, R.activation(xd, "prelu", 0.3)
    keep = [gamma.to(dev), beta.to(dev), slope.to(dev)]
    g, b = gamma.double().reshape(1, -1, 1), beta.double().reshape(1, -1, 1)
    if norm == _abi.PS_NORM_AFFINE:
        return H.make_prologue(norm, True, gamma=keep[0], beta=keep[1], slope=keep[2]), keep, R.activation(xd * g + b, "prelu", 0.3)
    keep.append(H.row_stats(_pad(H, dev, x), t))
    mean = xd.mean((1, 2), keepdim=True)
    var = ((xd - mean) ** 2).mean((1, 2), keepdim=True)
    pro = H.make_prologue(norm, True, keep[3], float(h * t), 1e-8, keep[0], keep[1], keep[2])
    return pro, keep, R.activation(g * (xd - mean) / torch.sqrt(var + 1e-8) + b, "prelu", 0.3)


@pytest.mark.parametrize("t", T_ROWS)
@pytest.mark.parametrize("nl,nr", [(0, 1), (1, 2), (2, 0), (1, 1)])
def test_gated_product(H, dev, t, nl, nr):
    """PReLU(norm(left)) * sigmoid(PReLU(norm(right))) with none / gLN / folded-bN prologues on either side, odd H"""
    n, h = 2, 9
    left, right = _rand((n, h, t), 151, -2, 2), _rand((n, h, t), 152, -2, 2) + 0.5
    pl, keep_l, rl = _gate_side(H, dev, nl, left, t, 153)
    pr, keep_r, rr = _gate_side(H, dev, nr, right, t, 155)
    y = H.gated_product(_pad(H, dev, left), _pad(H, dev, right), t, pl, pr)
    torch.cuda.synchronize()
    assert _err(y[..., :t], rl * torch.sigmoid(rr)) < FP32
    del keep_l, keep_r


def test_gated_product_refusals(H, dev):
    x = torch.zeros(1, 3, 128, device=dev)
    none = H.make_prologue(_abi.PS_NORM_NONE)
    with pytest.raises(RuntimeError):                       # a norm without gamma / beta
        H.gated_product(x, x, 100, H.make_prologue(_abi.PS_NORM_AFFINE), none)
    with pytest.raises(RuntimeError):                       # a global norm without statistics
        H.gated_product(x, x, 100, none, H.make_prologue(_abi.PS_NORM_GLOBAL, gamma=x, beta=x))
    with pytest.raises(RuntimeError):                       # PReLU without a slope
        H.gated_product(x, x, 100, H.make_prologue(_abi.PS_NORM_NONE, True), none)
    with pytest.raises(RuntimeError):                       # ld % 4
        y = torch.zeros(1, 3, 130, device=dev)
        H.gated_product(y, y, 100, none, none)


@pytest.mark.parametrize("t", T_ROWS)
@pytest.mark.parametrize("n,hid,d,views", [(2, 5, 2, False), (1, 7, 1, True), (3, 1, 1, False)])
def test_lstm_cell(H, dev, t, n, hid, d, views):
    """one cell update per (unit, frame); odd H (the four-units-per-workgroup tail), two directions, states as row views of a
    wider block (ld_gates != ld_state) for N = 1"""
    gates, c0 = _rand((n, d * 4 * hid, t), 161, -3, 3), _rand((n, d * hid, t), 162)
    gd = _pad(H, dev, gates)
    if views:
        wide = torch.full((n, 2 * d * hid + 3, gd.shape[-1] + 128), NAN, device=dev)
        c, h = wide[:, 1:1 + d * hid, :], wide[:, 2 + d * hid:2 + 2 * d * hid, :]
        c[..., :t] = c0.to(dev)
    else:
        c, h = _pad(H, dev, c0), torch.full((n, d * hid, gd.shape[-1]), NAN, device=dev)
    H.lstm_cell(gd, c, h, hid, d, t)
    torch.cuda.synchronize()
    g = gates.double().reshape(n, d, 4, hid, t)
    cn = torch.sigmoid(g[:, :, 1]) * c0.double().reshape(n, d, hid, t) + torch.sigmoid(g[:, :, 0]) * torch.tanh(g[:, :, 2])
    hn = torch.sigmoid(g[:, :, 3]) * torch.tanh(cn)
    assert _err(c[..., :t], cn.reshape(n, d * hid, t)) < FP32
    assert _err(h[..., :t], hn.reshape(n, d * hid, t)) < FP32
    if views:                                                  # nothing outside the two row blocks was written
        assert torch.isnan(wide[:, 0]).all() and torch.isnan(wide[:, 1 + d * hid]).all() and torch.isnan(wide[:, -1]).all()
        assert torch.isnan(c[..., t:]).all() and torch.isnan(h[..., t:]).all()


def test_lstm_cell_and_film_refusals(H, dev):
    g = torch.zeros(1, 8, 128, device=dev)
    with pytest.raises(RuntimeError):                       # gates that are not D * 4H rows
        H.lstm_cell(g, torch.zeros(1, 3, 128, device=dev), torch.zeros(1, 3, 128, device=dev), 3, 1, 100)
    with pytest.raises(RuntimeError):                       # more frames than the state rows hold
        H.lstm_cell(torch.zeros(1, 8, 256, device=dev), torch.zeros(1, 2, 128, device=dev), torch.zeros(1, 2, 128, device=dev),
                    2, 1, 200)
    with pytest.raises(RuntimeError):                       # three directions
        H.lstm_cell(torch.zeros(1, 24, 128, device=dev), torch.zeros(1, 6, 128, device=dev), torch.zeros(1, 6, 128, device=dev),
                    2, 3, 100)
    with pytest.raises(RuntimeError):                       # scale_bias that is not [N, 2C, ldt]
        H.film_apply(torch.zeros(1, 3, 128, device=dev), torch.zeros(1, 5, 128, device=dev), 100)
    with pytest.raises(RuntimeError):                       # ld % 4
        H.film_apply(torch.zeros(1, 3, 130, device=dev), torch.zeros(1, 6, 130, device=dev), 100)


@pytest.mark.parametrize("t", T_ROWS)
def test_film_apply(H, dev, t):
    n, c = 2, 7
    x, sb = _rand((n, c, t), 171), _rand((n, 2 * c, t), 172, -2, 2)
    y = H.film_apply(_pad(H, dev, x), _pad(H, dev, sb), t)
    torch.cuda.synchronize()
    assert _err(y[..., :t], sb[:, :c].double() * x.double() + sb[:, c:].double()) < EXACT1


# ------------------------------------------------------------------------------------------------
# masks and spectra: ps_real_mask_f32, ps_polar_mask_f32, ps_magphase_f32, ps_magnitude_f32, ps_fill_span_f32
# ------------------------------------------------------------------------------------------------
def _mask_act(m, act):
    return {"linear": m, "relu": m.clamp(min=0), "sigmoid": torch.sigmoid(m)}[act]


@pytest.mark.parametrize("t", T_ROWS)
@pytest.mark.parametrize("act", ["linear", "relu", "sigmoid"])
def test_real_mask(H, dev, t, act):
    x, m = _rand((2, 7, t), 181), _rand((2, 7, t), 182, -3, 3)
    y = H.real_mask(_pad(H, dev, x), _pad(H, dev, m), act)
    torch.cuda.synchronize()
    assert _err(y[..., :t], x.double() * _mask_act(m.double(), act)) < (FP32 if act == "sigmoid" else EXACT1)


def _spectrum(n, half, t, seed):
    """[re ; im] rows with the awkward bins: re < 0 with im = +-0, zero magnitude, a tiny magnitude"""
    x = _rand((n, 2 * half, t), seed, -2, 2)
    if t >= 4:
        x[:, 0, 0], x[:, half, 0] = -1.5, 0.0
        x[:, 0, 1], x[:, half, 1] = -0.5, -0.0
        x[:, 0, 2], x[:, half, 2] = 0.0, 0.0
        x[:, 1, 3], x[:, half + 1, 3] = 1e-6, -1e-6
    return x


@pytest.mark.parametrize("t", T_ROWS)
def test_polar_mask(H, dev, t):
    n, half = 2, 5
    x, m = _spectrum(n, half, t, 191), _spectrum(n, half, t, 192).flip(1)
    y = H.polar_mask(_pad(H, dev, x), _pad(H, dev, m))
    torch.cuda.synchronize()
    xd, md = x.double(), m.double()
    re, im, mre, mim = xd[:, :half], xd[:, half:], md[:, :half], md[:, half:]
    mag, mmag = torch.sqrt(re ** 2 + im ** 2 + 1e-8), torch.sqrt(mre ** 2 + mim ** 2 + 1e-8)
    ph = torch.atan2(im, re) + torch.atan2(mim / (mmag + 1e-8), mre / (mmag + 1e-8))
    est = mag * torch.tanh(mmag)
    assert _err(y[..., :t], torch.cat([est * torch.cos(ph), est * torch.sin(ph)], 1)) < FP32


@pytest.mark.parametrize("t", T_ROWS)
@pytest.mark.parametrize("take_sqrt", [False, True])
def test_magphase(H, dev, t, take_sqrt):
    n, half = 2, 5
    x = _spectrum(n, half, t, 201)
    y = H.magphase(_pad(H, dev, x), take_sqrt)[..., :t].cpu().double()
    re, im = x.double()[:, :half], x.double()[:, half:]
    p = re ** 2 + im ** 2
    assert _err(y[:, :half], torch.sqrt(p + 1e-8) if take_sqrt else p) < EXACT1
    ph = torch.atan2(im + 0.0, re)                             # compared as (cos, sin): a +-pi wrap is no failure
    assert _err(torch.cos(y[:, half:]), torch.cos(ph)) < FP32 and _err(torch.sin(y[:, half:]), torch.sin(ph)) < FP32
    assert float((y[:, half:].abs() - np.pi).max()) < 1e-6     # a phase, not a phase + 2 pi


@pytest.mark.parametrize("t", T_ROWS)
@pytest.mark.parametrize("drop,kind", [(False, 0), (True, 1), (True, 2), (False, 3), (True, 0)])
def test_magnitude(H, dev, t, drop, kind):
    n, half = 2, 5
    x = _spectrum(n, half, t, 211)
    y = H.magnitude(_pad(H, dev, x), t, drop, kind == 1, {2: "power", 3: "power_eps"}.get(kind))
    torch.cuda.synchronize()
    d = int(drop)
    p = x.double()[:, d:half] ** 2 + x.double()[:, half + d:] ** 2
    ref = {0: torch.sqrt(p + 1e-8), 1: torch.log1p(torch.sqrt(p + 1e-8)), 2: p, 3: p + 1e-8}[kind]
    assert y.shape[1] == half - d
    assert _err(y[..., :t], ref) < (FP32 if kind == 1 else EXACT1)


@pytest.mark.parametrize("t", T_ROWS)
def test_fill_span(H, dev, t):
    """rows (axis 1) and frames (axis 2), empty and full spans, spans that cut a four-float vector"""
    n, rows = 2, 7
    x = _rand((n, rows, t), 221)
    xd = H.pad_rows(x.to(dev))
    ld = xd.shape[-1]
    for axis, lo, hi in [(1, 0, 0), (1, 0, rows), (1, 2, 5), (1, 6, 7), (2, 0, 0), (2, 0, ld), (2, min(1, t - 1), t),
                         (2, t // 2, t // 2 + 1), (2, 3, 3), (2, t - 1, ld + 5)]:
        y = H.fill_span(xd, axis, lo, hi, -7.5)
        ref = xd.clone()
        if axis == 1:
            ref[:, lo:hi] = -7.5
        else:
            ref[:, :, lo:hi] = -7.5
        assert torch.equal(y, ref), (axis, lo, hi)
    with pytest.raises(RuntimeError):
        H.fill_span(xd, 3, 0, 1, 0.0)
    with pytest.raises(RuntimeError):
        H.fill_span(xd, 1, 3, 2, 0.0)
    with pytest.raises(RuntimeError):
        H.fill_span(torch.zeros(1, 2, 6, device=dev), 2, 0, 1, 0.0)


def test_mask_refusals(H, dev):
    x = torch.zeros(1, 4, 128, device=dev)
    with pytest.raises(RuntimeError):
        H.real_mask(x, torch.zeros(1, 4, 256, device=dev))
    with pytest.raises(RuntimeError):                       # ld % 4
        H.real_mask(torch.zeros(1, 4, 6, device=dev), torch.zeros(1, 4, 6, device=dev))
    with pytest.raises(RuntimeError):                       # rows that are no multiple of 128 frames
        H.polar_mask(torch.zeros(1, 4, 64, device=dev), torch.zeros(1, 4, 64, device=dev))
    with pytest.raises(RuntimeError):
        H.polar_mask(x, torch.zeros(1, 6, 128, device=dev))
    with pytest.raises(RuntimeError):
        H.magphase(torch.zeros(1, 4, 64, device=dev), True)
    with pytest.raises(RuntimeError):                       # nothing left after dropping the first bin
        H.magnitude(torch.zeros(1, 2, 128, device=dev), 100, True, False)
    with pytest.raises(RuntimeError):                       # more frames than the row holds
        H.magnitude(x, 129, False, False)


# ------------------------------------------------------------------------------------------------
# ps_attn_weights_f32, ps_attn_stats_pool_len_f32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,c,t", [(2, 24, 77), (3, 512, 249), (1, 40, 1500), (2, 16, 3999), (2, 8, 4096), (2, 8, 5000)])
def test_attention_pooling_with_lengths(H, dev, n, c, t):
    """relative lengths 1, 0.5, one valid frame and longer than the row, under both pooling kernels; masked weights are exact
    zeros, the weights' pad columns too"""
    logits, x = _rand((n, c, t), 231, -3.0, 3.0), _rand((n, c, t), 232)
    ld, xd = _pad(H, dev, logits), _pad(H, dev, x)
    for rel in (1.0, 0.5, 1.0 / t, 1.5):
        lengths = torch.tensor([rel, 1.0, rel][:n], dtype=torch.float32)
        k = R.valid_frames(lengths, t)
        assert int(k[0]) == min(t, int(np.ceil(rel * t - 1e-4)))
        w_ref, p_ref = R.attn_pool(logits, x, lengths, 1e-12)
        w = H.attn_weights(ld, t, lengths.to(dev))
        assert _err(w[..., :t], w_ref) < FP32, rel
        for i in range(n):
            assert float(w[i, :, int(k[i]):].abs().max() if int(k[i]) < w.shape[-1] else 0.0) == 0.0, rel
        for flags in (0, _abi.PS_DBG_POOL_THREE_PASS):
            with _abi.debug(flags):
                out = H.attn_stats_pool(ld, xd, t, lengths=lengths.to(dev))
                torch.cuda.synchronize()
            assert _err(out, p_ref) < FP32, (rel, flags)
    w = H.attn_weights(ld, t)                                  # no lengths: every frame
    assert _err(w[..., :t], torch.softmax(logits.double(), 2)) < FP32 and float(w[..., t:].abs().max()) == 0.0
    with pytest.raises(RuntimeError):
        H.attn_stats_pool(ld, xd, t, lengths=torch.ones(n + 1, device=dev))
    with pytest.raises(RuntimeError):
        H.attn_weights(ld, t, torch.ones(n + 1))
    with pytest.raises(RuntimeError):                       # more frames than the row holds
        H.attn_weights(ld, ld.shape[-1] + 1)


# ------------------------------------------------------------------------------------------------
# streaming harness: ps_overlap_average_f32, ps_stream_windows_f32, ps_stream_overlap_f32, ps_stream_commit_frames_f32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 64, 257])
@pytest.mark.parametrize("win,overlap,length", [(32, 16, 48), (32, 32, 32), (300, 1, 7), (16, 5, 5)])
def test_overlap_average(H, dev, b, win, overlap, length):
    prev, cur = _rand((b, length + 3), 241), _rand((b, win), 242)
    out = H.overlap_average(prev.to(dev)[:, :length], cur.to(dev), overlap)      # a row view: ld_tail != overlap
    ref = cur.double().clone()
    ref[:, :overlap] = (prev.double()[:, length - overlap:length] + cur.double()[:, :overlap]) / 2
    assert _err(out, ref) < EXACT1 and torch.equal(out[:, overlap:].cpu(), cur[:, overlap:])
    with pytest.raises(RuntimeError):                       # a tail shorter than the overlap
        H.overlap_average(prev.to(dev)[:, :2], cur.to(dev), 3)
    with pytest.raises(RuntimeError):
        H.overlap_average(prev.to(dev)[:1], cur.to(dev)[:1], win + 1)


@pytest.mark.parametrize("b", [1, 64, 257])
@pytest.mark.parametrize("win,hop,hops", [(32, 16, 8), (8, 8, 1), (16, 8, 3), (2, 1, 8), (1, 1, 1), (24, 8, 5)])
def test_stream_windows_and_overlap(H, dev, b, win, hop, hops):
    """all hops of a chunk in two launches against the offline framing / averaging overlap-add; win == hop, win = 2 hop and
    win = 3 hop for the windows, win = 2 hop for the overlap-add (anything else is refused)"""
    queue, chunk = _rand((b, win), 251), _rand((b, hops * hop), 252)
    wins = torch.full((hops, b * win), NAN, device=dev)
    H.stream_windows(queue.to(dev), chunk.to(dev), wins, hop)
    ref = R.stream_windows(queue.numpy(), chunk.numpy(), hop)
    assert np.array_equal(wins.cpu().numpy().reshape(hops, b, win), ref)
    frames, tail = _rand((hops, b, win), 253), _rand((b, hop), 254)
    td, qd = tail.to(dev), torch.full((b, win), NAN, device=dev)
    blocks = torch.full((b, hops * hop), NAN, device=dev)
    if win != 2 * hop:
        with pytest.raises(RuntimeError):
            H.stream_overlap(frames.to(dev), wins, td, blocks, qd, hop)
        return
    H.stream_overlap(frames.to(dev), wins, td, blocks, qd, hop)
    want, new_tail = R.stream_overlap(frames.double().numpy(), tail.double().numpy(), hop)
    assert rel_max(blocks.cpu().numpy(), want) < EXACT1
    assert np.array_equal(td.cpu().numpy(), new_tail.astype(np.float32))
    assert np.array_equal(qd.cpu().numpy(), ref[-1])


def test_stream_refusals(H, dev):
    q, c = torch.zeros(2, 8, device=dev), torch.zeros(2, 16, device=dev)
    with pytest.raises(RuntimeError):                       # win < hop
        H.stream_windows(q, torch.zeros(2, 32, device=dev), torch.zeros(2, 16, device=dev), 16)
    with pytest.raises(RuntimeError):                       # wins of the wrong shape
        H.stream_windows(q, c, torch.zeros(3, 16, device=dev), 4)
    tab = H.commit_table([(torch.zeros(8, device=dev), torch.zeros(16, device=dev))])
    with pytest.raises(RuntimeError):                       # frames < 1
        H.stream_commit_frames(tab, torch.zeros(1, dtype=torch.int32, device=dev), 0, dev)
    with pytest.raises(RuntimeError):                       # a slot size that is no multiple of 4 floats
        H.stream_commit_frames(H.commit_table([(torch.zeros(6, device=dev), torch.zeros(12, device=dev))]),
                               torch.zeros(1, dtype=torch.int32, device=dev), 1, dev)


@pytest.mark.parametrize("b", [1, 64, 257])
@pytest.mark.parametrize("frames", [1, 3, 11])
def test_stream_commit_frames(H, dev, b, frames):
    """rings of 1, 2 and 5 slots shift by one slot per commit whatever `frames` is (1, the chunk's 3, more than any ring
    holds); the counter advances by `frames`"""
    ld = _abi.padded_frames(b)
    srcs = [_rand((4, ld), 261), _rand((3, 2, ld), 262), _rand((ld,), 263)]
    rings = [_rand((1, 4, ld), 264), _rand((2, 3, 2, ld), 265), _rand((5, ld), 266)]
    sd, rd = [s.to(dev) for s in srcs], [r.to(dev) for r in rings]
    counter = torch.tensor([41], dtype=torch.int32, device=dev)
    tab = H.commit_table(list(zip(sd, rd)))
    for rep in range(2):
        H.stream_commit_frames(tab, counter, frames, dev)
        rings = [torch.cat([r[1:], s.unsqueeze(0)], 0) for s, r in zip(srcs, rings)]
        assert int(counter.cpu()) == 41 + (rep + 1) * frames
        for r, want in zip(rd, rings):
            assert torch.equal(r.cpu(), want)
    for s, s0 in zip(sd, srcs):
        assert torch.equal(s.cpu(), s0)


# ------------------------------------------------------------------------------------------------
# l2_normalize (ps_embed_bias_f32 with an identity weight)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,e", [(1, 1), (3, 63), (2, 64), (4, 65), (2, 256), (5, 1000)])
def test_l2_normalize(H, dev, n, e):
    import torch.nn.functional as F
    d = _rand((n, e), 271, -2, 2)
    d[0] = 0.0                                                 # a zero row stays zero (the 1e-12 floor), no NaN
    if n > 1:
        d[1] *= 1e-3
    got = H.l2_normalize(d.to(dev))
    ref = F.normalize(d.double(), p=2, dim=1)
    assert torch.equal(got[0].cpu(), torch.zeros(e))
    assert _err(got, ref) < FP32
    with pytest.raises(RuntimeError):                       # a weight on another device
        H.embed_bias(d.to(dev), torch.eye(e), True)
