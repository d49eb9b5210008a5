"""csrc/conv1x1_small.hip below its entries: every instantiation its launchers dispatch to by shape -- conv1x1_small_kernel<NCB, TR>,
conv1x1_small_fused_kernel<NCB, EPI> (+ _cells) with blockIdx.y / blockIdx.z above 0, proj_layernorm_kernel<8, 8> | <8> | <16>
(+ _cells), and the y_amax output of the three row kernels -- through the puresound_amd.hip wrappers, against the float64
references of abi_refs.py (proven on the CPU in test_abi_references.py; cases and inputs: short_row_cases.py).

Every case: the pad columns [t, ldt) of every input row hold NaN, outputs the caller hands in are pre-filled with a sentinel; the
valid frames must be finite and within TOL of fp64 (rel_max), the pad columns of the outputs must still hold the sentinel.  Each
figure is printed before it is asserted (pytest -s / -rP shows them)."""
import pytest
import torch

import abi_refs as R
import short_row_cases as SR
from conftest import rel_max
from puresound_amd import _abi

pytestmark = pytest.mark.gpu
TOL = 2e-5      # the bound of the existing direct tests of these kernels (test_fused_streaming_step_kernels)
SENT = -12345.0
PS_E_UNSUPPORTED = -3   # include/puresound_hip.h


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def H():
    from puresound_amd import hip
    hip.lib()
    return hip


@pytest.fixture
def nan_primed(dev):
    """Best effort, for the one output here that a wrapper allocates with torch.empty and the test reads whole (the maxima):
    freed NaN blocks in torch's caching allocator make it likely -- not certain -- that such an output starts as NaN rather
    than as the zeros of a fresh process, so a slot the kernel never writes shows.  Every other output is handed in pre-filled."""
    junk = [torch.full((n,), float("nan"), device=dev) for n in (1 << 7, 1 << 9, 1 << 11, 1 << 13, 1 << 15, 1 << 17)]
    del junk
    yield


def _rows(H, dev, x, t, min_frames=0, pad=float("nan")):
    """compact CPU rows -> padded device rows whose pad columns hold `pad`; None stays None"""
    if x is None:
        return None
    xd = H.pad_rows(x.to(dev), min_frames)
    xd[..., t:] = pad
    return xd


def _dv(x, dev):
    return None if x is None else x.to(dev)


def _check(group, got, ref, t, sentinel=True, note=""):
    valid = got[..., :t].cpu()
    assert torch.isfinite(valid).all(), note
    r = rel_max(valid.double().numpy(), ref.numpy())
    print(f"rel_max {group} {r:.3e} {note}")
    assert r < TOL, (r, note)
    if sentinel:
        assert bool((got[..., t:] == SENT).all()), f"frames >= T were written {note}"


def _prologue(H, dev, d, pname, glob_stats=None, count=0.0):
    pre_relu, affine, prelu, post_tanh = SR.PROLOGUES[pname]
    keep = (_dv(d["gamma"], dev), _dv(d["beta"], dev), _dv(d["slope"], dev), glob_stats)   # (the prologue carries raw pointers)
    if glob_stats is not None:
        return H.make_prologue(_abi.PS_NORM_GLOBAL, prelu, glob_stats, count, 1e-8, keep[0], keep[1], keep[2]), keep
    if pname == "none":
        return None, keep
    norm = _abi.PS_NORM_AFFINE if affine else _abi.PS_NORM_NONE
    return H.make_prologue(norm, prelu, gamma=keep[0] if affine else None, beta=keep[1] if affine else None,
                           slope=keep[2] if prelu else None, pre_relu=pre_relu, post_tanh=post_tanh), keep


# ------------------------------------------------------------------------------------------------
# ps_conv1x1_f32 on rows of <= 64 frames
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SR.CONV_CASES, ids=str)
def test_conv1x1_short_rows(H, dev, case):
    """conv1x1_small_kernel<NCB, TR> (flags 0) and, on the same rows, the 256 x 128 tile kernel (PS_DBG_CONV1X1_TILED): both
    held to fp64, so the two are pinned to each other through the reference.  The tiled kernel documents that it writes the pad
    columns of y ("never read as data"): the sentinel is asserted for the short-row kernel only."""
    n, k, m, t, _, _, _, pname = case
    d = SR.build_conv1x1(case)
    xd, resd, wt = _rows(H, dev, d["x"], t), _rows(H, dev, d["res"], t), H.pack_wt(d["w"].to(dev))
    pro, keep = _prologue(H, dev, d, pname)
    for flags in (0, _abi.PS_DBG_CONV1X1_TILED):
        out = torch.full((n, m, xd.shape[-1]), SENT, device=dev)
        with _abi.debug(flags):
            y, _ = H.conv1x1(xd, t, wt, m, pro, _dv(d["bias"], dev), _dv(d["bias_n"], dev), resd, out=out)
            torch.cuda.synchronize()
        assert y is out
        _check("conv1x1" if flags == 0 else "conv1x1_tiled", y, d["ref"], t, sentinel=flags == 0, note=f"flags={flags}")
    del keep


@pytest.mark.parametrize("how", ["want_stats", "global_norm"])
def test_conv1x1_short_rows_that_take_the_tiled_kernel_by_default(H, dev, how):
    """output statistics and a global-norm prologue send rows of <= 64 frames to the tiled kernel without a debug switch"""
    n, k, m, t = 3, 33, 70, 49
    case = (n, k, m, t, True, True, False, "prelu")
    d = SR.build_conv1x1(case, glob=how == "global_norm")
    xd, wt = _rows(H, dev, d["x"], t), H.pack_wt(d["w"].to(dev))
    stats = None
    if how == "global_norm":   # the producer's statistics over the valid frames: one exact part per utterance
        x64 = d["x"].double()
        stats = torch.stack([x64.sum((1, 2)), (x64 ** 2).sum((1, 2))], -1).reshape(n, 1, 2).to(dev)
    pro, keep = _prologue(H, dev, d, "prelu", stats, k * t)
    out = torch.full((n, m, xd.shape[-1]), SENT, device=dev)
    y, st = H.conv1x1(xd, t, wt, m, pro, d["bias"].to(dev), d["bias_n"].to(dev), None, want_stats=how == "want_stats", out=out)
    torch.cuda.synchronize()
    _check("conv1x1_tiled", y, d["ref"], t, sentinel=False, note=how)
    # that the tiled kernel ran: it stores whole 128-frame tiles, pad columns included (here NaN, from the NaN pad of x), where
    # the short-row kernel leaves every frame >= T alone (asserted in test_conv1x1_short_rows)
    assert bool((y[..., t:128] != SENT).all()), "the short-row kernel ran"
    if how == "want_stats":    # NaN pad columns of x reach pad columns of y only: the statistics cover t < T
        s = st.sum(1).cpu()
        assert torch.isfinite(s).all()
        torch.testing.assert_close(s[:, 0], d["ref"].sum((1, 2)), rtol=1e-5, atol=1e-3)
        torch.testing.assert_close(s[:, 1], (d["ref"] ** 2).sum((1, 2)), rtol=1e-5, atol=0)
    del keep


# ------------------------------------------------------------------------------------------------
# ps_film_conv_f32 / ps_lstm_gates_cell_f32
# ------------------------------------------------------------------------------------------------
def _film_device(H, dev, d, t):
    res = None if d["rs"] is None else R.film_pack_rows(d["rs"], d["rb"])
    xd = _rows(H, dev, d["x"], t)
    return xd, H.pack_wt(R.film_pack_weights(d["ws"], d["wb"]).to(dev)), _rows(H, dev, res, t), torch.full_like(xd, SENT)


@pytest.mark.parametrize("case", SR.FILM_CASES, ids=str)
def test_film_conv(H, dev, case):
    n, c, t, _ = case
    d = SR.build_film(case)
    xd, wt, resd, out = _film_device(H, dev, d, t)
    y = H.film_conv(xd, t, wt, resd, out=out)
    torch.cuda.synchronize()
    assert y is out
    _check("film_conv", y, d["ref"], t)


def _gates_device(H, dev, d, t, hid, state_frames):
    order = R.gate_unit_major(hid)
    xhd = _rows(H, dev, d["xh"], t)
    cd = _rows(H, dev, d["c"], t, state_frames, pad=SENT)   # a clone of the state; its pad columns must stay as they are
    bias = None if d["bias"] is None else d["bias"][order].to(dev)
    return xhd, H.pack_wt(d["w"][order].contiguous().to(dev)), bias, cd, torch.full_like(cd, SENT)


@pytest.mark.parametrize("case", SR.GATES_CASES, ids=str)
def test_lstm_gates_cell(H, dev, case):
    n, k, hid, t, state_frames, _ = case
    d = SR.build_gates(case)
    xhd, wt, bias, cd, hd = _gates_device(H, dev, d, t, hid, state_frames)
    if state_frames:
        assert cd.shape[-1] != xhd.shape[-1]   # the state rows have their own leading dimension
    H.lstm_gates_cell(xhd, t, wt, bias, cd, hd, hid)
    torch.cuda.synchronize()
    _check("lstm_gates_cell", cd, d["c_ref"], t, note="c'")
    _check("lstm_gates_cell", hd, d["h_ref"], t, note="h'")


# ------------------------------------------------------------------------------------------------
# the _cells launches against fp64 (their bit-equality with the single launches: test_cells_launches_equal_separate_launches)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", SR.CELLS_T)
@pytest.mark.parametrize("ncells", [1, _abi.PS_MAX_CELLS])
def test_cells_launches_against_fp64(H, dev, ncells, t):
    """different weights, inputs and states per cell (blockIdx.y picks the cell's arguments)"""
    assert ncells in (1, H.MAX_CELLS)
    for c in SR.CELLS_FILM_C:
        ds = [SR.build_film((1, c, t, i % 2 == 0), seed=100 * (i + 1)) for i in range(ncells)]
        dvs = [_film_device(H, dev, d, t) for d in ds]
        H.film_conv_cells(dvs, t)
        torch.cuda.synchronize()
        for i, (d, (_, _, _, out)) in enumerate(zip(ds, dvs)):
            _check("cells", out, d["ref"], t, note=f"film C={c} cell {i}")
    for k, hid in SR.CELLS_GATES_KH:
        ds = [SR.build_gates((1, k, hid, t, 0, i % 3 != 2), seed=100 * (i + 1)) for i in range(ncells)]
        dvs = [_gates_device(H, dev, d, t, hid, 0) for d in ds]
        H.lstm_gates_cell_cells(dvs, t, hid)
        torch.cuda.synchronize()
        for i, (d, (_, _, _, cd, hd)) in enumerate(zip(ds, dvs)):
            _check("cells", cd, d["c_ref"], t, note=f"gates K={k} H={hid} cell {i} c'")
            _check("cells", hd, d["h_ref"], t, note=f"gates K={k} H={hid} cell {i} h'")
    for k, m in SR.CELLS_PLN_KM:
        for res_inside in (False, True):
            _pln_cells(H, dev, ncells, t, k, m, res_inside)


def _pln_cells(H, dev, ncells, t, k, m, res_inside):
    """one ps_proj_layernorm_cells_f32 launch; per cell: bias / residual / second norm / copy present or not"""
    ds = [SR.build_pln((1, k, m, t, i % 2 == 0, i % 3 != 1, res_inside, i % 4 != 3, i % 2 == 1), seed=100 * (i + 1))
          for i in range(ncells)]
    cells = []
    for i, d in enumerate(ds):
        xd = _rows(H, dev, d["x"], t)
        g2 = None if d["norm2"] is None else (d["norm2"][0].to(dev), d["norm2"][1].to(dev), d["norm2"][2])
        y = torch.full((1, m, xd.shape[-1]), SENT, device=dev)
        cells.append(dict(x=xd, wt=H.pack_wt(d["w"].to(dev)), bias=_dv(d["bias"], dev), gamma=d["gamma"].to(dev),
                          beta=d["beta"].to(dev), eps=1e-5, res=_rows(H, dev, d["res"], t), norm2=g2, y=y,
                          y2=torch.full_like(y, SENT), x_copy=torch.full_like(xd, SENT) if i % 2 == 1 else None))
    H.proj_layernorm_cells(cells, t, m, res_inside=res_inside)
    torch.cuda.synchronize()
    for i, (d, cell) in enumerate(zip(ds, cells)):
        note = f"proj_ln K={k} M={m} T={t} res_inside={res_inside} cell {i}"
        _check("cells", cell["y"], d["y_ref"], t, note=note + " y")
        if d["norm2"] is not None:
            _check("cells", cell["y2"], d["y2_ref"], t, note=note + " y2")
        else:
            assert bool((cell["y2"] == SENT).all())
        if cell["x_copy"] is not None:
            assert torch.equal(cell["x_copy"][..., :t].cpu(), d["x"]) and bool((cell["x_copy"][..., t:] == SENT).all())


def test_proj_layernorm_cells_on_more_than_64_frame_blocks(H, dev):
    """ceil(T / 16) > 64 takes proj_layernorm_cells_kernel<8> (four waves) at M <= 128, as the single launch does"""
    t = SR.CELLS_T_MANY
    assert (t + 15) // 16 == 65
    for res_inside in (False, True):
        _pln_cells(H, dev, 2, t, 8, 12, res_inside)


# ------------------------------------------------------------------------------------------------
# ps_proj_layernorm_f32: the 16-frame kernel
# ------------------------------------------------------------------------------------------------
def _pln_call(H, dev, d, case, **kw):
    n, k, m, t, _, _, res_inside, _, has_copy = case
    xd = _rows(H, dev, d["x"], t)
    g2 = None if d["norm2"] is None else (d["norm2"][0].to(dev), d["norm2"][1].to(dev), d["norm2"][2])
    out = torch.full((n, m, xd.shape[-1]), SENT, device=dev)
    out2 = torch.full_like(out, SENT) if g2 is not None else None
    cp = torch.full_like(xd, SENT) if has_copy else None
    got = H.proj_layernorm(xd, t, H.pack_wt(d["w"].to(dev)), _dv(d["bias"], dev), m, d["gamma"].to(dev), d["beta"].to(dev), 1e-5,
                           _rows(H, dev, d["res"], t), g2, x_copy=cp, res_inside=res_inside, out=out, out2=out2, **kw)
    torch.cuda.synchronize()
    return got, cp


@pytest.mark.parametrize("case", SR.PLN_CASES, ids=str)
def test_proj_layernorm_16_frame_kernel(H, dev, case):
    n, k, m, t = case[:4]
    d = SR.build_pln(case)
    (y, y2), cp = _pln_call(H, dev, d, case)
    note = SR.pln_kernel(n, m, t)
    _check("proj_layernorm", y, d["y_ref"], t, note=note + " y")
    if d["norm2"] is not None:
        _check("proj_layernorm", y2, d["y2_ref"], t, note=note + " y2")
    else:
        assert y2 is None
    if cp is not None:   # the copy: the input bit for bit on [0, t), nothing beyond
        assert torch.equal(cp[..., :t].cpu(), d["x"]) and bool((cp[..., t:] == SENT).all())


def test_proj_layernorm_refuses_more_than_256_channels(H, dev):
    case = (1, 8, 257, 17, True, True, False, False, False)
    with pytest.raises(RuntimeError, match=rf"rc={PS_E_UNSUPPORTED}\): ps_proj_layernorm_f32: M=257 > 256"):
        _pln_call(H, dev, SR.build_pln(case), case)
    ok = (1, 8, 256, 17, True, True, False, False, False)     # (and the library goes on working)
    (y, _), _ = _pln_call(H, dev, SR.build_pln(ok), ok)
    _check("proj_layernorm", y, SR.build_pln(ok)["y_ref"], 17, note="after the refusal")


# ------------------------------------------------------------------------------------------------
# ps_proj_layernorm_amax_f32: the maxima of |y| the next fp16x2 GEMM takes as its input range
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SR.AMAX_CASES, ids=str)
def test_proj_layernorm_amax_is_exact(H, dev, nan_primed, case):
    n, k, m, t, res_inside, unpipelined = case
    d = SR.build_amax(case)
    full = (n, k, m, t, True, True, res_inside, False, False)
    with _abi.debug(_abi.PS_DBG_PROJ_LN_UNPIPELINED if unpipelined else 0):
        (y, y2, amax), _ = _pln_call(H, dev, d, full, want_amax=True)
    assert y2 is None and tuple(amax.shape) == (n, H.lib().ps_proj_layernorm_amax_parts(t)) == (n, 4 * ((t + 127) // 128))
    _check("proj_layernorm_amax", y, d["y_ref"], t, note=f"unpipelined={unpipelined}")
    # exact, as the fp16x2 GEMM's and the depthwise convolution's maxima: too small a range overflows fp16 or costs bits
    assert torch.equal(amax.amax(1), y[..., :t].abs().amax((1, 2)))


@pytest.mark.parametrize("why", ["short_rows", "norm2", "x_copy"])
def test_proj_layernorm_amax_refusal(H, dev, why):
    """off the row kernel's shapes the maxima do not exist: PS_E_UNSUPPORTED, and the next plain call is unaffected"""
    n, k, m = 3, 64, 128
    t = 127 if why == "short_rows" else 300
    case = (n, k, m, t, True, True, False, why == "norm2", why == "x_copy")
    d = SR.build_pln(case)
    with pytest.raises(RuntimeError, match=rf"rc={PS_E_UNSUPPORTED}\).*row kernel only"):
        _pln_call(H, dev, d, case, want_amax=True)
    (y, y2), cp = _pln_call(H, dev, d, case)
    _check("proj_layernorm", y, d["y_ref"], t, note=f"after the refusal ({why})")
    if y2 is not None:
        _check("proj_layernorm", y2, d["y2_ref"], t, note=f"after the refusal ({why}) y2")
    if cp is not None:
        assert torch.equal(cp[..., :t].cpu(), d["x"])
