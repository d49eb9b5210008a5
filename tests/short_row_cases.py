"""The cases of test_short_row_kernels_gpu.py and their inputs, on the CPU: the tables below pick, from the value lists of every
dispatch branch of csrc/conv1x1_small.hip, a few dozen combinations per kernel (not the full products); test_abi_references.py
checks here, without a GPU, that every listed value and every named combination is present and that the LayerNorm cases are
well conditioned.  Inputs are uniform random (Philox, fixed seeds), references come from abi_refs in float64."""
import abi_refs as R

# ---- ps_conv1x1_f32 on rows of <= 64 frames: conv1x1_small_kernel<NCB, TR> -------------------------------------------------
CONV_T = (1, 16, 17, 32, 33, 48, 49, 64)      # NCB = 1 | 2 | 4 boundaries, partially filled last column block
CONV_K = (3, 16, 33, 132, 272)                # K % 4 != 0, K % 16 != 0; one / two / three trips of the UN = 8 batch loop
CONV_M = (1, 15, 16, 17, 70, 256, 260)        # ragged 16-row workgroups, the second 256-row weight panel
CONV_N = (1, 3)
PROLOGUES = {  # name: (pre_relu, affine, prelu, post_tanh)
    "none": (False, False, False, False), "affine_prelu": (False, True, True, False), "prelu": (False, False, True, False),
    "pre_relu": (True, False, False, False), "post_tanh": (False, False, False, True), "all": (True, True, True, True)}


def _conv_cases():
    pros = list(PROLOGUES)
    out = []
    for i in range(48):
        terms = (5 * i + i // 8) % 8  # bit 0 bias, bit 1 bias_n, bit 2 res
        out.append((CONV_N[(i // 3) % 2], CONV_K[i % 5], CONV_M[i % 7], CONV_T[i % 8], bool(terms & 1), bool(terms & 2),
                    bool(terms & 4), pros[(i + i // 6) % 6]))
    out += [  # named: the second weight panel at every NCB with and without a prologue, three K trips, every term at once
        (3, 272, 260, 64, True, True, True, "all"), (1, 132, 260, 17, False, False, False, "none"),
        (1, 272, 260, 16, True, False, True, "affine_prelu"), (3, 33, 260, 1, False, True, False, "post_tanh"),
        (3, 3, 1, 1, False, False, False, "none"), (1, 33, 70, 1, True, True, False, "none"),
        (3, 272, 17, 32, False, True, True, "pre_relu"), (1, 16, 256, 33, True, False, False, "prelu"),
        (3, 132, 256, 32, True, True, True, "all"), (1, 272, 15, 49, False, False, True, "none"),
        (3, 16, 260, 16, True, True, True, "none"), (1, 33, 260, 48, False, True, False, "none")]
    return out


CONV_CASES = _conv_cases()


def conv_ncb(t):
    return 1 if t <= 16 else 2 if t <= 32 else 4


def build_conv1x1(case, glob=False):
    n, k, m, t, has_bias, has_bias_n, has_res, pname = case
    pre_relu, affine, prelu, post_tanh = PROLOGUES[pname]
    d = dict(x=R.rand((n, k, t), 601) + 0.1, w=R.rand((m, k), 602, -0.3, 0.3),
             bias=R.rand((m,), 603) if has_bias else None, bias_n=R.rand((n, m), 604) if has_bias_n else None,
             res=R.rand((n, m, t), 605) if has_res else None,
             gamma=R.rand((k,), 606, 0.5, 1.5), beta=R.rand((k,), 607, -0.3, 0.3), slope=R.rand((1,), 608, 0.1, 0.4))
    pro = dict(pre_relu=pre_relu, post_tanh=post_tanh)
    if glob:
        pro["glob"] = (d["gamma"], d["beta"], 1e-8)
    elif affine:
        pro["affine"] = (d["gamma"], d["beta"])
    if prelu:
        pro["prelu"] = float(d["slope"][0])
    d["ref"] = R.conv1x1_ref(d["x"], d["w"], d["bias"], d["bias_n"], d["res"], pro)
    return d


# ---- ps_film_conv_f32 / ps_lstm_gates_cell_f32: conv1x1_small_fused_kernel<NCB, EPI> ---------------------------------------
FUSED_T = (1, 16, 17, 32, 33, 64, 65, 128, 130, 257)   # T > 64: blockIdx.z > 0, a last z-block that is mostly past T
FUSED_N = (1, 3)
FILM_C = (2, 6, 12, 34, 128, 130)                      # C = 130: M = 260, the second weight panel
FILM_CASES = [(FUSED_N[(i // 2) % 2], FILM_C[i % 6], FUSED_T[(i + i // 10) % 10], bool((i // 3) % 2)) for i in range(40)] + [
    (3, 130, 257, True), (3, 2, 1, True), (3, 128, 65, True), (1, 130, 130, False), (3, 34, 128, False), (3, 12, 64, True)]

GATES_KH = [(k, h) for k in (5, 20, 132) for h in (1, 3, 8, 64, 65) if h < k]   # K = in + hid; H = 65: M = 260
# (n, k, hid, t, state_frames, bias): state_frames > 0 gives the state rows their own, longer leading dimension; bias False =
# bias_units NULL
GATES_CASES = [(FUSED_N[(i // 5) % 2], *GATES_KH[i % 10], FUSED_T[(i + i // 10) % 10], 0, i % 4 != 3) for i in range(40)] + [
    (1, 132, 65, 257, 0, True), (1, 132, 65, 65, 0, False), (1, 132, 64, 130, 0, True), (1, 20, 8, 17, 300, True),
    (3, 132, 65, 33, 300, False)]


def build_film(case, seed=0):
    n, c, t, has_res = case
    d = dict(x=R.rand((n, c, t), 611 + seed), ws=R.rand((c, c), 612 + seed, -0.3, 0.3), wb=R.rand((c, c), 613 + seed, -0.3, 0.3),
             rs=R.rand((n, c, t), 614 + seed) if has_res else None, rb=R.rand((n, c, t), 615 + seed) if has_res else None)
    d["ref"] = R.film_conv_ref(d["x"], d["ws"], d["wb"], d["rs"], d["rb"])
    return d


def build_gates(case, seed=0):
    n, k, hid, t, _, has_bias = case
    d = dict(xh=R.rand((n, k, t), 621 + seed), w=R.rand((4 * hid, k), 622 + seed, -0.3, 0.3),
             bias=R.rand((4 * hid,), 623 + seed) if has_bias else None, c=R.rand((n, hid, t), 624 + seed))
    d["c_ref"], d["h_ref"] = R.gates_cell_ref(d["xh"], d["w"], d["bias"], d["c"])
    return d


# ---- ps_proj_layernorm_f32, the 16-frame kernel: proj_layernorm_kernel<8, 8> | <8> | <16> ---------------------------------
PLN_M = (1, 12, 127, 128, 129, 200, 256)
PLN_K = (8, 20, 132, 256)
PLN_T = (1, 15, 16, 17, 37, 64, 127)
PLN_N = (1, 3)


def _pln_cases():
    # (n, k, m, t, bias, res, res_inside, norm2, x_copy)
    out = []
    for i in range(42):
        f = (7 * i + 3) % 32
        out.append((PLN_N[(i // 3) % 2], PLN_K[i % 4], PLN_M[i % 7], PLN_T[(i + i // 7) % 7], bool(f & 1), bool(f & 2), bool(f & 4),
                    bool(f & 8), bool(f & 16)))
    out += [  # the workgroup-count switch N * ceil(T / 16) = 64 | 65 (<8, 8> | <8>: another summation tree); the second norm
              # keeps these long rows on the 16-frame kernel
        (4, 132, 128, 256, True, True, False, True, False), (5, 132, 128, 208, True, True, False, True, False),
        (4, 8, 12, 256, False, True, True, True, True), (5, 8, 12, 208, False, True, True, True, True),
        # no bias, no residual, res_inside with the second norm: combined
        (3, 20, 200, 37, False, False, False, True, False), (1, 256, 127, 17, False, True, True, True, True),
        (3, 132, 256, 64, True, True, True, True, True), (1, 8, 1, 1, False, False, False, False, False)]
    return out


PLN_CASES = _pln_cases()


def pln_kernel(n, m, t):
    """the instantiation ps_proj_layernorm_f32 picks once it is on the 16-frame kernel"""
    if m > 128:
        return "<16>"
    return "<8,8>" if n * ((t + 15) // 16) <= 64 else "<8>"


def build_pln(case, seed=0):
    n, k, m, t, has_bias, has_res, res_inside, has_norm2, _ = case
    d = dict(x=R.rand((n, k, t), 631 + seed), w=R.rand((m, k), 632 + seed, -0.3, 0.3),
             bias=R.rand((m,), 633 + seed) if has_bias else None, res=R.rand((n, m, t), 634 + seed) if has_res else None,
             gamma=R.rand((m,), 635 + seed, 0.5, 1.5), beta=R.rand((m,), 636 + seed),
             norm2=(R.rand((m,), 637 + seed, 0.5, 1.5), R.rand((m,), 638 + seed), 1e-5) if has_norm2 else None)
    d["y_ref"], d["y2_ref"], d["min_var"] = R.proj_layernorm_ref(d["x"], d["w"], d["bias"], d["gamma"], d["beta"], 1e-5, d["res"],
                                                                 res_inside, d["norm2"], with_var=True)
    return d


# ---- ps_proj_layernorm_amax_f32: the three row kernels (pipelined K = 64 / M = 128, rows<4>, rows<8>) ----------------------
AMAX_KM = ((64, 128), (20, 100), (96, 256))
AMAX_CASES = [(n, k, m, t, ri, False) for k, m in AMAX_KM for t in (128, 129, 300) for n in (1, 3) for ri in (False, True)] + [
    (3, 64, 128, 300, False, True), (1, 64, 128, 129, True, True)]   # (..., unpipelined): PS_DBG_PROJ_LN_UNPIPELINED


def build_amax(case):
    n, k, m, t, res_inside, _ = case
    return build_pln((n, k, m, t, True, True, res_inside, False, False), seed=40)


# ---- the _cells launches ----------------------------------------------------------------------------------------------------
CELLS_T = (4, 17, 64, 130)
CELLS_T_MANY = 1040   # ceil(T / 16) = 65 > 64: proj_layernorm_cells_kernel<8> instead of <8, 8> at M <= 128
CELLS_FILM_C = (12, 130)
CELLS_GATES_KH = ((20, 8), (132, 65))
CELLS_PLN_KM = ((8, 12), (20, 200), (256, 128))
