"""What the Conv-TasNet masker driver (csrc/abi.hip behind ps_conv_tasnet_f32 / _ranged_f32 / _bf16_rows) calls, and what it
refuses -- without a GPU and without the project's library.

abi.hip holds no kernel.  It is compiled here with the Makefile's compiler and flags and linked against
tests/masker_probe_stubs.cpp: stand-ins for the launching entries that write one line per call into a ledger, pointers
printed as symbols (x_in, x_out, workspace+OFFSET, blocks[i].FIELD, dvec, x_amax, stream, null), and for the five pure
answers the driver asks for, which a row may set.  Pointers are aligned host memory that nothing dereferences.

Calls: every row of CALLS runs through the entries it names; the ledger must equal masker_driver_calls.txt line by line.
That file was recorded from commit 3331204 (`python tests/test_masker_driver_calls.py --record`, same build).

Refusals: every row of REFUSALS expects the return code and ps_last_error() text that commit 3331204 gives, and an EMPTY
ledger: a refused call launches nothing.  Commit 3331204 found a defect only once the launches in front of it had been
enqueued; PARENT_CALLS holds, for each row where that happened, how many calls its ledger held at the refusal.  Those rows
are the one behaviour change of the refactor that gave the driver a check pass; every row not named there refused before any
launch in 3331204 too.  They are twenty-three: the last-block row of every per-block defect that check_call's second loop
holds (8 calls for two whole blocks, 9 to 11 where ps_absmax_f32, ps_embed_bias_f32 or in_conv and the depthwise kernel of
the defective block ran too), the block-0 rows of the fp16x2 defects and of a plane count behind an embedding (1 to 3 calls:
the same launches of block 0), and two of the three rows with defects in two blocks.  A gemm_planes outside 0 .. 3 was
ps_conv1x1_bf16_io's to refuse, at the block's in_conv; the stand-in refuses it in the entry's words, so that the parent's
rows could be recorded, and check_call now says the same before any launch."""
import ctypes as C
import os
import subprocess
import sys
import time

import pytest

from puresound_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "puresound_amd", "csrc")
LEDGER = os.path.join(HERE, "masker_driver_calls.txt")
GLOBAL, AFFINE = _abi.PS_NORM_GLOBAL, _abi.PS_NORM_AFFINE
ENTRIES = {"f32": "ps_conv_tasnet_f32", "ranged": "ps_conv_tasnet_ranged_f32", "rows": "ps_conv_tasnet_bf16_rows"}
POINTER_FIELDS = [name for name, kind in _abi.TcnBlock._fields_ if kind is C.c_void_p]

_MEM = C.create_string_buffer((1 << 20) + 256)
BASE = (C.addressof(_MEM) + 255) // 256 * 256
WS, WS_BYTES = BASE, 1 << 18
X_IN, X_OUT, DVEC, X_AMAX, STREAM = (BASE + WS_BYTES + 4096 * k for k in range(5))
FIELDS = BASE + (1 << 19)   # block i's pointer field f points at FIELDS + 8192 * i + 256 * f


def build(out_dir, abi_source=None):
    """abi.hip + the stubs -> a shared object, with the Makefile's own compile line for abi.o"""
    line = subprocess.run(["make", "-n", "-B", "-C", CSRC, "abi.o"], capture_output=True, text=True, check=True).stdout
    compile_abi = [ln for ln in line.splitlines() if " -c abi.hip " in ln]
    assert len(compile_abi) == 1, line
    words = compile_abi[0].split()
    flags = words[1:words.index("-c")]
    obj, stubs, lib = (os.path.join(out_dir, n) for n in ("abi.o", "stubs.o", "masker_probe.so"))
    for src, dst, extra in ((abi_source or os.path.join(CSRC, "abi.hip"), obj, ["-I", CSRC]),
                            (os.path.join(HERE, "masker_probe_stubs.cpp"), stubs, ["-x", "c++"])):
        cmd = [words[0], *flags, "-I", os.path.join(ROOT, "include"), *extra, "-c", src, "-o", dst]
        done = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        assert done.returncode == 0, " ".join(cmd) + "\n" + done.stderr
    done = subprocess.run([words[0], "-shared", "-fPIC", "-o", lib, obj, stubs], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    handle = C.CDLL(lib)
    for name in (*ENTRIES.values(), "ps_last_error", "ps_conv_tasnet_workspace_bytes"):
        getattr(handle, name).restype, getattr(handle, name).argtypes = _abi.SIGNATURES[name]
    handle.probe_register.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t]
    handle.probe_ledger.restype = C.c_char_p
    return handle


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("masker_probe")))


def blk(**over):
    """a block in the fp32 arithmetic behind global norms, every pointer but in_embed_w and the *_wf images set"""
    b = dict(C=8, H=4, P=3, dilation=1, causal=0, in_norm=GLOBAL, dw_norm=GLOBAL, pw_norm=GLOBAL, E=0, gemm_planes=0,
             hidden_bf16=0, w_exp=(3, -2, 5), dw_gmax=1.5, dw_bmax=0.25, pw_gmax=2.5, pw_bmax=0.75, in_embed_w=None,
             in_wf=None, pw_wf=None, out_wf=None)
    b.update(over)
    return b


def stack(n, *per_block, **every):
    """n blocks of dilation 1, 2, 4 ...: `every` over all of them, then per_block[i] over block i"""
    return [blk(**{**dict(dilation=1 << i), **every, **(per_block[i] if i < len(per_block) else {})}) for i in range(n)]


BF16 = dict(gemm_planes=1, hidden_bf16=1)
F16X2 = dict(gemm_planes=2)
BN = dict(in_norm=AFFINE, dw_norm=AFFINE, pw_norm=AFFINE, causal=1)   # folded BatchNorms: what a causal block carries
WF = dict(in_wf=True, pw_wf=True, out_wf=True)
EMBED = dict(in_embed_w=True, E=6)

# name -> (entries, blocks, call arguments and answers that differ from the defaults of run())
CALLS = {
    "fp32_two_blocks": ("ranged f32", stack(2), {}),
    "embedding_as_it_is": ("ranged", stack(2, EMBED), dict(dvec=DVEC, embed_norm=0)),
    "embedding_normalised": ("ranged", stack(2, EMBED), dict(dvec=DVEC, embed_norm=1)),
    "planes_3": ("f32", stack(2, gemm_planes=3), {}),
    "planes_1_fp32_hidden_maps": ("f32", stack(2, gemm_planes=1), {}),
    "planes_1_bf16_hidden_maps": ("f32", stack(2, **BF16), {}),
    "fp16x2_global_measured_input": ("ranged f32", stack(3, **F16X2), {}),
    "fp16x2_global_given_input_range": ("ranged", stack(3, **F16X2), dict(x_amax=X_AMAX, x_amax_parts=5)),
    "fp16x2_global_zero_bounds": ("f32", stack(2, **F16X2, dw_gmax=0.0, dw_bmax=0.0, pw_gmax=0.0, pw_bmax=0.0), {}),
    "fp16x2_affine_measuring_depthwise": ("f32", stack(2, **F16X2, **BN), {}),
    "fp16x2_affine_measuring_depthwise_zero_scale": ("f32", stack(2, **F16X2, **BN, dw_gmax=0.0, pw_gmax=0.0), {}),
    "fp16x2_affine_extra_pass": ("f32", stack(2, **F16X2, **BN), dict(absmax_parts=5, dwconv_amax_ok=0)),
    "fp16x2_affine_extra_pass_zero_scale": ("f32", stack(2, **F16X2, **BN, dw_gmax=0.0, pw_gmax=0.0, dw_bmax=0.0),
                                            dict(absmax_parts=5, dwconv_amax_ok=0)),
    "range_chain_restarts_twice": ("ranged", stack(4, {}, F16X2, {}, F16X2), dict(x_amax=X_AMAX, x_amax_parts=5)),
    "P_5_non_causal": ("f32", stack(2, P=5), {}),
    "P_3_causal": ("f32", stack(3, **BN), {}),
    "bf16_rows_small_launches": ("rows", stack(2, **BF16, **WF), {}),
    "bf16_rows_f16_kernel": ("rows", stack(3, **BF16, **WF), dict(f16_rows_ok=1)),
    "bf16_rows_f16_kernel_one_block_without_out_wf": ("rows", stack(3, {}, dict(out_wf=None), **BF16, **WF), dict(f16_rows_ok=1)),
    "bf16_rows_f16_kernel_one_block_without_in_wf": ("rows", stack(3, {}, dict(in_wf=None), **BF16, **WF), dict(f16_rows_ok=1)),
    "bf16_rows_f16_kernel_affine_pw_norm": ("rows", stack(3, {}, dict(pw_norm=AFFINE), **BF16, **WF), dict(f16_rows_ok=1)),
    "bf16_rows_f16_kernel_affine_dw_norm": ("rows", stack(3, {}, dict(dw_norm=AFFINE), **BF16, **WF), dict(f16_rows_ok=1)),
}

NULLS = "ps_conv_tasnet_f32: null pointer or non-positive size"
SIZES = "ps_conv_tasnet_f32: block %d has inconsistent sizes (C=%d H=%d P=%d dilation=%d)"
CAUSAL = "ps_conv_tasnet_f32: block %d: global norms conflict with causal=1"
NOT_BF16 = "ps_conv_tasnet_bf16_rows: block %d is not in the bf16 arithmetic (gemm_planes = 1, hidden_bf16)"
NO_DVEC = "ps_conv_tasnet_f32: block expects an embedding (E=6) but dvec is NULL"
NO_RANGE = ("ps_conv_tasnet_f32: gemm_planes=2 (fp16x2) needs a global norm (a bound on the normalised values) or a per-channel "
            "affine norm (the producer's measured maxima) in front of the pointwise and output convs, and the range of the "
            "block's input")
NO_PLANES = "ps_conv_tasnet_f32: gemm_planes=%d needs the plane-packed weights in_wb / pw_wb / out_wb"
NO_ROOM = "ps_conv_tasnet_f32: no room for the maxima of the depthwise output (T=100)"
INVALID, ALIGN, UNSUPPORTED = -1, -2, -3

# name -> (entry, blocks, call arguments, code, text): the defects of the call itself ...
REFUSALS = {
    "x_amax_without_parts": ("ranged", stack(2), dict(x_amax=X_AMAX, x_amax_parts=0), INVALID,
                             "ps_conv_tasnet_ranged_f32: x_amax needs x_amax_parts > 0"),
    "null_blocks": ("f32", None, {}, INVALID, NULLS),
    "no_blocks": ("f32", stack(2), dict(n_blocks=0), INVALID, NULLS),
    "null_x_in": ("f32", stack(2), dict(x_in=None), INVALID, NULLS),
    "null_x_out": ("rows", stack(2, **BF16), dict(x_out=None), INVALID, NULLS),
    "null_workspace": ("f32", stack(2), dict(workspace=None), INVALID, NULLS),
    "N_zero": ("f32", stack(2), dict(N=0), INVALID, NULLS),
    "T_zero": ("ranged", stack(2), dict(T=0), INVALID, NULLS),
    "x_in_is_x_out": ("f32", stack(2), dict(x_in=X_OUT), INVALID,
                      "ps_conv_tasnet_f32: x_in must not alias x_out (the input is never modified)"),
    "ldt_even_tiles": ("f32", stack(2), dict(ldt=256), ALIGN, "ps_conv_tasnet_f32: ldt=256 must be ps_padded_frames(T=100)=128"),
    "workspace_one_byte_short": ("f32", stack(2), dict(workspace_bytes=-1), INVALID, None),   # (text: below, from the sizer)
    "workspace_misaligned": ("f32", stack(2), dict(workspace=WS + 128), ALIGN,
                             "ps_conv_tasnet_f32: workspace must be 256-byte aligned"),
}


def _per_block(name, entry, every, defect, call, code, text):
    """... and the defects of one block: once in block 0, once in the last of three blocks"""
    for i in (0, 2):
        REFUSALS[f"{name}_block_{i}"] = (entry, stack(3, *[{}] * i, defect, **every), call, code,
                                         text(i) if callable(text) else text % i if "block %d" in text else text)


_per_block("P_zero", "f32", {}, dict(P=0), {}, INVALID, lambda i: SIZES % (i, 8, 4, 0, 1 << i))
REFUSALS["dilation_zero_block_0"] = ("f32", stack(3, dict(dilation=0)), {}, INVALID, SIZES % (0, 8, 4, 3, 0))
REFUSALS["C_differs_block_2"] = ("f32", stack(3, {}, {}, dict(C=16)), {}, INVALID, SIZES % (2, 16, 4, 3, 4))
REFUSALS["H_differs_block_2"] = ("rows", stack(3, {}, {}, dict(H=8), **BF16), {}, INVALID, SIZES % (2, 8, 8, 3, 4))
_per_block("causal_global_norm", "f32", BN, dict(pw_norm=GLOBAL), {}, INVALID, CAUSAL)
_per_block("rows_planes_3", "rows", BF16, dict(gemm_planes=3), {}, UNSUPPORTED, NOT_BF16)
_per_block("rows_planes_2", "rows", BF16, dict(gemm_planes=2), {}, UNSUPPORTED, NOT_BF16)
_per_block("rows_fp32_hidden_maps", "rows", BF16, dict(hidden_bf16=0), {}, UNSUPPORTED, NOT_BF16)
_per_block("embedding_without_dvec", "f32", {}, EMBED, {}, INVALID, NO_DVEC)
_per_block("embedding_without_dvec_rows", "rows", BF16, EMBED, {}, INVALID, NO_DVEC)
_per_block("fp16x2_no_dw_norm", "f32", F16X2, dict(dw_norm=0), {}, UNSUPPORTED, NO_RANGE)
_per_block("fp16x2_no_pw_norm", "ranged", F16X2, dict(pw_norm=0), dict(x_amax=X_AMAX, x_amax_parts=5), UNSUPPORTED, NO_RANGE)
_per_block("fp16x2_embedding_unranged_norm", "f32", F16X2, dict(pw_norm=0, **EMBED), dict(dvec=DVEC), UNSUPPORTED, NO_RANGE)
_per_block("planes_1_no_in_wb", "f32", dict(gemm_planes=1), dict(in_wb=None), {}, INVALID, NO_PLANES % 1)
_per_block("planes_2_no_pw_wb", "f32", F16X2, dict(pw_wb=None), {}, INVALID, NO_PLANES % 2)
_per_block("planes_3_no_out_wb", "f32", dict(gemm_planes=3), dict(out_wb=None), {}, INVALID, NO_PLANES % 3)
_per_block("rows_no_in_wb", "rows", BF16, dict(in_wb=None), {}, INVALID, NO_PLANES % 1)
NO_SUCH_PLANES = "ps_conv1x1_bf16_f32: planes must be 1 (bf16 products) or 3 (fp32-accurate 3-way split), got %d"
_per_block("planes_4", "f32", {}, dict(gemm_planes=4), {}, INVALID, NO_SUCH_PLANES % 4)
_per_block("planes_minus_1_embedding", "f32", {}, dict(gemm_planes=-1, **EMBED), dict(dvec=DVEC), INVALID, NO_SUCH_PLANES % -1)
_per_block("no_room_for_depthwise_maxima", "f32", dict(**F16X2, **BN), dict(P=5), {}, UNSUPPORTED, NO_ROOM)
REFUSALS["no_room_for_depthwise_maxima_answered"] = ("f32", stack(3, **F16X2, **BN), dict(dwconv_amax_ok=0), UNSUPPORTED, NO_ROOM)
# defects in two blocks at once: the lower block's is reported
REFUSALS["block_1_no_pw_wb_block_2_no_dvec"] = ("f32", stack(3, {}, dict(pw_wb=None), EMBED, gemm_planes=3), {}, INVALID,
                                                NO_PLANES % 3)
REFUSALS["block_0_no_dvec_block_1_unranged"] = ("f32", stack(3, EMBED, dict(dw_norm=0), **F16X2), {}, INVALID, NO_DVEC)
REFUSALS["rows_block_1_planes_2_block_0_no_in_wb"] = ("rows", stack(3, dict(in_wb=None), dict(gemm_planes=2), **BF16), {},
                                                      INVALID, NO_PLANES % 1)

# calls in commit 3331204's ledger when it refused (rows not named: none)
PARENT_CALLS = {
    "rows_planes_3_block_2": 8, "rows_planes_2_block_2": 8, "rows_fp32_hidden_maps_block_2": 8,
    "embedding_without_dvec_block_2": 8, "embedding_without_dvec_rows_block_2": 8,
    "fp16x2_no_dw_norm_block_0": 1, "fp16x2_no_dw_norm_block_2": 9, "fp16x2_no_pw_norm_block_2": 8,
    "fp16x2_embedding_unranged_norm_block_0": 2, "fp16x2_embedding_unranged_norm_block_2": 10,
    "planes_1_no_in_wb_block_2": 8, "planes_2_no_pw_wb_block_0": 1, "planes_2_no_pw_wb_block_2": 9,
    "planes_3_no_out_wb_block_2": 8, "rows_no_in_wb_block_2": 8,
    "no_room_for_depthwise_maxima_block_0": 3, "no_room_for_depthwise_maxima_block_2": 11,
    "no_room_for_depthwise_maxima_answered": 3,
    "block_1_no_pw_wb_block_2_no_dvec": 4, "block_0_no_dvec_block_1_unranged": 1,
    "planes_4_block_2": 8, "planes_minus_1_embedding_block_0": 1, "planes_minus_1_embedding_block_2": 9,
}


def fill(probe, blocks):
    """the ps_tcn_block array of a stack; every pointer field gets an address of its own, registered under its name"""
    arr = (_abi.TcnBlock * len(blocks))()
    for i, b in enumerate(blocks):
        for f, name in enumerate(POINTER_FIELDS):
            at = FIELDS + 8192 * i + 256 * f
            probe.probe_register(f"blocks[{i}].{name}".encode(), at, 1)
            if b.get(name, True):
                setattr(arr[i], name, at)
        for k, v in b.items():
            if k == "w_exp":
                arr[i].w_exp[:] = [e + i for e in v]
            elif k not in POINTER_FIELDS:
                setattr(arr[i], k, v)
    return arr


def run(probe, entry, blocks, call):
    """-> (return code, ps_last_error(), ledger lines)"""
    call = dict(call)
    probe.probe_answers(call.pop("absmax_parts", 64), call.pop("dwconv_amax_ok", -1), call.pop("f16_rows_ok", 0))
    probe.probe_forget()
    probe.probe_clear()
    arr = fill(probe, blocks) if blocks is not None else None
    a = dict(blocks=arr, n_blocks=len(blocks or ()), x_in=X_IN, x_out=X_OUT, dvec=None, embed_norm=0, N=2, T=100, ldt=128,
             workspace=WS, workspace_bytes=WS_BYTES, x_amax=None, x_amax_parts=0, stream=STREAM)
    a.update(call)
    if a["workspace_bytes"] < 0:
        a["workspace_bytes"] += probe.ps_conv_tasnet_workspace_bytes(a["N"], 8, 4, a["T"])
    for name in ("x_in", "x_out", "dvec", "x_amax", "stream"):
        probe.probe_register(name.encode(), globals()[name.upper()], 1)
    probe.probe_register(b"workspace", WS, WS_BYTES)
    order = "blocks n_blocks x_in x_out dvec embed_norm N T ldt workspace workspace_bytes"
    order += " x_amax x_amax_parts stream" if entry == "ranged" else " stream"
    rc = getattr(probe, ENTRIES[entry])(*[a[k] for k in order.split()])
    return rc, probe.ps_last_error().decode(), probe.probe_ledger().decode().splitlines()


def read_ledger():
    want, key = {}, None
    with open(LEDGER) as f:
        for line in f.read().splitlines():
            if line.startswith("== "):
                key = line[3:]
                want[key] = []
            elif line:
                want[key].append(line)
    return want


@pytest.mark.parametrize("name", list(CALLS))
def test_calls(probe, name):
    entries, blocks, call = CALLS[name]
    want = read_ledger()
    for entry in entries.split():
        rc, err, lines = run(probe, entry, blocks, call)
        assert rc == 0, err
        assert all("?" not in ln for ln in lines), "a pointer no symbol covers:\n" + "\n".join(lines)
        expected = want[f"{name} {entry}"]
        for k, (got, exp) in enumerate(zip(lines, expected)):
            assert got == exp, f"call {k}"
        assert len(lines) == len(expected)


def test_plain_entry_is_the_ranged_entry_without_a_range():
    want = read_ledger()
    for name in ("fp32_two_blocks", "fp16x2_global_measured_input"):
        assert want[f"{name} f32"] == want[f"{name} ranged"] and want[f"{name} f32"]


def test_parts_laws_of_the_stubs_tell_C_from_H_and_each_other(probe):
    g, d = probe.ps_conv1x1_stats_parts, probe.ps_dwconv_stats_parts
    assert len({g(8, 100), g(4, 100), d(8, 100), d(4, 100)}) == 4


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(probe, name):
    entry, blocks, call, code, text = REFUSALS[name]
    if text is None:
        need = probe.ps_conv_tasnet_workspace_bytes(2, 8, 4, 100)
        text = f"ps_conv_tasnet_f32: workspace too small ({need - 1} < {need})"
    rc, err, lines = run(probe, entry, blocks, call)
    assert (rc, err) == (code, text)
    assert lines == [], "a refused call launches nothing"


def test_parent_calls_name_refusal_rows():
    assert set(PARENT_CALLS) <= set(REFUSALS) and len(PARENT_CALLS) == 23 and all(n > 0 for n in PARENT_CALLS.values())


def time_driver(probe, calls=10000):
    """seconds per call of a 24-block fp16x2 stack with the stubs returning at once"""
    blocks = stack(24, **F16X2)
    for b in blocks:
        b["dilation"] = 1 + b["dilation"] % 7
    probe.probe_recording(0)
    try:
        arr = fill(probe, blocks)
        fn = probe.ps_conv_tasnet_f32
        args = (arr, 24, X_IN, X_OUT, None, 0, 2, 100, 128, WS, WS_BYTES, STREAM)
        assert fn(*args) == 0, probe.ps_last_error()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn(*args)
        return (time.perf_counter() - t0) / calls
    finally:
        probe.probe_recording(1)


if __name__ == "__main__":   # --record [abi.hip]: the ledger and the refusals of that source; --time [abi.hip]: time_driver
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp, sys.argv[2] if len(sys.argv) > 2 else None)
        if sys.argv[1] == "--time":
            print(f"{time_driver(lib) * 1e6:.2f} us per call")
        else:
            with open(LEDGER, "w") as out:
                for case, (names, blks, kw) in CALLS.items():
                    for e in names.split():
                        code, msg, rows = run(lib, e, blks, kw)
                        assert code == 0, (case, msg)
                        out.write(f"== {case} {e}\n" + "\n".join(rows) + "\n\n")
            for case, (e, blks, kw, code, text) in REFUSALS.items():
                got = run(lib, e, blks, kw)
                print(f"{case!r}: {len(got[2])},   # {got[0]} {got[1]}" + ("" if (got[0], got[1]) == (code, text) else "   <-- DIFFERS"))
