"""The ledger of direct kernel tests: every entry of include/puresound_hip.h that launches a kernel is called by a GPU test
through its wrapper, not only from inside a model at the one shape of that model's golden vector.

How a symbol counts as hit:
  1. `lib().ps_xxx` inside a `def` of puresound_amd/hip.py names the wrapper(s) of ps_xxx (ast);
  2. a wrapper is hit when a test file carrying the `gpu` mark calls it as `H.<name>(` or `hip.<name>(`; a wrapper that another
     hit wrapper of hip.py calls by name is hit too (free_decode_moments -> wave_moments);
  3. VIA lists the entries no Python code calls because another entry reaches them inside the library: the test checks in
     csrc/ that the one calls the other, and that the other is hit;
  4. MODEL_PATH lists the entries whose wrapper only the models call (ps_conv_tasnet*: the models' torch.ops route ends in
     nnet/conv_tasnet.py -> hip.conv_tasnet); the test checks that call site and that a gpu-marked test file runs the named
     golden case through the model;
  5. EXEMPT may hold only entries that launch nothing; the test checks that their definitions hold no kernel launch."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXEMPT = {
    "ps_abi_version": "returns a constant",
    "ps_last_error": "returns the thread's message",
    "ps_profile_enable": "host-side switch of the launch timers",
    "ps_profile_read": "reads the launch timers",
    "ps_debug_flags": "host-side switch", "ps_debug_grid_cap": "host-side switch", "ps_debug_ablate": "host-side switch",
    "ps_debug_buffer": "host-side pointer",
    "ps_stats_parts": "size query", "ps_conv1x1_stats_parts": "size query", "ps_dwconv_stats_parts": "size query",
    "ps_conv2d_stats_parts": "size query", "ps_row_stats_parts": "size query", "ps_absmax_parts": "size query",
    "ps_proj_layernorm_amax_parts": "size query", "ps_free_decode_moments_parts": "size query",
    "ps_padded_frames": "size query", "ps_wave_moments_chunks": "size query",
    "ps_free_decode_workspace_bytes": "size query", "ps_free_decode_step_workspace_bytes": "size query",
    "ps_conv_tasnet_workspace_bytes": "size query", "ps_lstm_fmajor_coop_workspace_bytes": "size query",
    "ps_conv1x1_bf16_weight_bytes": "size query",
    "ps_conv1x1_f16_rows_ok": "shape predicate", "ps_conv1x1_f16x2_fmajor_ok": "shape predicate",
    "ps_conv1x1_f16x2_ln_ok": "shape predicate", "ps_dwconv_amax_ok": "shape predicate",
    "ps_lstm_fmajor_ok": "shape predicate", "ps_lstm_fmajor_h256_ok": "shape predicate",
}
EXEMPT_NAME = re.compile(r"^ps_(abi_version|last_error|profile_\w+|debug_\w+|\w+_parts|\w+_ok|\w+_workspace_bytes|\w+_weight_bytes|"
                         r"padded_frames|wave_moments_chunks)$")

VIA = {  # symbol: the entry on the other end of a call inside the library
    "ps_attn_stats_pool_f32": "ps_attn_stats_pool_len_f32",   # forwards with lengths = NULL
    "ps_conv1x1_bf16_f32": "ps_conv1x1_bf16_io",              # forwards with fp32 rows
    "ps_dwconv_f32": "ps_dwconv_io",                          # forwards with fp32 rows
    "ps_conv_tasnet_f32": "ps_conv_tasnet_ranged_f32",        # forwards without a range
    "ps_free_decode_f32": "ps_free_decode_ws_f32",            # the VALU kernels ps_free_decode_ws_f32 falls back to
    "ps_conv1x1_f16_rows": "ps_conv_tasnet_bf16_rows",        # the bf16-rows masker's GEMM on large launches
}

MODEL_PATH = {  # symbol: (call site of its wrapper in the package, gpu-marked test file, text that runs it there)
    "ps_conv_tasnet_ranged_f32": ("puresound_amd/nnet/conv_tasnet.py", "tests/test_hip_parity.py", "test_wrapper_inference_matches_reference_golden"),
    "ps_conv_tasnet_bf16_rows": ("puresound_amd/nnet/conv_tasnet.py", "tests/test_round4_gpu.py", "test_config3_with_the_residual_stream_in_bf16"),
}


def _read(rel):
    with open(os.path.join(ROOT, rel)) as f:
        return f.read()


def _entries():
    hdr = re.sub(r"/\*.*?\*/", "", _read("include/puresound_hip.h"), flags=re.S)
    return sorted(set(re.findall(r"^(?:int|size_t|const char\*)\s+(ps_\w+)\s*\(", hdr, flags=re.M)))


def _definitions():
    """symbol -> (file, body text) of its extern "C" definition in csrc/"""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "puresound_amd", "csrc", "*"))):
        if not path.endswith((".hip", ".inc", ".h")):
            continue
        src = open(path).read()
        for m in re.finditer(r'extern "C"\s+[\w\s\*]+?\b(ps_\w+)\s*\(', src):
            i = src.index("{", src.index(")", m.end()))
            while src[m.end():i].count("(") + 1 != src[m.end():i].count(")"):   # (a parenthesis inside the argument list)
                i = src.index("{", i + 1)
            depth, j = 0, i
            while True:
                depth += {"{": 1, "}": -1}.get(src[j], 0)
                j += 1
                if depth == 0:
                    break
            out[m.group(1)] = (path, src[i:j])
    return out


def _wrappers():
    """(symbol -> wrappers of hip.py calling it, wrapper -> wrappers of hip.py it calls by name)"""
    tree = ast.parse(_read("puresound_amd/hip.py"))
    defs = {f.name: f for f in tree.body if isinstance(f, ast.FunctionDef)}
    sym, calls = {}, {}
    for name, fn in defs.items():
        for node in ast.walk(fn):
            if isinstance(node, ast.Attribute) and node.attr.startswith("ps_") and isinstance(node.value, ast.Call) \
                    and getattr(node.value.func, "id", "") == "lib":
                sym.setdefault(node.attr, set()).add(name)
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in defs:
                calls.setdefault(name, set()).add(node.func.id)
    return sym, calls


def _gpu_test_files():
    # (the mark as a statement or decorator at the start of a line: this file only speaks of it)
    return [p for p in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py")))
            if re.search(r"^(?:pytestmark\s*=\s*|@)pytest\.mark\.gpu\b", open(p).read(), flags=re.M)]


def _hit_wrappers(calls):
    hit = set()
    for p in _gpu_test_files():
        hit |= set(re.findall(r"\b(?:H|hip)\.(\w+)\(", open(p).read()))
    grew = True
    while grew:
        more = set().union(*[calls.get(w, set()) for w in hit]) - hit
        grew = bool(more)
        hit |= more
    return hit


def test_every_launching_entry_has_a_direct_gpu_test():
    sym, calls = _wrappers()
    hit = _hit_wrappers(calls)
    hit_syms = {s for s, ws in sym.items() if ws & hit}
    for s, (site, test_file, needle) in MODEL_PATH.items():
        assert sym.get(s) and any(f"hip.{w}(" in _read(site) for w in sym[s]), f"{site} no longer calls the wrapper of {s}"
        assert "pytest.mark.gpu" in _read(test_file) and needle in _read(test_file), f"{test_file} no longer runs {needle}"
        hit_syms.add(s)
    defs = _definitions()
    for s, other in VIA.items():
        assert other in hit_syms, f"{s} is reached through {other}, which no gpu-marked test calls"
        assert (other + "(") in defs[s][1] or (s + "(") in open(defs[other][0]).read().replace(defs[s][1], ""), \
            f"csrc/ no longer connects {s} and {other}"
        hit_syms.add(s)
    missing = [s for s in _entries() if s not in hit_syms and s not in EXEMPT]
    table = "\n".join(f"  {s}  (wrapper: {', '.join(sorted(sym.get(s, []))) or 'none in hip.py'})" for s in missing)
    assert not missing, "entries of include/puresound_hip.h that no gpu-marked test calls through a wrapper:\n" + table


def test_exempt_entries_launch_nothing():
    defs = _definitions()
    entries = set(_entries())
    for s in EXEMPT:
        assert s in entries, f"{s} is not in the header any more: drop it from EXEMPT"
        assert EXEMPT_NAME.match(s), f"{s} is not the kind of entry that may be exempt"
        assert s in defs, f"no definition of {s} in csrc/"
        assert "hipLaunchKernelGGL" not in defs[s][1] and "<<<" not in defs[s][1], f"{s} launches a kernel: it needs a test"
    assert set(defs) >= entries, sorted(entries - set(defs))


# ---- the debug switches: each PS_DBG_* makes a dispatcher take the kernel it names, so that tests can run both -----------------
def _debug_switches():
    hdr = re.sub(r"/\*.*?\*/", "", _read("include/puresound_hip.h"), flags=re.S)
    return sorted(set(re.findall(r"\b(PS_DBG_[A-Z0-9_]+)\s*=\s*1\s*<<", hdr)))


def _unnamed_switches(test_texts):
    return [s for s in _debug_switches() if not any(re.search(rf"\b{s}\b", text) for text in test_texts)]


def test_every_debug_switch_is_read_by_a_kernel_launcher_and_named_by_a_gpu_test():
    """A switch no dispatcher reads is dead; a switch no gpu-marked test names leaves the kernel it selects (or the default it
    switches off) without a comparison.  PS_DBG_COOP_SABOTAGE counts through the bounded-poll test that names it."""
    switches = _debug_switches()
    assert len(switches) >= 22 and "PS_DBG_CONV1X1_TILED" in switches and "PS_DBG_GEMM_NO_PAIR" in switches
    csrc = "".join(open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "puresound_amd", "csrc", "*")))
                   if p.endswith((".hip", ".inc", ".h")))
    unread = [s for s in switches if not re.search(rf"\b{s}\b", csrc)]
    assert not unread, f"declared in include/puresound_hip.h, read nowhere in csrc/: {unread}"
    abi_py = _read("puresound_amd/_abi.py")
    assert not [s for s in switches if not re.search(rf"^{s} = ", abi_py, flags=re.M)], "puresound_amd/_abi.py lacks a switch"
    unnamed = _unnamed_switches([open(p).read() for p in _gpu_test_files()])
    assert not unnamed, f"debug switches that no gpu-marked test names: {unnamed}"
