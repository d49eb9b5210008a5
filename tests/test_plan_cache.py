"""The one cache of packed weights and kept scratch (nnet/_plans.py: PlanCache), on the CPU: plans build on torch.device("cpu").

Per user of the cache -- TCN, GatedTCN, ConvTasNet(normal), AttentiveStatisticsPooling, ConvSTFT (both plans),
ConvMelSpectrogram, FreeEncDec's bound, SegLSTM, Unet -- a second call returns the same plan object; an in-place edit of one of
its tensors, load_state_dict, a train() / eval() flip and a change of its own switch each give another object; an edit to a
sibling module's parameter gives the same one.  Then: the wrappers of the ledger presets (test_plan_cache_calls_gpu.py) are
deep-copied and pickled WITH plans built and a tensor in kept scratch; `_prepare_plans` misses no module; and the fingerprint,
`__getstate__` and the precision table exist once under nnet/."""
import copy
import glob
import os
import pickle
import re

import pytest
import torch
import torch.nn as nn

import cases
import puresound_amd.nnet as PA
from detweights import det_state_dict
from puresound_amd.nnet import _plans
from puresound_amd.nnet.conv_tasnet import TCN, ConvTasNet, GatedTCN
from puresound_amd.nnet.lobe.encoder import ConvMelSpectrogram, ConvSTFT, FreeEncDec
from puresound_amd.nnet.lobe.pooling import AttentiveStatisticsPooling
from puresound_amd.nnet.skim import SegLSTM
from puresound_amd.nnet.unet import Unet

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESETS = ["tiny_free", "tiny_stft", "cfg3_short", "cfg4_tse_short", "tse_skim_fbank_short", "ns_dparn_short",
           "tse_unet_tcn_short"]


def _set(attr, value):
    return lambda m: setattr(m, attr, value)


def _bf16_rows_off(m):
    m.gemm_precision, m.stream_bf16 = "bf16", False    # (stream_bf16 only matters to a block in the bf16 arithmetic)


# name -> (constructor, plan getters, what changes the module's own switch or None, whether it builds in train() mode)
USERS = {
    "TCN": (lambda: TCN(16, 8, 3, 2), [lambda m: m.plan(CPU)], _set("gemm_precision", "fp32"), True),
    "TCN_stream_bf16": (lambda: TCN(16, 8, 3, 2), [lambda m: m.plan(CPU)], _bf16_rows_off, True),
    "GatedTCN": (lambda: GatedTCN(16, 8, 3, 2), [lambda m: m.plan(CPU)], None, True),
    "ConvTasNet": (lambda: ConvTasNet(16, 0, False, tcn_dim=8, per_tcn_stack=2, repeat_tcn=2, tcn_with_embed=[0, 0]),
                   [lambda m: m.block_array(CPU)[0]], lambda m: m.set_gemm_precision("bf16x3"), True),
    "AttentiveStatisticsPooling": (lambda: AttentiveStatisticsPooling(16, 8), [lambda m: m._plan_get(CPU, m._build)],
                                   _set("gemm_precision", "fp32"), False),
    "ConvSTFT": (lambda: ConvSTFT(torch.hann_window(32), n_fft=32, hop_length=8, iSTFT=True, trainable=True),
                 [lambda m: m._analysis_plan(m.drop_first_bin), lambda m: m._synthesis_plan(m.drop_first_bin)],
                 _set("drop_first_bin", True), True),
    "ConvMelSpectrogram": (lambda: ConvMelSpectrogram(torch.hann_window(512), trainable=True, output_format="Magnitude", n_banks=8),
                           [lambda m: m._analysis_plan(False), lambda m: m._plan_get(CPU, m._build_mel)], None, True),
    "FreeEncDec": (lambda: FreeEncDec(16, 8, 8), [lambda m: m._plan_get(CPU, m._build)], None, True),
    "SegLSTM": (lambda: SegLSTM(8, 8), [lambda m: m._plan_get(CPU, m._build)], _set("gemm_precision", "fp32"), True),
    "Unet": (lambda: Unet(dropout=0.0), [lambda m: m._plan_get(CPU, m._build_unet)], _set("gemm_precision", "fp32"), False),
}


def _first_tensor(m):
    return next(iter(m.parameters()), None) if any(True for _ in m.parameters()) else next(m.buffers())


@pytest.mark.parametrize("name", sorted(USERS))
def test_a_plan_is_kept_until_something_it_depends_on_changes(name):
    make, getters, switch, trains = USERS[name]
    torch.manual_seed(0)
    root = nn.ModuleList([make().eval(), nn.Linear(3, 3)])
    m, sibling = root
    for get in getters:
        plan = get(m)
        assert get(m) is plan, "a second call returns the kept plan"
        with torch.no_grad():
            sibling.weight.mul_(2.0)
        assert get(m) is plan, "a sibling's parameter is not this module's business"

        def rebuilt(what):
            nonlocal plan
            new = get(m)
            assert new is not plan, what
            assert get(m) is new, what
            plan = new

        with torch.no_grad():
            _first_tensor(m).mul_(1.25)
        rebuilt("an in-place edit")
        m.load_state_dict(copy.deepcopy(m.state_dict()))
        rebuilt("load_state_dict")
        m.train()
        if trains:
            rebuilt("train()")
        else:
            with pytest.raises(RuntimeError, match="eval"):    # (refused while the plan is built, and no stale plan handed out)
                get(m)
        m.eval()
        if trains:
            rebuilt("eval()")
    if switch is not None:
        plans = [get(m) for get in getters]
        switch(m)
        assert all(get(m) is not p for get, p in zip(getters, plans)), "the module's own switch"


def test_the_masker_validates_each_block_once_per_pass(monkeypatch):
    """ConvTasNet.forward_padded reads the block array and the `fused` / `rows_bf16` flags from one _stack() call."""
    masker = cases.build(PA.NS, "cfg3_short").eval().masker
    blocks = [m for stack in masker.tcn_list for m in stack]
    walked = []
    real = _plans.param_signature
    monkeypatch.setattr(_plans, "param_signature", lambda module: walked.append(module) or real(module))
    for _ in range(2):    # cold, warm
        del walked[:]
        stack = masker._stack(CPU)
        assert len(walked) == len(blocks) == 24 and all(a is b for a, b in zip(walked, blocks))
        assert stack["fused"] and not stack["rows_bf16"] and len(stack["array"]) == 24
    assert masker.block_array(CPU) == (stack["array"], 24)


def test_only_modules_with_the_choice_carry_gemm_precision():
    """bench_configs.py, GraphedInference._signature and tests select modules with hasattr(m, "gemm_precision")."""
    for name in ("GatedTCN", "ConvSTFT", "ConvMelSpectrogram", "FreeEncDec", "ConvTasNet"):
        assert isinstance(USERS[name][0](), _plans.PlanCache) and not hasattr(USERS[name][0](), "gemm_precision"), name
    assert not hasattr(cases.build(PA.NS, "tiny_free"), "gemm_precision")
    for name in ("TCN", "AttentiveStatisticsPooling", "SegLSTM", "Unet"):
        assert USERS[name][0]().gemm_precision == "fp16x2", name


def test_set_gemm_precision_signatures():
    model = cases.build(PA.NS, "cfg3_short")
    for root in (model, model.masker, model.speaker_net[-2]):
        assert root.set_gemm_precision("fp32") is root
        with pytest.raises(ValueError, match=r"gemm precision must be one of \['bf16', 'bf16x3', 'fp16x2', 'fp32'\]"):
            root.set_gemm_precision("fp64")
    assert {m.gemm_precision for m in model.modules() if hasattr(m, "gemm_precision")} == {"fp32"}


@pytest.fixture(scope="module", params=PRESETS)
def prepared(request):
    """(preset, its wrapper with every plan built on the CPU and a tensor in kept scratch, the spied builds)"""
    model = cases.build(PA.NS, request.param).eval()
    model.load_state_dict(det_state_dict(model))
    built = []
    real = _plans.PlanCache._plan_build

    def spy(self, name, builder, device):
        built.append((self, name))
        return real(self, name, builder, device)

    _plans.PlanCache._plan_build = spy
    try:
        model._prepare_plans(CPU)
        first = list(built)
        model._prepare_plans(CPU)
        assert built == first, "a second _prepare_plans builds nothing"
    finally:
        _plans.PlanCache._plan_build = real
    for m in model.modules():
        if isinstance(m, _plans.PlanCache):
            m.keep_scratch("workspace", 1, torch.zeros(1 << 16))
    return request.param, model, first


def test_prepare_plans_misses_no_module(prepared):
    """Every plan that inference() reads is built by _prepare_plans, on the caller's stream, before the batch forks into lanes."""
    name, model, built = prepared
    want = {ConvSTFT: {"_build_analysis", "_build_synthesis"}, ConvMelSpectrogram: {"_build_analysis", "_build_mel"},
            ConvTasNet: {"_build_stack"}, type(model): set()}
    seen = set()
    for m in model.modules():
        if not isinstance(m, _plans.PlanCache):
            continue
        seen.add(type(m))
        names = {n for mod, n in built if mod is m}
        if isinstance(m, ConvTasNet) and m.tcn_layer.lower() != "normal":
            assert names == set()
        elif isinstance(m, Unet):
            assert names == {"_build_unet"}, type(m).__name__
        else:
            assert names == want.get(type(m), {"_build"}), type(m).__name__
        assert names == set(m._plans or {})
    assert FreeEncDec in seen or ConvSTFT in seen
    stft = [m for m in model.modules() if type(m) is ConvSTFT]
    assert all(m.drop_first_bin == bool(model.drop_first_bin) for m in stft), "the plans inference() will ask for"


def _holds_ctypes(obj, depth=0):
    import ctypes
    if isinstance(obj, (ctypes.Structure, ctypes.Array, ctypes._SimpleCData)):
        return True
    if isinstance(obj, dict):
        return any(_holds_ctypes(v, depth + 1) for v in obj.values())
    if isinstance(obj, (list, tuple)):
        return any(_holds_ctypes(v, depth + 1) for v in obj)
    return False


def test_deepcopy_and_pickle_drop_plans_and_scratch(prepared):
    name, model, _ = prepared
    fresh = cases.build(PA.NS, name).eval()
    fresh.load_state_dict(det_state_dict(fresh))
    limit = len(pickle.dumps(fresh)) * 1.01
    blob = pickle.dumps(model)
    assert len(blob) <= limit
    assert any(m._plans for m in model.modules() if isinstance(m, _plans.PlanCache)), "the original keeps its plans"
    for clone in (copy.deepcopy(model), pickle.loads(blob)):
        assert list(clone.state_dict()) == list(model.state_dict())
        for m in clone.modules():
            assert not any(_holds_ctypes(v) for k, v in m.__dict__.items() if k not in ("_parameters", "_buffers", "_modules"))
            if isinstance(m, _plans.PlanCache):
                assert m._plans is None and m._scratch is None and m.cached_tensors() == [] and m.kept_scratch() == []


def test_the_cache_lists_what_it_keeps(prepared):
    _, model, _ = prepared
    for m in model.modules():
        if isinstance(m, _plans.PlanCache):
            listed = {id(t) for t in m.cached_tensors()}
            assert id(m.scratch("workspace", 1)) in listed
            if isinstance(m, TCN):
                assert {id(t) for t in m.plan(CPU)["tensors"].values() if torch.is_tensor(t)} <= listed


def test_fingerprint_getstate_and_precision_table_exist_once():
    hits = {"._version": [], "def __getstate__": [], "planes table": []}
    for path in sorted(glob.glob(os.path.join(ROOT, "puresound_amd", "nnet", "**", "*.py"), recursive=True)):
        text = open(path).read()
        rel = os.path.relpath(path, os.path.join(ROOT, "puresound_amd", "nnet"))
        hits["._version"] += [rel] * text.count("._version")
        hits["def __getstate__"] += [rel] * text.count("def __getstate__")
        hits["planes table"] += [rel] * len(re.findall(r"^(?:GEMM_PLANES|_PLANES)\s*=", text, flags=re.M))
    assert hits == {"._version": ["_plans.py"], "def __getstate__": ["_plans.py"], "planes table": ["_plans.py"]}
