"""What `inference` hands to the C ABI around every event that invalidates a packed plan, against a ledger recorded from commit
24cedff, before the modules' packed weights and kept scratch got one cache (nnet/_plans.py: PlanCache).  Seven wrapper presets
of tests/golden/cases.py, which between them reach every user of the cache, at the B, L and L_enroll they have there, with the
deterministic weights, in eval(), hip_streams at its default.  Five inferences per preset: cold; warm; after an in-place
mul_(1.25) of the first weight with dim() > 1; after set_gemm_precision("fp32"); after switching back to "fp16x2".  Each
contributes its library calls with every argument (the recorder and the `c<i>` file format of test_streaming_calls_gpu.py) and
`sha256 out<i> <hex>` of its output.  A cache that misses an invalidation repeats a hash it must not, one that rebuilds a
plan differently or allocates other scratch differs in a line.

The file also holds the cache's own GPU checks: what it lists as kept alive is what a walk of every module's __dict__ finds,
and `_prepare_plans` leaves nothing for `inference` to build.

`python tests/test_plan_cache_calls_gpu.py --record [path]` writes plan_cache_calls.txt from the tree it runs in, each preset run
twice: a preset whose hashes differ between the two runs is named in the header and recorded without them."""
import hashlib
import os
import sys

import pytest
import torch

import conftest  # noqa: F401  (run as a script: it puts the repository and tests/golden on sys.path)
import cases
from detweights import det_state_dict, det_wave
from test_streaming_calls_gpu import Recorder, read_ledger, write_ledger

pytestmark = pytest.mark.gpu
LEDGER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_cache_calls.txt")
PRESETS = ["tiny_free", "tiny_stft", "cfg3_short", "cfg4_tse_short", "tse_skim_fbank_short", "ns_dparn_short",
           "tse_unet_tcn_short"]
HEADER = ("# recorded from commit 24cedff (the parent of the commit that gave every module one plan cache) by\n"
          "# `python tests/test_plan_cache_calls_gpu.py --record` on an MI355X, every preset twice.\n")


def _model(name, dev):
    import puresound_amd.nnet as PA
    model = cases.build(PA.NS, name).eval()
    model.load_state_dict(det_state_dict(model))
    return model.to(dev)


def _inputs(name, dev):
    c = cases.CASES[name]
    args = [det_wave(c["seed"], c["B"], c["L"]).to(dev)]
    if "L_enroll" in c:
        args.append(det_wave(c["seed"] + 1, c["B"], c["L_enroll"]).to(dev))
    return args


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def ledger_of(name, dev, patch):
    """The lines of one preset; `patch(value)` replaces puresound_amd.hip.lib."""
    from puresound_amd import _abi, hip
    model, args = _model(name, dev), _inputs(name, dev)
    rec = Recorder(hip.lib(), _abi.SIGNATURES)
    patch(lambda: rec)
    hashes = []

    def infer():
        with rec.recording():
            out = model.inference(*args)
        hashes.append(_sha(out))
        rec.lines.append(f"sha256 out{len(hashes)} {hashes[-1]}")

    infer()                                                                     # 1 cold
    infer()                                                                     # 2 warm
    with torch.no_grad():
        next(p for p in model.parameters() if p.dim() > 1).mul_(1.25)
    infer()                                                                     # 3 a parameter edited in place
    model.set_gemm_precision("fp32")
    infer()                                                                     # 4 exact fp32 products
    model.set_gemm_precision("fp16x2")
    infer()                                                                     # 5 the default again
    torch.cuda.synchronize(dev)
    return rec.lines, hashes


def _no_hashes(lines):
    return [ln for ln in lines if not ln.startswith("sha256 ")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def want():
    return read_ledger(LEDGER)


@pytest.mark.parametrize("name", PRESETS)
def test_calls_and_bits(dev, want, monkeypatch, name):
    from puresound_amd import hip
    lines, hashes = ledger_of(name, dev, lambda value: monkeypatch.setattr(hip, "lib", value))
    assert hashes[1] == hashes[0], "a warm call computes what the cold one did"
    assert hashes[2] != hashes[0], "an in-place edit of a weight reaches the packed plan"
    assert hashes[4] == hashes[2], "back at the default arithmetic, the default's result"
    expected = want[name]
    if not any(ln.startswith("sha256 ") for ln in expected):    # (named in the ledger's header: not bit-stable on the parent)
        lines = _no_hashes(lines)
    for k, (got, exp) in enumerate(zip(lines, expected)):
        assert got == exp, f"line {k}"
    assert len(lines) == len(expected) > 0


def _walked_tensors(model):
    """Every CUDA tensor a walk of every module's __dict__ finds outside parameters, buffers and submodules (the walk
    graphs._cached_tensors made before the cache could list what it keeps, twice as deep: that one stopped at six containers
    and so never reached the kept LSTM output rows of DPCRN / DPARN): the reference for PlanCache's own list."""
    seen, out = {id(t) for t in list(model.parameters()) + list(model.buffers())}, []    # (nn.LSTM._flat_weights lists them again)

    def walk(obj, depth):
        if torch.is_tensor(obj):
            if obj.is_cuda and id(obj) not in seen:
                seen.add(id(obj))
                out.append(obj)
        elif depth < 12:
            if isinstance(obj, dict):
                for v in obj.values():
                    walk(v, depth + 1)
            elif isinstance(obj, (list, tuple)):
                for v in obj:
                    walk(v, depth + 1)

    for m in model.modules():
        for k, v in m.__dict__.items():
            if k not in ("_parameters", "_buffers", "_modules"):
                walk(v, 0)
    return out


@pytest.mark.parametrize("name", PRESETS)
def test_the_cache_lists_every_tensor_a_module_keeps(dev, name):
    """A cache that a later change adds outside the mixin is found by the walk and not listed by the cache."""
    from puresound_amd import graphs, hip
    model = _model(name, dev)
    model.inference(*_inputs(name, dev))
    listed = sorted(t.data_ptr() for t in graphs._cached_tensors(model) if not any(t is e for e in hip._EYE.values()))
    walked = sorted(t.data_ptr() for t in _walked_tensors(model))
    assert listed == walked and len(walked) > 0


@pytest.mark.parametrize("name", ["tiny_free", "cfg3_short", "tse_skim_fbank_short"])
def test_prepare_plans_leaves_nothing_for_inference_to_build(dev, monkeypatch, name):
    from puresound_amd.nnet import _plans
    model, args = _model(name, dev), _inputs(name, dev)
    built = []
    real = _plans.PlanCache._plan_build

    def spy(self, name, builder, device):
        built.append((type(self).__name__, name))
        return real(self, name, builder, device)

    monkeypatch.setattr(_plans.PlanCache, "_plan_build", spy)
    model._prepare_plans(dev)
    assert built, "the spy sees the builds"
    del built[:]
    model.inference(*args)
    assert built == []


def record(path):
    from puresound_amd import hip
    device = torch.device("cuda:0")
    real = hip.lib
    recorded, unstable = {}, []
    for name in PRESETS:
        runs = []
        for _ in range(2):
            lines, hashes = ledger_of(name, device, lambda value: setattr(hip, "lib", value))
            hip.lib = real
            assert hashes[1] == hashes[0] and hashes[2] != hashes[0] and hashes[4] == hashes[2], (name, hashes)
            runs.append(lines)
        first, second = runs
        if first != second:
            assert _no_hashes(first) == _no_hashes(second), name
            unstable.append(name)
            first = _no_hashes(first)
        recorded[name] = first
        print(f"{name}: {len(first)} lines", flush=True)
    write_ledger(recorded, path)
    with open(path) as f:
        body = f.read()
    with open(path, "w") as f:
        f.write(HEADER + "".join(f"# no hashes: {name}: its output differed between two runs on that commit\n"
                                 for name in unstable) + body)


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"] and len(sys.argv) <= 3, __doc__
    record(sys.argv[2] if len(sys.argv) == 3 else LEDGER)
