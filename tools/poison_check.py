"""Uninitialised-memory check at the benchmark's batch (GPU box): the caching allocator is filled with NaN blocks of the sizes
a 32 x 4 s forward allocates (maps, partial-statistics slots, outputs), released, and the forward must return the bits of a
clean run.  NaN in the allocator reaches `torch.empty` memory only.  The scratch a model KEEPS from call to call -- the fused
masker driver's workspaces, which ConvTasNet and the wrapper keep per lane (nnet/_plans.py: PlanCache.keep_scratch) -- is
zero-filled when it is created, and the clean reference call creates it before anything is poisoned: so every kept workspace is overwritten
with 0xFF bytes (NaN as fp32 and as fp64) as well.  (The zeroed LSTM output rows of DPCRN / DPARN are left alone: their
pad frames are zero by contract, _plans._h_rows.)  tests/test_hip_parity.py::
test_results_do_not_depend_on_uninitialised_memory and tests/test_scratch_state_gpu.py do this at the fixtures' batch of 2,
where other kernel variants run.   python tools/poison_check.py [preset ...]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import cases  # noqa: E402
from detweights import det_state_dict  # noqa: E402
import puresound_amd.nnet as PA  # noqa: E402


def poison(dev):
    torch.cuda.empty_cache()
    junk = []
    for mb in (1, 2, 8, 32, 64, 128, 256, 300, 512, 600):
        for _ in range(4 if mb < 256 else 3):
            junk.append(torch.full((mb * 262144,), float("nan"), device=dev))
    for kb in (1, 4, 16, 64, 256):
        for _ in range(16):
            junk.append(torch.full((kb * 256,), float("nan"), device=dev))
    torch.cuda.synchronize()
    del junk


def kept_workspaces(model):
    """every fused-driver workspace the model holds on to (uint8 tensors)"""
    from puresound_amd.nnet._plans import PlanCache
    return [ws for m in model.modules() if isinstance(m, PlanCache) for ws in m.kept_scratch() if torch.is_tensor(ws)]


def main():
    dev = "cuda:0"
    g = torch.Generator().manual_seed(1234)
    noisy = ((torch.rand(32, 64000, generator=g) * 2 - 1) * 0.5).to(dev)
    enroll = ((torch.rand(32, 64000, generator=g) * 2 - 1) * 0.5).to(dev)
    bad = 0
    for name in sys.argv[1:] or ("cfg2_short", "cfg3_short", "cfg3_causal_short", "cfg4_short"):
        c = cases.CASES[name]
        model = cases.build(PA.NS, name).eval()
        model.load_state_dict(det_state_dict(model))
        model.to(dev)
        spk = bool(c.get("speaker_net") or c.get("spk") or getattr(model, "embedding_free_tse", False))
        args = (noisy, enroll) if spk else (noisy,)
        for prec in ("fp16x2", "fp32"):
            model.set_gemm_precision(prec)
            ref = model.inference(*args).clone()
            res = []
            for _ in range(3):
                poison(dev)
                dirtied = kept_workspaces(model)
                for ws in dirtied:
                    ws.fill_(0xFF)
                y = model.inference(*args)
                res.append((bool(torch.isfinite(y).all()), bool(torch.equal(y, ref))))
            ok = all(f and e for f, e in res)
            bad += not ok
            print(json.dumps({"preset": name, "arithmetic": prec, "kept_workspaces_dirtied": len(dirtied),
                              "finite_and_equal_after_poison": res, "ok": ok}), flush=True)
        del model
        torch.cuda.empty_cache()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
