"""One preset per kernel family at edge utterance lengths, through SoTaskWrapModule.inference, against the float64 oracle.

The kernel-level files sweep T over {1, 127, 128, 129, 1025} with arguments the tests build themselves, and every end-to-end
comparison runs a preset at one comfortable shape.  Between the two lies the code that turns an utterance's length into kernel
arguments -- segment padding (min_frames), padded_frames, the trim of the transposed convolutions, (T - 1) * hop + win, the
N/T-dependent dispatch of abi.hip, the Q / steps / strides of the attention and LSTM walks -- and these tests walk it:

(a) every preset over its frame ladder (edge_length_cases.FREE_T / STFT_T), B = 2, in "fp32" and "fp16x2";
(b) the enrolment of the four presets that take one at 1, 2, 128 and 129 frames;
(c) batches of 1, 3 and 17 (the recurrence kernels pack 16 sequences per workgroup across utterance boundaries), and an
    utterance inside the 17 against the same utterance on its own;
(d) one model object over the whole ladder, from both ends inwards, against freshly built models: the same bits;
(e) an utterance one sample short of a window is refused, and the object is as good as new afterwards.

Metrics and bounds are those of edge_length_cases.py: 2e-5 ("fp32") and 1e-4 ("fp16x2") on rel_max for the free-encoder
presets and on the window-weighted metric for the STFT presets, 1e-4 on the project's cut rel_max for the latter.  Measured
on the MI355X over all 132 tests (profiles/edge_lengths.txt has the table): the worst value under the 2e-5 / 1e-4 pair is
1.45e-6 ("fp32", weighted, ns_dparn_short at B = 17; "fp16x2": 1.18e-6, same case) and the worst of the project metric on an
STFT preset 5.71e-6 (cfg1_short, "fp32", T = 127); a row of the 17 equals its lone run bit for bit except in DPCRN / DPARN
under "fp16x2" and in SkiM (at most 7.1e-7 there).

With PS_EDGE_LENGTHS_TABLE=<path> in the environment the module writes the worst value per group, preset, arithmetic and
metric, with the case it occurred at, to that file when its last test has run."""
import os

import pytest
import torch

import cases
import edge_length_cases as E

pytestmark = pytest.mark.gpu

_MODELS = {}
_WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def PA():
    import puresound_amd.nnet as PA
    from puresound_amd import hip
    hip.lib()  # fail loudly if the extension is missing
    return PA


@pytest.fixture(autouse=True)
def _nan_in_the_allocator_cache(dev):
    """NaN-filled blocks in torch's caching allocator, as in test_hip_parity.py: scratch and pad frames that a length
    leaves unwritten hold NaN, not the zeros of a fresh process."""
    junk = [torch.full((1 << 22,), float("nan"), device=dev) for _ in range(16)]
    junk += [torch.full((n,), float("nan"), device=dev) for n in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20)]
    del junk
    yield


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    path = os.environ.get("PS_EDGE_LENGTHS_TABLE")
    if path:
        with open(path, "w") as f:
            f.write(f"{'group':<10} {'preset':<26} {'arith':<7} {'metric':<9} {'worst':>10}  at\n")
            for (group, name, prec, metric), (value, where) in sorted(_WORST.items()):
                f.write(f"{group:<10} {name:<26} {prec:<7} {metric:<9} {value:>10.3e}  {where}\n")
    _MODELS.clear()


def _fresh(PA, dev, name):
    model = cases.build(PA.NS, name).eval()
    model.load_state_dict(E.weights(name)[0])
    return model.to(dev)


def _model(PA, dev, name):
    if name not in _MODELS:
        _MODELS[name] = _fresh(PA, dev, name)
    return _MODELS[name]


def _run(model, dev, noisy, enroll):
    out = model.inference(noisy.to(dev), None if enroll is None else enroll.to(dev))
    torch.cuda.synchronize(dev)
    return out.cpu()


def _check(group, name, model, dev, noisy, enroll, ref, where):
    """Both arithmetics on one input: shape, finiteness and every metric of the preset against `ref` (the float64
    oracle's output, the clamp condition checked on it) -> {arithmetic: result}."""
    assert E.clamped_share(name, ref) <= E.CLAMP_CAP
    results, missed = {}, []
    for prec in E.PRECISIONS:
        model.set_gemm_precision(prec)
        out = _run(model, dev, noisy, enroll)
        assert out.dtype == torch.float32 and out.shape == ref.shape, (prec, out.shape, ref.shape)
        assert bool(torch.isfinite(out).all()), prec
        err = E.errors(name, out.numpy(), ref.numpy())
        print(f"{group} {name} {where} [{prec}]: {err}")
        for metric, bound in E.bounds(name, prec).items():
            key = (group, name, prec, metric)
            if key not in _WORST or err[metric] > _WORST[key][0]:
                _WORST[key] = (err[metric], where)
            if not err[metric] < bound:
                missed.append((prec, metric, err[metric], bound))
        results[prec] = out
    assert not missed, missed
    return results


@pytest.mark.parametrize("name,t", E.all_cases())
def test_preset_at_edge_length(PA, dev, name, t):
    noisy, enroll, ref = E.problem(name, E.length_of(name, t), 2)
    assert ref.shape == (2, E.out_length(name, t))
    _check("a-ladder", name, _model(PA, dev, name), dev, noisy, enroll, ref, f"T={t}")


@pytest.mark.parametrize("name,te", [(n, te) for n in E.ENROL_PRESETS for te in E.ENROL_T])
def test_enrolment_at_edge_length(PA, dev, name, te):
    win, hop = E.win_hop(name)
    t = E.mid_frames(name)
    noisy, enroll, ref = E.problem(name, win + hop * (t - 1) + 7, 2, win + hop * (te - 1) + 3)
    assert enroll.shape == (2, win + hop * (te - 1) + 3) and ref.shape == (2, E.out_length(name, t))
    assert bool(torch.isfinite(ref).all())
    _check("b-enrol", name, _model(PA, dev, name), dev, noisy, enroll, ref, f"Te={te}")


@pytest.mark.parametrize("name", E.PRESETS)
def test_odd_batches(PA, dev, name):
    t = E.mid_frames(name)
    length = E.length_of(name, t)
    model = _model(PA, dev, name)
    got = {}
    for b in E.ODD_BATCHES:
        noisy, enroll, ref = E.problem(name, length, b)
        assert ref.shape == (b, E.out_length(name, t))
        got[b] = _check("c-batch", name, model, dev, noisy, enroll, ref, f"B={b}")
    # An utterance inside the 17 against the same utterance on its own, the lone result standing in for the reference:
    # row 0 (det_wave's batch of one IS row 0 of its batch of 17), and row 16, the one past a full pack of 16.  The causal
    # SkiM hands the last segment state of utterance n - 1 to utterance n, as the reference does (skim.py:102-109), so
    # there only row 0 has a lone counterpart.
    assert torch.equal(E.problem(name, length, 17)[0][:1], E.problem(name, length, 1)[0])
    alone = {0: got[1]}
    if "skim" not in name:
        noisy, enroll, ref = E.problem(name, length, 1, row=16)
        assert torch.equal(noisy, E.problem(name, length, 17)[0][16:17])
        alone[16] = _check("c-batch", name, model, dev, noisy, enroll, ref, "B=1, utterance 16")
    missed = []
    for row, lone in alone.items():
        for prec in E.PRECISIONS:
            err = E.errors(name, got[17][prec][row:row + 1].numpy(), lone[prec].numpy())
            print(f"c-row {name} row {row} of 17 vs alone [{prec}]: {err}")
            for metric, bound in E.bounds(name, prec).items():
                key = ("c-row", name, prec, metric)
                if key not in _WORST or err[metric] > _WORST[key][0]:
                    _WORST[key] = (err[metric], f"row {row}")
                if not err[metric] < bound:
                    missed.append((row, prec, metric, err[metric], bound))
    assert not missed, missed


@pytest.mark.parametrize("name", E.PRESETS)
def test_one_model_object_walks_the_ladder(PA, dev, name):
    """A plan, workspace or kept-scratch entry keyed by a stale shape shows as a difference from a model that never saw
    another length (the same bits run to run: test_hip_parity.py::test_input_is_not_modified_and_result_is_deterministic,
    test_scratch_state_gpu.py)."""
    order = E.walk_order(name)
    again = (1, 129, order[-1])
    for prec in E.PRECISIONS:
        walked = _fresh(PA, dev, name).set_gemm_precision(prec)
        seen = {}
        for t in order:
            noisy, enroll = E.inputs(name, E.length_of(name, t), 2)
            seen[t] = _run(walked, dev, noisy, enroll)
            assert seen[t].shape == (2, E.out_length(name, t)) and bool(torch.isfinite(seen[t]).all()), (prec, t)
        del walked
        fresh = _fresh(PA, dev, name).set_gemm_precision(prec)
        for t in again:
            noisy, enroll = E.inputs(name, E.length_of(name, t), 2)
            assert torch.equal(_run(fresh, dev, noisy, enroll), seen[t]), (prec, t)
        del fresh


@pytest.mark.parametrize("name", E.PRESETS)
def test_too_short_is_refused(PA, dev, name):
    win, _ = E.win_hop(name)
    model = _fresh(PA, dev, name)
    noisy, enroll = E.inputs(name, win - 1, 2)
    for prec in E.PRECISIONS:
        model.set_gemm_precision(prec)
        with pytest.raises((RuntimeError, ValueError)):
            model.inference(noisy.to(dev), None if enroll is None else enroll.to(dev))
        torch.cuda.synchronize(dev)
    noisy, enroll, ref = E.problem(name, E.length_of(name, 3), 2)
    _check("e-refused", name, model, dev, noisy, enroll, ref, "T=3 after L=win-1")
