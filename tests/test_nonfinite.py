"""One NaN or infinity in a live input sample, on the CPU: the fp64 oracle and the package's CPU path against the masks the
reference itself produced (tests/golden/nonfinite_masks.json, written by tests/golden/make_nonfinite_golden.py).  The oracle
is the expected value of tests/test_nonfinite_gpu.py, so it is pinned here first: same NaN mask, same inf mask, for every
wrapper case and every placement of the bad sample."""
import numpy as np
import pytest
import torch

import cases
import nonfinite_cases as NF

PAIRS = [(n, s) for n in NF.CASES for s in NF.scenarios(n)]
# model.inference on CPU tensors exists for the Conv-TasNet family; these are the cases tests/test_cpu_path.py runs, at its 1e-4
CPU_PATH = ["cfg1_short", "tiny_stft", "tiny_stft_keepdc", "cfg2_short", "tiny_free", "tiny_free_relu_causal"]
# The reference runs a causal SkiM's rows as one sequence for the memory LSTM: row n starts from the state row n - 1 ended
# with (skim.py; tests/skim_step_ref.py), so a bad sample in row 0 reaches every later row and these scenarios have no clean
# row.  Everywhere else a row the bad sample is not in comes out untouched.
NO_CLEAN_ROW = {(n, s) for n in ("tse_skim_v1_short", "tse_skim_fbank_short", "tse_skim_v2_short", "tse_skim_vad_short",
                                 "tse_skim_causal_short")
                for s in ("first_row0_nan", "last_row0_nan", "enroll_row0_pinf")}


def test_fixture_covers_every_case_and_scenario():
    masks, look = NF.golden()
    assert sorted(masks) == sorted(NF.CASES)
    for name in NF.CASES:
        assert sorted(masks[name]) == sorted(NF.scenarios(name)) and len(masks[name]) <= 6
    assert sorted(look) == sorted(NF.PRESETS)


def test_fixture_is_not_degenerate():
    """No test below can pass on an empty or an all-NaN fixture: outside the SkiM row-0 scenarios named above every
    scenario leaves a row with an empty mask, every scenario has a NaN somewhere, and at least six cases have a bad row
    that is neither all-NaN nor NaN-free."""
    partial = set()
    no_clean = set()
    for name, sc in PAIRS:
        nan, inf = NF.golden_masks(name, sc)
        bad = nan | inf
        # (the last sample lies past the last whole frame of some encoders: there the reference's output stays clean)
        assert nan.any() or sc == "last_row0_nan", (name, sc)
        if not (~bad).all(axis=1).any():
            no_clean.add((name, sc))
        if any(0 < int(r.sum()) < r.size for r in nan):
            partial.add(name)
    assert no_clean == NO_CLEAN_ROW
    assert len(partial) >= 6, sorted(partial)


@pytest.mark.parametrize("name,sc", PAIRS)
def test_oracle_masks_equal_the_reference(name, sc):
    nan, inf = NF.golden_masks(name, sc)
    out = NF.oracle_out(name, sc)
    assert out.shape == nan.shape
    assert NF.runs(np.isnan(out)) == NF.runs(nan)
    assert NF.runs(np.isinf(out)) == NF.runs(inf)
    # rows the reference left clean are the clean batch's rows (the oracle has no cross-row arithmetic either)
    clean = ~(nan | inf).any(axis=1)
    assert np.array_equal(out[clean], NF.oracle_out(name, None)[clean])


@pytest.fixture(scope="module")
def cpu_models():
    import puresound_amd.nnet as PA
    made = {}

    def get(name):
        if name not in made:
            model = cases.build(PA.NS, name).eval()
            model.load_state_dict(NF.state_dict(name))
            made[name] = model
        return made[name]
    return get


@pytest.mark.parametrize("name,sc", [(n, s) for n, s in PAIRS if n in CPU_PATH])
def test_cpu_path_masks_and_finite_values(cpu_models, name, sc):
    """model.inference on CPU tensors: the reference's masks, its finite elements within test_cpu_path.py's 1e-4 of the
    oracle, and the clean rows bit-identical to the clean batch's."""
    model = cpu_models(name)
    nan, inf = NF.golden_masks(name, sc)
    noisy, enroll = NF.bad_inputs(name, sc)
    out = model.inference(noisy, enroll).numpy()
    assert NF.runs(np.isnan(out)) == NF.runs(nan)
    assert NF.runs(np.isinf(out)) == NF.runs(inf)
    err, den = NF.finite_error(name, out, NF.oracle_out(name, sc))
    print(f"{name} {sc}: finite error {err / den:.3e}")
    assert err / den < NF.TOL
    clean = ~(nan | inf).any(axis=1)
    cn, ce = NF.clean_inputs(name)
    assert np.array_equal(out[clean], model.inference(cn, ce).numpy()[clean])
