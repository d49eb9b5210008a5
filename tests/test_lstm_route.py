"""_plans.lstm_route without a GPU: for every case of tests/recurrent_route_cases.py the pure function names the arithmetic,
layout and kernel whose C entries tests/recurrent_calls.txt -- recorded from the commit before the function existed -- lists for
that case; the standalone choice differs from the maskers' in the four documented ways and no other; and the cooperative
switch of hip.coop_lstm_off() is scoped to the block and to the thread."""
import itertools
import threading

import pytest

from puresound_amd import hip
from puresound_amd._abi import padded_frames
from puresound_amd.nnet import _plans
from recurrent_route_cases import CASES, GEMM_ENTRIES, KERNEL_ENTRIES, LEDGER, switched
from test_streaming_calls_gpu import read_ledger

LSTM_CASES = [c for c in CASES if c["kind"] == "LSTM"]
H256_OK = hip.lstm_h256_f32_ok


@pytest.fixture(scope="module")
def want():
    return read_ledger(LEDGER)


def _plan(planes, inp, hid, d):
    """lstm_plan's scalars, as lstm_route reads them."""
    plan = dict(planes=planes, I=inp, H=hid, D=d, rows=d * 4 * hid)
    if planes == 0 and hid in (256, 192):
        plan["whh_h256_f32"] = True
    return plan


@pytest.mark.parametrize("case", LSTM_CASES, ids=[c["name"].replace(" ", "_") for c in LSTM_CASES])
def test_route_names_the_entries_the_parent_called(want, monkeypatch, case):
    lines = want[case["name"]]
    calls = [ln.split()[0] for ln in lines if not ln.startswith("sha256 ")]
    n, q, q_stride, steps, step_stride, t = case["walk"]
    asked = []
    # (ps_conv1x1_f16x2_fmajor_ok depends on the device's CU count: the recorded answer)
    monkeypatch.setattr(hip, "conv1x1_f16x2_fmajor_ok",
                        lambda *a: asked.append("ps_conv1x1_f16x2_fmajor_ok") or "ps_conv1x1_f16x2_fmajor_f32" in calls)
    monkeypatch.setattr(hip, "lstm_h256_f32_ok", lambda *a, **k: asked.append("ps_lstm_h256_ok"))
    with switched(case["switches"]):
        route = _plans.lstm_route(_plan(_plans._PLANES[case["gemm"]], case["C"], case["H"], case["D"]), n, padded_frames(t), t,
                                  (q, q_stride, steps, step_stride), carried=bool(case["states"]),
                                  state_shift=case["state_shift"], standalone=case["call"] == "single_rnn")
    assert tuple(route) == case["route"]
    gemm = next(ln for ln in lines if ln.split()[0] in GEMM_ENTRIES.values()).split()
    assert gemm[0] == GEMM_ENTRIES[route.gemm, route.layout]
    if route.gemm == "bf16":
        assert int(gemm[11]) == route.planes                       # (ps_conv1x1_bf16_io's eleventh argument)
    recurrences = set().union(*KERNEL_ENTRIES.values())
    assert {c for c in calls if c in recurrences} <= KERNEL_ENTRIES[route.kernel]
    assert any(c in KERNEL_ENTRIES[route.kernel] for c in calls)
    # the route asks ps_conv1x1_f16x2_fmajor_ok where the ledger has it, once per call of the case, and never ps_lstm_h256_ok:
    # lstm_recurrence asks that behind the GEMM, and the ledger has it exactly in the cases routed to "h256_f32", where the
    # library, asked for real, takes the launch
    assert asked * (1 + len(case["then"])) == [c for c in calls if c == "ps_conv1x1_f16x2_fmajor_ok"]
    assert ("ps_lstm_h256_ok" in calls) == (route.kernel == "h256_f32")
    if route.kernel == "h256_f32":
        assert H256_OK(n, padded_frames(t), case["H"], case["D"], q, q_stride, steps, step_stride, state_shift=case["state_shift"],
                       ldq=padded_frames(q) if case["states"] else 0)


def test_standalone_differs_from_the_masker_in_the_four_documented_ways_only(monkeypatch):
    monkeypatch.setattr(hip, "conv1x1_f16x2_fmajor_ok", lambda *a: True)
    differences = set()
    for planes, inp, hid, d, fmajor, carried in itertools.product((0, 1, 2, 3), (32, 64), (64, 128, 192, 256), (1, 2),
                                                                  (True, False), (False, True)):
        monkeypatch.setattr(_plans, "FMAJOR_LSTM", fmajor)
        args = (_plan(planes, inp, hid, d), 2, 128, 128, (64, 2, 2, 1), carried)
        masker, alone = _plans.lstm_route(*args), _plans.lstm_route(*args, standalone=True)
        if masker == alone:
            continue
        assert planes == 2, "the fp32 and bf16 arithmetics choose alike"
        if masker.kernel == "fmajor128":
            assert alone == ("bf16", 3, "rows", "generic") and hid == 128 and fmajor and not carried
            differences.add(1)
        elif alone.kernel == "fmajor256":
            assert masker == ("f16x2", 0, "rows", "generic_f16x2") and hid in (256, 192) and not fmajor
            differences.add(2)
        elif inp >= 64:
            assert (masker, alone) == (("f16x2", 0, "rows", "generic_f16x2"), ("bf16", 3, "rows", "generic"))
            differences.add(3)
        else:
            assert (masker, alone) == (("fp32", 0, "rows", "generic_f16x2"), ("fp32", 0, "rows", "generic"))
            differences.add(4)
    assert differences == {1, 2, 3, 4}


def test_coop_lstm_off_is_scoped_to_the_block_and_the_thread():
    assert hip._COOP_OFF.depth == 0
    seen = []
    with hip.coop_lstm_off():
        assert hip._COOP_OFF.depth == 1
        with hip.coop_lstm_off():
            assert hip._COOP_OFF.depth == 2
        assert hip._COOP_OFF.depth == 1
        other = threading.Thread(target=lambda: seen.append(hip._COOP_OFF.depth))
        other.start()
        other.join()
    assert hip._COOP_OFF.depth == 0 and seen == [0]
    with pytest.raises(KeyError):
        with hip.coop_lstm_off():
            with hip.coop_lstm_off():
                raise KeyError("inside the block")
    assert hip._COOP_OFF.depth == 0
