"""What one recurrent pass hands to the C ABI: every library call that _plans.lstm_path and SingleRNN.forward_padded make, the
predicates they ask included, with every argument, and the sha256 of what they return -- against a ledger recorded from commit
d8737a9, before the choice of GEMM, layout and recurrence entry became one function (_plans.lstm_route).  A route that
asks another predicate, packs for another kernel or launches in another order differs from the ledger in a line; one that
computes other bits differs in a hash.

The cases (tests/recurrent_route_cases.py) are one direct call each on modules built from nn.LSTM / nn.Linear / nn.LayerNorm
with name-keyed weights, on the smallest rows that reach the branch; the recorder and the argument format are those of
test_streaming_calls_gpu.py.  A case's lines: the calls, then `sha256 out<i> <hex>` over the valid frames of each call's
output and `sha256 h` / `sha256 c` over the returned states' Q columns where there are any.

`python tests/test_recurrent_calls_gpu.py --record [path]` writes recurrent_calls.txt from the tree it runs in, each case
run twice: a case whose hashes differ between the two runs is named in the header and recorded without them."""
import hashlib
import sys

import pytest
import torch
import torch.nn as nn

import conftest  # noqa: F401  (run as a script: it puts the repository and tests/golden on sys.path)
from detweights import det_state_dict, det_wave
from recurrent_route_cases import CASES, GEMM_ENTRIES, KERNEL_ENTRIES, LEDGER, PROJ_ENTRIES, WANTED_ROUTES, switched
from test_streaming_calls_gpu import Recorder, read_ledger, write_ledger

pytestmark = pytest.mark.gpu
HEADER = ("# recorded from commit d8737a9 (the parent of the commit that added _plans.lstm_route) by\n"
          "# `python tests/test_recurrent_calls_gpu.py --record` on an MI355X; every hash was the same in two recordings.\n")


def _rows(seed, n, c, ld, valid, dev):
    """[n, c, ld] with name-free deterministic values in the first `valid` columns and zeros behind them."""
    x = torch.zeros(n, c, ld)
    x[:, :, :valid] = det_wave(seed, n * c, valid).view(n, c, valid)
    return x.to(dev)


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def ledger_of(case, dev):
    """The lines of one case."""
    from puresound_amd import _abi, hip
    from puresound_amd.nnet import _plans
    from puresound_amd.nnet.lobe.rnn import SingleRNN
    c, hid, d = case["C"], case["H"], case["D"]
    if case["call"] == "single_rnn":
        mod = SingleRNN(case["kind"], c, hid, bidirectional=d == 2).eval()
        mod.set_gemm_precision(case["gemm"])
    else:
        mod = nn.ModuleDict(dict(rnn=nn.LSTM(c, hid, 1, batch_first=True, bidirectional=d == 2), proj=nn.Linear(d * hid, c),
                                 norm=nn.LayerNorm(c))).eval()
    mod.load_state_dict(det_state_dict(mod))
    mod.to(dev)
    if case["call"] == "lstm_path":
        plans = (_plans.lstm_plan(mod["rnn"], dev, case["gemm"]), _plans.linear_plan(mod["proj"], dev),
                 _plans.layernorm_plan(mod["norm"], dev))
    rec = Recorder(hip.lib(), _abi.SIGNATURES)
    lines, states = [], None
    with switched(dict(case["switches"], **{"hip.lib": lambda: rec})), \
            _abi.debug(_abi.PS_DBG_GEMM_ANY_SIZE if case["any_size"] else 0):
        for i, (n, q, q_stride, steps, step_stride, t) in enumerate((case["walk"],) + case["then"]):
            x = _rows(41 + i, n, c, hip.padded_frames(t), t, dev)
            if case["call"] == "single_rnn":
                with rec.recording():
                    y = mod.forward_padded(x, t)
            else:
                kw = {}
                if case["states"]:
                    h0, c0 = (_rows(s, n, d * hid, hip.padded_frames(q), q, dev) for s in (51, 52))
                    kw = dict(h0=h0, c0=c0, want_state=True) if case["states"] == "init" else dict(h0=h0, c0=c0, state_out=(h0, c0))
                amax = {None: None, "empty": [None], "measured": [hip.absmax(x, t)]}[case["amax"]]
                with rec.recording():
                    y, states = _plans.lstm_path(x, t, *plans, q=q, q_stride=q_stride, steps=steps, step_stride=step_stride,
                                                 state_shift=case["state_shift"], amax=amax, skip=case["skip"], **kw)
            lines.append(f"sha256 out{i} {_sha(y[..., :t])}")
            if states is not None:
                lines += [f"sha256 {name} {_sha(s[..., :q])}" for name, s in zip("hc", states)]
    torch.cuda.synchronize(dev)
    return rec.lines + lines


def _calls(lines):
    return [ln.split()[0] for ln in lines if not ln.startswith("sha256 ")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def want():
    return read_ledger(LEDGER)


@pytest.mark.parametrize("case", CASES, ids=[c["name"].replace(" ", "_") for c in CASES])
def test_calls_and_bits(dev, want, case):
    expected = want[case["name"]]
    lines = ledger_of(case, dev)
    if not any(ln.startswith("sha256 ") for ln in expected):    # (named in the ledger's header: not bit-stable on the parent)
        lines = [ln for ln in lines if not ln.startswith("sha256 ")]
    for k, (got, exp) in enumerate(zip(lines, expected)):
        assert got == exp, f"line {k}"
    assert len(lines) == len(expected) > 0


def test_every_branch_is_in_the_ledger_under_the_entry_its_tag_names(want):
    """Each case's ledger holds the input GEMM, the recurrence entry and the projection branch its tag names, every wanted
    route and every projection branch has a case, and only a cooperative launch may go without hashes."""
    assert {c["route"] for c in CASES} == WANTED_ROUTES and {c["proj"] for c in CASES} == set(PROJ_ENTRIES)
    assert set(want) == {c["name"] for c in CASES}
    recurrences = set().union(*KERNEL_ENTRIES.values())
    for case in CASES:
        calls = _calls(want[case["name"]])
        arith, planes, layout, kernel = case["route"]
        assert {c for c in calls if c in recurrences} <= KERNEL_ENTRIES[kernel] and any(c in recurrences for c in calls), case["name"]
        gemm = next(ln for ln in want[case["name"]] if ln.split()[0] in GEMM_ENTRIES.values()).split()
        assert gemm[0] == GEMM_ENTRIES[arith, layout] and (arith != "bf16" or int(gemm[11]) == planes), case["name"]
        last = max(k for k, c in enumerate(calls) if c in recurrences)
        assert calls[last + 1:] == PROJ_ENTRIES[case["proj"]], case["name"]
        if not any(ln.startswith("sha256 ") for ln in want[case["name"]]):
            assert "ps_lstm_fmajor_coop_f16x2_f32" in calls, case["name"]


def record(path):
    device = torch.device("cuda:0")
    recorded, unstable = {}, []
    for case in CASES:
        first, second = ledger_of(case, device), ledger_of(case, device)
        if first != second:
            assert _calls(first) == _calls(second) and [ln for ln in first if not ln.startswith("sha256 ")] == \
                [ln for ln in second if not ln.startswith("sha256 ")], case["name"]
            unstable.append(case["name"])
            first = [ln for ln in first if not ln.startswith("sha256 ")]
        recorded[case["name"]] = first
        print(f"{case['name']}: {' '.join(_calls(first))}", flush=True)
    write_ledger(recorded, path)
    with open(path) as f:
        body = f.read()
    with open(path, "w") as f:
        f.write(HEADER + "".join(f"# no hashes: {name}: its output differed between two runs on that commit\n"
                                 for name in unstable) + body)


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"] and len(sys.argv) <= 3, __doc__
    record(sys.argv[2] if len(sys.argv) == 3 else LEDGER)
