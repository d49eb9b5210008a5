"""set_gemm_precision("fp32") on the SkiM presets takes ps_lstm_h256_f32 for every 256- / 192-unit recurrence: the calls the
models hand to the C ABI (a proxy around hip.lib(), the pattern of test_streaming_calls_gpu.py), the result against the
reference's golden vector and the float64 oracle, the switch hip.H256_F32_LSTM, batch lanes, graph replay, and the fp16x2
default, which must not see the new entry.

The models take the new entry from hip.H256_F32_MIN_SEQS[(H, D)] sequences per launch on (128; H = 192 in one direction never): below
that ps_lstm_f32 measured faster (profiles/lstm_h256_f32.txt).  The golden vectors are B = 2 utterances of 0.25 s -- 4 sequences per segment launch -- so the
tests on them lower the threshold to 1 (the `every_launch` fixture); test_the_default_threshold_* runs without it."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cases
from conftest import rel_max
from detweights import det_state_dict, det_wave
from edge_length_cases import FP32_TOL, weights
from oracle import separator_oracle as O
from puresound_amd import _abi, hip

pytestmark = pytest.mark.gpu
GOLDEN_TOL = 1e-4      # the bound of test_hip_parity.py's golden tests for these cases
SWITCH_TOL = 2e-5      # new entry against ps_lstm_f32 through a whole model
NAMES = ["tse_skim_causal_short", "tse_skim_v0_short", "tse_skim_v1_short"]
LSTM_ENTRIES = ("ps_lstm_f32", "ps_lstm_f16x2_f32", "ps_lstm_h256_f32")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def every_launch(monkeypatch):
    """The new entry for every launch it can take, however few its sequences."""
    monkeypatch.setattr(hip, "H256_F32_MIN_SEQS", {(h, d): 1 for h in (256, 192) for d in (1, 2)})


class Recorder:
    """hip.lib()'s stand-in: the library, with one (entry, arguments as text) per call while `on`; a recurrence entry's line
    carries its ps_lstm_args' integers and which of its pointers are set."""

    def __init__(self, real):
        self.real, self.on, self.calls = real, False, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not self.on:
            return fn

        def call(*args):
            text = ""
            if name in LSTM_ENTRIES:
                a = args[0]._obj
                text = " ".join(f"{k}={getattr(a, k) if kind is C.c_int else ('set' if getattr(a, k) else 'null')}"
                                for k, kind in _abi.LstmArgs._fields_)
            self.calls.append((name, text))
            return fn(*args)
        return call


def _hidden(text):
    return int(dict(kv.split("=") for kv in text.split())["H"])


def _model(name, dev, precision="fp32"):
    import puresound_amd.nnet as PA
    model = cases.build(PA.NS, name).eval()
    model.load_state_dict(det_state_dict(model))
    model.to(dev)
    if precision is not None:
        model.set_gemm_precision(precision)
    return model


def _inputs(name, dev, batch=None):
    c = cases.CASES[name]
    b = batch or c["B"]
    return det_wave(c["seed"], b, c["L"]).to(dev), det_wave(c["seed"] + 1, b, c["L_enroll"]).to(dev)


def _recorded(model, noisy, enroll, monkeypatch):
    rec = Recorder(hip.lib())
    with monkeypatch.context() as m:
        m.setattr(hip, "lib", lambda: rec)
        rec.on = True
        try:
            out = model.inference(noisy, enroll)
        finally:
            rec.on = False
    torch.cuda.synchronize()
    return out, rec.calls


@pytest.mark.parametrize("name", NAMES)
def test_fp32_takes_the_new_entry_and_matches_golden_and_fp64(name, dev, golden_dir, monkeypatch, every_launch):
    """Fails on a tree without ps_lstm_h256_f32: there every H = 256 / 192 recurrence is a ps_lstm_f32 call."""
    model = _model(name, dev)
    noisy, enroll = _inputs(name, dev)
    wav, calls = _recorded(model, noisy, enroll, monkeypatch)
    new = [t for n, t in calls if n == "ps_lstm_h256_f32"]
    old = [t for n, t in calls if n in ("ps_lstm_f32", "ps_lstm_f16x2_f32")]
    assert new and all(_hidden(t) in (256, 192) for t in new)
    assert not [t for t in old if _hidden(t) in (256, 192)], "an H = 256 / 192 recurrence still runs on ps_lstm_f32"
    # once per recurrence launch: as many as the switched-off model hands to ps_lstm_f32 with H = 256 / 192, same arguments
    speaker = 1 if cases.CASES[name]["speaker_net"].get("block") == "rnn" else 0
    assert {_hidden(t) for t in new} == ({256, 192} if speaker else {256})
    monkeypatch.setattr(hip, "H256_F32_LSTM", False)
    _, calls_off = _recorded(model, noisy, enroll, monkeypatch)
    off = [t for n, t in calls_off if n == "ps_lstm_f32" and _hidden(t) in (256, 192)]
    assert [t.replace("whh_t=null", "whh_t=set") for t in new] == off

    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    assert wav.shape == g["wav"].shape
    e_golden = rel_max(wav.cpu().numpy(), g["wav"])
    with torch.no_grad():
        ref = O.inference(noisy.cpu().double(), weights(name)[1], cases.oracle_cfg(name), enroll.cpu().double())
    e_fp64 = rel_max(wav.cpu().numpy(), ref.numpy())
    print(f"SKIMFP32 {name}: against the golden {e_golden:.3e}, against fp64 {e_fp64:.3e}")
    assert e_golden < GOLDEN_TOL
    assert e_fp64 < FP32_TOL


@pytest.mark.parametrize("name", NAMES)
def test_the_switch_restores_ps_lstm_f32_and_nothing_else(name, dev, monkeypatch, every_launch):
    """hip.H256_F32_LSTM = False: the call list is the one of a tree without the new entry -- the same calls in the same order
    with the same arguments, ps_lstm_f32 (whh_t set) where ps_lstm_h256_f32 (whh_t not read: null) stood -- and the result is
    within 2e-5 of the new one."""
    model = _model(name, dev)
    noisy, enroll = _inputs(name, dev)
    new, calls_new = _recorded(model, noisy, enroll, monkeypatch)
    monkeypatch.setattr(hip, "H256_F32_LSTM", False)
    old, calls_old = _recorded(model, noisy, enroll, monkeypatch)
    assert not [n for n, _ in calls_old if n == "ps_lstm_h256_f32"]
    # (the predicate is asked only where the new entry could run: it is no call of the old list)
    mapped = [("ps_lstm_f32", t.replace("whh_t=null", "whh_t=set")) if n == "ps_lstm_h256_f32" else (n, t)
              for n, t in calls_new if n != "ps_lstm_h256_ok"]
    assert [c for c in calls_old if c[0] != "ps_lstm_h256_ok"] == mapped
    assert rel_max(old.cpu().numpy(), new.cpu().numpy()) < SWITCH_TOL


def test_two_lanes_equal_one(dev, every_launch):
    """model.hip_streams = 2 at B = 4: bit-equal to one lane (below 16 utterances inference() keeps one lane whatever the
    setting).  At B = 16 the non-causal preset really runs two lanes of 8, the new entry on both streams at once: each half is
    bit-equal to that half run alone in one lane, the comparison test_scratch_state_gpu.py makes for lanes."""
    for name in ("tse_skim_causal_short", "tse_skim_v0_short"):
        model = _model(name, dev)
        noisy, enroll = _inputs(name, dev, 4)
        one = model.inference(noisy, enroll)
        model.hip_streams = 2
        assert torch.isfinite(one).all() and torch.equal(one, model.inference(noisy, enroll)), name
    model = _model("tse_skim_v0_short", dev)
    noisy, enroll = _inputs("tse_skim_v0_short", dev, 16)
    halves = torch.cat([model.inference(noisy[i:i + 8], enroll[i:i + 8]) for i in (0, 8)])
    model.hip_streams = 2
    for _ in range(2):   # (the first forked call runs its lanes one after the other)
        assert torch.equal(model.inference(noisy, enroll), halves)


def test_graph_replay_equals_eager(dev, every_launch):
    from puresound_amd.graphs import GraphedInference
    model = _model("tse_skim_causal_short", dev)
    noisy, enroll = _inputs("tse_skim_causal_short", dev)
    eager = model.inference(noisy, enroll)
    fast = GraphedInference(model)
    for _ in range(2):
        assert torch.equal(fast(noisy, enroll), eager)
    assert len(fast._graphs) == 1


def test_the_default_threshold_sends_128_sequences_to_the_new_entry_and_4_to_ps_lstm_f32(dev, monkeypatch):
    """Nothing lowered: 64 utterances of 0.25 s are 128 sequences per segment launch -- the new entry -- and 64 per Mem-LSTM
    launch -- ps_lstm_f32; the golden's 2 utterances stay on ps_lstm_f32 throughout."""
    assert hip.H256_F32_MIN_SEQS[(256, 1)] == 128 and hip.H256_F32_LSTM
    model = _model("tse_skim_causal_short", dev)
    for batch, want_new in ((64, True), (2, False)):
        noisy, enroll = _inputs("tse_skim_causal_short", dev, batch)
        out, calls = _recorded(model, noisy, enroll, monkeypatch)
        assert torch.isfinite(out).all()
        seqs = {n: [int(dict(kv.split("=") for kv in t.split())[k]) for k in ("N", "Q")] for n, t in calls if n in LSTM_ENTRIES}
        new = [t for n, t in calls if n == "ps_lstm_h256_f32"]
        assert bool(new) == want_new, (batch, seqs)
        for n, t in calls:
            if n in LSTM_ENTRIES and _hidden(t) in (256, 192):
                f = dict(kv.split("=") for kv in t.split())
                assert (n == "ps_lstm_h256_f32") == (int(f["N"]) * int(f["Q"]) >= 128), t


def test_the_fp16x2_default_does_not_see_the_new_entry(dev, monkeypatch):
    model = _model("tse_skim_causal_short", dev, precision=None)
    noisy, enroll = _inputs("tse_skim_causal_short", dev)
    _, calls = _recorded(model, noisy, enroll, monkeypatch)
    names = [n for n, _ in calls]
    assert "ps_lstm_h256_f32" not in names and "ps_lstm_h256_ok" not in names
    assert [n for n in names if n.startswith("ps_lstm")], "the model ran no recurrence"
