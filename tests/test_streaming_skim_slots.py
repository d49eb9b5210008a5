"""Slot sessions of StreamingSkiMExtractor (puresound_amd/streaming/skim.py) without a GPU: the slot reference of
tests/skim_slots_ref.py against the block reference, the declarations of the slot kernel, what its entry refuses before any
launch, and the host-only half of init_slots / open / end / close."""
import ctypes as C
import os
import re

import pytest
import torch

import skim_slots_ref as RS
import skim_step_ref as R
from test_streaming_skim import _DIMS, BUF, REFUSALS, _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MAX = 2 ** 31 - 1
NAME, SIBLING = "ps_skim_block_step_slots_f32", "ps_skim_block_step_f32"


# -------------------------------------------------------------------------------------------------------------------------
# the reference against itself
# -------------------------------------------------------------------------------------------------------------------------
def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1


def _chunks(total, k_max=16):
    """Chunk lengths 1, 2, ..., k_max, 1, 2, ... covering `total` frames."""
    out, k = [], 1
    while sum(out) < total:
        out.append(min(k, total - sum(out)))
        k = k % k_max + 1
    return out


@pytest.mark.parametrize("variant", list(R.VARIANTS))
@pytest.mark.parametrize("c,h,k", [(16, 8, 5), (5, 20, 10)])
def test_slot_reference_against_block_reference(c, h, k, variant):
    """A column born at frame s and fed from there is block_step of that column alone started at t0 = 0 on the same frames,
    states and banks, whatever the session's counter says: outputs, every state, both banks and the slots visited.  A column
    with an empty span is left alone."""
    film, incoming, mem = R.VARIANTS[variant]
    births = [1, 2, k - 1, k + 1, 3 * k + 2]
    assert all(s % k for s in births) and len(set(births)) == len(births)
    spans = [(s, I32_MAX) for s in births] + [(0, 0)]
    b, t_len, ns = len(spans), 5 * k + 3, R.slots_needed(16, k)
    blk = R.make_block(c, h, 5, film, mem, torch.float64)
    x = _rand((t_len, b, c), 10)
    state = R.new_state(b, h, mem)
    for n, key in enumerate(sorted(state)):
        state[key] = _rand((b, h), 20 + n)
    rs, rb = (_rand((b, c), 30), _rand((b, c), 31)) if film else (None, None)
    bank_in = (_rand((ns, b, h), 40), _rand((ns, b, h), 41)) if incoming else None
    bank_out = (_rand((ns, b, h), 42), _rand((ns, b, h), 43)) if mem else None
    before = {key: t.clone() for key, t in state.items()}
    out_before = None if bank_out is None else tuple(t.clone() for t in bank_out)
    in_before = None if bank_in is None else tuple(t.clone() for t in bank_in)
    xin = x.clone()
    for col, (birth, _) in enumerate(spans[:-1]):
        xin[:birth, col] = float("nan")                               # dead frames are not read
    xin[:, b - 1] = float("nan")
    outs, t0 = [], 0
    read, written = [set() for _ in spans], [set() for _ in spans]
    for n in _chunks(t_len):
        o, rd, wr = RS.block_step_slots(xin[t0:t0 + n], t0, k, blk, state, spans, rs, rb, bank_in, bank_out)
        outs.append(o)
        read = [a | v for a, v in zip(read, rd)]
        written = [a | v for a, v in zip(written, wr)]
        t0 += n
    out = torch.cat(outs)
    one_col = lambda t, col: t[..., col:col + 1, :].clone()  # noqa: E731
    for col, s in enumerate(births):
        one = {key: one_col(t, col) for key, t in before.items()}
        b_in = None if in_before is None else tuple(one_col(t, col) for t in in_before)
        b_out = None if out_before is None else tuple(one_col(t, col) for t in out_before)
        want, rd, wr = R.block_step(x[s:, col:col + 1], 0, k, blk, one, rs[col:col + 1] if film else None,
                                    rb[col:col + 1] if film else None, b_in, b_out)
        assert bool(torch.isnan(out[:s, col]).all())
        assert torch.equal(out[s:, col:col + 1], want), s
        for key, t in one.items():
            assert torch.equal(state[key][col:col + 1], t), (s, key)
        if mem:
            for got, ref in zip(bank_out, b_out):
                assert torch.equal(got[:, col:col + 1], ref), s
        assert read[col] == rd and written[col] == wr
    assert any(len(w) > 1 for w in written) == mem and any(len(r) > 1 for r in read) == incoming
    # the column that never lives: nothing computed, nothing changed; and the incoming banks are only read
    assert bool(torch.isnan(out[:, b - 1]).all()) and read[b - 1] == set() and written[b - 1] == set()
    for key, t in before.items():
        assert torch.equal(state[key][b - 1], t[b - 1]), key
    if mem:
        assert all(torch.equal(got[:, b - 1], ref[:, b - 1]) for got, ref in zip(bank_out, out_before))
    if incoming:
        assert all(torch.equal(got, ref) for got, ref in zip(bank_in, in_before))


# -------------------------------------------------------------------------------------------------------------------------
# declarations
# -------------------------------------------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "puresound_hip.h")) as f:
        return f.read()


def test_slot_entry_point_is_bound_and_declared():
    from puresound_amd import _abi
    assert NAME in _abi.SIGNATURES
    assert re.search(r"^int %s\(" % NAME, _header(), re.M), f"{NAME} is not declared in the header"
    n = lambda key: len(_abi.SIGNATURES[key][1])  # noqa: E731
    assert n(NAME) == n(SIBLING) + 1                                   # the span


def test_the_addition_keeps_the_abi_number():
    from puresound_amd import _abi
    assert _abi.ABI_VERSION == 24
    assert re.search(r"^#define PS_ABI_VERSION 24$", _header(), re.M)


def test_slot_kernel_is_in_the_source_as_a_compile_time_variant():
    with open(os.path.join(ROOT, "puresound_amd", "csrc", "skim_step.hip")) as f:
        src = f.read()
    assert re.search(r'extern "C" int %s\(' % NAME, src)
    assert re.search(r"^template <bool SLOTS", src, re.M)
    assert "if constexpr (SLOTS)" in src
    assert len(re.findall(r"^static int skim_block_step_launch\(", src, re.M)) == 1    # one check / launch path for both


# -------------------------------------------------------------------------------------------------------------------------
# what the entry refuses before any launch
# -------------------------------------------------------------------------------------------------------------------------
_SPAN_TEXT = NAME + ": span must be an 8-byte aligned device array [B][2] of int"
SLOT_REFUSALS = {name: (over, rc, text.replace(SIBLING, NAME)) for name, (over, rc, text) in REFUSALS.items()}
SLOT_REFUSALS["null_span"] = (dict(span=None), -1, _SPAN_TEXT)
SLOT_REFUSALS["span_misaligned"] = (dict(span=BUF + 3072 + 4), -1, _SPAN_TEXT)


def test_every_refusal_of_the_sibling_is_here():
    assert set(SLOT_REFUSALS) == set(REFUSALS) | {"null_span", "span_misaligned"}
    assert all(NAME in text for _, _, text in SLOT_REFUSALS.values())


@pytest.mark.parametrize("case", sorted(SLOT_REFUSALS))
def test_slot_entry_refuses_before_any_launch(case):
    """(host pointers, never dereferenced: the call returns first)"""
    from puresound_amd import _abi
    over, rc_want, text = SLOT_REFUSALS[case]
    a = dict(_DIMS, x=BUF, y=BUF + 1024, counter=BUF + 2048, span=BUF + 3072, blk=True, st=True)
    a.update({k: v for k, v in over.items() if k in a})
    if a["y"] == "x":
        a["y"] = a["x"]
    blk, st = _abi.SkimBlock(), _abi.SkimState()
    for p in (blk.seg, blk.mem_h, blk.mem_c):
        for name in ("wt", "bias", "pt", "pbias", "gamma", "beta"):
            setattr(p, name, BUF)
    blk.film_wt = blk.film_gamma = blk.film_beta = BUF
    for name, _ in _abi.SkimState._fields_:
        setattr(st, name, over.get(name, BUF))
    if "seg_pt" in over:
        blk.seg.pt = None
    lib = _abi.lib()
    rc = lib.ps_skim_block_step_slots_f32(a["x"], a["y"], a["counter"], a["span"], C.byref(blk) if a["blk"] else None,
                                          C.byref(st) if a["st"] else None, a["C"], a["H"], a["K"], a["NS"], a["B"], a["k"],
                                          a["ld"], a["ldb"], None)
    assert rc == rc_want
    assert lib.ps_last_error().decode() == text.format(**a)


# -------------------------------------------------------------------------------------------------------------------------
# the host half of the slot calls
# -------------------------------------------------------------------------------------------------------------------------
def _host_streamer(model):
    """A streamer around a model on the CPU: the constructor's last check (a ROCm device) is what a machine without one
    cannot pass, so the session core is set up directly.  Only calls that launch nothing are made on it."""
    from puresound_amd.streaming import StreamingSkiMExtractor
    from puresound_amd.streaming._session import HopSession
    s = StreamingSkiMExtractor.__new__(StreamingSkiMExtractor)
    HopSession.__init__(s, model, model.encoder.win_length, model.encoder.hop_length)
    s.win_length = s.window
    return s


def _raises(exc, words, fn, *a, **kw):
    with pytest.raises(exc) as info:
        fn(*a, **kw)
    assert words.lower() in str(info.value).lower(), str(info.value)


def test_slot_calls_outside_a_slot_session_name_the_way_out():
    import puresound_amd.nnet as PA
    s = _host_streamer(_build())
    assert hasattr(s, "init_slots") and "init_slots()" in s._how_to_start
    for fn, a in ((s.open, (0,)), (s.end, (0, 1)), (s.close, (0,))):
        _raises(RuntimeError, "init_slots()", fn, *a)
    assert s.active == []
    _raises(ValueError, "capacity >= 1", s.init_slots, 0)
    # a block session (a masker without an embedding input starts one with no tensor from the caller)
    plain = PA.SoTaskWrapModule(PA.FreeEncDec(32, 16, 16, output_active=True),
                                PA.SkiM(16, 8, 16, n_blocks=2, seg_size=5, causal=True), verbose=False).eval()
    sp = _host_streamer(plain)
    sp._begin(2, torch.device("cpu"), False)                           # what init_streams() does first
    for fn, a in ((sp.open, (0,)), (sp.end, (0, 1)), (sp.close, (0,))):
        _raises(RuntimeError, "init_slots()", fn, *a)
        _raises(RuntimeError, "flush()", fn, *a)


def test_init_slots_and_the_rules_of_open():
    s = _host_streamer(_build())
    m = s.model.masker
    assert m.embed_dim == 192
    s.init_slots(3)
    assert s.streams == 3 and s.active == [] and tuple(s._span.shape) == (3, 2) and s._span.dtype == torch.int32
    assert len(s._banks) == m.n_blocks - 1 and s._banks[0][0].shape[0] == (16 - 1) // m.seg_size + 3
    assert all(t is None or (float(t[0].abs().sum()), float(t[1].abs().sum())) == (0.0, 0.0) for t in s._terms)
    assert not s._priming()                                            # no priming phase in a slot session
    _raises(RuntimeError, "close(slot)", s.flush)
    e, d = torch.zeros(4000), torch.zeros(192)
    _raises(ValueError, "exactly one of enroll [L'] and embed [192]", s.open, 0)
    _raises(ValueError, "exactly one of enroll [L'] and embed [192]", s.open, 0, enroll=e, embed=d)
    _raises(ValueError, "exactly one of enroll [L'] and embed [192]", s.open, 0, e, d)
    _raises(IndexError, "0 .. 2", s.open, 3, embed=d)
    _raises(IndexError, "0 .. 2", s.close, -1)
    _raises(RuntimeError, "open(0)", s.end, 0, 1)
    _raises(RuntimeError, "open(1)", s.close, 1)
    _raises(RuntimeError, "ROCm device", s.open, 0, enroll=e)          # (tensors on the CPU are refused before any work)
    _raises(RuntimeError, "ROCm device", s.open, 0, embed=d)
    assert s.active == [] and s.frames == 0 and int(s._span.abs().sum()) == 0


def test_open_of_a_masker_without_an_embedding_takes_neither():
    import puresound_amd.nnet as PA
    plain = PA.SoTaskWrapModule(PA.FreeEncDec(32, 16, 16, output_active=True),
                                PA.SkiM(16, 8, 16, n_blocks=2, seg_size=5, causal=True), verbose=False).eval()
    s = _host_streamer(plain)
    s.init_slots(1)
    assert s._terms == [None, None]
    _raises(ValueError, "pass neither enroll nor embed", s.open, 0, enroll=torch.zeros(4000))
    _raises(ValueError, "pass neither enroll nor embed", s.open, 0, embed=torch.zeros(192))
    assert s.active == []


def test_the_siblings_keep_their_open():
    """HopSession.open takes (slot, enroll) as before; only the SkiM streamer's takes an embedding."""
    import inspect
    from puresound_amd.streaming import StreamingSkiMExtractor
    from puresound_amd.streaming._session import HopSession
    from puresound_amd.streaming.dprnn import StreamingDPRNN
    assert list(inspect.signature(HopSession.open).parameters) == ["self", "slot", "enroll"]
    assert StreamingDPRNN.open is HopSession.open
    assert list(inspect.signature(StreamingSkiMExtractor.open).parameters) == ["self", "slot", "enroll", "embed"]
