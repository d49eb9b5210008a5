"""Slot sessions of StreamingSeparator (puresound_amd/streaming/spectral.py) without a GPU: the ABI of the one new entry,
ps_state_gate_slots_f32, and the span rule for a CARRIED state in fp64 on a toy model -- a causal 2-tap convolution, a
one-step LSTM whose (h, c) is carried from hop to hop, an overlap-add -- against the same toy run on each stream alone.  The
same toy without the gate on the state differs: the test sees the defect the gate is there for."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "ps_state_gate_slots_f32"
# three streams: births 0 / 4 / 9, lengths 7 / 1 / 11 frames; dead frames hold 1e6
BIRTHS, LENGTHS, DEAD = (0, 4, 9), (7, 1, 11), 1e6
SPAN = torch.tensor([[b, b + n] for b, n in zip(BIRTHS, LENGTHS)])
HOPS = max(b + n for b, n in zip(BIRTHS, LENGTHS)) + 6
C, HID, HOP, N_FFT = 3, 4, 2, 6


def _read(*rel):
    with open(os.path.join(ROOT, *rel)) as f:
        return f.read()


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_state_gate_entry_is_declared_bound_and_defined():
    from puresound_amd import _abi
    header = re.sub(r"/\*.*?\*/", "", _read("include", "puresound_hip.h"), flags=re.S)
    decl = re.search(r"^int %s\((.*?)\);" % ENTRY, header, re.M | re.S)
    assert decl, f"{ENTRY} is not declared in the header"
    args = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
    assert args == ["const ps_state_rows* states_host", "int n_states", "const int* counter", "const int* span", "int shift",
                    "int B", "int ld", "void* stream"]
    assert re.search(r"typedef struct ps_state_rows \{\s*float\* x;\s*int64_t rows;\s*\} ps_state_rows;", header)
    assert ENTRY in _abi.SIGNATURES and len(_abi.SIGNATURES[ENTRY][1]) == len(args)
    assert [n for n, _ in _abi.StateRows._fields_] == ["x", "rows"]
    src = _read("puresound_amd", "csrc", "stream_step.hip")
    assert re.search(r'extern "C" int %s\(' % ENTRY, src)
    # beside the other conv-STFT slot entries, after the table's size
    assert header.index("#define PS_MAX_RING_PAIRS") < header.index("int " + ENTRY) < header.index("int ps_conv2d_step_slots_f32(")
    hip_py = _read("puresound_amd", "hip.py")
    body = hip_py[hip_py.index("def state_gate("):]
    body = body[:body.index("\ndef ", 1)]
    assert f"lib().{ENTRY}(" in body and "shift: int = 1" in body


def test_the_addition_keeps_the_abi_number_and_the_commit_entries():
    from puresound_amd import _abi
    assert _abi.ABI_VERSION == 24
    assert [n for n, _ in _abi.RingPair._fields_] == ["src", "ring", "count", "slots", "reserved"]
    src = _read("puresound_amd", "csrc", "stream_step.hip")
    # the gate is a launch of its own: the commit kernel still reads no span and advances the counter alone
    commit = src[src.index("void stream_commit_kernel("):]
    commit = commit[:commit.index("\n}\n")]
    assert "span" not in commit and "counter[0] += advance" in commit


def test_streamer_has_the_slot_calls_and_says_so():
    from puresound_amd.streaming import StreamingSeparator as S
    for name in ("init_slots", "open", "end", "close", "_flush_slot", "_open_slot", "_enrolment_rule", "_allocate"):
        assert callable(getattr(S, name)), name
    required, why = S._enrolment_rule(None)
    assert required is False and "no enroll" in why
    assert "StreamingSeparator has no slot sessions" not in _read("README.md")


# ---- the span rule for a carried state, fp64 --------------------------------------------------------------------------------
def _toy(seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1  # noqa: E731
    return dict(w0=r(C, C), w1=r(C, C), bias=r(C), wih=r(4 * HID, C), whh=r(4 * HID, HID), b=r(4 * HID), v=r(N_FFT, HID),
                window=torch.hann_window(N_FFT, periodic=True, dtype=torch.float64) + 0.1)


def _cell(p, y, h, c):
    """One LSTM step for [B, C] inputs from the states [B, HID]."""
    z = y @ p["wih"].t() + h @ p["whh"].t() + p["b"]
    i, f, g, o = z.chunk(4, dim=1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


def _live(span, g):
    return (span[:, 0] <= g) & (g < span[:, 1])


def _session(p, x, span, gate_state=True, state0=DEAD):
    """x [B, C, HOPS] -> [B, HOPS * HOP + N_FFT - HOP]: the hop body of a slot session, every stream a column.  Nothing is
    cleared: the ring and the carried state start as DEAD and go on holding whatever the dead frames leave there.
    Frame g of a tensor is read as an exact 0 for stream b unless span[b, 0] <= g < span[b, 1] -- the convolution's two taps
    (frames t - 1, t), the carried state (frame t - 1, the gate before the hop's first reader), the synthesis (frame t)."""
    b = x.shape[0]
    ring = torch.full((b, C), DEAD, dtype=torch.float64)
    h, c = torch.full((b, HID), state0, dtype=torch.float64), torch.full((b, HID), state0, dtype=torch.float64)
    out = torch.zeros(b, HOPS * HOP + N_FFT - HOP, dtype=torch.float64)
    zero = torch.zeros((), dtype=torch.float64)
    for t in range(HOPS):
        now, before = _live(span, t)[:, None], _live(span, t - 1)[:, None]
        if gate_state:                                                   # ps_state_gate_slots_f32, shift = 1: a select
            h, c = torch.where(before, h, zero), torch.where(before, c, zero)
        cur = x[:, :, t]
        y = torch.where(before, ring, zero) @ p["w0"].t() + torch.where(now, cur, zero) @ p["w1"].t() + p["bias"]
        h, c = _cell(p, y, h, c)                                         # the commit: h', c' become the carried state
        frame = (h @ p["v"].t()) * p["window"]
        out[:, t * HOP:t * HOP + N_FFT] += torch.where(now, frame, zero)
        ring = cur
    return out


def _alone(p, x):
    """x [C, n], one stream from frame 0 with zero padding and zero states -> [(n - 1) * HOP + N_FFT]"""
    n = x.shape[1]
    h, c = torch.zeros(1, HID, dtype=torch.float64), torch.zeros(1, HID, dtype=torch.float64)
    out = torch.zeros((n - 1) * HOP + N_FFT, dtype=torch.float64)
    prev = torch.zeros(1, C, dtype=torch.float64)
    for t in range(n):
        cur = x[None, :, t]
        h, c = _cell(p, prev @ p["w0"].t() + cur @ p["w1"].t() + p["bias"], h, c)
        out[t * HOP:t * HOP + N_FFT] += ((h @ p["v"].t()) * p["window"])[0]
        prev = cur
    return out


def _streams(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.full((len(BIRTHS), C, HOPS), DEAD, dtype=torch.float64)
    own = []
    for b, (birth, n) in enumerate(zip(BIRTHS, LENGTHS)):
        own.append(torch.rand(C, n, generator=g, dtype=torch.float64) * 2 - 1)
        x[b, :, birth:birth + n] = own[-1]
    return x, own


def _errors(p, got, own):
    errs = []
    for b, (birth, n) in enumerate(zip(BIRTHS, LENGTHS)):
        want = _alone(p, own[b])
        first = birth * HOP
        mine = got[b, first:first + want.shape[0]]
        rest = torch.cat([got[b, :first], got[b, first + want.shape[0]:]])
        errs.append((float((mine - want).abs().max()), float(rest.abs().max()) if rest.numel() else 0.0))
    return errs


def test_carried_state_under_the_span_rule_is_each_streams_own_run():
    p = _toy(3)
    x, own = _streams(4)
    errs = _errors(p, _session(p, x, SPAN), own)
    for b, (err, outside) in enumerate(errs):
        assert err <= 1e-13, (b, err)
        assert outside == 0.0, b                                         # before the stream and after its tail: exact zeros


def test_without_the_gate_on_the_state_the_late_streams_differ():
    """The convolution of zeros plus its bias is not zero, so without the gate the LSTM has stepped on dead frames by the time a
    stream is born.  With the states zeroed at the session's start (what init_slots does) only the stream born at frame 0 is
    right; with nothing cleared (a reused slot) not even that one."""
    p = _toy(3)
    x, own = _streams(4)
    errs = _errors(p, _session(p, x, SPAN, gate_state=False, state0=0.0), own)
    assert errs[0][0] <= 1e-13
    assert errs[1][0] > 1e-3 and errs[2][0] > 1e-3, errs
    errs = _errors(p, _session(p, x, SPAN, gate_state=False), own)
    assert all(err > 1e-3 for err, _ in errs), errs
