"""ps_lstm_rows_f32 through hip.lstm_rows against a float64 LSTM that walks each utterance's own steps.

Ten utterances of 27 steps whose step counts lie on both sides of the prefetch distance (LSTM_PF = 8) and of the row's end:
0, 1, 7, 8, 9, 17, 26, 27, 40 and -3 (the last two are clamped to 27 and 0).  H = 64 keeps W_hh in registers, 192 and 256
stream it; one and two directions; the walks of the two callers (one sequence per utterance over consecutive frames) and a
strided walk of five sequences (a partial group of the kernel's four sequences per workgroup).

House rules of test_abi_kernels_gpu.py: seeded Philox inputs, NaN in the caching allocator; gx holds NaN at every frame
behind a row's own last step; hout starts as a sentinel, which must survive at every frame the walk does not visit, and must
be exact 0.0 at the frames of the steps behind a row's end.  The bound is the FP32 class of test_abi_kernels_gpu.py (2e-5:
sums of products and transcendentals).  At H = 192 / 256 the plain entry runs the same kernel: row n is torch.equal to
hip.lstm on that row alone with steps = s_n."""
import pytest
import torch

from abi_refs import rand
from conftest import rel_max

pytestmark = pytest.mark.gpu
FP32 = 2e-5
NAN = float("nan")
SENTINEL = 777.0
STEPS = 27
STEPS_ROWS = (0, 1, 7, 8, 9, 17, 26, 27, 40, -3)
WALKS = {"callers": (1, 0, STEPS, 1, 40),       # Q, q_stride, steps, step_stride, ldt
         "strided": (5, 1, STEPS, 8, 216)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def H():
    from puresound_amd import hip
    hip.lib()
    return hip


@pytest.fixture(autouse=True)
def _nan_in_the_allocator_cache(dev):
    junk = [torch.full((1 << 22,), NAN, device=dev) for _ in range(8)]
    del junk
    yield


def _clamped():
    return [min(max(s, 0), STEPS) for s in STEPS_ROWS]


def _reference(gx, whh_t, hid, d, walk, h0, c0):
    """float64: every sequence (n, q) walks its utterance's own s_n steps -> (hout with SENTINEL where nothing is written,
    h_last, c_last [N, D*H, Q])"""
    q, qs, steps, ss, ldt = walk
    n = gx.shape[0]
    gx, w = gx.double(), whh_t.double()
    hout = torch.full((n, d * hid, ldt), SENTINEL, dtype=torch.float64)
    h_last, c_last = torch.zeros(n, d * hid, q, dtype=torch.float64), torch.zeros(n, d * hid, q, dtype=torch.float64)
    for i, sn in enumerate(_clamped()):
        for di in range(d):
            for qi in range(q):
                h = h0[i, di * hid:(di + 1) * hid, qi].double().clone() if h0 is not None else torch.zeros(hid, dtype=torch.float64)
                c = c0[i, di * hid:(di + 1) * hid, qi].double().clone() if c0 is not None else torch.zeros(hid, dtype=torch.float64)
                for s in (range(sn) if di == 0 else range(sn - 1, -1, -1)):
                    f = qi * qs + s * ss
                    pre = gx[i, di * 4 * hid:(di + 1) * 4 * hid, f] + h @ w[di]
                    assert bool(torch.isfinite(pre).all())        # no live step reads the NaN behind a row's end
                    gi, gf, gg, go = pre.split(hid)
                    c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
                    h = torch.sigmoid(go) * torch.tanh(c)
                    hout[i, di * hid:(di + 1) * hid, f] = h
                for s in range(sn, steps):
                    hout[i, di * hid:(di + 1) * hid, qi * qs + s * ss] = 0.0
                h_last[i, di * hid:(di + 1) * hid, qi], c_last[i, di * hid:(di + 1) * hid, qi] = h, c
    return hout, h_last, c_last


def _problem(hid, d, walk, seed):
    q, qs, steps, ss, ldt = walk
    n = len(STEPS_ROWS)
    gx = rand((n, d * 4 * hid, ldt), seed) * 2.0
    for i, sn in enumerate(_clamped()):          # NaN behind each row's own last step (and in the frames no step visits)
        live = torch.zeros(ldt, dtype=torch.bool)
        for qi in range(q):
            for s in range(sn):
                live[qi * qs + s * ss] = True
        gx[i][:, ~live] = NAN
    whh_t = rand((d, hid, 4 * hid), seed + 1) * (hid ** -0.5)
    return gx, whh_t


@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("hid", [64, 192, 256])
def test_lstm_rows_walks_each_utterances_own_steps(H, dev, hid, d, walk):
    q, qs, steps, ss, ldt = WALKS[walk]
    n = len(STEPS_ROWS)
    gx, whh_t = _problem(hid, d, WALKS[walk], 4100 + hid + d)
    ldq = 8
    h0 = torch.zeros(n, d * hid, ldq)
    c0 = torch.zeros(n, d * hid, ldq)
    h0[..., :q], c0[..., :q] = rand((n, d * hid, q), 4200 + hid) * 0.9, rand((n, d * hid, q), 4300 + hid) * 1.5
    rows = torch.tensor(STEPS_ROWS, dtype=torch.int32, device=dev)
    gxd, wd = gx.to(dev), whh_t.to(dev)
    for states in (False, True):
        hd, cd = (h0.to(dev), c0.to(dev)) if states else (None, None)
        out = torch.full((n, d * hid, ldt), SENTINEL, device=dev)
        got, (hl, cl) = H.lstm_rows(gxd, wd, hid, d, q, qs, steps, ss, rows, hd, cd, want_state=True, out=out)
        assert got is out
        ref, rh, rc = _reference(gx, whh_t, hid, d, WALKS[walk], h0 if states else None, c0 if states else None)
        got = got.cpu()
        written = ref != SENTINEL
        # frames the walk does not visit keep the sentinel; the steps behind a row's end hold exact zeros
        assert torch.equal(got[~written], torch.full_like(got[~written], SENTINEL)), (hid, d, walk, states)
        zeros = written & (ref == 0.0)
        assert zeros.any() and float(got[zeros].abs().max()) == 0.0
        assert bool(torch.isfinite(got).all())
        e = [rel_max(got[written].double().numpy(), ref[written].numpy()),
             rel_max(hl[..., :q].cpu().double().numpy(), rh.numpy()), rel_max(cl[..., :q].cpu().double().numpy(), rc.numpy())]
        print(f"lstm_rows H={hid} D={d} {walk} states={states}: hout {e[0]:.2e} h_last {e[1]:.2e} c_last {e[2]:.2e}")
        assert max(e) < FP32, e
        # s_n = 0: the final states are the initial ones (or zeros), bit for bit
        for i, sn in enumerate(_clamped()):
            if sn == 0:
                want = (h0[i, :, :q], c0[i, :, :q]) if states else (torch.zeros(d * hid, q),) * 2
                assert torch.equal(hl[i, :, :q].cpu(), want[0]) and torch.equal(cl[i, :, :q].cpu(), want[1])
        if hid > 64:
            # the plain entry runs the same kernel at these sizes: row n alone with steps = s_n, bit for bit
            for i, sn in enumerate(_clamped()):
                if sn == 0:
                    continue
                alone, (ah, ac) = H.lstm(gxd[i:i + 1], wd, hid, d, q, qs, sn, ss,
                                         None if hd is None else hd[i:i + 1], None if cd is None else cd[i:i + 1],
                                         want_state=True, out=torch.full((1, d * hid, ldt), SENTINEL, device=dev))
                live = (alone != SENTINEL)[0]
                assert torch.equal(out[i][live], alone[0][live]), (hid, d, walk, states, i)
                assert torch.equal(hl[i, :, :q], ah[0, :, :q]) and torch.equal(cl[i, :, :q], ac[0, :, :q])


def test_lstm_rows_refuses_what_the_wrapper_can_see(H, dev):
    gx = torch.zeros(2, 4 * 64, 40, device=dev)
    w = torch.zeros(1, 64, 256, device=dev)
    rows = torch.tensor([3, 4], dtype=torch.int32, device=dev)
    with pytest.raises((RuntimeError, ValueError)):
        H.lstm_rows(gx, w, 64, 1, 1, 0, 27, 1, rows.long())
    with pytest.raises((RuntimeError, ValueError)):
        H.lstm_rows(gx, w, 64, 1, 1, 0, 27, 1, rows[:1])
    with pytest.raises(RuntimeError, match="last frame"):
        H.lstm_rows(gx, w, 64, 1, 1, 0, 41, 1, rows)
