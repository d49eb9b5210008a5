"""A result is a function of the inputs and the weights only: not of what a kept scratch buffer held before the call, and
not of which other lane is running.  Three kinds of scratch live from call to call -- the workspaces ConvTasNet and the
wrapper keep per lane (the fused masker driver's hidden maps, fp64 statistics partials, bias_n and range maxima,
re-carved at other offsets whenever a smaller (N, T) reuses them) and the zeroed LSTM output rows of DPCRN / DPARN
(_plans._h_rows) -- and none of them is reached by NaN in the caching allocator: they are zero-filled when created.

1. the driver (hip.conv_tasnet(..., workspace=)) on a workspace of zeros, of 0xFF bytes (NaN as fp32 and as fp64), of the fp32
   value 1e30 (a huge finite sum as fp64, a huge finite maximum as fp32) and on a dirty one of twice the size: the same bits.
   The workspace holds floats and doubles only, so none of this can move an address.  (The cooperative LSTM's workspace
   holds barrier counters its launcher initialises; it is left alone.)
2. one model instance over a sequence of (B, L) shapes against a freshly built model at every step: the same bits.
   And one model on freed memory full of NaN, of constants and of noise of several sizes: the same bits.
3. two lanes (hip_streams = 2) against one lane on each half: the same bits, and no byte of kept scratch handed to
   launches on two streams within one call.  (A preset that inference() runs in one lane whatever hip_streams says: the
   same bits as with hip_streams = 1, and each half inside the bound batch independence has in the split arithmetics.)

No tolerance is new: bit equality is torch.equal, and every comparison with the float64 oracle names the test of the same
preset and arithmetic it takes its bound from."""
import functools
import inspect
import itertools

import numpy as np
import pytest
import torch

import cases
from conftest import rel_max
from detweights import det_state_dict, det_tensor, det_wave
from oracle import separator_oracle as O
from puresound_amd import _abi
from test_hip_parity import TOL

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def H():
    from puresound_amd import hip
    hip.lib()
    return hip


@pytest.fixture(scope="module")
def PA():
    import puresound_amd.nnet as PA
    return PA


def _fill_allocator_cache(dev, value):
    junk = [torch.full((1 << 22,), value, device=dev) for _ in range(16)]
    junk += [torch.full((n,), value, device=dev) for n in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20)]
    del junk


@pytest.fixture(autouse=True)
def _nan_in_the_allocator_cache(dev):
    """NaN-filled blocks in torch's caching allocator: a "fresh" buffer (`torch.empty` scratch, outputs, pad frames) is
    never accidentally clean."""
    _fill_allocator_cache(dev, NAN)
    yield


def _l2rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ------------------------------------------------------------------------------------------------
# 1. dirty workspace at the driver
# ------------------------------------------------------------------------------------------------
# one frame inside and one frame past the row lengths 128 and 384 (ps_padded_frames), an even and an odd batch
DRIVER_SHAPES = [(n, t) for n in (2, 3) for t in (100, 129, 385)]
PLANES = {"fp32": 0, "bf16x3": 3, "fp16x2": 2, "bf16": 1}
# (what, PS_DBG_* switches, cap of the persistent GEMM grids): kernel choices a full batch makes, forced at these sizes
SETTINGS = [("persistent GEMM grids of 5 workgroups", _abi.PS_DBG_GEMM_ANY_SIZE, 5),
            ("persistent GEMM grids of 5 workgroups, no register-B kernel", _abi.PS_DBG_GEMM_ANY_SIZE | _abi.PS_DBG_GEMM_NO_RB, 5),
            ("the workgroup depthwise kernel", _abi.PS_DBG_DWCONV_WG, 0)]
BN_DILATION = 8


@functools.lru_cache(maxsize=None)
def _driver_masker(case):
    """-> (modules in execution order, C, H, E, embed_norm, oracle(x, dvec)) for a driver case, weights by det_state_dict:
    the masker of tiny_free (plain gLN blocks), ctn_embed (bias_n, embed_norm) and one causal bN1d block, built as
    test_bn_block_in_fp16x2_over_input_scales builds it (its fp16x2 form leaves measured maxima in statistics slots)."""
    import puresound_amd.nnet as PA
    import puresound_amd.nnet.conv_tasnet as CT
    if case == "bn_block":
        blk = CT.TCN(256, 512, 3, BN_DILATION, causal=True, tcn_norm="bN1d", dconv_norm="bN1d").eval()
        sd = det_state_dict(blk, mode="wild")
        blk.load_state_dict(sd)
        return [blk], 256, 512, 0, False, lambda x, dvec: O.tcn_block(x, sd, "", 3, BN_DILATION, True, "bN1d", "bN1d")
    spec = cases.CASES[case]["masker"]
    m = cases.build_masker(PA.NS, spec).eval()
    sd = det_state_dict(m)
    m.load_state_dict(sd)
    args = cases.full_masker_args(spec)
    return ([b for stack in m.tcn_list for b in stack], m.input_dim, m.tcn_dim, m.embed_dim if any(m.tcn_with_embed) else 0,
            bool(m.embed_norm), lambda x, dvec: O.conv_tasnet(x, sd, "", args, dvec))


@functools.lru_cache(maxsize=None)
def _driver_problem(case, n, t):
    """-> (x [N, C, T], dvec [N, E] or None, the float64 oracle's output); computed once per case and shape"""
    _, c, _, e, _, oracle = _driver_masker(case)
    x = det_wave(900 + n, n * c, t).reshape(n, c, t) * 2.0
    dvec = det_wave(901 + n, n, e) + 0.1 if e else None
    with torch.no_grad():
        ref = oracle(x.double(), None if dvec is None else dvec.double())
    assert ref.dtype == torch.float64 and ref.shape == x.shape
    return x, dvec, ref


def _workspaces(H, dev, n, c, h, t):
    """the four workspaces of section 1: zeros, 0xFF bytes, fp32 1e30, and twice the size with every byte dirty"""
    need = H.lib().ps_conv_tasnet_workspace_bytes(n, c, h, t)
    assert need > 0 and need % 4 == 0
    return {"zeros": torch.zeros(need, dtype=torch.uint8, device=dev),
            "0xFF": torch.full((need,), 0xFF, dtype=torch.uint8, device=dev),
            "1e30": torch.full((need // 4,), 1e30, dtype=torch.float32, device=dev).view(torch.uint8),
            "twice the size, 0xFF": torch.full((2 * need,), 0xFF, dtype=torch.uint8, device=dev)}


# "bf16": the bf16-rows entry with hidden_bf16 (hidden maps and residual stream as bf16 rows)
@pytest.mark.parametrize("case,arith", [(c, a) for c in ("tiny_free", "ctn_embed", "bn_block")
                                        for a in ("fp32", "bf16x3", "fp16x2")] + [("tiny_free", "bf16"), ("ctn_embed", "bf16")])
def test_driver_result_does_not_depend_on_the_workspace_contents(H, dev, case, arith):
    mods, c, h, e, embed_norm, _ = _driver_masker(case)
    for m in mods:
        m.to(dev)
        m.gemm_precision = arith
    # the planes the plan ran with: a silent fall-back to another arithmetic would empty the case
    assert all(m.gemm_planes_for_plan() == PLANES[arith] for m in mods)
    plans = [m.plan(dev) for m in mods]
    blocks = (_abi.TcnBlock * len(plans))(*[p["block"] for p in plans])
    assert all(p["fused"] and blocks[i].gemm_planes == PLANES[arith] for i, p in enumerate(plans))
    rows_bf16 = arith == "bf16"
    assert all(bool(blocks[i].hidden_bf16) == rows_bf16 and p["rows_bf16"] == rows_bf16 for i, p in enumerate(plans))
    for n, t in DRIVER_SHAPES:
        x, dvec, ref = _driver_problem(case, n, t)
        x_pad = H.pad_rows(x.to(dev))
        x_pad[..., t:] = NAN            # frames past T are undefined on the way in, too
        dv = None if dvec is None else dvec.to(dev)
        outs = {}
        for what, ws in _workspaces(H, dev, n, c, h, t).items():
            assert H.conv_tasnet_workspace(n, c, h, t, dev, ws) is ws           # the driver runs on THIS buffer
            y = H.conv_tasnet(blocks, len(plans), x_pad, t, c, h, dv, embed_norm, workspace=ws, bf16_rows=rows_bf16)
            torch.cuda.synchronize()
            outs[what] = y[..., :t].clone()
        clean = outs["zeros"]
        got, want = clean.cpu().double().numpy(), ref.numpy()
        err = _l2rel(got, want) if rows_bf16 else rel_max(got, want)
        print(f"{case} [{arith}] N={n} T={t}: {'l2-rel' if rows_bf16 else 'rel-max'} error against float64 {err:.3e}, "
              + ", ".join(f"{k}: {'same bits' if torch.equal(v, clean) else 'DIFFERENT'}" for k, v in outs.items()))
        assert bool(torch.isfinite(clean).all()), (n, t)
        if rows_bf16:
            assert err < 3e-2, (n, t)             # test_config3_with_the_residual_stream_in_bf16 (l2-rel)
        else:
            assert err < TOL, (n, t)              # test_masker_matches_reference_golden / test_conv_tasnet_on_the_bf16_matrix_pipe
        for what, y in outs.items():
            assert torch.equal(y, clean), f"N={n} T={t}: a workspace of {what} changes the result"
        # The kernels a full batch runs, at this size: the persistent GEMM grids (PS_DBG_GEMM_ANY_SIZE), capped so that a
        # workgroup's run spans several tiles and utterances and the last workgroups' runs are empty, with and without the
        # register-B kernel, and the workgroup depthwise kernel.  Other kernels, other bits: each against its own clean run.
        for what, flags, cap in SETTINGS:
            pair = []
            for ws in list(_workspaces(H, dev, n, c, h, t).values())[:2]:
                with _abi.debug(flags, grid_cap=cap):
                    y = H.conv_tasnet(blocks, len(plans), x_pad, t, c, h, dv, embed_norm, workspace=ws, bf16_rows=rows_bf16)
                    torch.cuda.synchronize()
                pair.append(y[..., :t].clone())
            got = pair[0].cpu().double().numpy()
            assert (_l2rel(got, want) < 3e-2) if rows_bf16 else (rel_max(got, want) < TOL), (n, t, what)   # (as above)
            assert torch.equal(pair[0], pair[1]), f"N={n} T={t}, {what}: a workspace of 0xFF changes the result"
    if case == "bn_block" and arith != "fp32":
        # a batch whose GEMMs fill the persistent grids by themselves, with tiles left over: 65 x 4 x 2 tiles of 128 frames x
        # 256 channels for at most 512 workgroups.  Bits only.
        n, t = 65, 385
        x_pad = H.pad_rows((det_wave(990, n * c, t).reshape(n, c, t) * 2.0).to(dev))
        pair = []
        for ws in list(_workspaces(H, dev, n, c, h, t).values())[:2]:
            y = H.conv_tasnet(blocks, len(plans), x_pad, t, c, h, None, embed_norm, workspace=ws)
            torch.cuda.synchronize()
            pair.append(y[..., :t].clone())
        assert bool(torch.isfinite(pair[0]).all()) and torch.equal(pair[0], pair[1])
    if case == "bn_block" and arith == "fp16x2":
        # the measured maxima through the norm against exact fp32 products (test_bn_block_in_fp16x2_over_input_scales)
        n, t = DRIVER_SHAPES[-1]
        x, _, _ = _driver_problem(case, n, t)
        y16 = H.conv_tasnet(blocks, 1, H.pad_rows(x.to(dev)), t, c, h, None, False)[..., :t].cpu().numpy()
        mods[0].gemm_precision = "fp32"
        exact = H.conv_tasnet((_abi.TcnBlock * 1)(mods[0].plan(dev)["block"]), 1, H.pad_rows(x.to(dev)), t, c, h, None, False)
        assert rel_max(y16, exact[..., :t].cpu().numpy()) < 4e-6


@pytest.mark.parametrize("arith", ["fp32", "fp16x2"])
def test_staged_cln_masker_keeps_no_scratch(PA, H, dev, arith):
    """tcn_cln (causal, cLN everywhere) has no fused form: ConvTasNet runs it block by block, stage by stage, on
    `torch.empty` maps of its own, and keeps nothing.  So the driver's workspace is not what this case can dirty: its
    scratch is the allocator's, filled with NaN and then with 1e30 -- the same bits, and no workspace kept."""
    model = cases.build(PA.NS, "tcn_cln").eval()
    sd = det_state_dict(model)
    model.load_state_dict(sd)
    model.to(dev)
    model.set_gemm_precision(arith)
    mods = [m for stack in model.tcn_list for m in stack]
    assert not any(m.plan(dev)["fused"] for m in mods)
    assert all(m.gemm_planes_for_plan() == (0 if arith == "fp32" else 3) for m in mods)   # (cLN: fp16x2 plans bf16x3)
    args = cases.full_masker_args(cases.CASES["tcn_cln"]["masker"])
    for n, t in DRIVER_SHAPES:
        x = det_wave(910 + n, n * 16, t).reshape(n, 16, t) * 2.0
        with torch.no_grad():
            ref = O.conv_tasnet(x.double(), sd, "", args)
        x_pad = H.pad_rows(x.to(dev))
        x_pad[..., t:] = NAN
        outs = []
        for junk in (NAN, 1e30):
            _fill_allocator_cache(dev, junk)
            outs.append(model.forward_padded(x_pad, t)[..., :t].clone())
            torch.cuda.synchronize()
        assert model.kept_scratch() == []
        assert rel_max(outs[0].cpu().double().numpy(), ref.numpy()) < TOL, (n, t)    # test_masker_matches_reference_golden
        assert torch.equal(outs[0], outs[1]), (n, t)


# ------------------------------------------------------------------------------------------------
# 2. one model instance over a sequence of shapes
# ------------------------------------------------------------------------------------------------
# name -> ((L1, L2, L3), enrolment lengths or None).  L1 is the preset's length, L2 gives 20 frames fewer inside the same
# row length (ps_padded_frames: 128, 384, 640, ...), L3 another row length: a smaller one where there is one, else (the
# preset already sits in the smallest, or the segment padding allows no smaller) a larger one, which the steps after it
# then re-carve for the smaller shapes.  Frames T = (L - win) // hop + 1; rows = ps_padded_frames(what the masker needs):
#   tiny_free          win 16, hop 8:    T = 124, 104 (rows 128); 249 (rows 384)
#   cfg3_short         win 32, hop 16:   T = 249, 229 (rows 384); 100 (rows 128); the enrolment has the same lengths
#   cfg4_short         segments of 20:   T = 249, 229 -> 260, 240 padded (rows 384); 100 -> 120 (rows 128)
#   tse_skim_v0_short  segments of 150:  T = 249, 229 -> 300 (rows 384); 400 -> 450 (rows 640); enrolment T = 186, 166 (rows
#                      384), 100 (rows 128)
#   the STFT presets   n_fft 512, hop 128: T = 28, 8 (rows 128: the 2-D maps hold F rows of them); 150 (rows 384);
#                      tse_unet_tcn_short's enrolment T = 20, 10 (rows 128), 150 (rows 384)
SEQUENCES = {
    "tiny_free": ((1003, 843, 2000), None),
    "cfg3_short": ((4000, 3680, 1616), (4000, 3680, 1616)),
    "cfg4_short": ((4000, 3680, 1616), None),
    "tse_skim_v0_short": ((4000, 3680, 6416), (3000, 2680, 1616)),
    "ns_dpcrn_short": ((4000, 1440, 19584), None),
    "ns_dparn_short": ((4000, 1440, 19584), None),
    "tse_unet_tcn_short": ((4000, 1440, 19584), (3000, 1720, 19584)),
}


@functools.lru_cache(maxsize=None)
def _state_dict(name):
    import puresound_amd.nnet as PA
    return det_state_dict(cases.build(PA.NS, name).eval())


def _model(PA, dev, name, arith=None, sd=None):
    """a freshly built model of the preset: no plan, no kept scratch, its first call still ahead"""
    model = cases.build(PA.NS, name).eval()
    model.load_state_dict(_state_dict(name) if sd is None else sd)
    model.to(dev)
    if arith is not None:
        model.masker.set_gemm_precision(arith)
    return model


def _infer(model, noisy, enroll):
    out = model.inference(noisy) if enroll is None else model.inference(noisy, enroll)
    torch.cuda.synchronize()
    return out


def _oracle_error(name, out, noisy, enroll, sd=None):
    """rel-max against the float64 oracle as the preset's own parity test measures it (STFT: 16 samples off each edge)"""
    with torch.no_grad():
        ref = O.inference(noisy.cpu().double(), _state_dict(name) if sd is None else sd, cases.oracle_cfg(name),
                          None if enroll is None else enroll.cpu().double())
    sl = slice(16, ref.shape[1] - 16) if cases.CASES[name]["enc"]["kind"] == "stft" else slice(None)
    return rel_max(out.cpu().double().numpy()[:, sl], ref.numpy()[:, sl])


class _HRowsSpy:
    """what _plans._h_rows hands out while `on`: the tensors themselves (held, so that no address comes back for another)"""

    def __init__(self, monkeypatch):
        from puresound_amd.nnet import _plans
        self.on, self.calls = False, []
        orig = _plans._h_rows

        def spy(*a, **kw):
            buf = orig(*a, **kw)
            if self.on and buf is not None:
                self.calls.append(buf)
            return buf
        monkeypatch.setattr(_plans, "_h_rows", spy)

    def kept(self, before):
        """how many of the buffers handed out since call number `before` had been handed out earlier"""
        return sum(any(b is a for a in self.calls[:before]) for b in self.calls[before:])


@pytest.mark.parametrize("name,arith", [("tiny_free", "fp32"), ("tiny_free", "bf16x3"), ("tiny_free", "fp16x2"),
                                        ("cfg3_short", None), ("cfg4_short", None), ("tse_skim_v0_short", None),
                                        ("ns_dpcrn_short", None), ("ns_dparn_short", None), ("tse_unet_tcn_short", None)])
def test_one_model_over_a_sequence_of_shapes_equals_fresh_models(PA, dev, monkeypatch, name, arith):
    c = cases.CASES[name]
    (l1, l2, l3), enrolments = SEQUENCES[name]
    assert l1 == c["L"] and (enrolments is None or enrolments[0] == c["L_enroll"])
    e1, e2, e3 = enrolments or (None, None, None)
    b = c["B"]
    spy = _HRowsSpy(monkeypatch)
    model = _model(PA, dev, name, arith)
    if arith is not None:
        assert all(m.gemm_planes_for_plan() == PLANES[arith] for stack in model.masker.tcn_list for m in stack)
    steps = [(b, l1, e1), (b, l2, e2), (b, l3, e3), (b + 1, l1, e1), (1, l1, e1), (b, l1, e1)]
    kept_rows = 0
    for i, (n, length, le) in enumerate(steps):
        seed = c["seed"] if i in (0, len(steps) - 1) else 700 + 10 * i      # first and last: the preset's own input
        noisy = det_wave(seed, n, length).to(dev)
        enroll = None if le is None else det_wave(seed + 1, n, le).to(dev)
        before = len(spy.calls)
        spy.on = True
        out = _infer(model, noisy, enroll)
        spy.on = False
        kept_rows += spy.kept(before)
        fresh = _infer(_model(PA, dev, name, arith), noisy, enroll)
        assert bool(torch.isfinite(out).all()), (i, n, length)
        assert torch.equal(out, fresh), (f"step {i} (B={n}, L={length}): the model that ran {steps[:i]} before differs from a "
                                         f"fresh one by {float((out - fresh).abs().max()):.3e}")
    err = _oracle_error(name, out, noisy, enroll)
    print(f"{name} [{arith or 'default'}]: rel-max error of the last call against float64 {err:.3e}; kept LSTM rows handed "
          f"out again {kept_rows} times")
    # test_results_do_not_depend_on_uninitialised_memory (all three arithmetics of tiny_free), test_tse_wrapper_ /
    # test_dprnn_wrapper_ / test_more_tse_presets_ / test_ns_dpcrn_preset_matches_reference_golden
    assert err < TOL
    if name in ("ns_dpcrn_short", "ns_dparn_short"):
        assert kept_rows > 0, "no call ran on LSTM output rows kept from an earlier one: the case proves nothing"


def _junk_in_freed_memory(dev, value, seed=None):
    """3.5 GiB of `value` -- with a seed: of normal noise times `value`, as an earlier forward's activations are -- back
    into an emptied allocator cache: what `torch.empty` then hands out holds it"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    if seed is None:
        fill = lambda n: torch.full((n,), value, device=dev)  # noqa: E731
    else:
        g = torch.Generator(device=dev).manual_seed(seed)
        fill = lambda n: torch.randn(n, device=dev, generator=g) * value  # noqa: E731
    # blocks of 1 GiB, 256 MiB and 64 MiB: a 16-utterance forward asks for single buffers of 200 MB, which only a block of
    # that size can give back
    junk = [fill(1 << 28) for _ in range(2)] + [fill(1 << 26) for _ in range(4)] + [fill(1 << 24) for _ in range(8)]
    junk += [fill(n) for n in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20)]
    torch.cuda.synchronize()
    del junk


@pytest.mark.parametrize("batch", ["preset", 16])
@pytest.mark.parametrize("name", ["tiny_free", "cfg3_short", "cfg4_short", "tse_skim_v0_short", "ns_dpcrn_short",
                                  "ns_dparn_short", "tse_unet_tcn_short"])
def test_result_does_not_depend_on_what_freed_memory_holds(PA, dev, name, batch):
    """NaN in `torch.empty` memory is the kind of junk a maximum ignores; what earlier work leaves there is mostly finite.
    A pad frame that no launch wrote and a range maximum runs over shows with finite junk only: values of the
    activations' own size, constant and noise, tiny and huge ones, against the run on NaN -- the same bits."""
    c = cases.CASES[name]
    n = c["B"] if batch == "preset" else batch
    model = _model(PA, dev, name)
    noisy = det_wave(c["seed"] + 70, n, c["L"]).to(dev)
    enroll = det_wave(c["seed"] + 71, n, c["L_enroll"]).to(dev) if "L_enroll" in c else None
    _junk_in_freed_memory(dev, NAN)
    want = _infer(model, noisy, enroll).clone()
    assert bool(torch.isfinite(want).all())
    for junk, seed in ((3.0, None), (-37.0, None), (1e30, None), (1.0, 1), (30.0, 2), (1e4, 3), (1e-3, 4)):
        _junk_in_freed_memory(dev, junk, seed)
        got = _infer(model, noisy, enroll)
        assert torch.equal(got, want), (f"freed memory full of {'noise times ' if seed else ''}{junk} changes the result by "
                                        f"{float((got - want).abs().max()):.3e}")


# ------------------------------------------------------------------------------------------------
# 3. lanes
# ------------------------------------------------------------------------------------------------
class _ScratchRecorder:
    """Wraps the hip wrappers that take kept scratch -- conv_tasnet(workspace=), and out= of lstm / lstm_fmajor /
    lstm_fmajor_h256 -- and records (wrapper, stream, byte range, the buffer) of every call."""
    TAKES = (("conv_tasnet", "workspace"), ("lstm", "out"), ("lstm_fmajor", "out"), ("lstm_fmajor_h256", "out"))

    def __init__(self, monkeypatch, H):
        self.calls = []
        for fn, arg in self.TAKES:
            monkeypatch.setattr(H, fn, self._wrap(getattr(H, fn), fn, arg))

    def _wrap(self, orig, fn, arg):
        sig = inspect.signature(orig)

        def wrapped(*a, **kw):
            buf = sig.bind(*a, **kw).arguments.get(arg)
            rng = None if buf is None else (buf.data_ptr(), buf.data_ptr() + buf.numel() * buf.element_size())
            self.calls.append((fn, torch.cuda.current_stream().cuda_stream, rng, buf))
            return orig(*a, **kw)
        return wrapped

    def watch(self, obj, method):
        """record the stream of every call of obj.method, which takes no kept scratch itself"""
        orig = getattr(obj, method)

        def wrapped(*a, **kw):
            self.calls.append((method, torch.cuda.current_stream().cuda_stream, None, None))
            return orig(*a, **kw)
        setattr(obj, method, wrapped)

    def streams(self):
        return {s for _, s, _, _ in self.calls}

    def shared(self):
        """messages, one per byte range of kept scratch that launches on two different streams were handed"""
        held = [(fn, s, rng) for fn, s, rng, _ in self.calls if rng is not None]
        return sorted({f"{fa} on stream {sa:#x} and {fb} on stream {sb:#x} are handed the same kept scratch: bytes "
                       f"[{max(ra[0], rb[0]):#x}, {min(ra[1], rb[1]):#x})"
                       for (fa, sa, ra), (fb, sb, rb) in itertools.combinations(held, 2)
                       if sa != sb and ra[0] < rb[1] and rb[0] < ra[1]})


# name -> lanes inference() really runs with hip_streams = 2 on 16 utterances.  One for the STFT presets (the STFT branch
# of SoTaskWrapModule._inference returns before the split) and for a causal SkiM (its Mem-LSTM hand-over runs from one
# utterance of the batch into the next, so the batch stays in one piece).
LANES = {"cfg3_short": 2, "cfg4_short": 2, "tse_skim_v0_short": 2, "ns_dpcrn_short": 1, "ns_dparn_short": 1,
         "tse_unet_tcn_short": 1, "tse_skim_causal_short": 1}


@pytest.mark.parametrize("name", list(LANES))
def test_two_lanes_equal_one_lane_on_each_half_and_share_no_scratch(PA, H, dev, monkeypatch, name):
    c = cases.CASES[name]
    model = _model(PA, dev, name)
    noisy = det_wave(c["seed"] + 50, 16, c["L"]).to(dev)
    enroll = det_wave(c["seed"] + 51, 16, c["L_enroll"]).to(dev) if "L_enroll" in c else None
    rec = _ScratchRecorder(monkeypatch, H)
    rec.watch(model.masker, "forward_padded")     # (every family, whatever scratch its masker takes)
    model.hip_streams = 2
    two = _infer(model, noisy, enroll)
    assert bool(torch.isfinite(two).all())
    assert len(rec.streams()) == LANES[name], f"{name}: launches on {len(rec.streams())} streams"
    shared = rec.shared()
    assert not shared, f"{name}: " + "; ".join(shared)
    model.hip_streams = 1
    if LANES[name] == 1:
        # one lane whatever hip_streams says: the same launches, the same bits
        again = _infer(model, noisy, enroll)
        assert torch.equal(again, two), (f"{name}: hip_streams = 1 and 2 run the same launches on the same 16 utterances and "
                                         f"differ by {float((again - two).abs().max()):.3e}")
        if name == "tse_skim_causal_short":
            return   # (rows 8.. of the whole batch carry utterance 7's segment state, those of the half do not)
    else:
        # each half as one lane runs it: the same launches (the lanes keep off the cooperative LSTM, so do these)
        monkeypatch.setattr(H, "COOP_LSTM", False)
    for sl in (slice(0, 8), slice(8, 16)):
        one = _infer(model, noisy[sl], None if enroll is None else enroll[sl])
        diff = float((two[sl] - one).abs().max())
        print(f"{name}: rows {sl.start}..{sl.stop - 1} of 16 against their own batch of 8: max |difference| {diff:.3e}")
        if LANES[name] == 2:
            # the half is what its lane ran, launch for launch: the same bits
            assert torch.equal(two[sl], one), f"{name}: rows {sl.start}..{sl.stop - 1} differ by {diff:.3e}"
        else:
            # one lane ran all 16: a launch of 16 utterances may take another kernel than one of 8 (the GEMM and recurrence
            # kernels are chosen by the size of the launch), the same sums in another order -- a row against its run in a
            # smaller batch, in the split arithmetics: test_full_size_properties_of_the_other_baseline_configs
            assert diff <= 1e-5, f"{name}: rows {sl.start}..{sl.stop - 1} differ by {diff:.3e}"


@pytest.mark.parametrize("name", ["ns_dpcrn_short", "ns_dparn_short"])
def test_recurrent_bottleneck_keeps_its_lstm_rows_per_lane(PA, H, dev, monkeypatch, name):
    """The wrapper never splits an STFT preset, so the lane argument of DPCRN / DPARN is exercised here as inference()
    would: the two halves of 16 utterances through masker.forward_padded(..., lane=i) on two streams."""
    c = cases.CASES[name]
    model = _model(PA, dev, name)
    noisy = det_wave(c["seed"] + 60, 16, c["L"]).to(dev)
    feats, t = model.encoder.encoder.encode_padded(noisy, model.drop_first_bin)
    halves = [feats[:8].contiguous(), feats[8:].contiguous()]
    one = [model.masker.forward_padded(h, t, None, lane=0)[..., :t].clone() for h in halves]   # (also builds every plan)
    torch.cuda.synchronize()
    spy = _HRowsSpy(monkeypatch)
    rec = _ScratchRecorder(monkeypatch, H)
    cur = torch.cuda.current_stream(dev)
    pool = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    two = []
    spy.on = True
    for i, s in enumerate(pool):
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            two.append(model.masker.forward_padded(halves[i], t, None, lane=i))
    for s in pool:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    assert spy.calls and len(rec.streams()) == 2
    shared = rec.shared()
    assert not shared, f"{name}: " + "; ".join(shared)
    for i in range(2):
        assert torch.equal(two[i][..., :t], one[i]), i


# ------------------------------------------------------------------------------------------------
# plans follow weights replaced off the device
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_free", "cfg4_short"])
def test_plans_follow_weights_replaced_off_the_device(PA, dev, name):
    """to(device), inference, cpu(), load_state_dict of other weights, to(device), inference: the plans are keyed on
    (data_ptr, _version) of the parameters, and the allocator may well hand the new ones the old addresses."""
    c = cases.CASES[name]
    model = _model(PA, dev, name)
    noisy = det_wave(c["seed"], c["B"], c["L"]).to(dev)
    first = _infer(model, noisy, None)
    # test_wrapper_inference_ / test_dprnn_wrapper_matches_reference_golden, here and below
    assert _oracle_error(name, first, noisy, None) < TOL
    model.cpu()
    torch.cuda.empty_cache()
    other = {k: det_tensor("other." + k, v) for k, v in _state_dict(name).items()}    # (the key's last part picks the law)
    model.load_state_dict(other)
    model.to(dev)
    second = _infer(model, noisy, None)
    assert not torch.equal(first, second)
    assert _oracle_error(name, second, noisy, None, other) < TOL
