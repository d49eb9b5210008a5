"""The Python side of the Conv-TasNet masker driver on the GPU: what TCN.plan() packs in each arithmetic, and what
hip.conv_tasnet refuses before it allocates its output.

TCN.plan: the ps_tcn_block of a TCN(8, 4, 3, 2) in the four gemm_precisions and in the bf16-rows form is compared, pointer
fields masked, with a block filled in here field by field; its weight images, exponents and bounds with what hip.py's
packing functions (pack_wt / pack_wt_bf16 / pack_wt_f16x2) give for the same weights in the same run.

hip.conv_tasnet: operands the C call would take as wild pointers or mis-sized arrays (dvec, workspace, x_pad).  The wrapper
passed these on before it had an operand check; each must now raise RuntimeError with torch.empty_like and torch.zeros
(the output, a new workspace) never called."""
import ctypes as C

import pytest
import torch

from puresound_amd import _abi

pytestmark = pytest.mark.gpu
N, CH, H, T, LDT, E = 2, 8, 4, 100, 128, 6
POINTERS = [name for name, kind in _abi.TcnBlock._fields_ if kind is C.c_void_p]
# form -> (gemm_precision, stream_bf16, gemm_planes, hidden_bf16, the fields that hold fp16 images)
FORMS = {
    "fp32": ("fp32", True, 0, 0, ()),
    "bf16x3": ("bf16x3", True, 3, 0, ()),
    "fp16x2": ("fp16x2", True, 2, 0, ("in_wb", "pw_wb", "out_wb")),
    "bf16": ("bf16", False, 1, 1, ()),
    "bf16_rows": ("bf16", True, 1, 1, ("in_wf", "pw_wf", "out_wf")),
}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _tcn(dev, dilation, emb_dim=0):
    from puresound_amd.nnet.conv_tasnet import TCN
    torch.manual_seed(11 + dilation)
    m = TCN(CH, H, 3, dilation, emb_dim=emb_dim).eval()
    with torch.no_grad():   # norms and slopes away from their initial 1 / 0 / 0.25, one slope beyond 1
        for p in m.parameters():
            p.copy_(torch.rand_like(p) * 2 - 1)
        m.dconv[0].depthwise[2].weight.fill_(-1.5)
    return m.to(dev)


def _masked(block):
    out = _abi.TcnBlock.from_buffer_copy(block)
    for name in POINTERS:
        setattr(out, name, None)
    return bytes(out)


@pytest.mark.parametrize("form", list(FORMS))
def test_plan_packs_what_the_packing_functions_give(dev, form):
    from puresound_amd import hip
    precision, stream_bf16, planes, hidden, images = FORMS[form]
    m = _tcn(dev, 2)
    m.gemm_precision, m.stream_bf16 = precision, stream_bf16
    plan = m.plan(dev)
    block, t = plan["block"], plan["tensors"]
    dsc = m.dconv[0]
    weights = [m.in_conv[0].weight.detach()[:, :CH, 0], dsc.pointwise[0].weight.detach(), m.out_conv.weight.detach()]
    want = _abi.TcnBlock()
    want.C, want.H, want.P, want.dilation, want.causal = CH, H, 3, 2, 0
    want.in_norm = want.dw_norm = want.pw_norm = _abi.PS_NORM_GLOBAL
    want.gemm_planes, want.hidden_bf16 = planes, hidden
    for key, w in zip(("in_wt", "pw_wt", "out_wt"), weights):
        assert torch.equal(t[key], hip.pack_wt(w))
    if planes in (1, 3):
        for key, w in zip(("in_wb", "pw_wb", "out_wb"), weights):
            assert torch.equal(t[key], hip.pack_wt_bf16(w, planes))
    for i, (key, w) in enumerate(zip(images, weights)):
        image, want.w_exp[i] = hip.pack_wt_f16x2(w)
        assert torch.equal(t[key], image)
    if images:
        dw_norm, pw_norm = dsc.depthwise[1], dsc.pointwise[1]
        fd, fp = (max(1.0, abs(float(act.weight.detach()))) for act in (dsc.depthwise[2], dsc.pointwise[2]))
        assert fd == 1.5
        want.dw_gmax, want.dw_bmax = float(dw_norm.weight.abs().max()) * fd, float(dw_norm.bias.abs().max()) * fd
        want.pw_gmax, want.pw_bmax = float(pw_norm.weight.abs().max()) * fp, float(pw_norm.bias.abs().max()) * fp
        assert want.dw_gmax > 0 and want.pw_gmax > 0
    assert _masked(block) == bytes(want)
    held = {name for name in POINTERS if getattr(block, name)}
    assert held == {k for k, v in t.items() if v is not None}
    for name in held:
        assert getattr(block, name) == t[name].data_ptr()
    assert plan["rows_bf16"] == (form == "bf16_rows")


def _stack(dev, emb_dim=0):
    mods = [_tcn(dev, 1, emb_dim), _tcn(dev, 2)]
    for m in mods:
        m.gemm_precision = "fp32"
    plans = [m.plan(dev) for m in mods]
    return (_abi.TcnBlock * 2)(*[p["block"] for p in plans]), plans


def _refusals(dev):
    x = torch.zeros(N, CH, LDT, device=dev)
    dvec = torch.ones(N, E, device=dev)
    big = torch.zeros(1 << 16, device=dev)
    return {
        "dvec_on_the_cpu": dict(dvec=dvec.cpu()),
        "dvec_fp64": dict(dvec=dvec.double()),
        "dvec_strided": dict(dvec=torch.ones(N, 2 * E, device=dev)[:, ::2]),
        "dvec_of_another_E": dict(dvec=torch.ones(N, E - 1, device=dev)),
        "dvec_of_another_N": dict(dvec=torch.ones(N + 1, E, device=dev)),
        "dvec_1d": dict(dvec=torch.ones(E, device=dev)),
        "workspace_fp32": dict(dvec=dvec, workspace=big),
        "workspace_strided": dict(dvec=dvec, workspace=torch.zeros(1 << 17, dtype=torch.uint8, device=dev)[::2]),
        "x_pad_strided": dict(dvec=dvec, x_pad=torch.zeros(N, CH, 2 * LDT, device=dev)[:, :, ::2]),
        "x_pad_transposed": dict(dvec=dvec, x_pad=torch.zeros(N, LDT, CH, device=dev).transpose(1, 2)),
        "x_pad_of_another_C": dict(dvec=dvec, x_pad=torch.zeros(N, CH + 1, LDT, device=dev)),
        "x_pad_2d": dict(dvec=dvec, x_pad=torch.zeros(N * CH, LDT, device=dev)),
        "x_pad_bf16_strided": dict(dvec=dvec, x_pad=torch.zeros(N, CH, 2 * LDT, dtype=torch.bfloat16, device=dev)[:, :, ::2]),
    }, x


REFUSALS = ["dvec_on_the_cpu", "dvec_fp64", "dvec_strided", "dvec_of_another_E", "dvec_of_another_N", "dvec_1d",
            "workspace_fp32", "workspace_strided", "x_pad_strided", "x_pad_transposed", "x_pad_of_another_C", "x_pad_2d",
            "x_pad_bf16_strided"]


@pytest.mark.parametrize("name", REFUSALS)
def test_conv_tasnet_refuses_before_it_allocates(dev, monkeypatch, name):
    from puresound_amd import hip
    blocks, plans = _stack(dev, emb_dim=E)
    cases, x = _refusals(dev)
    assert sorted(cases) == sorted(REFUSALS)
    a = dict(x_pad=x, dvec=None, workspace=None)
    a.update(cases[name])

    def no_allocation(*args, **kwargs):
        raise AssertionError("the output or a workspace was allocated before the refusal")
    monkeypatch.setattr(torch, "empty_like", no_allocation)
    monkeypatch.setattr(torch, "zeros", no_allocation)
    with pytest.raises(RuntimeError, match="conv_tasnet: "):
        hip.conv_tasnet(blocks, 2, a["x_pad"], T, CH, H, a["dvec"], False, a["workspace"])


def test_conv_tasnet_takes_what_it_took(dev):
    """the accepted forms next to the refusals: a [N, E] dvec, a cached workspace (reused when large enough, replaced when too
    small or on another device), and a mis-shaped x_amax still a ValueError"""
    from puresound_amd import hip
    blocks, plans = _stack(dev, emb_dim=E)
    x = torch.randn(N, CH, LDT, device=dev)
    dvec = torch.randn(N, E, device=dev)
    ws = hip.conv_tasnet_workspace(N, CH, H, T, dev)
    assert ws.dtype == torch.uint8 and ws.numel() == hip.lib().ps_conv_tasnet_workspace_bytes(N, CH, H, T) and not ws.any()
    assert hip.conv_tasnet_workspace(N, CH, H, T, dev, ws) is ws
    assert hip.conv_tasnet_workspace(N, CH, H, T // 2, dev, ws) is ws
    grown = hip.conv_tasnet_workspace(2 * N, CH, H, T, dev, ws)
    assert grown is not ws and grown.numel() > ws.numel() and not grown.any()
    assert hip.conv_tasnet_workspace(N, CH, H, T, dev, ws.cpu()).device == ws.device
    a = hip.conv_tasnet(blocks, 2, x, T, CH, H, dvec, False)
    b = hip.conv_tasnet(blocks, 2, x, T, CH, H, dvec, False, ws)
    assert torch.equal(a[..., :T], b[..., :T]) and bool(torch.isfinite(a[..., :T]).all())
    with pytest.raises(ValueError, match="x_amax must be a contiguous"):
        hip.conv_tasnet(blocks, 2, x, T, CH, H, dvec, False, ws, x_amax=torch.ones(N + 1, 4, device=dev))
