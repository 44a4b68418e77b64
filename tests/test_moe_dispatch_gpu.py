"""Fused MoE routing / dispatch / gather / combine kernels (E16) against
float64 references."""

from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

B = 256  # tokens per moe_dispatch workgroup (asserted against the build)


@pytest.fixture(scope="module", autouse=True)
def _check_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vllm_tgis_adapter_amd import ops

    assert ops.has_native(), "HIP extension must be built on a GPU box"
    assert ops.moe_dispatch_block_tokens() == B


def _ref_dispatch(logits, k):
    """float64: stable descending sort picks the experts (ties to the lower
    index), softmax over the picked logits, stable sort of the pairs."""
    e = logits.shape[1]
    vals, ids = torch.sort(logits.double().cpu(), dim=-1, descending=True, stable=True)
    ids = ids[:, :k]
    flat = ids.reshape(-1)
    order = torch.sort(flat, stable=True).indices
    seg = torch.zeros(e + 1, dtype=torch.int64)
    seg[1:] = torch.bincount(flat, minlength=e).cumsum(0)
    pos = torch.empty_like(order)
    pos[order] = torch.arange(order.numel())
    return torch.softmax(vals[:, :k], -1), ids, seg, order // k, pos.view(-1, k)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize(("t", "e", "k", "kind"), [
    (1, 8, 2, "rand"), (5, 4, 2, "rand"), (B + 1, 8, 2, "rand"),
    (3 * B + 7, 64, 8, "rand"), (300, 8, 1, "rand"),
    (37, 8, 2, "bias"),  # every token picks expert 5; some segments empty
    (37, 8, 2, "ties"),  # all-equal rows: the tie rule alone decides
])
def test_moe_dispatch(t, e, k, kind, dtype):
    from vllm_tgis_adapter_amd import ops

    torch.manual_seed(3)
    logits = torch.randn(t, e)
    if kind == "bias":
        logits[:, :3] -= 20
        logits[:, 5] += 20
    if kind == "ties":
        logits[::3] = 0.5
    logits = logits.to(dtype).cuda()
    w, ids, seg, src_row, pos = (o.cpu() for o in ops.moe_dispatch(logits, k))
    rw, rids, rseg, rsrc, rpos = _ref_dispatch(logits, k)
    assert (w.dtype, ids.dtype, seg.dtype) == (torch.float32, torch.int32, torch.int32)
    assert torch.equal(ids.long(), rids)
    assert torch.equal(seg.long(), rseg)
    assert torch.equal(src_row.long(), rsrc)
    assert torch.equal(pos.long(), rpos)
    err = (w.double() - rw).abs().max().item()
    print(f"weights max abs err {err:.3e}")
    assert err <= 1e-5
    assert torch.equal(src_row[pos.long()].long(),
                       torch.arange(t)[:, None].expand(t, k))
    if kind == "rand":  # the router op is the same route stage
        tw, tids = ops.topk_softmax(logits, k)
        assert tids.dtype == torch.int64 and torch.equal(tids.cpu(), rids)
        assert torch.equal(tw.cpu(), w)


@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize(("t", "e", "h", "inter"), [
    (12, 4, 256, 512),
    (130, 8, 512, 1024),  # expert 1 owns 130 rows: crosses a 128-row chunk
])
def test_moe_gemm_gather(t, e, h, inter, gated):
    from vllm_tgis_adapter_amd import ops

    torch.manual_seed(5)
    logits = torch.randn(t, e)
    logits[:, 1] += 20
    _, _, seg, src_row, _ = ops.moe_dispatch(logits.cuda(), 2)
    x = torch.randn(t, h, dtype=torch.bfloat16, device="cuda") / 4
    w = torch.randn(e, 2 * inter if gated else inter, h,
                    dtype=torch.bfloat16, device="cuda") / 8
    got = ops.moe_gemm(x, w, seg, gated, rows=src_row)
    want = ops.moe_gemm(x[src_row.long()].contiguous(), w, seg, gated)
    assert got.shape == (2 * t, inter)
    assert torch.equal(got, want)


@pytest.mark.parametrize(("t", "h", "k"), [(1, 128, 1), (3, 128, 2), (130, 512, 8)])
def test_moe_combine(t, h, k):
    from vllm_tgis_adapter_amd import ops

    torch.manual_seed(7)
    ye = torch.randn(t * k, h, dtype=torch.bfloat16, device="cuda")
    pos = torch.randperm(t * k).to(torch.int32).view(t, k).cuda()
    w = torch.softmax(torch.randn(t, k), -1).cuda()
    out = ops.moe_combine(ye, pos, w).cpu()
    terms = ye.cpu().double()[pos.cpu().long()] * w.cpu().double()[..., None]
    ref = terms.sum(1)
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * terms.abs().sum(1)
    assert out.dtype == torch.bfloat16
    assert bool(((out.double() - ref).abs() <= bound).all())


@pytest.mark.parametrize(("t", "e", "h", "inter"), [(24, 4, 256, 512), (130, 8, 512, 1024)])
def test_moe_block_fused(t, e, h, inter, monkeypatch):
    from vllm_tgis_adapter_amd import ops
    from vllm_tgis_adapter_amd.engine import ModelConfig
    from vllm_tgis_adapter_amd.models.mixtral import MoEBlock

    mc = ModelConfig.from_model_arg("tiny-mixtral", dtype="bfloat16")
    mc.num_experts, mc.num_experts_per_tok = e, 2
    mc.hidden_size, mc.intermediate_size = h, inter
    torch.manual_seed(9)
    moe = MoEBlock(mc).cuda()
    moe.gate.data.normal_()
    moe.w13.data.copy_(torch.randn_like(moe.w13) / 8)
    moe.w2.data.copy_(torch.randn_like(moe.w2) / 8)
    x = torch.randn(t, h, dtype=torch.bfloat16, device="cuda") / 4

    rw, rids, _, _, _ = _ref_dispatch(torch.nn.functional.linear(x, moe.gate), 2)
    xd, w13, w2 = x.double().cpu(), moe.w13.double().cpu(), moe.w2.double().cpu()
    ref = torch.zeros(t, h, dtype=torch.float64)
    for i in range(t):
        for j in range(2):
            ee = int(rids[i, j])
            g, u = xd[i] @ w13[ee, :inter].t(), xd[i] @ w13[ee, inter:].t()
            ref[i] += rw[i, j] * ((torch.nn.functional.silu(g) * u) @ w2[ee].t())

    fused = moe(x)
    assert torch.allclose(fused.double().cpu(), ref, atol=0.5, rtol=3e-2)

    # the switch: with VTA_MOE_FUSED=0 the torch chain runs, never the dispatch
    def _not_here(*a, **kw):
        raise AssertionError("VTA_MOE_FUSED=0 must not reach moe_dispatch")

    monkeypatch.setenv("VTA_MOE_FUSED", "0")
    monkeypatch.setattr(ops, "moe_dispatch", _not_here)
    unfused = moe(x)
    assert torch.allclose(unfused.double().cpu(), ref, atol=0.5, rtol=3e-2)
