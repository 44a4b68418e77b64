"""Quantized grouped MoE GEMM (kernels/moe_gemm_q.hip) against the float64
per-segment product of the torch-chain dequantised weights.

Tolerance: the bf16 ops.moe_gemm on the same bf16 weights has error e_ref
against that reference; both kernels round one f32 sum to bf16 once and
differ only in summation order, so the quantized kernel must stay within
2 * e_ref plus one bf16 ulp of max|ref|."""

import functools
import math

import pytest
import torch
import torch.nn.functional as F

from vllm_tgis_adapter_amd import ops

pytestmark = pytest.mark.gpu

E = 4
# rows per expert: an empty expert, a 1-row segment, one row past 32 and 64
# (the 32-row tile, R <= 32 E) and one row past 128 (the 128-row tile)
SMALL, TALL = (0, 1, 33, 65), (130, 0, 1, 33)
# K 128 = one int4 scale group, 384 = odd group count; N one / three n-tiles
SHAPES = [(SMALL, 128, 128), (SMALL, 384, 384), (TALL, 128, 384),
          (TALL, 384, 128)]


@functools.lru_cache(maxsize=None)
def _case(qbits, gated, segs, n, k):
    """Seeded inputs on the GPU, the float64 reference and the error bound.
    Weight magnitude differs per expert (2x steps), per row (5 levels) and
    per 128-k group (64x range), so a wrong expert, row, group or nibble
    order lands far outside the bound.  x is in a shuffled order; src_row
    sorts it."""
    r, wn = sum(segs), (2 * n if gated else n)
    g = torch.Generator().manual_seed(1000 * qbits + 100 * gated + r + n + k)
    x = torch.randn(r, k, generator=g).to(torch.bfloat16)
    src_row = torch.randperm(r, generator=g).to(torch.int32)
    xs = x[src_row.long()].contiguous()
    group = 2.0 ** (torch.arange(k // 128) % 7 - 3).repeat_interleave(128)
    row = 0.5 * (1 + torch.arange(wn) % 5).unsqueeze(1)
    expert = 2.0 ** (torch.arange(E) - 2.0).view(E, 1, 1)
    w = torch.randn(E, wn, k, generator=g) * 0.05 * group * row * expert
    packed = [ops.quantize_weight(w[e], qbits) for e in range(E)]
    wq = torch.stack([q for q, _ in packed])
    scales = torch.stack([s for _, s in packed])
    seg = torch.tensor((0,) + segs, dtype=torch.int32).cumsum(0).to(torch.int32)
    ref = torch.zeros(r, n, dtype=torch.float64)
    deq = torch.empty(E, wn, k, dtype=torch.bfloat16)
    for e in range(E):
        deq[e] = ops.dequantize_weight(wq[e], scales[e], qbits)  # torch chain
        w64 = ops.dequantize_weight(wq[e], scales[e], qbits, torch.float32).double()
        prod = xs[seg[e]:seg[e + 1]].double() @ w64.T
        ref[seg[e]:seg[e + 1]] = F.silu(prod[:, :n]) * prod[:, n:] if gated else prod
    seg = seg.cuda()
    base = ops.moe_gemm(xs.cuda(), deq.cuda(), seg, gated)
    e_ref = (base.double().cpu() - ref).abs().max().item()
    ulp = 2.0 ** (math.floor(math.log2(ref.abs().max().item())) - 7)
    return (x.cuda(), xs.cuda(), src_row.cuda(), wq.cuda(), scales.cuda(), seg,
            ref, e_ref, 2 * e_ref + ulp)


@pytest.mark.parametrize("gather", [True, False])
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("qbits", [8, 4])
@pytest.mark.parametrize("segs,n,k", SHAPES)
def test_moe_gemm_q_numerics(qbits, gated, gather, segs, n, k):
    x, xs, src_row, wq, scales, seg, ref, e_ref, bound = _case(qbits, gated, segs, n, k)
    r = sum(segs)
    assert ops._C.moe_gemm_q_tile_rows(r, E) == (32 if segs == SMALL else 128)
    y = torch.full((r + 8, n), 777.0, dtype=torch.bfloat16, device="cuda")
    ops._C.moe_gemm_q(y[:r], x if gather else xs, wq, scales, seg,
                      src_row if gather else None, gated, qbits)
    err = (y[:r].double().cpu() - ref).abs().max().item()
    print(f"qbits={qbits} gated={gated} gather={gather} R={r} N={n} K={k} "
          f"e_ref={e_ref:.4g} err={err:.4g} bound={bound:.4g}")
    assert (y[r:] == 777.0).all(), "rows past R were written"
    assert err <= bound


@pytest.mark.parametrize("qbits", [8, 4])
def test_moe_gemm_q_repeatable(qbits):
    x, _, src_row, wq, scales, seg = _case(qbits, True, SMALL, 384, 384)[:6]
    a = ops.moe_gemm(x, wq, seg, True, rows=src_row, scales=scales, qbits=qbits)
    b = ops.moe_gemm(x, wq, seg, True, rows=src_row, scales=scales, qbits=qbits)
    assert torch.equal(a, b)


@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("qbits", [8, 4])
def test_moe_gemm_quant_dispatch(qbits, gated, monkeypatch):
    n, k = 384, 384
    x, xs, src_row, wq, scales, seg = _case(qbits, gated, SMALL, n, k)[:6]
    direct = torch.empty((xs.shape[0], n), dtype=torch.bfloat16, device="cuda")
    ops._C.moe_gemm_q(direct, xs, wq, scales, seg, None, gated, qbits)
    assert torch.equal(
        ops.moe_gemm(xs, wq, seg, gated, scales=scales, qbits=qbits), direct)
    # cutover 0: one-pass dequant of the flattened stack + the bf16 kernel
    monkeypatch.setenv("VTA_MOE_QGEMM_MAX_ROWS", "0")
    deq = ops.dequantize_weight(wq.flatten(0, 1), scales.flatten(0, 1), qbits)
    want = ops.moe_gemm(x, deq.view(E, -1, k), seg, gated, rows=src_row)
    got = ops.moe_gemm(x, wq, seg, gated, rows=src_row, scales=scales, qbits=qbits)
    assert torch.equal(got, want)


@pytest.mark.parametrize("qbits", [8, 4])
@pytest.mark.parametrize(("t", "e", "h", "inter"), [(24, 4, 256, 512), (130, 8, 512, 1024)])
def test_moe_block_quantized(t, e, h, inter, qbits):
    """Fused chain on packed experts against float64 on the dequantised
    weights (test_moe_block_fused's tolerance), then the same block captured
    in a graph: every replay equals the eager result."""
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
    assert moe.quantize_(qbits) and moe.quant_bits == qbits
    assert not hasattr(moe, "w13") and not hasattr(moe, "w2")
    x = torch.randn(t, h, dtype=torch.bfloat16, device="cuda") / 4

    vals, ids = torch.sort(F.linear(x, moe.gate).double().cpu(), dim=-1,
                           descending=True, stable=True)
    rw, xd = torch.softmax(vals[:, :2], -1), x.double().cpu()
    w13, w2 = (torch.stack([
        ops.dequantize_weight(q[i], s[i], qbits, torch.float32).double()
        for i in range(e)]) for q, s in ((moe.w13_q.cpu(), moe.w13_scale.cpu()),
                                         (moe.w2_q.cpu(), moe.w2_scale.cpu())))
    ref = torch.zeros(t, h, dtype=torch.float64)
    for i in range(t):
        for j in range(2):
            ee = int(ids[i, j])
            g, u = xd[i] @ w13[ee, :inter].t(), xd[i] @ w13[ee, inter:].t()
            ref[i] += rw[i, j] * ((F.silu(g) * u) @ w2[ee].t())

    eager = moe(x)
    assert torch.allclose(eager.double().cpu(), ref, atol=0.5, rtol=3e-2)
    if t == 24:
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = moe(x)
        for _ in range(3):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
