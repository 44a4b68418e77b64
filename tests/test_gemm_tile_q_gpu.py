"""Weight-quantized tile GEMM for M > 64 (kernels/gemm_tile_q.hip) and the
one-pass dequant kernel, against the float64 product of the torch-chain
dequantised weights.

Tolerance: torch's own bf16 GEMM on the same bf16 weights has error e_ref
against that reference; both paths round one f32 sum to bf16 and differ only
in summation order, so the kernel must stay within 2 * max(e_ref) plus one
bf16 ulp of max|ref|."""

import functools
import math

import pytest
import torch
import torch.nn.functional as F

from vllm_tgis_adapter_amd import ops

pytestmark = pytest.mark.gpu

# (M, N, K): M 65 = one row past the skinny kernel, 128 = full tile, 200 =
# tiles + tail; N one / three n-tiles; K 128 = one scale group, 384 = odd
# group count; K >= 1024 takes the K-split; N = 16384 selects the 128-row
# tile (two m-tiles already fill the device), with and without the K-split.
SHAPES = [
    (65, 128, 128), (128, 128, 128), (128, 384, 128), (200, 128, 384),
    (200, 384, 384), (65, 384, 1024), (200, 384, 2048), (200, 16384, 384),
    (129, 16384, 1024),
]


@functools.lru_cache(maxsize=None)
def _case(qbits, m, n, k):
    """Seeded inputs on the GPU, the float64 reference and the error bound.
    Weight magnitude varies 64x across 128-wide k groups and 3x across rows,
    so a wrong group, row or nibble order lands far outside the bound."""
    g = torch.Generator().manual_seed(1000 * qbits + m + n + k)
    x = torch.randn(m, k, generator=g).to(torch.bfloat16)
    group = 2.0 ** (torch.arange(k // 128) % 7 - 3).repeat_interleave(128)
    row = 0.5 * (1 + torch.arange(n) % 5).unsqueeze(1)
    w = torch.randn(n, k, generator=g) * 0.05 * group * row
    wq, scales = ops.quantize_weight(w, qbits)
    ref = x.double() @ ops.dequantize_weight(
        wq, scales, qbits, torch.float32).double().T
    deq = ops.dequantize_weight(wq, scales, qbits).cuda()  # CPU torch chain
    e_ref = (F.linear(x.cuda(), deq).double().cpu() - ref).abs().max().item()
    ulp = 2.0 ** (math.floor(math.log2(ref.abs().max().item())) - 7)
    return x.cuda(), wq.cuda(), scales.cuda(), ref, e_ref, 2 * e_ref + ulp


@pytest.mark.parametrize("qbits", [8, 4])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_gemm_tile_q_numerics(qbits, m, n, k):
    x, wq, scales, ref, e_ref, bound = _case(qbits, m, n, k)
    if k >= 1024:
        assert ops._C.gemm_tile_q_ksplit(m, n, k) > 1
    y = torch.full((m + 8, n), 777.0, dtype=torch.bfloat16, device="cuda")
    ops._C.gemm_tile_q(y[:m], x, wq, scales, qbits)
    err = (y[:m].double().cpu() - ref).abs().max().item()
    print(f"qbits={qbits} M={m} N={n} K={k} e_ref={e_ref:.4g} err={err:.4g} "
          f"bound={bound:.4g}")
    assert (y[m:] == 777.0).all(), "rows past M were written"
    assert err <= bound


@pytest.mark.parametrize("qbits", [8, 4])
def test_gemm_tile_q_repeatable(qbits):
    m, n, k = 200, 384, 2048
    x, wq, scales = _case(qbits, m, n, k)[:3]
    assert ops._C.gemm_tile_q_ksplit(m, n, k) > 1
    a = torch.empty((m, n), dtype=torch.bfloat16, device="cuda")
    b = torch.empty_like(a)
    ops._C.gemm_tile_q(a, x, wq, scales, qbits)
    ops._C.gemm_tile_q(b, x, wq, scales, qbits)
    assert torch.equal(a, b)


@pytest.mark.parametrize("qbits", [8, 4])
def test_linear_quant_dispatch(qbits):
    m, n, k = 200, 384, 384
    x, wq, scales, ref, _, _ = _case(qbits, m, n, k)
    direct = torch.empty((m, n), dtype=torch.bfloat16, device="cuda")
    ops._C.gemm_tile_q(direct, x, wq, scales, qbits)
    assert torch.equal(ops.linear_quant(x, wq, scales, qbits), direct)
    y3 = ops.linear_quant(x.view(2, 100, k), wq, scales, qbits)
    assert y3.shape == (2, 100, n) and torch.equal(y3.view(m, n), direct)
    # a bias takes the dequant + F.linear path
    bias = torch.linspace(-1, 1, n).to(torch.bfloat16).cuda()
    ref_b = ref + bias.double().cpu()
    deq = ops.dequantize_weight(wq.cpu(), scales.cpu(), qbits).cuda()
    e_ref = (F.linear(x, deq, bias).double().cpu() - ref_b).abs().max().item()
    ulp = 2.0 ** (math.floor(math.log2(ref_b.abs().max().item())) - 7)
    got = ops.linear_quant(x, wq, scales, qbits, bias)
    assert (got.double().cpu() - ref_b).abs().max().item() <= 2 * e_ref + ulp


@pytest.mark.parametrize("qbits", [8, 4])
@pytest.mark.parametrize("n,k", [(128, 128), (384, 384)])
def test_dequantize_weight_matches_torch_chain(qbits, n, k):
    _, wq, scales = _case(qbits, 200 if n == 384 else 128, n, k)[:3]
    got = ops.dequantize_weight(wq, scales, qbits)
    want = ops.dequantize_weight(wq.cpu(), scales.cpu(), qbits)
    assert got.dtype == torch.bfloat16 and torch.equal(got.cpu(), want)
