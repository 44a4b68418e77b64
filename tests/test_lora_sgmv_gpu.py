"""GPU tests for the segmented MFMA LoRA kernels (ops.lora_sgmv) and their
dispatch in engine/lora.apply_lora, against float64 / float32 loops.

Bound, everywhere: |out - ref| <= 2e-3 + 2^-7 |ref|.  2^-7 |ref| is one bf16
ulp for the single final rounding of out; 2e-3 covers the f32 accumulation and
the 2^-16 residue of the hi/lo split of tmp.  A tmp rounded once to bf16
exceeds it severalfold at K >= 4096."""

from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

DT = torch.bfloat16
OFF = 16


@pytest.fixture(scope="module", autouse=True)
def _check_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vllm_tgis_adapter_amd import ops

    assert ops.has_native(), "HIP extension must be built on a GPU box"


def _within(out, ref):
    err = (out.double().cpu() - ref.double().cpu()).abs()
    bound = 2e-3 + 2.0 ** -7 * ref.double().cpu().abs()
    print("worst err/bound", (err / bound).max().item())
    return bool((err <= bound).all())


def _inputs(t, k, n, ranks, pattern):
    """test_lora_bgmv's scaling; out is the first t rows of a larger buffer."""
    torch.manual_seed(11)
    L, rmax = len(ranks), max(ranks)
    x = torch.randn(t, k, dtype=DT, device="cuda") / 4
    big = torch.randn(t + 8, n + 32, dtype=DT, device="cuda")
    a_stack = torch.zeros(L, rmax, k, dtype=DT, device="cuda")
    b_stack = torch.zeros(L, n, rmax, dtype=DT, device="cuda")
    scales = torch.rand(L, dtype=torch.float32, device="cuda") + 0.5
    for s, r in enumerate(ranks):
        a_stack[s, :r] = torch.randn(r, k, dtype=DT, device="cuda") / 8
        b_stack[s, :, :r] = torch.randn(n, r, dtype=DT, device="cuda") / 8
    if pattern == "segments":  # 11-token runs: boundaries fall off tile edges
        order = list(range(L)) + [-1]
        slots = torch.tensor([order[(i // 11) % len(order)] for i in range(t)])
    elif pattern == "random":
        slots = torch.randint(-1, L, (t,))
    else:
        slots = torch.full((t,), -1)
    return x, big, a_stack, b_stack, slots.to(torch.int32).cuda(), scales


@pytest.mark.parametrize("pattern", ["segments", "random", "none"])
@pytest.mark.parametrize(("t", "k", "n", "ranks"), [
    (1, 512, 256, [4]),            # single row, R < 16, no K split
    (17, 512, 256, [8, 16]),       # tile tail
    (50, 4096, 512, [40]),         # R % 16 != 0, two m-blocks plus a tail
    (96, 4096, 6144, [64]),        # full R, several N tiles, K split
    (33, 14336, 256, [16, 64]),    # down_proj K, mixed ranks
])
def test_lora_sgmv_numerics(t, k, n, ranks, pattern):
    from vllm_tgis_adapter_amd import ops

    x, big, a_stack, b_stack, slots, scales = _inputs(t, k, n, ranks, pattern)
    out = big[:t]
    before = big.clone()
    assert ops.lora_sgmv_usable(x, out, a_stack, b_stack, OFF)
    ops.lora_sgmv(out, x, a_stack, b_stack, slots, scales, OFF)

    ref = before[:t].double().cpu()
    x64, a64, b64 = x.double().cpu(), a_stack.double().cpu(), b_stack.double().cpu()
    live = torch.zeros(t, dtype=torch.bool)
    for i in range(t):
        s = int(slots[i])
        if s < 0:
            continue
        live[i] = True
        ref[i, OFF:OFF + n] += (b64[s] @ (a64[s] @ x64[i])) * float(scales[s])
    assert _within(out, ref)
    # untouched: rows past T, columns outside the slice, rows with no adapter
    assert torch.equal(big[t:], before[t:])
    assert torch.equal(out[:, :OFF], before[:t, :OFF])
    assert torch.equal(out[:, OFF + n:], before[:t, OFF + n:])
    assert torch.equal(out[~live.cuda()], before[:t][~live.cuda()])


def test_lora_sgmv_repeats_bitwise():
    from vllm_tgis_adapter_amd import ops

    x, big, a_stack, b_stack, slots, scales = _inputs(96, 4096, 6144, [64], "random")
    outs = []
    for _ in range(2):
        out = big[:96].clone()
        ops.lora_sgmv(out, x, a_stack, b_stack, slots, scales, OFF)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


PROJS = [("q_proj", 0, 128), ("v_proj", 128, 192)]


def _apply(x, out, ids, ranks, dtype, first_id):
    """lora.apply_lora on x/out's device over synthetic adapters first_id,
    first_id+1, ... (weights drawn from a fixed seed, so a CPU float32 call
    sees the same values as the GPU call in ``dtype``)."""
    from vllm_tgis_adapter_amd.engine import lora

    g = torch.Generator().manual_seed(5)
    adapters = {}
    for j, r in enumerate(ranks):
        w = {}
        for name, lo, hi in PROJS:
            a = (torch.randn(r, x.shape[1], generator=g) / 8).to(dtype)
            b = (torch.randn(hi - lo, r, generator=g) / 16).to(dtype)
            w[(0, name)] = (a.to(x.device, x.dtype), b.to(x.device, x.dtype))
        adapters[first_id + j] = lora.LoRAAdapter(first_id + j, r, 0.25 * (j + 1), w)
    try:
        lora.set_context(ids.to(x.device), adapters)
        return lora.apply_lora(0, PROJS, x, out)
    finally:
        lora.clear_context()
        for lid in adapters:
            lora.invalidate_adapter(lid)


def _batch(dtype, t=40, k=256):
    torch.manual_seed(3)
    wide = (torch.randn(t, 2 * k) / 4).to(dtype).cuda()
    out = torch.randn(t, 192).to(dtype).cuda()
    return wide, out


@pytest.mark.parametrize("min_t", ["1", "1000"])  # SGMV, then BGMV kept intact
def test_apply_lora_dispatch(monkeypatch, min_t):
    monkeypatch.setenv("VTA_LORA_SGMV_MIN_T", min_t)
    wide, out = _batch(DT)
    x = wide[:, :256].contiguous()
    ids = torch.tensor([9101] * 13 + [0] * 6 + [9102] * 17 + [0] * 4)
    ref = _apply(x.float().cpu(), out.float().cpu(), ids, [8, 16], DT, 9101)
    got = _apply(x, out, ids, [8, 16], DT, 9101)
    assert _within(got, ref)


@pytest.mark.parametrize(("dtype", "rank", "contiguous"), [
    (torch.float16, 16, True), (torch.float32, 16, True),
    (DT, 65, True), (DT, 16, False),
])
def test_lora_sgmv_predicate_rejects(monkeypatch, dtype, rank, contiguous):
    from vllm_tgis_adapter_amd import ops

    monkeypatch.setenv("VTA_LORA_SGMV_MIN_T", "1")
    wide, out = _batch(dtype)
    x = wide[:, :256] if not contiguous else wide[:, :256].contiguous()
    a_stack = torch.zeros(1, rank, 256, dtype=dtype, device="cuda")
    b_stack = torch.zeros(1, 128, rank, dtype=dtype, device="cuda")
    assert not ops.lora_sgmv_usable(x, out, a_stack, b_stack, 0)
    ids = torch.tensor([9103] * 25 + [0] * 15)
    ref = _apply(x.float().cpu(), out.float().cpu(), ids, [rank], dtype, 9103)
    got = _apply(x, out, ids, [rank], dtype, 9103)
    assert _within(got, ref)
