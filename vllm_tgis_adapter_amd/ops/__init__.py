"""Custom-op dispatch.

GPU tensors run the hand-written CDNA4 HIP kernels from the in-tree ``_C``
extension (kernels/ — built by ``__graft_entry__.build()`` for gfx950).  CPU
tensors run the plain-PyTorch reference (ops/reference.py), which keeps the
full engine runnable in CPU-only CI like the reference's CPU vLLM build
(SURVEY.md §4).  On a GPU box a missing extension is a hard error — there is
deliberately no silent eager fallback.
"""

from __future__ import annotations

import os

import torch

from . import reference

_C = None
_load_error: str | None = None


def _try_load_native() -> None:
    global _C, _load_error
    if _C is not None:
        return
    try:
        from vllm_tgis_adapter_amd import _C as ext  # in-tree built .so

        _C = ext
    except ImportError as e:
        _load_error = str(e)


_try_load_native()

_FORCE_REFERENCE = os.environ.get("VTA_FORCE_REFERENCE", "0") == "1"


def has_native() -> bool:
    return _C is not None


def native_enabled(t: torch.Tensor) -> bool:
    """True when the HIP path applies to this tensor (device, build, and the
    VTA_FORCE_REFERENCE escape hatch all considered) — non-raising."""
    return t.device.type == "cuda" and not _FORCE_REFERENCE and _C is not None


def _native(t: torch.Tensor) -> bool:
    if t.device.type != "cuda":
        return False
    if _FORCE_REFERENCE:
        return False
    if _C is None:
        raise RuntimeError(
            "vllm_tgis_adapter_amd._C HIP extension is not built but a GPU "
            f"tensor reached a custom op (import error: {_load_error}). "
            "Run `python -c 'import __graft_entry__; __graft_entry__.build()'` "
            "or kernels/build.py first."
        )
    return True


# ---------------------------------------------------------------------------


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    if _native(x):
        out = torch.empty_like(x)
        _C.rms_norm(out, x, weight, eps)
        return out
    return reference.rms_norm(x, weight, eps)


def fused_add_rms_norm(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float
) -> tuple[torch.Tensor, torch.Tensor]:
    """x <- rmsnorm(x + residual); residual <- x + residual (in place on GPU)."""
    if _native(x):
        _C.fused_add_rms_norm(x, residual, weight, eps)
        return x, residual
    return reference.fused_add_rms_norm(x, residual, weight, eps)


def silu_and_mul(x: torch.Tensor) -> torch.Tensor:
    if x.numel() == 0:
        return x[..., : x.shape[-1] // 2].clone()
    if _native(x):
        d = x.shape[-1] // 2
        out = torch.empty(*x.shape[:-1], d, dtype=x.dtype, device=x.device)
        _C.silu_and_mul(out, x)
        return out
    return reference.silu_and_mul(x)


def rotary_embedding(
    positions: torch.Tensor,
    q: torch.Tensor,
    k: torch.Tensor,
    head_dim: int,
    cos_sin_cache: torch.Tensor,
) -> tuple[torch.Tensor, torch.Tensor]:
    """NeoX rotary; in place on GPU, out-of-place on CPU."""
    if _native(q):
        _C.rotary_embedding(positions, q, k, head_dim, cos_sin_cache)
        return q, k
    return reference.rotary_embedding(positions, q, k, head_dim, cos_sin_cache)


def reshape_and_cache(
    k: torch.Tensor,
    v: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    slot_mapping: torch.Tensor,
) -> None:
    if _native(k):
        _C.reshape_and_cache(k, v, k_cache, v_cache, slot_mapping)
        return
    if k_cache.dtype == torch.uint8:  # fp8 KV: quantize via torch e4m3
        reference.reshape_and_cache(
            k.to(torch.float8_e4m3fn).view(torch.uint8),
            v.to(torch.float8_e4m3fn).view(torch.uint8),
            k_cache, v_cache, slot_mapping)
        return
    reference.reshape_and_cache(k, v, k_cache, v_cache, slot_mapping)


def paged_attention_decode(
    q: torch.Tensor,            # [N, num_heads, head_dim] — one token per seq
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,  # [N, max_blocks] int32, device
    seq_lens: torch.Tensor,      # [N] int32, device
    scale: float,
    max_seq_len: int,
    out: torch.Tensor | None = None,
) -> torch.Tensor:
    if _native(q):
        if out is None:
            out = torch.empty_like(q)
        _C.paged_attention_decode(
            out, q, k_cache, v_cache, block_tables, seq_lens, scale
        )
        return out
    n = q.shape[0]
    qsl = torch.arange(n + 1, dtype=torch.int32)
    if k_cache.dtype == torch.uint8:  # fp8 KV: dequantize for the reference
        k_cache = k_cache.view(torch.float8_e4m3fn).to(q.dtype)
        v_cache = v_cache.view(torch.float8_e4m3fn).to(q.dtype)
    r = reference.paged_attention(
        q, k_cache, v_cache, block_tables.cpu(), qsl, seq_lens.cpu(), scale
    )
    if out is not None:
        out.copy_(r)
        return out
    return r


def paged_attention_multiq_usable(
    q: torch.Tensor,        # [T, num_heads, head_dim]
    k_cache: torch.Tensor,  # [num_blocks, block_size, kv_heads, head_dim]
    max_query_len: int,
) -> bool:
    """The short-chunk MFMA attention kernel serves bf16 queries with head_dim
    64 or 128 over a bf16 or e4m3 (uint8) cache when every sequence's
    ``q_len * group`` query rows fit its 32-column blocks: GQA group <= 8 and
    ``max_query_len * group`` <= 64 at head_dim 64 (two blocks), <= 32 at
    head_dim 128 (one block; two would spill registers there).  That covers
    speculative verify, prefix-cache hits and short prompts; longer chunks
    stay on the prefill kernels.  VTA_ATTN_MULTIQ=0 (read per call) turns the
    route off."""
    if not (native_enabled(q) and q.dim() == 3 and k_cache.dim() == 4):
        return False
    if os.environ.get("VTA_ATTN_MULTIQ", "1") == "0":
        return False
    if q.dtype != torch.bfloat16 or k_cache.dtype not in (torch.bfloat16, torch.uint8):
        return False
    if not (q.is_contiguous() and k_cache.is_contiguous()):
        return False
    nheads, hd, kvh = q.shape[1], q.shape[2], k_cache.shape[2]
    if hd not in (64, 128) or kvh < 1 or nheads % kvh != 0:
        return False
    group = nheads // kvh
    cols = 64 if hd == 64 else 32
    return 1 <= group <= 8 and 1 <= max_query_len and max_query_len * group <= cols


def paged_attention_prefill(
    q: torch.Tensor,               # [T, num_heads, head_dim]
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,    # [num_seqs, max_blocks] int32 device
    query_start_loc: torch.Tensor,  # [num_seqs+1] int32 device
    seq_lens: torch.Tensor,         # [num_seqs] int32 device
    scale: float,
    max_query_len: int,
    max_seq_len: int,
) -> torch.Tensor:
    if _native(q):
        out = torch.empty_like(q)
        if paged_attention_multiq_usable(q, k_cache, max_query_len):
            _C.paged_attention_multiq(
                out, q, k_cache, v_cache, block_tables, query_start_loc,
                seq_lens, scale, max_query_len
            )
            return out
        _C.paged_attention_prefill(
            out, q, k_cache, v_cache, block_tables, query_start_loc, seq_lens,
            scale, max_query_len
        )
        return out
    if k_cache.dtype == torch.uint8:  # fp8 KV: dequantize for the reference
        k_cache = k_cache.view(torch.float8_e4m3fn).to(q.dtype)
        v_cache = v_cache.view(torch.float8_e4m3fn).to(q.dtype)
    return reference.paged_attention(
        q, k_cache, v_cache, block_tables.cpu(), query_start_loc.cpu(),
        seq_lens.cpu(), scale
    )


def linear(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """F.linear with a custom CDNA4 skinny-GEMM path for small decode batches.

    hipBLASLt runs the M<=64 llama decode shapes at 22-43% of the HBM
    roofline (tools/gemm_bench.py); the hand-written MFMA kernel streams the
    weight matrix once with waves splitting K in-workgroup.  Larger M stays
    on hipBLASLt (the in-tree tile kernel only reached parity there —
    VTA_GEMM_MAX_M raises the cutover for experiments).
    """
    max_m = int(os.environ.get("VTA_GEMM_MAX_M", "64"))
    tile_max_m = int(os.environ.get("VTA_GEMM_TILE_MAX_M", "0"))
    if (
        bias is None
        and x.dim() == 2
        and _native(x)
        and x.dtype == torch.bfloat16
        and weight.dtype == torch.bfloat16
        and weight.shape[0] % 128 == 0
        and x.shape[1] % 64 == 0
        and x.is_contiguous()
        and weight.is_contiguous()
    ):
        m = x.shape[0]
        if 1 <= m <= max_m:
            out = torch.empty(
                (m, weight.shape[0]), dtype=x.dtype, device=x.device
            )
            _C.gemm_skinny(out, x, weight)
            return out
        if max_m < m <= tile_max_m:
            out = torch.empty(
                (m, weight.shape[0]), dtype=x.dtype, device=x.device
            )
            _C.gemm_tile(out, x, weight)
            return out
    return torch.nn.functional.linear(x, weight, bias)


def gemm_tile(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """Direct 128x128-tile GEMM path (benchmarks/tests)."""
    assert _native(x)
    out = torch.empty((x.shape[0], weight.shape[0]), dtype=x.dtype, device=x.device)
    _C.gemm_tile(out, x, weight)
    return out


# ---------------------------------------------------------------------------
# Weight-only quantization: RTN into int8 (per-out-channel
# scale) or packed int4 with group-128 scales (the --quantize awq/gptq/
# squeezellm 4-bit surface; offline RTN since checkpoint-specific scales
# don't exist in this environment).
# ---------------------------------------------------------------------------

def quantize_weight(w: torch.Tensor, qbits: int) -> tuple[torch.Tensor, torch.Tensor]:
    """Returns (wq, scales). int8: wq [N,K] int8, scales [N] f32.
    int4: wq [N,K/2] uint8 offset-binary nibbles, scales [N,K/128] f32."""
    assert qbits in (8, 4)
    wf = w.float()
    if qbits == 8:
        scales = wf.abs().amax(dim=1).clamp(min=1e-8) / 127.0
        q = torch.round(wf / scales.unsqueeze(1)).clamp(-127, 127).to(torch.int8)
        return q, scales.contiguous()
    n, k = wf.shape
    assert k % 128 == 0
    g = wf.view(n, k // 128, 128)
    scales = g.abs().amax(dim=2).clamp(min=1e-8) / 7.0
    q = torch.round(g / scales.unsqueeze(2)).clamp(-8, 7).to(torch.int16) + 8
    q = q.view(n, k)
    packed = (q[:, 0::2] | (q[:, 1::2] << 4)).to(torch.uint8)
    return packed.contiguous(), scales.contiguous()


def dequantize_weight(wq: torch.Tensor, scales: torch.Tensor, qbits: int,
                      dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """bf16 on a GPU runs the one-pass HIP kernel (bit-identical to the torch
    chain below, which serves CPU tensors, other dtypes and
    VTA_FORCE_REFERENCE=1; VTA_QDEQUANT_NATIVE=0 forces the chain for
    comparison)."""
    n = wq.shape[0]
    k = wq.shape[1] * (8 // qbits)
    if (
        dtype == torch.bfloat16
        and _native(wq)
        and n % 128 == 0
        and k % 128 == 0
        and wq.is_contiguous()
        and scales.is_contiguous()
        and os.environ.get("VTA_QDEQUANT_NATIVE", "1") != "0"
    ):
        out = torch.empty((n, k), dtype=dtype, device=wq.device)
        _C.dequant_weight(out, wq, scales, qbits)
        return out
    if qbits == 8:
        return (wq.float() * scales.unsqueeze(1)).to(dtype)
    lo = (wq & 0xF).to(torch.float32) - 8.0
    hi = (wq >> 4).to(torch.float32) - 8.0
    q = torch.stack([lo, hi], dim=2).view(n, -1)  # interleave even/odd k
    k = q.shape[1]
    return (q.view(n, k // 128, 128) * scales.unsqueeze(2)).view(n, k).to(dtype)


# largest M served by gemm_tile_q, per qbits: the largest measured M at which
# it beats one-pass dequant + hipBLASLt on all four llama-3-8b linears
_QGEMM_TILE_MAX_M = {8: 256, 4: 256}


def linear_quant(x: torch.Tensor, wq: torch.Tensor, scales: torch.Tensor,
                 qbits: int, bias: torch.Tensor | None = None) -> torch.Tensor:
    """W8A16/W4A16 linear, native at every batch size.

    M <= 64 runs the skinny dequant-GEMM (weight-stream bound).  Above that,
    up to the cutover, the dequant-in-LDS tile GEMM (gemm_tile_q.hip) reads
    the packed weights directly; past the cutover, where the conversion work
    no longer hides under the MFMAs, the weight is dequantised in one HIP
    pass and handed to hipBLASLt.  A bias or a shape the kernels reject
    (N or K not a multiple of 128) also takes the dequant + F.linear path.
    All three see bit-identical effective weights.  The cutover defaults to
    _QGEMM_TILE_MAX_M[qbits] (measured, profiles/r08_gemm_tile_q.txt);
    VTA_QGEMM_TILE_MAX_M overrides it and 0 disables the tile kernel."""
    x2 = x.reshape(-1, x.shape[-1])
    m = x2.shape[0]
    n = wq.shape[0]
    k = x2.shape[1]
    if (
        bias is None
        and _native(x)
        and x.dtype == torch.bfloat16
        and m >= 1
        and n % 128 == 0
        and k % 128 == 0
        and x2.is_contiguous()
    ):
        tile_max_m = int(os.environ.get("VTA_QGEMM_TILE_MAX_M",
                                        _QGEMM_TILE_MAX_M[qbits]))
        if m <= 64 or m <= tile_max_m:
            out = torch.empty((m, n), dtype=x.dtype, device=x.device)
            if m <= 64:
                _C.gemm_skinny_q(out, x2, wq, scales, qbits)
            else:
                _C.gemm_tile_q(out, x2, wq, scales, qbits)
            return out.view(*x.shape[:-1], n)
    w = dequantize_weight(wq, scales, qbits, x.dtype)
    return torch.nn.functional.linear(x, w, bias)


def gated_mlp_up(x: torch.Tensor, w13: torch.Tensor) -> torch.Tensor | None:
    """Fused silu(x@Wg^T) * (x@Wu^T) for merged [gate; up] weights.

    Returns None when the fused CDNA4 path doesn't apply (caller falls back
    to linear + silu_and_mul).
    """
    max_m = int(os.environ.get("VTA_GEMM_MAX_M", "64"))
    if (
        x.dim() == 2
        and 1 <= x.shape[0] <= max_m
        and x.dtype == torch.bfloat16
        and w13.dtype == torch.bfloat16
        and w13.shape[0] % 256 == 0
        and x.shape[1] % 64 == 0
        and x.is_contiguous()
        and w13.is_contiguous()
        and _native(x)
    ):
        inter = w13.shape[0] // 2
        out = torch.empty((x.shape[0], inter), dtype=x.dtype, device=x.device)
        _C.gemm_skinny_gated(out, x, w13)
        return out
    return None


def lora_bgmv(
    out: torch.Tensor,      # [T, out_w] updated in place
    x: torch.Tensor,        # [T, K]
    a_stack: torch.Tensor,  # [L, R, K]
    b_stack: torch.Tensor,  # [L, N, R]
    slots: torch.Tensor,    # [T] int32, -1 = no adapter
    scales: torch.Tensor,   # [L] float32
    off: int,
) -> None:
    """Batched LoRA delta for a mixed-adapter batch (GPU only)."""
    assert _native(x), "lora_bgmv is the GPU path; CPU uses the torch loop"
    tmp = torch.empty(
        (x.shape[0], a_stack.shape[1]), dtype=torch.float32, device=x.device
    )
    _C.lora_bgmv(out, x, a_stack, b_stack, tmp, slots, scales, off)


def lora_sgmv_usable(
    x: torch.Tensor,        # [T, K]
    out: torch.Tensor,      # [T, out_w]
    a_stack: torch.Tensor,  # [L, R, K]
    b_stack: torch.Tensor,  # [L, N, R]
    off: int,
) -> bool:
    """The segmented MFMA LoRA path serves contiguous, 16-byte-aligned bf16
    with rank <= 64.  K % 128: the four waves of a shrink workgroup split K into whole 32-k MFMA
    steps of 16-byte fragment loads.  N % 32, off % 8, out_w % 8: the expand
    updates ``out`` in 16-byte pieces of 8 columns, two interleaved 16-row
    n-blocks at a time.  Everything else stays on lora_bgmv."""
    if not (native_enabled(x) and x.dim() == 2 and out.dim() == 2
            and a_stack.dim() == 3 and b_stack.dim() == 3):
        return False
    if any(t.dtype != torch.bfloat16 or not t.is_contiguous()
           or t.data_ptr() % 16 != 0 for t in (x, out, a_stack, b_stack)):
        return False
    k, r, n, out_w = x.shape[1], a_stack.shape[1], b_stack.shape[1], out.shape[1]
    return (x.shape[0] >= 1 and 1 <= r <= 64
            and k >= 128 and k % 128 == 0
            and n >= 32 and n % 32 == 0
            and off >= 0 and off % 8 == 0 and out_w % 8 == 0)


def lora_sgmv(
    out: torch.Tensor,      # [T, out_w] updated in place
    x: torch.Tensor,        # [T, K]
    a_stack: torch.Tensor,  # [L, R, K]
    b_stack: torch.Tensor,  # [L, N, R]
    slots: torch.Tensor,    # [T] int32, -1 = no adapter
    scales: torch.Tensor,   # [L] float32
    off: int,
) -> None:
    """lora_bgmv's contract on the segmented MFMA kernels for prefill-sized
    batches: tokens are grouped by adapter inside the kernel (no sort, no host
    sync), the shrink's K-split partials are summed in fixed order so results
    repeat bit-for-bit.  Launch only."""
    assert lora_sgmv_usable(x, out, a_stack, b_stack, off), \
        "lora_sgmv needs lora_sgmv_usable(); lora_bgmv serves the rest"
    t, k = x.shape
    tmp = torch.empty(
        (_C.lora_sgmv_num_ksplit(t, k), t, (a_stack.shape[1] + 15) // 16 * 16),
        dtype=torch.float32, device=x.device,
    )
    _C.lora_sgmv(out, x, a_stack, b_stack, tmp, slots, scales, off)


def sample_argmax(
    out: torch.Tensor,     # [N] int64
    logits: torch.Tensor,  # [N, V]
    temps: torch.Tensor,   # [N] float32, 0 = greedy
    noise: torch.Tensor | None,  # [N, V] float32 Exp(1) draws for temp>0 rows
) -> None:
    """Fused temperature + exponential-race sampling / greedy argmax (E7)."""
    assert _native(logits), "sample_argmax is the GPU path"
    _C.sample_argmax(out, logits, temps, noise)


def sample_topk_topp_usable(logits: torch.Tensor) -> bool:
    """The fused top-k/top-p sampler serves contiguous 16-bit logits; f32
    logits stay on the torch path."""
    return (native_enabled(logits) and logits.dim() == 2
            and logits.dtype in (torch.bfloat16, torch.float16)
            and logits.is_contiguous()
            and 1 <= logits.shape[1] <= _C.sample_topk_topp_max_vocab())


def sample_topk_topp(
    out: torch.Tensor,     # [N] int64
    logits: torch.Tensor,  # [N, V] bf16 / f16, contiguous
    temps: torch.Tensor,   # [N] float32, 0 = greedy (filters ignored)
    noise: torch.Tensor | None,  # [N, V] float32 Exp(1) draws for temp>0 rows
    top_k: torch.Tensor,   # [N] int32, <=0 or >=V = off
    top_p: torch.Tensor,   # [N] float32, >=1 = off
    kept: torch.Tensor | None = None,  # [N] int32 out: kept-set size
) -> None:
    """Fused top-k / top-p sampling for a mixed batch (E7): tokens ordered by
    logit descending (ties: lower index first), the first
    c = max(1, min(top_k, #{j : prefix-mass_j <= top_p})) are kept, and the
    exponential race argmax(logits/T - log noise) runs over those.  ``kept``
    receives c (V for greedy / unfiltered rows).  Launch only, no host sync."""
    assert sample_topk_topp_usable(logits), "sample_topk_topp is the GPU path"
    _C.sample_topk_topp(out, logits, temps, noise, top_k, top_p, kept)


def token_bitmap_words(vocab: int) -> int:
    """uint32 words per token-bitmap row: ceil(V / 32) rounded up to a
    multiple of 4, so rows are 16-byte aligned."""
    return ((vocab + 31) // 32 + 3) // 4 * 4


def pack_token_bitmap(ids, vocab: int):
    """Host-side bitmap row (numpy uint32 [W]) with the bit of every id in
    [0, vocab) set: bit ``t & 31`` of word ``t >> 5`` stands for token t."""
    import numpy as np

    bits = np.zeros(token_bitmap_words(vocab) * 32, dtype=np.uint8)
    idx = np.asarray(ids, dtype=np.int64).reshape(-1)
    bits[idx[(idx >= 0) & (idx < vocab)]] = 1
    return np.packbits(bits, bitorder="little").view("<u4")


def token_bitmap_scatter(
    bitmap: torch.Tensor,  # [slots, W] int32 (the uint32 words' bits)
    slots: torch.Tensor,   # [P] int32
    tokens: torch.Tensor,  # [P] int32
    vocab: int | None = None,  # tokens outside [0, vocab) are dropped
) -> torch.Tensor:
    """OR the bit of every (slot, token) pair into ``bitmap``, in place.
    Duplicates, slots outside the bitmap and tokens outside the vocab are
    harmless.  Launch only, no host sync."""
    if vocab is None:
        vocab = bitmap.shape[1] * 32
    if _native(bitmap):
        _C.token_bitmap_scatter(bitmap, slots, tokens, vocab)
        return bitmap
    return reference.token_bitmap_scatter(bitmap, slots, tokens, vocab)


def logits_edit_usable(logits: torch.Tensor) -> bool:
    """The bitmap-driven edit kernel serves contiguous 2-D bf16/f16/f32 GPU
    logits with V % 8 == 0 (a bitmap byte is one 8-token piece).
    ``VTA_SAMPLE_EDIT=0``, read per call, turns the route off."""
    return (native_enabled(logits) and logits.dim() == 2
            and logits.dtype in (torch.bfloat16, torch.float16, torch.float32)
            and logits.is_contiguous() and logits.shape[1] % 8 == 0
            and logits.shape[1] > 0
            and os.environ.get("VTA_SAMPLE_EDIT", "1") != "0")


def logits_edit(
    logits: torch.Tensor,       # [N, V], edited in place
    rows: torch.Tensor,         # [E] int32 logit row of each edit row
    penalties: torch.Tensor,    # [E] float32 repetition penalty, 1.0 = none
    seen: torch.Tensor | None,  # [S, W] int32 bitmaps of seen tokens
    seen_slots: torch.Tensor | None,   # [E] int32 row of `seen`, -1 = none
    allow: torch.Tensor | None,        # [G, W] int32 bitmaps of allowed tokens
    allow_slots: torch.Tensor | None,  # [E] int32 row of `allow`, -1 = none
) -> torch.Tensor:
    """Repetition penalty and guided-decoding mask as one sparse in-place
    pass (E7): a seen token's logit becomes ``x / p if x > 0 else x * p``
    (f32, rounded once), then a token outside the allow set becomes -inf.
    Rows not listed in ``rows`` are not touched; the bitmaps decide which
    logits are read or written at all.  Launch only, no host sync."""
    if _native(logits):
        assert logits.dim() == 2 and logits.shape[1] % 8 == 0, \
            "logits_edit needs logits_edit_usable()"
        _C.logits_edit(logits, rows, penalties, seen, seen_slots,
                       allow, allow_slots)
        return logits
    return reference.logits_edit(logits, rows, penalties, seen, seen_slots,
                                 allow, allow_slots)


def logsoftmax_topk_usable(logits: torch.Tensor) -> bool:
    # V >= 2048 guarantees every lane feeds both accumulator pairs
    return (native_enabled(logits) and logits.dtype == torch.bfloat16
            and logits.shape[1] % 8 == 0 and logits.shape[1] >= 2048)


def logsoftmax_topk(
    logits: torch.Tensor,  # [N, V] bf16 (contiguous)
    chosen: torch.Tensor,  # [N] int64 sampled/actual token per row
    k: int,
):
    """Fused log-softmax + top-K + chosen-token logprob/rank in one HBM
    pass (E8 wire details).  Returns (topv f32 [N,K], topi i32 [N,K],
    chosen_lp f32 [N], ranks i32 [N]); launch only, no host sync."""
    assert logsoftmax_topk_usable(logits), "logsoftmax_topk is the GPU path"
    n = logits.shape[0]
    dev = logits.device
    topv = torch.empty((n, k), dtype=torch.float32, device=dev)
    topi = torch.empty((n, k), dtype=torch.int32, device=dev)
    chosen_lp = torch.empty((n,), dtype=torch.float32, device=dev)
    ranks = torch.empty((n,), dtype=torch.int32, device=dev)
    _C.logsoftmax_topk(topv, topi, chosen_lp, ranks,
                       logits.contiguous(), chosen.contiguous())
    return topv, topi, chosen_lp, ranks


# largest sorted-row count served by the fused quantized grouped GEMM, per
# qbits: the largest measured R at which its slowest round beats one-pass
# dequant + bf16 moe_gemm's fastest on both the gated and the down GEMM, at
# mixtral-8x7b's TP=1 and TP=4 dims (profiles/r09_moe_gemm_q.txt)
_MOE_QGEMM_MAX_ROWS = {8: 4096, 4: 4096}


def moe_gemm(
    x: torch.Tensor,        # [T, K] rows sorted by expert
    w: torch.Tensor,        # [E, 2N, K] (gated) or [E, N, K]
    seg_off: torch.Tensor,  # [E+1] int32 device row offsets
    gated: bool,
    rows: torch.Tensor | None = None,  # [R] int32: sorted row r is x[rows[r]]
    scales: torch.Tensor | None = None,
    qbits: int | None = None,
) -> torch.Tensor:
    """Grouped GEMM over expert segments (E16); gated fuses SiLU(g)*u.  With
    ``rows`` (moe_dispatch's src_row) x stays in token order and the kernel
    gathers its rows itself: same bits as on ``x[rows].contiguous()``.

    With ``scales`` and ``qbits`` (8 | 4), ``w`` is quantize_weight's storage
    stacked per expert: int8 [E, rows, K] with scales [E, rows], or uint8
    nibbles [E, rows, K/2] with scales [E, rows, K/128].  Up to the cutover in
    sorted rows the dequant-in-LDS kernel (moe_gemm_q.hip) reads the packed
    weights directly; past it, where the conversion work no longer hides
    under the MFMAs, the flattened stack is dequantised in one HIP pass into a
    transient bf16 tensor for the bf16 kernel.  Both see bit-identical
    weights.  The cutover defaults to _MOE_QGEMM_MAX_ROWS[qbits];
    VTA_MOE_QGEMM_MAX_ROWS overrides it and 0 disables the fused kernel."""
    assert _native(x)
    assert (scales is None) == (qbits is None)
    n = w.shape[1] // 2 if gated else w.shape[1]
    r = rows.numel() if rows is not None else x.shape[0]
    out = torch.empty((r, n), dtype=x.dtype, device=x.device)
    if scales is not None:
        max_rows = int(os.environ.get("VTA_MOE_QGEMM_MAX_ROWS",
                                      _MOE_QGEMM_MAX_ROWS[qbits]))
        if r <= max_rows:
            _C.moe_gemm_q(out, x, w, scales, seg_off, rows, gated, qbits)
            return out
        w = dequantize_weight(w.flatten(0, 1), scales.flatten(0, 1), qbits,
                              x.dtype).view(w.shape[0], w.shape[1], -1)
    if rows is not None:
        _C.moe_gemm_gather(out, x, w, seg_off, rows, gated)
    else:
        _C.moe_gemm(out, x, w, seg_off, gated)
    return out


def moe_gemm_usable(x: torch.Tensor, hidden: int, inter: int) -> bool:
    return (
        native_enabled(x)
        and x.dtype == torch.bfloat16
        and inter % 128 == 0
        and hidden % 128 == 0
        and hidden % 64 == 0
    )


def moe_dispatch_usable(router_logits: torch.Tensor, top_k: int) -> bool:
    """The route + dispatch kernels serve contiguous [T, E] bf16 / f16 / f32
    logits with 2 <= E <= 64 and 1 <= top_k <= min(E, 8)."""
    return (native_enabled(router_logits) and router_logits.dim() == 2
            and router_logits.dtype in (torch.bfloat16, torch.float16, torch.float32)
            and router_logits.is_contiguous()
            and 2 <= router_logits.shape[1] <= 64
            and 1 <= top_k <= min(router_logits.shape[1], 8)
            and router_logits.shape[0] * top_k < 2 ** 31)


def moe_dispatch_block_tokens() -> int:
    """Tokens per moe_dispatch workgroup: up to this T the op is one launch,
    above it two."""
    return _C.moe_dispatch_block_tokens()


def moe_dispatch(router_logits: torch.Tensor, top_k: int):
    """MoE routing and dispatch (E16) -> (weights f32 [T,k], ids i32 [T,k],
    seg_off i32 [E+1], src_row i32 [T*k], pos i32 [T,k]).

    Top-k on the logits by descending value (ties to the lower expert),
    softmax over the selected logits, and a stable counting sort of the
    (token, slot) pairs by expert, token, slot: ``seg_off`` is moe_gemm's
    segment array, ``src_row`` its ``rows``, ``pos`` what moe_combine reads.
    Launch only, no host sync; repeats bit for bit."""
    if not _native(router_logits):
        return reference.moe_dispatch(router_logits, top_k)
    assert moe_dispatch_usable(router_logits, top_k), \
        "moe_dispatch needs moe_dispatch_usable()"
    t, e = router_logits.shape
    dev = router_logits.device
    weights = torch.empty((t, top_k), dtype=torch.float32, device=dev)
    ids = torch.empty((t, top_k), dtype=torch.int32, device=dev)
    src_row = torch.empty((t * top_k,), dtype=torch.int32, device=dev)
    pos = torch.empty((t, top_k), dtype=torch.int32, device=dev)
    if t == 0:
        return (weights, ids, torch.zeros(e + 1, dtype=torch.int32, device=dev),
                src_row, pos)
    seg_off = torch.empty((e + 1,), dtype=torch.int32, device=dev)
    blk = _C.moe_dispatch_block_tokens()
    hist = None
    if t > blk:
        hist = torch.empty(((t + blk - 1) // blk, e), dtype=torch.int32, device=dev)
    _C.moe_dispatch(router_logits, weights, ids, seg_off, src_row, pos, hist, False)
    return weights, ids, seg_off, src_row, pos


def moe_combine(
    ye: torch.Tensor,       # [T*k, H] expert outputs in sorted order
    pos: torch.Tensor,      # [T, k] int32 sorted position of each pair
    weights: torch.Tensor,  # [T, k] float32
) -> torch.Tensor:
    """out[t] = sum_j weights[t, j] * ye[pos[t, j]]: f32 accumulation in slot
    order, rounded once (E16)."""
    if not _native(ye):
        return reference.moe_combine(ye, pos, weights)
    out = torch.empty((pos.shape[0], ye.shape[1]), dtype=ye.dtype, device=ye.device)
    _C.moe_combine(out, ye, pos, weights)
    return out


def topk_softmax(gate_logits: torch.Tensor, top_k: int):
    """MoE router -> (f32 weights [T,k], int64 ids [T,k]).  GPU logits inside
    moe_dispatch_usable() run the route stage of moe_dispatch; everything
    else is the torch reference."""
    if gate_logits.shape[0] > 0 and moe_dispatch_usable(gate_logits, top_k):
        t = gate_logits.shape[0]
        dev = gate_logits.device
        weights = torch.empty((t, top_k), dtype=torch.float32, device=dev)
        ids = torch.empty((t, top_k), dtype=torch.int32, device=dev)
        none = torch.empty((0,), dtype=torch.int32, device=dev)
        _C.moe_dispatch(gate_logits, weights, ids, none, none, none, None, True)
        return weights, ids.long()
    return reference.topk_softmax(gate_logits, top_k)


make_cos_sin_cache = reference.make_cos_sin_cache
