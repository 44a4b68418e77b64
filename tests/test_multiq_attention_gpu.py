"""Short query chunks over a paged context (speculative verify) on the
multi-query MFMA kernel: the (token, head) column packing, the per-column
causal limit at tile edges, both launch shapes, fp8 KV, bit identity with the
decode kernel at q_len 1, empty chunks, the routing predicate and hipGraph
replay.

Reference: fp32 dense causal attention per sequence (K/V gathered by block
table, query j of a chunk sees keys <= seq_len - q_len + j), with the bf16 and
fp8 tolerances of test_decode_attention_tiles_gpu.py.  Every sequence owns
shuffled blocks, the table is wider than needed and unused entries hold -1.

head_dim 128 serves q_len * group <= 32 (one column block); head_dim 64 also
runs the two-block kernel up to 64.
"""

from __future__ import annotations

import random

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16_TOL = dict(atol=3e-2, rtol=2e-2)
FP8_TOL = dict(atol=5e-2, rtol=5e-2)


@pytest.fixture(scope="module", autouse=True)
def _check_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vllm_tgis_adapter_amd import ops

    assert ops.has_native(), "HIP extension must be built on a GPU box"


class Pool:
    """Paged KV in which every sequence owns `max_blocks` shuffled, filled
    blocks, so lengths can change without refilling."""

    def __init__(self, nseq, kvh, hd, max_blocks, bs=16, fp8=False, dtype=torch.bfloat16, seed=0):
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.nseq, self.kvh, self.hd, self.bs, self.max_blocks = nseq, kvh, hd, bs, max_blocks
        nb = nseq * max_blocks + 3
        k = torch.randn((nb, bs, kvh, hd), dtype=dtype, device="cuda", generator=g)
        v = torch.randn((nb, bs, kvh, hd), dtype=dtype, device="cuda", generator=g)
        if fp8:
            k, v = k.to(torch.float8_e4m3fn), v.to(torch.float8_e4m3fn)
            self.kc, self.vc = k.view(torch.uint8), v.view(torch.uint8)
        else:
            self.kc, self.vc = k, v
        self.k32, self.v32 = k.float(), v.float()
        perm = list(range(nb))
        random.Random(seed).shuffle(perm)
        self.owned = torch.tensor(perm[: nseq * max_blocks], dtype=torch.int32).view(nseq, max_blocks)

    def inputs(self, q_lens, seq_lens):
        """(tables, query_start_loc, seq_lens) on the device."""
        t = torch.full((self.nseq, self.max_blocks), -1, dtype=torch.int32)
        for i, s in enumerate(seq_lens):
            n = (s + self.bs - 1) // self.bs
            t[i, :n] = self.owned[i, :n]
        qsl = torch.tensor([0] + q_lens).cumsum(0).to(torch.int32)
        return t.cuda(), qsl.cuda(), torch.tensor(seq_lens, dtype=torch.int32, device="cuda")

    def reference(self, q, q_lens, seq_lens):
        group = q.shape[1] // self.kvh
        out = torch.zeros(q.shape, dtype=torch.float32, device="cuda")
        start = 0
        for i, (ql, s) in enumerate(zip(q_lens, seq_lens)):
            blocks = self.owned[i, : (s + self.bs - 1) // self.bs].long().cuda()
            k = self.k32[blocks].reshape(-1, self.kvh, self.hd)[:s].repeat_interleave(group, 1)
            v = self.v32[blocks].reshape(-1, self.kvh, self.hd)[:s].repeat_interleave(group, 1)
            sc = torch.einsum("jhd,shd->hjs", q[start:start + ql].float(), k) * self.hd ** -0.5
            key = torch.arange(s, device="cuda")[None, :]
            qpos = s - ql + torch.arange(ql, device="cuda")[:, None]
            sc = sc.masked_fill(key > qpos, float("-inf"))
            out[start:start + ql] = torch.einsum("hjs,shd->jhd", torch.softmax(sc, -1), v)
            start += ql
        return out


def _q(tokens, nheads, hd, seed, dtype=torch.bfloat16):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(tokens, nheads, hd, dtype=dtype, device="cuda", generator=g)


def _prefill(pool, q, tables, qsl, sl, max_q):
    from vllm_tgis_adapter_amd import ops

    return ops.paged_attention_prefill(
        q, pool.kc, pool.vc, tables, qsl, sl, pool.hd ** -0.5, max_q,
        pool.max_blocks * pool.bs)


def _run_and_check(pool, group, q_lens, seq_lens, tol, seed, routed=True):
    from vllm_tgis_adapter_amd import ops

    qdt = torch.float32 if pool.kc.dtype == torch.float32 else torch.bfloat16
    q = _q(sum(q_lens), pool.kvh * group, pool.hd, seed, dtype=qdt)
    assert ops.paged_attention_multiq_usable(q, pool.kc, max(q_lens)) == routed
    out = _prefill(pool, q, *pool.inputs(q_lens, seq_lens), max(q_lens))
    ref = pool.reference(q, q_lens, seq_lens)
    err = (out.float() - ref).abs().max().item()
    assert torch.allclose(out.float(), ref, **tol), err
    return q, out


def _num_partitions(nseq, kvh, max_context):
    """Mirror of decode_mfma_num_partitions, to assert which path a case takes."""
    npart = max(1, min(32, 512 // (nseq * kvh)))
    return min(npart, max(1, ((max_context + 31) // 32) // 2))


def _edge_batch(q_lens):
    pairs = [(ql, s if s else ql) for ql in q_lens for s in (0, 31, 32, 33, 34, 65, 257)]
    return [ql for ql, s in pairs if s >= ql], [s for ql, s in pairs if s >= ql]


@pytest.mark.parametrize(
    ("kvh", "group", "hd", "blocks", "q_lens"),
    [
        (8, 4, 128, 1, [1, 2, 5, 8]),
        (8, 8, 128, 1, [1, 2, 3, 4]),
        (2, 1, 64, 1, [1, 2, 5, 32]),
        (2, 1, 64, 2, [33, 64]),
        (2, 2, 64, 1, [1, 2, 5, 16]),
        (2, 2, 64, 2, [17, 32]),
    ],
)
def test_column_packing_and_causal_edge(kvh, group, hd, blocks, q_lens):
    """q_len up to a full column block, context lengths that put the causal
    limit on both sides of a tile edge; seq_len == q_len is a fresh prompt."""
    assert (max(q_lens) * group - 1) // 32 + 1 == blocks
    ql, sl = _edge_batch(q_lens)
    pool = Pool(len(ql), kvh, hd, max_blocks=32, seed=1)
    _run_and_check(pool, group, ql, sl, BF16_TOL, seed=2)


@pytest.mark.parametrize("shape", ["single", "partitioned"])
def test_both_launch_shapes(shape):
    if shape == "single":
        kvh, group, nseq, max_blocks = 8, 4, 64, 24
        ql = [(1, 2, 5, 8)[i % 4] for i in range(nseq)]
        sl = [max(ql[i], (53 * i) % 380 + 1) for i in range(nseq)]
    else:  # the 40-long sequence leaves later partitions and waves without tiles
        kvh, group, nseq, max_blocks = 2, 4, 3, 128
        ql, sl = [5, 8, 2], [40, 700, 2000]
    assert (_num_partitions(nseq, kvh, max_blocks * 16) == 1) == (shape == "single")
    pool = Pool(nseq, kvh, 128, max_blocks=max_blocks, seed=3)
    _run_and_check(pool, group, ql, sl, BF16_TOL, seed=4)


@pytest.mark.parametrize("hd", [128, 64])
def test_fp8_kv(hd):
    ql, sl = _edge_batch([1, 5, 8])
    pool = Pool(len(ql), 8, hd, max_blocks=32, fp8=True, seed=5)
    _run_and_check(pool, 4, ql, sl, FP8_TOL, seed=6)


@pytest.mark.parametrize("nseq", [4, 64], ids=["partitioned", "single"])
def test_qlen1_equals_decode_bitwise(nseq):
    from vllm_tgis_adapter_amd import ops

    kvh, group, hd = 8, 4, 128
    sl = [(97 * i) % 600 + 1 for i in range(nseq)]
    pool = Pool(nseq, kvh, hd, max_blocks=40, seed=7)
    assert (_num_partitions(nseq, kvh, 40 * 16) > 1) == (nseq == 4)
    q, out = _run_and_check(pool, group, [1] * nseq, sl, BF16_TOL, seed=8)
    tables, _, sl_dev = pool.inputs([1] * nseq, sl)
    dec = ops.paged_attention_decode(q, pool.kc, pool.vc, tables, sl_dev, hd ** -0.5, 640)
    assert torch.equal(out, dec)


def test_empty_chunk_writes_nothing():
    """q_len 0 between two chunks; rows past the last chunk stay untouched."""
    from vllm_tgis_adapter_amd import ops

    ql, sl = [3, 0, 5], [70, 50, 33]
    pool = Pool(3, 8, 128, max_blocks=16, seed=9)
    q = _q(sum(ql) + 2, 32, 128, seed=10)
    out = torch.full_like(q, 7.0)
    ops._C.paged_attention_multiq(
        out, q, pool.kc, pool.vc, *pool.inputs(ql, sl), 128 ** -0.5, max(ql))
    ref = pool.reference(q[:8], ql, sl)
    assert torch.allclose(out[:8].float(), ref, **BF16_TOL)
    assert (out[8:] == 7.0).all()


@pytest.mark.parametrize(
    ("kvh", "group", "hd", "dtype", "q_len"),
    [(2, 4, 128, torch.float32, 3), (1, 16, 128, torch.bfloat16, 3),
     (2, 1, 64, torch.bfloat16, 65), (2, 8, 128, torch.bfloat16, 5)],
    ids=["f32", "group16", "65cols", "hd128-40cols"],
)
def test_predicate_false_keeps_old_path(kvh, group, hd, dtype, q_len):
    pool = Pool(2, kvh, hd, max_blocks=16, dtype=dtype, seed=11)
    tol = BF16_TOL if dtype == torch.bfloat16 else dict(atol=1e-4, rtol=2e-2)
    _run_and_check(pool, group, [q_len, q_len], [100, q_len], tol, seed=12, routed=False)


def test_predicate_false_for_head_dim_96():
    from vllm_tgis_adapter_amd import ops

    q = _q(4, 8, 96, seed=13)
    kc = torch.zeros(4, 16, 2, 96, dtype=torch.bfloat16, device="cuda")
    assert not ops.paged_attention_multiq_usable(q, kc, 2)


@pytest.mark.parametrize("nseq", [4, 64], ids=["partitioned", "single"])
def test_graph_replay_and_repeatability(nseq):
    """Capture once, then change seq_lens, query_start_loc (same total) and
    tables in place: replays match the reference and an eager call exactly."""
    kvh, group, hd, max_blocks = 8, 4, 128, 40
    pool = Pool(nseq, kvh, hd, max_blocks=max_blocks, seed=14)
    plans = [([4] * 4, [100] * 4), ([1, 8, 2, 5], [33, 640, 2, 65]),
             ([8, 0, 7, 1], [8, 31, 300, 97])]
    plans = [([a[i % 4] for i in range(nseq)], [b[i % 4] for i in range(nseq)]) for a, b in plans]
    q = _q(4 * nseq, kvh * group, hd, seed=15)
    tables, qsl, sl = pool.inputs(*plans[0])
    _prefill(pool, q, tables, qsl, sl, 8)  # warm-up, eager
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _prefill(pool, q, tables, qsl, sl, 8)
    for ql, s in plans[1:] + plans[:1]:
        for dst, src in zip((tables, qsl, sl), pool.inputs(ql, s)):
            dst.copy_(src)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone()
        assert torch.allclose(got.float(), pool.reference(q, ql, s), **BF16_TOL), ql[:4]
        eager = _prefill(pool, q, tables, qsl, sl, 8)
        assert torch.equal(got, eager), ql[:4]
        assert torch.equal(eager, _prefill(pool, q, tables, qsl, sl, 8))
