"""Decode attention at the places where a pipelined, LDS-staged kernel can go
wrong: tile boundaries, waves and partitions with no work, the prefetch at the
end of a sequence, unused block-table entries, the single-launch path taken
when one partition per (sequence, KV head) already fills the device, the
partitioned path, fp8 KV, and hipGraph replay with changed lengths.

Reference: fp32 dense attention (gather K/V by block table, softmax in fp32),
as in test_ops_gpu.py, with that file's bf16 tolerance; fp8 KV uses the
tolerance of test_fp8_kv.py against the dequantized cache.

Unused block-table entries hold -1: a kernel that looks at one reads the wrong
rows and fails the comparison.
"""

from __future__ import annotations

import random

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16_TOL = dict(atol=3e-2, rtol=2e-2)
FP8_TOL = dict(atol=5e-2, rtol=5e-2)

BOUNDARY_LENS = [1, 31, 32, 33, 63, 64, 65, 127, 129, 257]


@pytest.fixture(scope="module", autouse=True)
def _check_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vllm_tgis_adapter_amd import ops

    assert ops.has_native(), "HIP extension must be built on a GPU box"


class Paged:
    """A paged KV pool in which every sequence owns `max_blocks` shuffled
    blocks, all filled with data, so lengths can change without refilling."""

    def __init__(self, nseq, kvh, hd, bs, max_blocks, fp8=False, seed=0):
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.nseq, self.kvh, self.hd, self.bs, self.max_blocks = nseq, kvh, hd, bs, max_blocks
        nb = nseq * max_blocks + 3
        shape = (nb, bs, kvh, hd)
        k = torch.randn(shape, dtype=torch.bfloat16, device="cuda", generator=g)
        v = torch.randn(shape, dtype=torch.bfloat16, device="cuda", generator=g)
        if fp8:
            k8, v8 = k.to(torch.float8_e4m3fn), v.to(torch.float8_e4m3fn)
            self.kc, self.vc = k8.view(torch.uint8), v8.view(torch.uint8)
            self.k32, self.v32 = k8.float(), v8.float()
        else:
            self.kc, self.vc = k, v
            self.k32, self.v32 = k.float(), v.float()
        perm = list(range(nb))
        random.Random(seed).shuffle(perm)
        self.owned = torch.tensor(perm[: nseq * max_blocks], dtype=torch.int32).view(
            nseq, max_blocks
        )

    def tables(self, seq_lens):
        t = torch.full((self.nseq, self.max_blocks), -1, dtype=torch.int32)
        for i, s in enumerate(seq_lens):
            n = (s + self.bs - 1) // self.bs
            t[i, :n] = self.owned[i, :n]
        return t.cuda()

    def reference(self, q, seq_lens):
        """fp32 dense attention per sequence; rows with seq_len 0 are None."""
        group = q.shape[1] // self.kvh
        outs = []
        for i, s in enumerate(seq_lens):
            if s == 0:
                outs.append(None)
                continue
            n = (s + self.bs - 1) // self.bs
            blocks = self.owned[i, :n].long().cuda()
            k = self.k32[blocks].reshape(-1, self.kvh, self.hd)[:s]
            v = self.v32[blocks].reshape(-1, self.kvh, self.hd)[:s]
            kk = k.repeat_interleave(group, dim=1)
            vv = v.repeat_interleave(group, dim=1)
            scores = torch.einsum("hd,shd->hs", q[i].float(), kk) * self.hd ** -0.5
            outs.append(torch.einsum("hs,shd->hd", torch.softmax(scores, -1), vv))
        return outs


def _decode(pool, q, seq_lens, tables=None, sl=None, out=None):
    from vllm_tgis_adapter_amd import ops

    if tables is None:
        tables = pool.tables(seq_lens)
    if sl is None:
        sl = torch.tensor(seq_lens, dtype=torch.int32, device="cuda")
    return ops.paged_attention_decode(
        q, pool.kc, pool.vc, tables, sl, pool.hd ** -0.5,
        pool.max_blocks * pool.bs, out=out,
    )


def _check(out, ref, tol, what=""):
    for i, r in enumerate(ref):
        if r is None:
            continue
        err = (out[i].float() - r).abs().max().item()
        assert torch.allclose(out[i].float(), r, **tol), (what, i, err)


def _q(nseq, nheads, hd, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(nseq, nheads, hd, dtype=torch.bfloat16, device="cuda", generator=g)


def _num_partitions(nseq, kvh, max_context):
    """Mirror of decode_mfma_num_partitions, to assert which path a case takes."""
    npart = max(1, min(32, 512 // (nseq * kvh)))
    return min(npart, max(1, ((max_context + 31) // 32) // 2))


SHAPES = [(8, 4, 128), (8, 8, 128), (2, 1, 64), (1, 8, 128), (2, 2, 64)]


@pytest.mark.parametrize("bs", [16, 32])
@pytest.mark.parametrize(("kvh", "group", "hd"), SHAPES)
def test_tile_boundaries_mixed_batch(kvh, group, hd, bs):
    """Tile-boundary lengths in one batch, table far wider than needed."""
    lens = BOUNDARY_LENS
    pool = Paged(len(lens), kvh, hd, bs, max_blocks=1024 // bs, seed=1)
    q = _q(len(lens), kvh * group, hd, seed=2)
    out = _decode(pool, q, lens)
    _check(out, pool.reference(q, lens), BF16_TOL)


@pytest.mark.parametrize(
    "lens", [[40], [700], [2000], [40, 700, 2000]], ids=["40", "700", "2000", "all3"]
)
def test_few_sequences_partitioned(lens):
    """npart > 1; the length-40 sequence leaves its later partitions empty."""
    kvh, group, hd, bs = 2, 4, 128, 16
    pool = Paged(len(lens), kvh, hd, bs, max_blocks=128, seed=3)
    assert _num_partitions(len(lens), kvh, 128 * bs) > 2
    q = _q(len(lens), kvh * group, hd, seed=4)
    out = _decode(pool, q, lens)
    _check(out, pool.reference(q, lens), BF16_TOL)


def _many_short_lens(kind):
    if kind == "drawn":
        rng = random.Random(7)
        return [rng.randint(1, 130) for _ in range(64)]
    return [BOUNDARY_LENS[i % len(BOUNDARY_LENS)] for i in range(64)]


@pytest.mark.parametrize("kind", ["drawn", "boundaries"])
def test_many_short_sequences_single_partition(kind):
    """nseq*kvh >= 512: one partition per (seq, head), output written by the
    attention kernel itself."""
    kvh, group, hd, bs = 8, 4, 128, 16
    lens = _many_short_lens(kind)
    pool = Paged(64, kvh, hd, bs, max_blocks=24, seed=5)
    assert _num_partitions(64, kvh, 24 * bs) == 1
    q = _q(64, kvh * group, hd, seed=6)
    out = _decode(pool, q, lens)
    _check(out, pool.reference(q, lens), BF16_TOL)


@pytest.mark.parametrize("nseq", [4, 64], ids=["partitioned", "single"])
def test_zero_length_row(nseq):
    """A row with seq_len 0 gives finite output and leaves its neighbours alone."""
    kvh, group, hd, bs = 8, 4, 128, 16
    lens = [(37 * i) % 200 + 1 for i in range(nseq)]
    lens[1] = 0
    pool = Paged(nseq, kvh, hd, bs, max_blocks=16, seed=8)
    q = _q(nseq, kvh * group, hd, seed=9)
    out = _decode(pool, q, lens)
    assert torch.isfinite(out.float()).all()
    _check(out, pool.reference(q, lens), BF16_TOL)


@pytest.mark.parametrize("nseq", [10, 64], ids=["partitioned", "single"])
def test_fp8_cache(nseq):
    kvh, group, hd, bs = 8, 4, 128, 16
    lens = [BOUNDARY_LENS[i % len(BOUNDARY_LENS)] for i in range(nseq)]
    lens[3] = 0
    pool = Paged(nseq, kvh, hd, bs, max_blocks=32, fp8=True, seed=10)
    q = _q(nseq, kvh * group, hd, seed=11)
    out = _decode(pool, q, lens)
    assert torch.isfinite(out.float()).all()
    _check(out, pool.reference(q, lens), FP8_TOL)


@pytest.mark.parametrize("nseq", [8, 64], ids=["partitioned", "single"])
def test_graph_replay_with_changed_lengths(nseq):
    """Capture once, then change seq_lens and block_tables in place: replays
    match the reference and an eager call bit for bit."""
    kvh, group, hd, bs = 8, 4, 128, 16
    max_blocks = 80
    pool = Paged(nseq, kvh, hd, bs, max_blocks=max_blocks, seed=12)
    assert (_num_partitions(nseq, kvh, max_blocks * bs) > 1) == (nseq == 8)
    q = _q(nseq, kvh * group, hd, seed=13)
    base = [[100] * 8,
            [1, 32, 33, 64, 65, 300, 641, 1279],
            [1280, 129, 2, 160, 161, 31, 97, 700]]
    plans = [[b[i % 8] for i in range(nseq)] for b in base]

    tables = pool.tables(plans[0])
    sl = torch.tensor(plans[0], dtype=torch.int32, device="cuda")
    out = torch.empty_like(q)
    _decode(pool, q, None, tables=tables, sl=sl, out=out)  # warm-up, eager
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _decode(pool, q, None, tables=tables, sl=sl, out=out)

    for lens in plans[1:] + plans[:1]:
        tables.copy_(pool.tables(lens))
        sl.copy_(torch.tensor(lens, dtype=torch.int32))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone()
        _check(got, pool.reference(q, lens), BF16_TOL, what=lens[:8])
        eager = _decode(pool, q, None, tables=tables, sl=sl)
        assert torch.equal(got, eager), lens[:8]


@pytest.mark.parametrize("nseq", [3, 64], ids=["partitioned", "single"])
def test_deterministic(nseq):
    kvh, group, hd, bs = 8, 4, 128, 16
    lens = [(53 * i) % 500 + 1 for i in range(nseq)]
    pool = Paged(nseq, kvh, hd, bs, max_blocks=32, seed=14)
    q = _q(nseq, kvh * group, hd, seed=15)
    a = _decode(pool, q, lens)
    b = _decode(pool, q, lens)
    assert torch.equal(a, b)
