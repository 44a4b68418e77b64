"""Bitmap-driven logit edits (kernels/logits_edit.hip): the kernel and its CPU
reference against a plain f32 formula, the bitmap scatter against numpy, and
the sampler route that keeps penalised / guided rows on the fused path."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

INF = float("inf")
GPU = pytest.param("cuda", marks=pytest.mark.gpu)
EDIT_ROWS = [0, 2, 4]
PENALTIES = [1.3, 0.8, 1.3]


def _bitmap(sets, v, pad=False):
    """int32 [len(sets), W] bitmap built with numpy; pad sets the bits >= v."""
    w = ((v + 31) // 32 + 3) // 4 * 4
    bits = np.zeros((len(sets), w * 32), dtype=np.uint8)
    for r, ids in enumerate(sets):
        bits[r, list(ids)] = 1
    if pad:
        bits[:, v:] = 1
    words = np.packbits(bits, axis=1, bitorder="little").view("<u4")
    return torch.from_numpy(words.view(np.int32).copy())


def _raw(x):
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)


@functools.lru_cache(maxsize=None)
def _case(dtype, v):
    """Logits [5, v] and, per edit row, a seen set and an allow set (None on
    the last edit row).  Row 0 allows exactly one token; row 2 leaves word 0
    all-disallowed, word 1 all-allowed, word 2 mixed, and half of the rest."""
    g = torch.Generator().manual_seed(7 + v)
    logits = (torch.randn(5, v, generator=g) * 3).to(dtype)
    special = [5, 40, 70, 100]  # positive, negative, zero, -inf logits
    seen = []
    for r in EDIT_ROWS:
        logits[r, torch.tensor(special)] = torch.tensor(
            [1.5, -2.25, 0.0, -INF]).to(dtype)
        extra = torch.randint(0, v, (24,), generator=g).tolist()
        seen.append(sorted({0, v - 1, *special, *extra}))
    rest = torch.arange(96, v)[torch.rand(v - 96, generator=g) < 0.5].tolist()
    allow = [[40], sorted({*range(32, 64), *range(64, 80, 3), *rest}), None]
    assert 0 in seen[1] and 0 not in allow[1]  # seen and disallowed
    return logits, seen, allow


def _reference(logits, seen, allow, mode):
    ref = logits.clone()
    v = logits.shape[1]
    for e, r in enumerate(EDIT_ROWS):
        x = logits[r].float()
        if mode != "allow":
            hit = torch.zeros(v, dtype=torch.bool)
            hit[seen[e]] = True
            p = torch.tensor(PENALTIES[e], dtype=torch.float32)
            x = torch.where(hit, torch.where(x > 0, x / p, x * p), x)
        if mode != "penalty" and allow[e] is not None:
            ok = torch.zeros(v, dtype=torch.bool)
            ok[allow[e]] = True
            x = x.masked_fill(~ok, -INF)
        ref[r] = x.to(logits.dtype)
    return ref


@pytest.mark.parametrize("mode", ["penalty", "allow", "both"])
@pytest.mark.parametrize("v", [136, 5000, 128256])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("device", ["cpu", GPU])
def test_logits_edit_matches_f32_reference(device, dtype, v, mode):
    from vllm_tgis_adapter_amd import ops

    logits, seen, allow = _case(dtype, v)
    ref = _reference(logits, seen, allow, mode)
    assert not torch.equal(_raw(ref[0]), _raw(logits[0]))
    # seen bitmaps live in slots 1, 0, 2 of their pool; allow in 0, 1, none
    seen_bm = _bitmap([seen[1], seen[0], seen[2]], v).to(device)
    allow_bm = _bitmap([a for a in allow if a is not None], v, pad=True).to(device)
    rows = torch.tensor(EDIT_ROWS, dtype=torch.int32, device=device)
    pens = torch.tensor(PENALTIES if mode != "allow" else [1.0] * 3,
                        dtype=torch.float32, device=device)
    seen_slots = torch.tensor([1, 0, 2], dtype=torch.int32, device=device)
    allow_slots = torch.tensor([0, 1, -1], dtype=torch.int32, device=device)
    runs = []
    for _ in range(2):
        x = logits.clone().to(device)
        out = ops.logits_edit(
            x, rows, pens,
            seen_bm if mode != "allow" else None, seen_slots,
            allow_bm if mode != "penalty" else None, allow_slots)
        assert out is x
        runs.append(_raw(x.cpu()))
    assert torch.equal(runs[0][[1, 3]], _raw(logits)[[1, 3]])  # never touched
    assert torch.equal(runs[0], _raw(ref))
    assert torch.equal(runs[1], runs[0])  # bit-repeatable


@pytest.mark.parametrize("device", ["cpu", GPU])
def test_token_bitmap_scatter_matches_numpy(device):
    from vllm_tgis_adapter_amd import ops

    v = 5000
    first = [(0, 0), (0, 31), (0, 32), (0, 4999), (0, 31), (1, 7), (1, 4096),
             (1, 7), (0, 5000), (1, -1), (2, 5), (-1, 5), (0, 5119)]
    again = [(1, 9), (1, 4998), (0, 64)]

    def scatter(bm, pairs):
        s, t = (torch.tensor(c, dtype=torch.int32, device=device)
                for c in zip(*pairs))
        assert ops.token_bitmap_scatter(bm, s, t, v) is bm

    bm = _bitmap([[], []], v).to(device)
    scatter(bm, first)
    want = _bitmap([[0, 31, 32, 4999], [7, 4096]], v)
    assert torch.equal(bm.cpu(), want)
    # slot 1 is cleared and re-used; slot 0 keeps accumulating
    bm.index_fill_(0, torch.tensor([1], device=device), 0)
    scatter(bm, again)
    want = _bitmap([[0, 31, 32, 64, 4999], [9, 4998]], v)
    assert torch.equal(bm.cpu(), want)
    assert np.array_equal(ops.pack_token_bitmap([9, 4998, 5000, -1], v),
                          want[1].numpy().view(np.uint32))


def _requests(params, prompt):
    from vllm_tgis_adapter_amd.engine.request import Request

    return [Request(request_id=f"r{i}", prompt=None,
                    prompt_token_ids=list(prompt), sampling_params=p)
            for i, p in enumerate(params)]


def _penalise(row, ids, p):
    x = row.float().cpu().clone()
    idx = torch.tensor(sorted(set(ids)))
    x[idx] = torch.where(x[idx] > 0, x[idx] / p, x[idx] * p)
    return x.to(row.dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_sampler_keeps_penalty_rows_on_fused_path(dtype, monkeypatch):
    from vllm_tgis_adapter_amd.engine.sampler import Sampler
    from vllm_tgis_adapter_amd.engine.types import SamplingParams

    g = torch.Generator().manual_seed(11)
    logits = (torch.randn(4, 5000, generator=g) * 3).to(dtype)
    logits[1, 1234] = 30.0  # the penalised row's raw argmax, in its prompt
    logits[1, 77] = 25.0    # wins once 1234 is penalised: 30 / 1.5 = 20
    logits[1, 99] = 22.0    # wins once 77 is penalised too
    raw = torch.argmax(logits.float(), dim=-1).tolist()
    prompt = [1234, 2]

    def make():
        params = [SamplingParams(temperature=0.0, max_tokens=4) for _ in range(4)]
        params[1] = SamplingParams(temperature=0.0, max_tokens=4,
                                   repetition_penalty=1.5)
        return _requests(params, prompt)

    reqs = make()
    sampler = Sampler(device="cuda")
    out = sampler.try_launch_fused(logits.cuda(), reqs)
    assert out is not None  # the whole batch took the torch path before
    toks = out.tolist()
    assert toks[1] == int(torch.argmax(_penalise(logits[1], prompt, 1.5).float()))
    assert toks[1] == 77 and [toks[i] for i in (0, 2, 3)] == [raw[i] for i in (0, 2, 3)]
    # the sampled token joins the history: only the delta is scattered
    for r, t in zip(reqs, toks):
        r.output_token_ids.append(t)
    toks2 = sampler.try_launch_fused(logits.cuda(), reqs).tolist()
    assert toks2[1] == int(torch.argmax(
        _penalise(logits[1], prompt + [77], 1.5).float())) == 99
    assert [toks2[i] for i in (0, 2, 3)] == [raw[i] for i in (0, 2, 3)]
    if dtype == torch.float32:
        monkeypatch.setenv("VTA_SAMPLE_EDIT", "0")
        reqs = make()
        assert sampler.try_launch_fused(logits.cuda(), reqs) is None
        assert Sampler(device="cuda").sample(logits.cuda(), reqs).token_ids == toks


class _Guide:
    dead = False

    def __init__(self, ids):
        self.ids = ids

    def allowed_token_ids(self):
        return self.ids

    def advance(self, token_id):
        pass


@pytest.mark.gpu
@pytest.mark.parametrize("sampling", [False, True])
def test_sampler_keeps_guided_rows_on_fused_path(sampling):
    from vllm_tgis_adapter_amd.engine.sampler import Sampler
    from vllm_tgis_adapter_amd.engine.types import SamplingParams

    g = torch.Generator().manual_seed(12)
    logits = (torch.randn(4, 5000, generator=g) * 3).to(torch.bfloat16)
    raw = torch.argmax(logits.float(), dim=-1).tolist()
    allowed = [3, 999, 2500, 4999]
    best = allowed[int(torch.argmax(logits[2, allowed].float()))]

    def run():
        params = [SamplingParams(temperature=0.0, max_tokens=4) for _ in range(4)]
        if sampling:
            params[2] = SamplingParams(temperature=1.0, top_k=40, seed=5,
                                       max_tokens=4)
        reqs = _requests(params, [1, 2])
        reqs[2].guided_state = _Guide(allowed)
        out = Sampler(device="cuda").try_launch_fused(logits.cuda(), reqs)
        assert out is not None
        return out.tolist()

    a, b = run(), run()
    assert a == b
    assert [a[i] for i in (0, 1, 3)] == [raw[i] for i in (0, 1, 3)]
    assert a[2] in allowed and (sampling or a[2] == best)
