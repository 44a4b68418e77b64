"""Fused top-k / top-p sampler (kernels/sampling_topk_topp.hip) against a
float64 CPU reference written from its semantics: stable descending sort,
whole-row softmax, exclusive prefix mass, kept = first max(1, min(k, m_p))."""

from __future__ import annotations

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

INF = float("inf")


def _sorted_row(logits_row, temp):
    """(z, stable descending order, exclusive prefix mass along it), f64."""
    z = logits_row.double() / temp
    order = torch.sort(z, descending=True, stable=True).indices
    probs = torch.softmax(z, dim=0)[order]
    return z, order, probs.cumsum(0) - probs


@functools.lru_cache(maxsize=None)
def _case(dtype, v):
    """One row per kind of request: logits, temps, top_k, top_p (f32 values the
    kernel sees), all on the CPU.  top_p is the midpoint of two successive
    prefix masses at least 2e-3 apart, so f32 accumulation cannot move the
    cut."""
    g = torch.Generator().manual_seed(1234 + v)
    # (temperature, top_k, number kept by top_p or None, literal top_p)
    spec = [
        (0.0, 5, 2, None),      # 0 greedy, filters ignored
        (0.8, -1, None, 1.0),   # 1 plain temperature
        (0.7, 1, None, 1.0),    # 2
        (0.7, 7, None, 1.0),    # 3
        (1.0, v + 5, None, 1.0),  # 4 top_k >= V: off
        (1.0, -1, 4, None),     # 5 top_p only
        (1.2, 3, 6, None),      # 6 both, k binds
        (0.9, 20, 5, None),     # 7 both, p binds
        (1.0, -1, None, 1e-6),  # 8 keeps exactly one
        (1.0, 3, None, 1.0),    # 9 all logits equal: keeps indices 0, 1, 2
        (0.7, 5, None, 1.0),    # 10 some -inf
        (0.7, 7, None, 1.0),    # 11 cut inside a tie group
    ]
    n = len(spec)
    logits = (torch.randn(n, v, generator=g) * 3).to(dtype)
    logits[9] = 1.25
    logits[10, torch.tensor([0, 3, v // 2, v - 1])] = -INF
    # row 11: the 7th-largest value also at one earlier and one later index
    order = torch.sort(logits[11].double(), descending=True, stable=True).indices
    i6 = int(order[6])
    top7 = set(order[:7].tolist())
    early = next(i for i in range(i6 - 1, -1, -1) if i not in top7)
    late = next(i for i in range(i6 + 1, v) if i not in top7)
    logits[11, early] = logits[11, i6]
    logits[11, late] = logits[11, i6]

    temps = torch.tensor([s[0] for s in spec], dtype=torch.float32)
    top_k = torch.tensor([s[1] for s in spec], dtype=torch.int32)
    top_p = []
    for i, (t, _, keep_p, lit) in enumerate(spec):
        if keep_p is None:
            top_p.append(lit)
            continue
        _, _, s = _sorted_row(logits[i], t if t > 0 else 1.0)
        assert s[keep_p] - s[keep_p - 1] >= 2e-3, (i, s[:8])
        top_p.append(float((s[keep_p] + s[keep_p - 1]) / 2))
    return logits, temps, top_k, torch.tensor(top_p, dtype=torch.float32)


def _reference(logits, temps, top_k, top_p, noise, probe):
    """Applies the probe to `noise` in place; returns (tokens, kept counts,
    smallest best-vs-second race margin over the sampling rows)."""
    n, v = logits.shape
    toks, kept, margin = [], [], INF
    for i in range(n):
        t, k, p = float(temps[i]), int(top_k[i]), float(top_p[i])
        if t == 0.0:
            toks.append(int(torch.argmax(logits[i].double())))
            kept.append(v)
            continue
        z, order, s = _sorted_row(logits[i], t)
        k = k if 0 < k < v else v
        c = max(1, min(k, int((s <= p).sum()))) if (k < v or p < 1.0) else v
        if c < v:  # make the mask boundary decide the outcome
            noise[i, order[c] if probe == "first_excluded" else order[c - 1]] = 1e-30
        idx = order[:c].sort().values  # index order: argmax ties -> lowest
        race = z[idx] - noise[i, idx].double().log()
        toks.append(int(idx[torch.argmax(race)]))
        kept.append(c)
        if c > 1:
            top2 = torch.topk(race, 2).values
            margin = min(margin, float(top2[0] - top2[1]))
    return toks, kept, margin


@pytest.mark.parametrize("probe", ["first_excluded", "last_kept"])
# 5003: rows start off a 16-byte boundary (head and tail tokens)
@pytest.mark.parametrize("v", [264, 5000, 5003, 128256])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_kernel_matches_reference(dtype, v, probe):
    from vllm_tgis_adapter_amd import ops

    logits, temps, top_k, top_p = _case(dtype, v)
    n = logits.shape[0]
    noise = torch.empty(n, v).exponential_(
        generator=torch.Generator().manual_seed(99))
    ref_tok, ref_kept, margin = _reference(
        logits, temps, top_k, top_p, noise, probe)
    # an f32 near-tie in the race must not be what decides a mismatch
    assert margin > 1e-3, margin
    assert ref_kept[2] == 1 and ref_kept[8] == 1 and ref_kept[9] == 3
    assert ref_kept[6] == 3 and ref_kept[7] == 5 and ref_kept[11] == 7

    dev = [x.cuda() for x in (logits, temps, noise, top_k, top_p)]
    runs = []
    for _ in range(2):
        out = torch.full((n,), -1, dtype=torch.long, device="cuda")
        kept = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        ops.sample_topk_topp(out, dev[0], dev[1], dev[2], dev[3], dev[4], kept)
        runs.append((out.tolist(), kept.tolist()))
    assert runs[0][0] == ref_tok
    assert runs[0][1] == ref_kept
    assert runs[1] == runs[0]  # run-to-run deterministic


def _requests(params):
    from vllm_tgis_adapter_amd.engine.request import Request

    return [Request(request_id=f"r{i}", prompt=None, prompt_token_ids=[1, 2],
                    sampling_params=p) for i, p in enumerate(params)]


@pytest.mark.parametrize("filt", [{"top_k": 1}, {"top_p": 1e-6}])
def test_sampler_keeps_filtered_rows_on_fused_path(filt):
    from vllm_tgis_adapter_amd.engine.sampler import Sampler
    from vllm_tgis_adapter_amd.engine.types import SamplingParams

    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(4, 5000, generator=g) * 3).to(torch.bfloat16).cuda()
    reqs = _requests([SamplingParams(temperature=1.0, max_tokens=4, **filt)
                      for _ in range(4)])
    out = Sampler(device="cuda").try_launch_fused(logits, reqs)
    assert out is not None  # the torch path took such batches before
    assert out.tolist() == torch.argmax(logits.float().cpu(), dim=-1).tolist()


def test_sampler_mixed_seeded_top_k_and_greedy():
    from vllm_tgis_adapter_amd.engine.sampler import Sampler
    from vllm_tgis_adapter_amd.engine.types import SamplingParams

    g = torch.Generator().manual_seed(6)
    logits = (torch.randn(4, 5000, generator=g) * 3).to(torch.bfloat16).cuda()
    argmax = torch.argmax(logits.float().cpu(), dim=-1).tolist()
    kth = torch.topk(logits[1], 40).values[-1]

    def run():
        params = [SamplingParams(temperature=0.0, max_tokens=4)
                  for _ in range(4)]
        params[1] = SamplingParams(temperature=1.0, top_k=40, seed=77,
                                   max_tokens=4)
        out = Sampler(device="cuda").try_launch_fused(
            logits.clone(), _requests(params))
        assert out is not None
        return out.tolist()

    a, b = run(), run()
    assert a == b
    assert [a[i] for i in (0, 2, 3)] == [argmax[i] for i in (0, 2, 3)]
    assert logits[1, a[1]] >= kth
