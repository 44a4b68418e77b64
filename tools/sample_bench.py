"""Microbench: fused top-k/top-p sampler vs the torch chain it replaces (E7).

Times, at [512, 128256] bf16 with top_k=50 / top_p=0.9 on every row:
  torch_chain       float() -> divide -> _apply_top_k_top_p -> softmax ->
                    divide by noise -> argmax (the sampler's slow path)
  sample_topk_topp  the fused radix-select kernel
  sample_argmax     the unfiltered one-pass kernel on the same logits (scale)
  sample_topk_topp_unfiltered  the fused kernel with every filter off, which
                    must cost what sample_argmax costs
The variants alternate inside each round so drift hits them alike; the
median round is reported with the min-max spread.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from vllm_tgis_adapter_amd import ops
from vllm_tgis_adapter_amd.engine.sampler import _apply_top_k_top_p


class _Guide:
    """guided_state stand-in with a fixed allow list, packed on every call
    (a real GuidedState packs once per automaton state)."""
    dead = False

    def __init__(self, ids):
        self.ids = ids

    def allowed_token_ids(self):
        return self.ids


def edit_bench(args):
    """--edit: a batch with repetition-penalty / guided rows through today's
    Sampler.sample torch route (VTA_SAMPLE_EDIT=0) against logits_edit + the
    fused sampler, greedy rows, bf16 logits.  Each call is timed on the host
    clock up to the token list (which synchronises), so Python set building,
    uploads and kernels all count.  Cases:
      all_first   every row penalised, 640-token history, first step: a new
                  sampler scatters every prompt
      all_steady  the same batch afterwards: one new token per row per step
      one_of_n    1 penalised row, the rest plain
      guided_8    8 guided rows allowing ~100 tokens each, the rest plain
    """
    import os
    import random

    from vllm_tgis_adapter_amd.engine.request import Request
    from vllm_tgis_adapter_amd.engine.sampler import Sampler
    from vllm_tgis_adapter_amd.engine.types import SamplingParams

    n, v = args.rows, args.vocab
    torch.manual_seed(0)
    base = (torch.randn(n, v, device="cuda") * 3).to(torch.bfloat16)
    logits = base.clone()

    rng = random.Random(0)
    prompts = [[rng.randrange(v) for _ in range(640)] for _ in range(n)]
    allowed = [sorted(rng.sample(range(v), 100)) for _ in range(n)]

    def requests(pen_rows=(), guided_rows=()):
        reqs = []  # both routes, and every first step, see the same requests
        for i in range(n):
            pen = 1.2 if i in pen_rows else 1.0
            r = Request(
                request_id=f"r{i}", prompt=None, prompt_token_ids=prompts[i],
                sampling_params=SamplingParams(
                    temperature=0.0, max_tokens=4096, repetition_penalty=pen))
            if i in guided_rows:
                r.guided_state = _Guide(allowed[i])
            reqs.append(r)
        return reqs

    def call(sampler, reqs, fused):
        os.environ["VTA_SAMPLE_EDIT"] = "1" if fused else "0"
        logits.copy_(base)  # what the lm-head does: fresh logits every step
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if fused:
            out = sampler.try_launch_fused(logits, reqs)
            assert out is not None, "batch left the fused path"
            toks = sampler.finish_fused(out.tolist()).token_ids
        else:
            toks = sampler.sample(logits, reqs).token_ids
        dt = (time.perf_counter() - t0) * 1e3
        for r, t in zip(reqs, toks):
            r.output_token_ids.append(t)
        return dt, toks

    every = range(n)
    cases = {
        "all_first": dict(pen_rows=every, fresh=True),
        "all_steady": dict(pen_rows=every),
        "one_of_n": dict(pen_rows=(n // 2,)),
        "guided_8": dict(guided_rows=tuple(range(0, n, max(1, n // 8)))[:8]),
    }
    res = {"rows": n, "vocab": v, "rounds": args.rounds, "iters": args.iters}
    for name, spec in cases.items():
        fresh = spec.pop("fresh", False)
        state = {}
        for fused in (False, True):
            sampler, reqs = Sampler(device="cuda"), requests(**spec)
            for _ in range(2):  # warm-up: code objects, pinned staging, pool
                _, toks = call(sampler, reqs, fused)
            state[fused] = [sampler, reqs, toks]
        res[name + "_tokens_agree"] = sum(
            a == b for a, b in zip(state[False][2], state[True][2])) / n
        ms = {False: [], True: []}
        for _ in range(args.rounds):
            for fused in (False, True):
                total = 0.0
                for _ in range(args.iters):
                    if fresh:  # first step: nothing scattered yet
                        state[fused][0]._seen = None
                        state[fused][1] = requests(**spec)
                    total += call(state[fused][0], state[fused][1], fused)[0]
                ms[fused].append(total / args.iters)
        for fused, label in ((False, "torch"), (True, "fused")):
            res[f"{name}_{label}_ms"] = round(statistics.median(ms[fused]), 3)
            print(f"{name} {label}: median {statistics.median(ms[fused]):.3f} ms"
                  f"  (min {min(ms[fused]):.3f}, max {max(ms[fused]):.3f}, "
                  f"{args.rounds} rounds x {args.iters} calls)")
        # the gate: slowest fused round under the fastest torch round
        res[name + "_fused_wins"] = max(ms[True]) < min(ms[False])
    os.environ.pop("VTA_SAMPLE_EDIT", None)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--edit", action="store_true",
                    help="penalty / guided rows: torch route vs logits_edit")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sample_bench needs a GPU"
    if args.edit:
        return edit_bench(args)
    n, v = args.rows, args.vocab
    torch.manual_seed(0)
    logits = (torch.randn(n, v, device="cuda") * 3).to(torch.bfloat16)
    noise = torch.empty(n, v, dtype=torch.float32, device="cuda").exponential_()
    temps = torch.full((n,), 0.8, dtype=torch.float32, device="cuda")
    top_k = torch.full((n,), 50, dtype=torch.int32, device="cuda")
    top_p = torch.full((n,), 0.9, dtype=torch.float32, device="cuda")
    top_k_l = top_k.long()
    out = torch.empty(n, dtype=torch.long, device="cuda")
    kept = torch.empty(n, dtype=torch.int32, device="cuda")

    def torch_chain():
        sub = logits.float() / temps.unsqueeze(1)
        sub = _apply_top_k_top_p(sub, top_k_l, top_p)
        probs = torch.softmax(sub, dim=-1)
        return torch.argmax(probs / noise, dim=-1)

    def fused():
        ops.sample_topk_topp(out, logits, temps, noise, top_k, top_p, kept)
        return out

    def argmax_only():
        ops.sample_argmax(out, logits, temps, noise)
        return out

    off_k = torch.zeros_like(top_k)
    off_p = torch.ones_like(top_p)

    def fused_unfiltered():
        ops.sample_topk_topp(out, logits, temps, noise, off_k, off_p)
        return out

    # (name, fn, iterations per timed window): the kernels get 10x the
    # iterations so their windows are not clock-resolution sized
    variants = (("torch_chain", torch_chain, args.iters),
                ("sample_topk_topp", fused, 10 * args.iters),
                ("sample_argmax", argmax_only, 10 * args.iters),
                ("sample_topk_topp_unfiltered", fused_unfiltered,
                 10 * args.iters))
    # same tokens wherever the unstable torch sort cannot matter (no tie at
    # the cut) — reported, not asserted: the GPU tests own correctness
    agree = (torch_chain() == fused().clone()).float().mean().item()
    for _, fn, _ in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in variants}
    for _ in range(args.rounds):
        for name, fn, iters in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / iters * 1e3)
    res = {"rows": n, "vocab": v, "rounds": args.rounds, "iters": args.iters,
           "token_agreement_with_torch_chain": round(agree, 4),
           "mean_kept": round(kept.float().mean().item(), 2)}
    for name, _, _ in variants:
        med = statistics.median(ms[name])
        res[name + "_ms"] = round(med, 4)
        print(f"{name}: median {med:.3f} ms  (min {min(ms[name]):.3f}, "
              f"max {max(ms[name]):.3f}, {args.rounds} rounds)")
    res["speedup_vs_torch_chain"] = round(
        res["torch_chain_ms"] / res["sample_topk_topp_ms"], 2)
    res["ratio_to_sample_argmax"] = round(
        res["sample_topk_topp_ms"] / res["sample_argmax_ms"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
