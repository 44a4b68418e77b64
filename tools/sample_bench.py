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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sample_bench needs a GPU"
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
