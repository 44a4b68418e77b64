"""Microbench: fused MoE dispatch chain vs the torch chain (E16).

Times one MoEBlock.forward at the mixtral-8x7b dimensions (E=8, k=2, H=4096,
I=14336, TP=1, bf16) for T in {1, 64, 256, 512, 2048, 8192}, with the fused
route/dispatch/gather/combine kernels (the default) and with VTA_MOE_FUSED=0
(torch topk/argsort/histogram/gather/index_add_ around the same two grouped
GEMMs).  The two paths alternate inside each round so drift hits them alike;
the median round is reported with the min-max spread, plus the kernel launches
each path issues per forward.  The fused path passes at a T when its slowest
round is not slower than the torch chain's fastest round.
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from vllm_tgis_adapter_amd import ops
from vllm_tgis_adapter_amd.engine import ModelConfig
from vllm_tgis_adapter_amd.ops import reference
from vllm_tgis_adapter_amd.models.mixtral import MoEBlock

TOKENS = (1, 64, 256, 512, 2048, 8192)
PATHS = {"fused": "1", "torch": "0"}


def count_launches(fn) -> int:
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for ev in prof.events()
               if ev.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="mixtral-8x7b")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0,
                    help="least work per timed window")
    ap.add_argument("--tokens", type=int, nargs="*", default=list(TOKENS))
    ap.add_argument("--no-launch-count", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "moe_bench needs a GPU"
    mc = ModelConfig.from_model_arg(args.model, dtype="bfloat16")
    torch.manual_seed(0)
    moe = MoEBlock(mc).cuda()
    moe.gate.data.normal_(std=0.5)

    native_topk = ops.topk_softmax

    def run(path, x):
        # the baseline is the chain as it was before the fused kernels, so its
        # router runs the torch reference, not the new route stage
        os.environ["VTA_MOE_FUSED"] = PATHS[path]
        ops.topk_softmax = (native_topk if path == "fused"
                            else reference.topk_softmax)
        try:
            return moe(x)
        finally:
            ops.topk_softmax = native_topk

    rows = []
    for t in args.tokens:
        x = torch.randn(t, mc.hidden_size, dtype=torch.bfloat16, device="cuda") / 4
        res, iters, launches = {}, {}, {}
        for path in PATHS:
            res[path] = run(path, x).float()
            # warm up, then size the window from a rough timing
            for _ in range(3):
                run(path, x)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                run(path, x)
            torch.cuda.synchronize()
            rough = (time.perf_counter() - t0) / 5 * 1e3
            iters[path] = max(10, int(args.window_ms / rough))
            if not args.no_launch_count:
                launches[path] = count_launches(lambda: run(path, x))
        # faster-and-different is not faster: the torch chain rounds the
        # weights and each scaled row to bf16 and sums in bf16, the fused one
        # rounds once from f32: a few bf16 ulps of the largest term.  Rows
        # whose k-th and (k+1)-th logits are equal are left out: torch.topk
        # does not say which of two equal experts it takes.
        srt = torch.nn.functional.linear(x, moe.gate).sort(-1, descending=True).values
        clear = srt[:, moe.top_k - 1] != srt[:, moe.top_k]
        diff = (res["fused"] - res["torch"]).abs()[clear]
        tol = (2.0 ** -6 * res["torch"].abs()
               + 2.0 ** -7 * res["torch"].abs().max())[clear]
        assert bool((diff <= tol).all()), (t, diff.max().item())
        ms = {path: [] for path in PATHS}
        for _ in range(args.rounds):
            for path in PATHS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters[path]):
                    run(path, x)
                torch.cuda.synchronize()
                ms[path].append((time.perf_counter() - t0) / iters[path] * 1e3)
        row = {"T": t}
        for path in PATHS:
            row[path + "_ms"] = round(statistics.median(ms[path]), 4)
            row[path + "_min"] = round(min(ms[path]), 4)
            row[path + "_max"] = round(max(ms[path]), 4)
            row[path + "_launches"] = launches.get(path)
        row["torch_over_fused"] = round(row["torch_ms"] / row["fused_ms"], 3)
        row["fused_not_slower_beyond_spread"] = row["fused_max"] <= row["torch_min"]
        rows.append(row)
        print(f"T={t:5d} fused {row['fused_ms']:8.4f} ms "
              f"({row['fused_min']:.4f}-{row['fused_max']:.4f}, "
              f"{row['fused_launches']} launches)  "
              f"torch {row['torch_ms']:8.4f} ms "
              f"({row['torch_min']:.4f}-{row['torch_max']:.4f}, "
              f"{row['torch_launches']} launches)  "
              f"x{row['torch_over_fused']:.3f}", flush=True)
    os.environ.pop("VTA_MOE_FUSED", None)
    print(json.dumps({"model": args.model, "rounds": args.rounds, "rows": rows}))


if __name__ == "__main__":
    main()
