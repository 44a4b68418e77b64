"""Microbench: fused MoE dispatch chain vs the torch chain (E16).

Times one MoEBlock.forward at the mixtral-8x7b dimensions (E=8, k=2, H=4096,
I=14336, TP=1, bf16) for T in {1, 64, 256, 512, 2048, 8192}, with the fused
route/dispatch/gather/combine kernels (the default) and with VTA_MOE_FUSED=0
(torch topk/argsort/histogram/gather/index_add_ around the same two grouped
GEMMs).  The two paths alternate inside each round so drift hits them alike;
the median round is reported with the min-max spread, plus the kernel launches
each path issues per forward.  The fused path passes at a T when its slowest
round is not slower than the torch chain's fastest round.

--quant {int8,int4} instead times the block with packed expert weights
(kernels/moe_gemm_q.hip) against the bf16 block holding the same effective
weights, alternating inside each round, and the two grouped GEMMs on their own
on the same routing, with the GB/s of weight bytes they stream (packed bytes
and scales of the experts that own rows, computed from shapes).  --inter 3584
runs the TP=4 slice.  With --cutover the two sides are the fused quantized
GEMM and one-pass dequant + bf16 moe_gemm, which places
ops._MOE_QGEMM_MAX_ROWS.
"""
import argparse
import copy
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


def alternate(fns, rounds, window_ms, before=lambda name: None):
    """Per-call ms of each fn over `rounds` rounds, alternating inside a
    round; every window holds at least window_ms of work.  before(name) runs
    ahead of each of name's windows, outside the timed region."""
    iters = {}
    for name, fn in fns.items():
        before(name)
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        rough = (time.perf_counter() - t0) / 5 * 1e3
        iters[name] = max(10, int(window_ms / rough))
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            before(name)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters[name]):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / iters[name] * 1e3)
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}


def quant_main(args, mc):
    """Quantized experts against bf16 (default), or, with --cutover, the
    fused quantized GEMMs against dequant + bf16 moe_gemm."""
    qbits = 8 if args.quant == "int8" else 4
    torch.manual_seed(0)
    base = torch.cuda.memory_allocated()
    with torch.device("cuda"):
        moe = MoEBlock(mc)
    moe.gate.data.normal_(std=0.5)
    bf16_alloc = torch.cuda.memory_allocated() - base
    moe_q = copy.deepcopy(moe)
    moe_q.quantize_(qbits)
    torch.cuda.empty_cache()
    q_alloc = torch.cuda.memory_allocated() - base - bf16_alloc
    # both blocks hold the same effective weights
    for name in ("w13", "w2"):
        wq, sc = getattr(moe_q, name + "_q"), getattr(moe_q, name + "_scale")
        getattr(moe, name).data.copy_(ops.dequantize_weight(
            wq.flatten(0, 1), sc.flatten(0, 1), qbits).view_as(getattr(moe, name)))
    e, h, i = moe.num_experts, moe.hidden, moe.inter
    shape = {"gated": (2 * i, h), "down": (h, i)}  # (rows, K) per expert
    elems = {g: n * k for g, (n, k) in shape.items()}
    # packed bytes + f32 scales (one per row, or per row and 128-k group)
    qbytes = {g: n * k * qbits // 8 + 4 * n * (1 if qbits == 8 else k // 128)
              for g, (n, k) in shape.items()}
    mem = {"expert_bytes_bf16": e * 3 * i * h * 2,
           "expert_bytes_" + args.quant: e * sum(qbytes.values()),
           "block_allocated_bf16": bf16_alloc, "block_allocated_quant": q_alloc,
           "fallback_transient_bf16_bytes": e * max(elems.values()) * 2}
    print(json.dumps(mem), flush=True)

    rows = []
    for t in args.tokens:
        x = torch.randn(t, h, dtype=torch.bfloat16, device="cuda") / 4
        _, _, seg, src_row, _ = ops.moe_dispatch(
            torch.nn.functional.linear(x, moe.gate), moe.top_k)
        active = int((seg[1:] > seg[:-1]).sum())
        hq = moe_q._grouped(x, "w13", seg, True, rows=src_row)
        quant = {"gated": lambda: moe_q._grouped(x, "w13", seg, True, rows=src_row),
                 "down": lambda: moe_q._grouped(hq, "w2", seg, False)}
        other = {"gated": lambda: ops.moe_gemm(x, moe.w13, seg, True, rows=src_row),
                 "down": lambda: ops.moe_gemm(hq, moe.w2, seg, False)}
        os.environ["VTA_MOE_QGEMM_MAX_ROWS"] = str(2 ** 30)
        want, got = moe(x).float(), moe_q(x).float()
        tol = 2.0 ** -6 * want.abs() + 2.0 ** -7 * want.abs().max()
        assert bool(((got - want).abs() <= tol).all()), t
        if args.cutover:  # the comparator is the fallback on the same packed weights
            other = quant
            fns = {}
        else:
            fns = {"block_q": lambda: moe_q(x), "block_ref": lambda: moe(x)}
        for g in ("gated", "down"):
            fns[g + "_q"], fns[g + "_ref"] = quant[g], other[g]

        def set_cutover(name):  # 0 sends the comparator down the fallback
            os.environ["VTA_MOE_QGEMM_MAX_ROWS"] = (
                "0" if args.cutover and name.endswith("_ref") else str(2 ** 30))

        res = alternate(fns, args.rounds, args.window_ms, set_cutover)
        row = {"T": t, "R": t * moe.top_k, "active_experts": active,
               "tile_rows": ops._C.moe_gemm_q_tile_rows(t * moe.top_k, e)}
        for name, (med, lo, hi) in res.items():
            row[name + "_ms"] = [round(v, 4) for v in (med, lo, hi)]
        for g in ("gated", "down"):
            row[g + "_q_GBps"] = round(active * qbytes[g] / res[g + "_q"][0] / 1e6, 1)
            if not args.cutover:
                row[g + "_ref_GBps"] = round(
                    active * elems[g] * 2 / res[g + "_ref"][0] / 1e6, 1)
            row[g + "_q_wins"] = res[g + "_q"][2] <= res[g + "_ref"][1]
        if not args.cutover:
            row["block_q_wins"] = res["block_q"][2] <= res["block_ref"][1]
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.environ.pop("VTA_MOE_QGEMM_MAX_ROWS", None)
    print(json.dumps({"model": args.model, "inter": i, "quant": args.quant,
                      "mode": "cutover" if args.cutover else "vs_bf16",
                      "rounds": args.rounds, "memory": mem, "rows": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="mixtral-8x7b")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0,
                    help="least work per timed window")
    ap.add_argument("--tokens", type=int, nargs="*", default=list(TOKENS))
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--quant", choices=("int8", "int4"),
                    help="time packed experts against bf16 (see module doc)")
    ap.add_argument("--cutover", action="store_true",
                    help="with --quant: fused quantized GEMM vs dequant + bf16")
    ap.add_argument("--inter", type=int,
                    help="intermediate size override (3584 = the TP=4 slice)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "moe_bench needs a GPU"
    mc = ModelConfig.from_model_arg(args.model, dtype="bfloat16")
    if args.inter:
        mc.intermediate_size = args.inter
    if args.quant:
        return quant_main(args, mc)
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
