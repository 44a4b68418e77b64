"""Microbench: BGMV vs segmented MFMA multi-LoRA kernels (E12).

Times ops.lora_bgmv against ops.lora_sgmv on the llama-3-8b projection shapes
(K=4096 with N=6144 / N=4096, K=14336 with N=4096), R in {16, 64}, T in
{64, 256, 512, 1024, 8192}, 4 adapters, and two slot patterns:
  prefill  contiguous per-sequence segments of 512 tokens, adapters cycling
  decode   a random slot per token
The two kernels alternate inside each round so drift hits them alike; the
median round is reported with the min-max spread.  The dispatch only sees T,
so the threshold is the smallest benched T from which (at that T and every
larger one) SGMV's slowest round beats BGMV's fastest round on every prefill
shape and, for T a pure decode step can reach (<= max_num_seqs = 256), its
median is not above BGMV's on any decode-like shape.
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

SHAPES = ((4096, 6144), (4096, 4096), (14336, 4096))  # (K, N)
RANKS = (16, 64)
TOKENS = (64, 256, 512, 1024, 8192)
ADAPTERS = 4
SEGMENT = 512
# SchedulerConfig.max_num_seqs: a step with more tokens than this holds
# multi-token prefill runs, so a slot per token cannot be its pattern
MAX_DECODE_T = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0,
                    help="least work per timed window")
    ap.add_argument("--tokens", type=int, nargs="*", default=list(TOKENS))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lora_bench needs a GPU"
    dt = torch.bfloat16
    rows = []
    for k, n in SHAPES:
        for r in RANKS:
            torch.manual_seed(0)
            a_stack = torch.randn(ADAPTERS, r, k, dtype=dt, device="cuda") / 8
            b_stack = torch.randn(ADAPTERS, n, r, dtype=dt, device="cuda") / 8
            scales = torch.rand(ADAPTERS, dtype=torch.float32, device="cuda") + 0.5
            for t in args.tokens:
                x = torch.randn(t, k, dtype=dt, device="cuda") / 4
                base = torch.randn(t, n, dtype=dt, device="cuda")
                out = base.clone()
                assert ops.lora_sgmv_usable(x, out, a_stack, b_stack, 0)
                patterns = {
                    "prefill": (torch.arange(t) // SEGMENT) % ADAPTERS,
                    "decode": torch.randint(0, ADAPTERS, (t,)),
                }
                for pname, slots in patterns.items():
                    slots = slots.to(torch.int32).cuda()
                    fns = {"bgmv": ops.lora_bgmv, "sgmv": ops.lora_sgmv}
                    res, iters = {}, {}
                    for name, fn in fns.items():
                        out.copy_(base)
                        fn(out, x, a_stack, b_stack, slots, scales, 0)
                        res[name] = out.float()
                        # warm up, then size the window from a rough timing
                        for _ in range(3):
                            fn(out, x, a_stack, b_stack, slots, scales, 0)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(5):
                            fn(out, x, a_stack, b_stack, slots, scales, 0)
                        torch.cuda.synchronize()
                        rough = (time.perf_counter() - t0) / 5 * 1e3
                        iters[name] = max(10, int(args.window_ms / rough))
                    # faster-and-different is not faster: same seeded inputs,
                    # both round out once from an f32 sum
                    diff = (res["bgmv"] - res["sgmv"]).abs()
                    tol = 2e-3 + 2.0 ** -7 * res["bgmv"].abs()
                    assert bool((diff <= 2 * tol).all()), (k, n, r, t, pname)
                    ms = {name: [] for name in fns}
                    for _ in range(args.rounds):
                        for name, fn in fns.items():
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            for _ in range(iters[name]):
                                fn(out, x, a_stack, b_stack, slots, scales, 0)
                            torch.cuda.synchronize()
                            ms[name].append(
                                (time.perf_counter() - t0) / iters[name] * 1e3)
                    row = {"K": k, "N": n, "R": r, "T": t, "pattern": pname,
                           "ksplit": ops._C.lora_sgmv_num_ksplit(t, k)}
                    for name in fns:
                        row[name + "_ms"] = round(statistics.median(ms[name]), 4)
                        row[name + "_min"] = round(min(ms[name]), 4)
                        row[name + "_max"] = round(max(ms[name]), 4)
                    row["bgmv_over_sgmv"] = round(row["bgmv_ms"] / row["sgmv_ms"], 2)
                    row["sgmv_wins_beyond_spread"] = row["sgmv_max"] < row["bgmv_min"]
                    rows.append(row)
                    print(f"K={k:5d} N={n:4d} R={r:2d} T={t:4d} {pname:7s} "
                          f"bgmv {row['bgmv_ms']:8.4f} ms "
                          f"({row['bgmv_min']:.4f}-{row['bgmv_max']:.4f})  "
                          f"sgmv {row['sgmv_ms']:8.4f} ms "
                          f"({row['sgmv_min']:.4f}-{row['sgmv_max']:.4f})  "
                          f"x{row['bgmv_over_sgmv']:.2f}", flush=True)
    threshold = None
    for t in sorted(args.tokens, reverse=True):
        at_t = [r for r in rows if r["T"] == t]
        if all(r["sgmv_wins_beyond_spread"] if r["pattern"] == "prefill"
               else t > MAX_DECODE_T or r["sgmv_ms"] <= r["bgmv_ms"]
               for r in at_t):
            threshold = t
        else:
            break
    print(json.dumps({"rounds": args.rounds, "threshold_min_t": threshold,
                      "rows": rows}))


if __name__ == "__main__":
    main()
