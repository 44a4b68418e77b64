"""Decode-GEMM shape microbench (r1 profile follow-up).

rocprofv3 r1 showed the hipBLASLt default picks for the llama-3-8b decode
shapes run at ~45% of HBM roofline and the lm-head GEMM at ~22%.  This
script times each shape as torch.matmul (the F.linear path) and prints
achieved GB/s vs the 8 TB/s roofline, optionally under TunableOp
(PYTORCH_TUNABLEOP_ENABLED=1 env) to evaluate shipping tuned configs.

Run on a GPU box:
  python tools/gemm_bench.py [--m 64] [--iters 200]
  PYTORCH_TUNABLEOP_ENABLED=1 PYTORCH_TUNABLEOP_TUNING=1 python tools/gemm_bench.py
  python tools/gemm_bench.py --quant   # int8/int4 linears at M > 64, four paths
"""

from __future__ import annotations

import argparse
import json
import os

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

# (name, N, K) for y[M,N] = x[M,K] @ W[N,K]^T — llama-3-8b TP=1 decode shapes
SHAPES = [
    ("qkv", 6144, 4096),
    ("o_proj", 4096, 4096),
    ("gate_up", 28672, 4096),
    ("down", 4096, 14336),
    ("lm_head", 128256, 4096),
]


def _fn(native):
    from vllm_tgis_adapter_amd import ops

    if native == "tile":
        return lambda x, w: ops.gemm_tile(x, w)
    if native:
        return ops.linear
    return torch.nn.functional.linear


def bench_shape(m: int, n: int, k: int, iters: int, dtype=torch.bfloat16,
                native: bool = False) -> float:
    fn = _fn(native)
    x = torch.randn(m, k, dtype=dtype, device="cuda")
    w = torch.randn(n, k, dtype=dtype, device="cuda")
    for _ in range(20):
        y = fn(x, w)
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        y = fn(x, w)
    t1.record()
    torch.cuda.synchronize()
    del y
    return t0.elapsed_time(t1) / iters  # ms


# --quant: the weight-quantized linears at M > 64 ------------------------------
QUANT_MS = [128, 256, 512, 1024, 2048, 8192]
PEAK_BF16_FLOPS = 2.5e15  # MI355X dense bf16 matrix peak
PEAK_HBM_BYTES = 8e12

# env that selects each path inside ops.linear_quant
QUANT_PATHS = {
    "a_torch_chain": {"VTA_QGEMM_TILE_MAX_M": "0", "VTA_QDEQUANT_NATIVE": "0"},
    "b_dequant_hip": {"VTA_QGEMM_TILE_MAX_M": "0", "VTA_QDEQUANT_NATIVE": "1"},
    "c_tile_q": {"VTA_QGEMM_TILE_MAX_M": "1000000", "VTA_QDEQUANT_NATIVE": "1"},
    "d_bf16": None,
}


def _time_ms(fn, iters):
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def quant_main(args):
    """Times the four paths alternately, `--rounds` times per shape, with
    device events; prints one JSON line per (qbits, shape, M) with each
    path's median ms and min..max spread, the bytes and FLOPs the fused
    kernel needs and which of the two bounds it."""
    from vllm_tgis_adapter_amd import ops

    def call(path, x, w, wq, sc, qbits):
        env = QUANT_PATHS[path]
        if env is None:
            return ops.linear(x, w)
        os.environ.update(env)
        return ops.linear_quant(x, wq, sc, qbits)

    shapes = [s for s in SHAPES if s[0] != "lm_head"]
    ms_list = [int(v) for v in args.quant_m.split(",")] if args.quant_m else QUANT_MS
    for qbits in (8, 4):
        for name, n, k in shapes:
            w = torch.randn(n, k, dtype=torch.bfloat16, device="cuda") * 0.05
            wq, sc = ops.quantize_weight(w, qbits)
            for m in ms_list:
                x = torch.randn(m, k, dtype=torch.bfloat16, device="cuda")
                fns = {p: (lambda p=p: call(p, x, w, wq, sc, qbits))
                       for p in QUANT_PATHS}
                iters = {}
                for p, fn in fns.items():  # warm every path at this shape
                    for _ in range(3):
                        fn()
                    torch.cuda.synchronize()
                    iters[p] = max(5, min(200, int(args.window_ms / _time_ms(fn, 3))))
                times = {p: [] for p in fns}
                for _ in range(args.rounds):
                    for p, fn in fns.items():
                        times[p].append(_time_ms(fn, iters[p]))
                flops = 2 * m * n * k
                nbytes = (m * k * 2 + n * k * qbits // 8 + sc.numel() * 4
                          + m * n * 2)
                t_f, t_b = flops / PEAK_BF16_FLOPS, nbytes / PEAK_HBM_BYTES
                row = {"qbits": qbits, "shape": name, "M": m, "N": n, "K": k,
                       "GFLOP": round(flops / 1e9, 2),
                       "MB": round(nbytes / 1e6, 2),
                       "bound": "flops" if t_f > t_b else "bytes",
                       "floor_ms": round(max(t_f, t_b) * 1e3, 4)}
                for p, ts in times.items():
                    ts = sorted(ts)
                    row[p] = {"ms": round(ts[len(ts) // 2], 4),
                              "min": round(ts[0], 4), "max": round(ts[-1], 4)}
                print(json.dumps(row), flush=True)
            if name == "gate_up":  # peak memory of one call, above the inputs
                x = torch.randn(512, k, dtype=torch.bfloat16, device="cuda")
                peak = {}
                for p in ("a_torch_chain", "b_dequant_hip", "c_tile_q"):
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    call(p, x, w, wq, sc, qbits)
                    torch.cuda.synchronize()
                    peak[p] = round(
                        (torch.cuda.max_memory_allocated() - base) / 2**20, 1)
                print(json.dumps({"qbits": qbits, "shape": name, "M": 512,
                                  "peak_MiB_above_inputs": peak}), flush=True)
            del w, wq, sc


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--m", type=int, default=64)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--quant", action="store_true",
                   help="time the quantized linears at M > 64: torch chain, "
                        "one-pass dequant, fused tile kernel, bf16")
    p.add_argument("--quant-m", default="",
                   help="comma-separated M list for --quant")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--window-ms", type=float, default=60.0,
                   help="--quant: device time per timed window")
    p.add_argument("--native", action="store_true",
                   help="route through ops.linear (custom skinny kernel)")
    p.add_argument("--tile", action="store_true",
                   help="force the 128x128-tile kernel (gemm_tile)")
    args = p.parse_args()
    assert torch.cuda.is_available()
    if args.quant:
        return quant_main(args)
    results = {}
    for name, n, k in SHAPES:
        ms = bench_shape(args.m, n, k, args.iters,
                         native="tile" if args.tile else args.native)
        bytes_moved = (args.m * k + n * k + args.m * n) * 2
        gbs = bytes_moved / (ms * 1e-3) / 1e9
        tf = 2 * args.m * n * k / (ms * 1e-3) / 1e12
        results[name] = {
            "ms": round(ms, 4),
            "GB/s": round(gbs, 1),
            "pct_of_8TBs": round(100 * gbs / 8000, 1),
            "TF": round(tf, 1),
        }
        print(name, results[name], flush=True)
    print(json.dumps({
        "native": "tile" if args.tile else args.native,
        "m": args.m,
        "tunableop": os.environ.get("PYTORCH_TUNABLEOP_ENABLED", "0"),
        "results": results,
    }))


if __name__ == "__main__":
    main()
