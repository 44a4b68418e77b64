"""Paged-attention kernel microbench (prefill + decode) on llama-3-8b shapes."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from vllm_tgis_adapter_amd import ops


def bench(fn, iters=50):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3  # us


def copy_probe_tbps(nbytes):
    """Memory ceiling for a decode case: a plain device copy of a buffer the
    size of the case's KV stream, timed like the kernel.  Counts the bytes
    read plus the bytes written."""
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty_like(src)
    us = bench(lambda: dst.copy_(src))
    return 2 * nbytes / us / 1e6


def bench_alternating(fns, windows=7, iters=20):
    """Time several callables in alternating windows (same process, same
    inputs) so drift on a shared host hits all of them alike.  Returns per
    callable (median us, min us, max us) over the windows."""
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) / iters * 1e3)
    return {n: (statistics.median(t), min(t), max(t)) for n, t in times.items()}


# (name, heads, kv heads, head_dim, q_len, fp8 KV); batch 512 x ctx 576
VERIFY_CASES = [
    ("verify q2", 32, 8, 128, 2, False),
    ("verify q5", 32, 8, 128, 5, False),
    ("verify q8", 32, 8, 128, 8, False),
    ("verify q5 group8 (64h/8kv)", 64, 8, 128, 5, False),
    ("verify q5 fp8-kv", 32, 8, 128, 5, True),
]


def verify_cases(bs, out):
    """Short verify chunks over a long context: the routed path, the parent
    path (VTA_ATTN_MULTIQ=0, read per call) and single-token decode on the
    same KV.  TB/s counts every KV byte once."""
    nseq, ctx = 512, 576
    nb = (ctx + bs - 1) // bs
    for name, heads, kvh, hd, q_len, fp8 in VERIFY_CASES:
        kc = torch.randn(nseq * nb + 8, bs, kvh, hd, dtype=torch.bfloat16, device="cuda")
        vc = torch.randn_like(kc)
        if fp8:
            kc = kc.to(torch.float8_e4m3fn).view(torch.uint8)
            vc = vc.to(torch.float8_e4m3fn).view(torch.uint8)
        q = torch.randn(nseq * q_len, heads, hd, dtype=torch.bfloat16, device="cuda")
        q1 = q[:nseq].contiguous()
        tables = torch.arange(nseq * nb, dtype=torch.int32, device="cuda").reshape(nseq, nb)
        qsl = torch.arange(0, nseq * q_len + 1, q_len, dtype=torch.int32, device="cuda")
        sl = torch.full((nseq,), ctx, dtype=torch.int32, device="cuda")
        scale = hd ** -0.5

        def prefill(flag):
            os.environ["VTA_ATTN_MULTIQ"] = flag
            return ops.paged_attention_prefill(q, kc, vc, tables, qsl, sl, scale, q_len, ctx)

        routed = ops.paged_attention_multiq_usable(q, kc, q_len)
        diff = (prefill("1").float() - prefill("0").float()).abs().max().item()
        t = bench_alternating({
            "new": lambda: prefill("1"),
            "parent": lambda: prefill("0"),
            "decode": lambda: ops.paged_attention_decode(q1, kc, vc, tables, sl, scale, ctx),
        })
        os.environ["VTA_ATTN_MULTIQ"] = "1"
        kv_bytes = nseq * ctx * kvh * hd * 2 * kc.element_size()
        del kc, vc
        probe = copy_probe_tbps(kv_bytes)
        res = {"routed": routed, "max_abs_diff_vs_parent": round(diff, 4),
               "KV_MB": round(kv_bytes / 1e6, 1), "copy_probe_TBps": round(probe, 2)}
        for k, (med, lo, hi) in t.items():
            res[k] = {"us": round(med, 1), "min_us": round(lo, 1), "max_us": round(hi, 1),
                      "TBps": round(kv_bytes / med / 1e6, 2)}
        res["speedup_vs_parent"] = round(t["parent"][0] / t["new"][0], 2)
        out[name] = res
        print(name, res, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kvh", type=int, default=8)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--hd", type=int, default=128)
    ap.add_argument("--bs", type=int, default=16)
    ap.add_argument("--only", choices=["prefill", "decode", "verify"], default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available()
    torch.manual_seed(0)
    dt = torch.bfloat16
    out = {}

    prefill_cases = [("prefill 16x512", 16, 512), ("prefill 4x2048", 4, 2048)]
    if args.only == "verify":
        verify_cases(args.bs, out)
        print(json.dumps(out))
        return
    if args.only == "decode":
        prefill_cases = []
    for name, nseq, ctx in prefill_cases:
        total_q = nseq * ctx
        nb = (ctx + args.bs - 1) // args.bs
        kc = torch.randn(nseq * nb + 8, args.bs, args.kvh, args.hd, dtype=dt, device="cuda")
        vc = torch.randn_like(kc)
        q = torch.randn(total_q, args.heads, args.hd, dtype=dt, device="cuda")
        tables = torch.arange(nseq * nb, dtype=torch.int32, device="cuda").reshape(nseq, nb)
        qsl = torch.arange(0, total_q + 1, ctx, dtype=torch.int32, device="cuda")
        sl = torch.full((nseq,), ctx, dtype=torch.int32, device="cuda")
        us = bench(lambda: ops.paged_attention_prefill(
            q, kc, vc, tables, qsl, sl, args.hd ** -0.5, ctx, ctx))
        kv_mb = nseq * ctx * args.kvh * args.hd * 2 * 2 / 1e6
        flops = 2 * 2 * nseq * args.heads * (ctx * ctx / 2) * args.hd
        out[name] = {"us": round(us, 1), "KV_MB": round(kv_mb, 1),
                     "TFLOPs": round(flops / us / 1e6, 1)}
        print(name, out[name], flush=True)

    decode_cases = [("decode 256x576", 256, 576), ("decode 64x512", 64, 512),
                    ("decode 512x544", 512, 544), ("decode 512x576", 512, 576),
                    ("decode 512x800", 512, 800), ("decode 512x1024", 512, 1024)]
    if args.only == "prefill":
        decode_cases = []
    for name, nseq, ctx in decode_cases:
        nb = (ctx + args.bs - 1) // args.bs
        kc = torch.randn(nseq * nb + 8, args.bs, args.kvh, args.hd, dtype=dt, device="cuda")
        vc = torch.randn_like(kc)
        q = torch.randn(nseq, args.heads, args.hd, dtype=dt, device="cuda")
        tables = torch.arange(nseq * nb, dtype=torch.int32, device="cuda").reshape(nseq, nb)
        sl = torch.full((nseq,), ctx, dtype=torch.int32, device="cuda")
        us = bench(lambda: ops.paged_attention_decode(
            q, kc, vc, tables, sl, args.hd ** -0.5, ctx))
        # K and V are each read once at 2 bytes per element
        kv_bytes = nseq * ctx * args.kvh * args.hd * 2 * 2
        tbps = kv_bytes / us / 1e6
        del kc, vc
        probe = copy_probe_tbps(kv_bytes)
        out[name] = {"us": round(us, 1), "KV_MB": round(kv_bytes / 1e6, 1),
                     "TBps": round(tbps, 2), "copy_probe_TBps": round(probe, 2),
                     "of_probe": round(tbps / probe, 2)}
        print(name, out[name], flush=True)

    print(json.dumps(out))


if __name__ == "__main__":
    main()
