"""The gradient-accumulation kernels at the 1B model's sizes (1.07e9 matrix elements in ~20 buckets, 1.3e6 vector elements): us per launch and
TB/s of `ivh_shard_sum_bf16_acc` (overwriting / accumulating; W = 1 as on a 1-rank group and W = 8) and of `ivh_grad_accumulate`, beside
the `at::native` adds (`acc.add_(grad)`) that the replicated accumulate() used before.  One JSON line per case; run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel view (the cases differ in kernel name or grid size).  Single GPU: no wire traffic is
measured here.  Usage: python tools/bench_accum_kernels.py [--n-mat N] [--buckets K] [--n-vec N]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-mat", type=int, default=1024 * 1045000)
    ap.add_argument("--buckets", type=int, default=20)
    ap.add_argument("--n-vec", type=int, default=1_300_485, help="not a multiple of 8: the scalar tail runs")
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    from internvideo_amd import ops
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    bucket = a.n_mat // a.buckets // 64 * 64
    grad = (torch.randn(a.n_mat, device=dev, generator=g) * 1e-3).bfloat16()
    acc = torch.zeros(a.n_mat, device=dev)
    gvec = torch.randn(a.n_vec, device=dev, generator=g)
    avec = torch.zeros(a.n_vec, device=dev)
    recv, shard1, shard8 = grad[:bucket], acc[:bucket], acc[:bucket // 8]
    cases = [
        ("shard_sum_bf16_acc overwrite, W=1, one bucket", lambda: ops.shard_sum_bf16_acc(recv, 1, shard1, False), bucket * 6),
        ("shard_sum_bf16_acc accumulate, W=1, one bucket", lambda: ops.shard_sum_bf16_acc(recv, 1, shard1, True), bucket * 10),
        ("shard_sum_bf16_acc overwrite, W=8, one bucket", lambda: ops.shard_sum_bf16_acc(recv, 8, shard8, False), bucket * 2 + bucket // 8 * 4),
        ("shard_sum_bf16_acc accumulate, W=8, one bucket", lambda: ops.shard_sum_bf16_acc(recv, 8, shard8, True), bucket * 2 + bucket // 8 * 8),
        ("grad_accumulate bf16, matrix region", lambda: ops.grad_accumulate(grad, acc), a.n_mat * 10),
        ("torch add_ bf16, matrix region", lambda: acc.add_(grad), a.n_mat * 10),
        ("grad_accumulate fp32, vector region", lambda: ops.grad_accumulate(gvec, avec), a.n_vec * 12),
        ("torch add_ fp32, vector region", lambda: avec.add_(gvec), a.n_vec * 12),
    ]
    for name, fn, nbytes in cases:
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1000.0 / a.iters
        print(json.dumps(dict(case=name, us=round(us, 1), tbps=round(nbytes / us / 1e6, 3), bytes=nbytes)), flush=True)


if __name__ == "__main__":
    main()
