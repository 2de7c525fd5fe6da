"""The headline training step with erf-GELU and with tanh-GELU, alternately, in one invocation (profiles/tanh_gelu_step_ab.md).

    python tools/bench_gelu_flavours.py                       # 1B stage-1 student, B = 128, drop_path 0.25, one captured HIP graph
    python tools/bench_gelu_flavours.py --model 6B --fp8      # the 6B encoder on the e4m3 GEMM path, B = 16

The step is bench.py's: the same model factory and keyword arguments (bench.MODELS), the same engine construction, synthetic batch and
capture_step / train_step_graphed calls; only `fused_mlp_act` differs between the runs.  Every run is a fresh child process (one process on
the GPU at a time, no allocator or graph-pool state carried from one flavour to the next) that prints ONE JSON line: ms/step, clips/s, whether
DropPath skipping ran (`droppath_skip.enabled`, counted on the device as in bench.py) and which GEMM kernel the router picks for the fc1
forward launch of that flavour.  The parent process never touches the GPU."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="1B", choices=["1B", "6B"])
    ap.add_argument("--fp8", action="store_true")
    ap.add_argument("--batch", type=int, default=None, help="clips; default 128 (1B), 16 (6B)")
    ap.add_argument("--drop-path", type=float, default=0.25)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--order", default="erf,tanh,erf,tanh", help="comma-separated flavours, run in this order")
    ap.add_argument("--timeout", type=int, default=400, help="seconds per run (child process)")
    ap.add_argument("--one", default=None, choices=["erf", "tanh"], help="(internal) run one flavour in this process")
    return ap.parse_args()


def fc1_forward_kernel(model, B, L, fp8, skipping):
    """(kernel, how it is known) for the fc1 forward launch of this model.  bf16: the router's own answer (ivh_gemm_select) for the descriptor
    BlockStackFn builds -- gelu(n2 W1^T + b1) with the second output.  e4m3: the library has no such query, so the answer is INFERRED from the
    documented rules of ivh_gemm_fp8 (include/internvideo_hip.h) and labelled so: a count-carrying launch runs on the 256x256 kernel or raises;
    without a count, act = 2 and problems under 512^2 outputs or K < 512 go to the 128x128 kernel"""
    from internvideo_amd import functional as Fn, lib, ops
    act = ops.ACT[Fn._act_d(model.fused_mlp_act)]
    F, D = model.blocks[0].mlp.fc1.weight.shape
    M = B * L
    if fp8:
        big = skipping or (act != 2 and M * F >= 512 * 512 and D >= 512)
        return ("256x256 e4m3" if big else "128x128 e4m3"), "inferred from the documented ivh_gemm_fp8 rules"
    d = lib.GemmDesc()
    d.M, d.N, d.K, d.a_kc, d.b_kc, d.batch, d.alpha = M, F, D, 1, 1, 1, 1.0
    d.lda, d.ldb, d.ldc, d.ldp = D, D, F, F
    d.act = act
    d.A = d.B = d.C = d.preact = 16                              # the query reads which fields are set, never the memory behind them
    return {1: "128x128", 2: "256x256"}[lib.load().ivh_gemm_select(C.byref(d))], "ivh_gemm_select"


def bench_args(args):
    """bench.py's own argument namespace for this run: every setting the tool does not vary (checkpointing, fp8 scaling, residual type, engine
    switches, kernel overrides) is read from it, so a changed default in bench.py changes this step too"""
    import bench
    argv, sys.argv = sys.argv, ["bench.py", "--gpus", "1", "--model", args.model, "--batch", str(args.batch), "--drop-path", str(args.drop_path),
                                "--steps", str(args.steps), "--warmup", str(args.warmup)] + (["--fp8"] if args.fp8 else [])
    try:
        return bench.parse()
    finally:
        sys.argv = argv


def run_one(args):
    import torch
    import bench                                                 # the factory table and the synthetic workload are bench.py's
    from internvideo_amd import internvideo2_pretrain as M, ops
    from internvideo_amd.engine import IVTrainEngine

    b = bench_args(args)
    spec = bench.MODELS[args.model]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    with torch.device(dev):
        model = getattr(M, spec["factory"])(drop_path_rate=b.drop_path, num_frames=spec["frames"], use_checkpoint=b.checkpoint_num > 0,
                                            checkpoint_num=b.checkpoint_num, fused_mlp_act=args.one, **spec["kw"])
    model.fp8_gemm = bool(b.fp8)
    model.fp8_scaling = b.fp8_scaling
    model.fp8_weight_scales = b.fp8_weight_scales
    model.residual_dtype = b.residual
    model.drop_path_skip = False if b.no_droppath_skip else "auto"
    model.train()
    model.dp_count_acc = torch.zeros((model.depth, 2, 2), dtype=torch.int64, device=dev)
    engine = IVTrainEngine(model, lr=1.5e-4, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.05, max_grad_norm=3.0,
                           wgrad_stream=b.wgrad_stream, force_comm=b.force_dist, reduce_mode=b.reduce_mode, reduce_dtype=b.reduce_dtype,
                           check_finite=b.check_finite)
    ops.set_gemm_kernel(b.gemm_kernel)
    ops.set_attn_kernel(b.attn_kernel)
    B, T, n_vis = args.batch, spec["frames"], spec["n_vis"]
    gh = spec["img"] // 14
    L = 1 + T * n_vis
    gen = torch.Generator(device=dev).manual_seed(1234)
    video = torch.rand((B, 3, T, spec["img"], spec["img"]), device=dev, generator=gen).to(torch.bfloat16)
    perm = torch.rand((B, T, gh * gh), device=dev, generator=gen).argsort(-1)
    mask = torch.ones((B, T, gh * gh), dtype=torch.bool, device=dev)
    mask.scatter_(2, perm[:, :, :n_vis], False)
    mask = torch.cat([torch.zeros((B, 1), dtype=torch.bool, device=dev), mask.reshape(B, -1)], 1).to(torch.uint8)

    def unit(*shape):
        t = torch.randn(shape, device=dev, generator=gen)
        return (t / t.norm(dim=-1, keepdim=True)).to(torch.bfloat16)

    targets = (unit(len(model.clip_decoder), B, L, model.clip_decoder[0].head.out_features),
               unit(B, model.final_clip_decoder.head.out_features),
               unit(len(model.mae_decoder), B, L - 1, model.mae_decoder[0].head[2].out_features))
    engine.capture_step(video, mask, targets, L=L)
    for _ in range(args.warmup):
        loss, _ = engine.train_step_graphed()
    torch.cuda.synchronize()
    model.dp_count_acc.zero_()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss, _ = engine.train_step_graphed()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    dp = bench.droppath_account(model, args.steps, B, L, spec["flop"])
    kernel, how = fc1_forward_kernel(model, B, L, bool(args.fp8), bool(dp["enabled"]))
    out = dict(tool="bench_gelu_flavours", model=args.model, fp8=bool(args.fp8), act=args.one, batch=B, drop_path=args.drop_path, steps=args.steps,
               warmup=args.warmup, graph=True, ms_per_step=round(elapsed / args.steps * 1e3, 2), clips_per_s=round(B * args.steps / elapsed, 2),
               droppath_skip=dict(enabled=bool(dp["enabled"]), kept_fraction=dp["kept_fraction"]),
               fc1_forward_kernel=kernel, fc1_forward_kernel_from=how,
               loss=round(float(loss), 5), finite=bool(torch.isfinite(loss).item()))
    engine.close()
    print(json.dumps(out), flush=True)
    return 0


def main():
    args = parse()
    if args.batch is None:
        args.batch = 16 if args.model == "6B" else 128
    if args.one:
        return run_one(args)
    base = [sys.executable, os.path.abspath(__file__), "--model", args.model, "--batch", str(args.batch), "--drop-path", str(args.drop_path),
            "--steps", str(args.steps), "--warmup", str(args.warmup)] + (["--fp8"] if args.fp8 else [])
    for act in [a.strip() for a in args.order.split(",") if a.strip()]:
        try:
            r = subprocess.run(base + ["--one", act], capture_output=True, text=True, timeout=args.timeout, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(tool="bench_gelu_flavours", act=act, error=f"no result within {args.timeout} s")), flush=True)
            return 1                                             # nothing more is started on the GPU after a run that did not end
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stderr[-4000:])
            print(json.dumps(dict(tool="bench_gelu_flavours", act=act, error=f"exit status {r.returncode}")), flush=True)
            return 1
        print(lines[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
