"""Gradient accumulation under ZeRO-1 (`--zero_stage 1 --update_freq N`, run_pretraining.py:42,375; scripts/pretraining/1B_pt.sh:65), the
reduction logic on two gloo ranks with host tensors -- no GPU.  The worker is tests/zero1_accum_worker.py (mode `host`)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_rank_gloo_zero1_accumulates_into_the_fp32_shard():
    """Two ranks, overlap on and off, gas = 3 micro-steps of rank- and micro-step-dependent bf16 matrix / fp32 vector gradients, the buckets
    driven through the block hooks, then accumulate(); two cycles per engine.
      * every rank's slice of `grad_shard32`, and `_acc_vec`, equal the fp64 sum over all (micro-step, rank) terms within
        gas W 2^-24 sum|terms| elementwise -- the first-order bound of an fp32 sum of gas W exact inputs in any order (bf16 widens exactly);
      * no full-size accumulator (`_acc_mat is None`); every bucket goes out once per micro-step, in order;
      * the second cycle starts from an overwritten shard: it is poisoned with NaN between the cycles;
      * the boundary step issues no gradient collective and hands `grad_shard32` / `_acc_vec` to AdamW (kernels stubbed: no CPU path);
      * refused: optimizer_step() in the middle of a cycle, accumulate() on an engine whose graph captured its collectives, replicated
        accumulate() after a bucket went to the wire, save_checkpoint in the middle of a cycle;
      * ds_compat.initialize(zero_stage=1, update_freq=2) reaches optimizer_step(accumulated=True) at the boundary, and only there."""
    import socket
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "zero1_accum_worker.py"), "host"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, OMP_NUM_THREADS="1"), cwd=ROOT)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("OK") == 2, r.stdout
