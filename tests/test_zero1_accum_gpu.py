"""Gradient accumulation under ZeRO-1 on the GPU: the two kernels bit for bit, the engine on a 1-rank RCCL group against the replicated
accumulate(), two real processes against the single-rank step on the concatenated batch, and the reference's own `--update_freq 2` loop through
ds_compat with `--zero_stage 1`.  Every child process (tests/zero1_accum_worker.py) runs under its own timeout; its exit code is checked
before anything further is started."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from internvideo_amd import ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "zero1_accum_worker.py")
DEV = "cuda"
GRID_SPAN = 4096 * 256 * 8                                   # elements one pass of the shard-sum grid covers (4096 workgroups x 256 threads x 8)


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("chunk", [8, 4096, GRID_SPAN + 8])
@pytest.mark.parametrize("W", [1, 2, 8])
def test_shard_sum_acc_matches_torch_fp32_in_rank_order_bitwise(W, chunk):
    """accumulate = 0: `out` is not read (it is poisoned with NaN) and the bits are ivh_shard_sum_bf16's; accumulate = 1: the bits of
    out + piece 0 + piece 1 + ... added in torch fp32 in that order.  The largest chunk is one 8-element group past what the capped grid
    covers in one pass, so the grid-stride loop takes a second trip."""
    g = torch.Generator(device=DEV).manual_seed(W * 131 + chunk % 977)
    recv = (torch.randn(W * chunk, device=DEV, generator=g) * 3).to(torch.bfloat16)
    want0 = torch.empty(chunk, dtype=torch.float32, device=DEV)
    ops.shard_sum_bf16(recv, W, want0)
    out = torch.full((chunk,), float("nan"), dtype=torch.float32, device=DEV)
    ops.shard_sum_bf16_acc(recv, W, out, False)
    assert torch.equal(_bits(out), _bits(want0))
    prev = torch.randn(chunk, device=DEV, generator=g)
    want1 = prev.clone()
    for r in range(W):
        want1 += recv[r * chunk:(r + 1) * chunk].float()
    out = prev.clone()
    ops.shard_sum_bf16_acc(recv, W, out, True)
    assert torch.equal(_bits(out), _bits(want1))
    assert not torch.equal(_bits(out), _bits(want0))


@pytest.mark.parametrize("n", [5, 1029, 8192 * 256 * 8 + 29])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_grad_accumulate_is_torch_add_bitwise(dtype, n):
    """acc += grad for bf16 and fp32 sources, n not a multiple of 8 (only a tail; vector trips + tail; past one pass of the capped grid)"""
    g = torch.Generator(device=DEV).manual_seed(n % 1000 + (7 if dtype == torch.float32 else 0))
    grad = torch.randn(n, device=DEV, generator=g).to(dtype)
    acc = torch.randn(n, device=DEV, generator=g)
    want = acc.clone().add_(grad)
    ops.grad_accumulate(grad, acc)
    assert torch.equal(_bits(acc), _bits(want))
    with pytest.raises(ops.InternVideoHipError):
        ops.grad_accumulate(grad[1:], acc[1:])                # not 16-byte aligned: refused, not mis-read


def _child(cmd, timeout):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, [ln for ln in r.stdout.splitlines() if ln.startswith("STEP ")], r.stderr[-3000:])
    return r


def _result(r):
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0][7:])


def _rel(got, want):
    return [abs(a - b) / abs(b) for a, b in zip(got, want)]


def test_one_rank_rccl_zero1_accumulation_equals_the_replicated_accumulate():
    """real RCCL (1-rank group, own subprocess, force_comm): two optimizer steps of gas = 2 on the tiny student, eager with overlap, against the
    plain single-process engine's replicated accumulate() on the same micro-batches.  At W = 1 the additions are the same in the same order:
    `grad_shard32` before each boundary is the replicated `_acc_mat` bit for bit; losses 1e-5 and master weights 1e-6 (the bars
    test_one_rank_rccl_reduce_modes holds zero1 to).  Then the same cycles as replayed graph segments (capture_step(segmented=True),
    replay_micro_step(), optimizer_step(accumulated=True, average=True)): master weights 1e-4, the bar of `segments_zero1` there."""
    res = _result(_child([sys.executable, WORKER, "rccl1"], 300))
    print("zero1 accumulation on 1-rank RCCL:", json.dumps(res))
    assert res["buckets"] >= 2 and res["acc_mat_is_none"]
    assert res["shard_bitwise"] == [True, True], res
    assert max(_rel(res["eager"], res["ref"])) < 1e-5, res
    assert res["eager_master_rel"] < 1e-6, res
    assert res["segments"] >= 3 and res["seg_reduce_log_ok"]
    assert max(_rel(res["seg"], res["ref"])) < 1e-5, res
    assert res["seg_master_rel"] < 1e-4, res


def _dp_line(world):
    if world == 1:
        cmd = [sys.executable, WORKER, "dp"]
    else:
        with socket.socket() as s_:
            s_.bind(("127.0.0.1", 0))
            port = s_.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), WORKER, "dp", "--share-gpu"]
    r = _child(cmd, 300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_two_ranks_times_two_micro_steps_equal_the_single_rank_step_on_the_concatenated_batch():
    """two REAL processes on the one GPU (collectives over gloo staged through host memory, as tests/test_multiproc_gpu.py): 2 ranks x gas 2
    x 2 clips under zero1 against 1 rank x the same 8 clips in one plain step, three optimizer steps of the S/14 student.  The bars of
    test_two_rank_step_equals_the_single_rank_step_on_the_concatenated_batch: step 1 (identical weights) loss 2e-6 and gradient norm 5e-3,
    later steps loss 1e-3 and gradient norm 2e-2."""
    one = _dp_line(1)
    two = _dp_line(2)
    assert two["world"] == 2 and two["gas"] == 2 and two["buckets"] >= 2 and two["reduce"].startswith("zero1")
    assert len(two["losses"]) == len(one["losses"]) == 3
    rel, gn = _rel(two["losses"], one["losses"]), _rel(two["grad_norms"], one["grad_norms"])
    print("zero1 accumulation equivalence (loss rel dev per step, grad-norm rel dev per step):", json.dumps([rel, gn]))
    notes = os.environ.get("IVH_ZERO1_ACCUM_NOTES")           # the deviations as a JSON file, only when the caller names one: the test
    if notes:                                                 # itself writes nothing into the repository
        os.makedirs(os.path.dirname(os.path.abspath(notes)), exist_ok=True)
        with open(notes, "w") as f:
            json.dump({"single_rank": one, "two_ranks_gas2": two, "loss_rel_dev": rel, "grad_norm_rel_dev": gn}, f)
    assert rel[0] < 2e-6, rel
    assert gn[0] < 5e-3, gn
    assert max(rel[1:]) < 1e-3, rel
    assert max(gn[1:]) < 2e-2, gn


def test_reference_step_loop_with_update_freq_2_and_zero_stage_1():
    """tests/golden/step_protocol_gas2.json (the reference's own train_one_epoch, four iterations = two optimizer steps) replayed through
    ds_compat.initialize(args(update_freq=2, zero_stage=1), force_comm=True) on a 1-rank RCCL group: the bars of
    test_reference_step_loop_with_update_freq_2_on_the_hip_path (iterations 1-2 on identical weights 1e-3, 3-4 3e-3, boundary norms 3 %)."""
    res = _result(_child([sys.executable, WORKER, "protocol"], 300))
    rel_l, rel_g = _rel(res["losses"], res["want_losses"]), _rel(res["grad_norms"], res["want_grad_norms"])
    print("update_freq 2 + zero_stage 1 replay: loss dev", rel_l, "grad-norm dev", rel_g)
    assert res["n_buckets"] >= 2 and res["buckets_per_micro_step"] == [res["n_buckets"]] * 4 and res["acc_mat_is_none"], res
    assert max(rel_l[:2]) < 1e-3 and max(rel_l) < 3e-3, rel_l
    assert len(rel_g) == 2 and max(rel_g) < 3e-2, rel_g
    assert res["micro_steps"] == 4 and res["global_steps"] == 2
