"""Worker processes of the ZeRO-1 gradient-accumulation tests (tests/test_zero1_accum_host.py, tests/test_zero1_accum_gpu.py).

    python -m torch.distributed.run --nproc-per-node 2 ... tests/zero1_accum_worker.py host
        two gloo ranks on host tensors: the reduction logic of accumulate() under reduce_mode='zero1' (no GPU, the kernels are stubbed)
    python tests/zero1_accum_worker.py rccl1
        1-rank RCCL group on the GPU: two optimizer steps of gas = 2 on the tiny student, eager with overlap and as replayed graph segments,
        against the plain single-process engine's replicated accumulate()
    python tests/zero1_accum_worker.py dp            (1 process)   |   torch.distributed.run --nproc-per-node 2 ... dp --share-gpu
        W ranks x gas micro-steps x 2 clips under zero1 (W = 2, gas = 2) or one plain step on the same 8 clips (W = 1): ONE JSON line from rank 0
    python tests/zero1_accum_worker.py protocol
        tests/golden/step_protocol_gas2.json replayed through ds_compat.initialize(update_freq=2, zero_stage=1, force_comm=True), 1-rank RCCL

`--update_freq` is DeepSpeed's gradient_accumulation_steps (InternVideo2/single_modality/run_pretraining.py:42,375); the shipped scripts run
`--zero_stage 1` (scripts/pretraining/1B_pt.sh:65)."""
from __future__ import annotations

import argparse
import json
import os
import socket
import sys
import tempfile

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _student(cfg, device=None, drop_path_rate=0.0):
    from internvideo_amd import internvideo2_pretrain as M
    kw = dict(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio,
              num_frames=cfg.num_frames, attn_pool_num_heads=cfg.attn_pool_num_heads, clip_embed_dim=cfg.clip_embed_dim,
              clip_teacher_embed_dim=cfg.clip_teacher_embed_dim, clip_teacher_final_dim=cfg.clip_teacher_final_dim,
              clip_return_layer=cfg.clip_return_layer, mae_teacher_embed_dim=cfg.mae_teacher_embed_dim, mae_return_layer=cfg.mae_return_layer,
              drop_path_rate=drop_path_rate)
    if device is None:
        return M.PretrainInternVideo2(**kw)
    with torch.device(device):
        return M.PretrainInternVideo2(**kw)


def _one_rank_rccl():
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda", 0))


def _finish(res):
    """the result is complete; the RCCL communicator is not torn down (see tests/test_fullsize_gpu.py _RCCL_MODES: its destruction aborted in
    one of ~10 runs on this RCCL / runtime pair): a hard exit skips the teardown"""
    torch.cuda.synchronize()
    print("RESULT " + json.dumps(res), flush=True)
    sys.stdout.flush(); sys.stderr.flush()
    os._exit(0)


# ---- host: two gloo ranks, host tensors -------------------------------------------------------------------------------------------------
def host():
    from types import SimpleNamespace
    from internvideo_amd import ds_compat, ops
    from internvideo_amd.engine import IVTrainEngine
    from oracle import internvideo2_oracle as O
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = O.named_config("tiny64")
    GAS, U = 3, 2.0 ** -24

    def fresh():
        torch.manual_seed(0)
        return _student(cfg)

    # there is no CPU compute path: the three optimizer kernels are stood in for by recorders, so that optimizer_step's control flow (which
    # buffers it hands to AdamW, which collectives it issues) runs on host tensors
    adamw_calls, collectives = [], []

    def sqnorm(g, out, accumulate, scratch=None):
        v = (g.double() ** 2).sum().float().reshape(1)
        out.copy_(out + v if accumulate else v)

    def clip_coef(sumsq, max_norm):
        nrm = sumsq.sqrt()
        return (max_norm / (nrm + 1e-6)).clamp(max=1.0), nrm

    def adamw_step(master, exp_avg, exp_avg_sq, grad, shadow, lr, b1, b2, eps, wd, step, grad_scale=1.0, clip_coef=None, lr_segments=None, seg_base=0):
        adamw_calls.append((grad.data_ptr(), grad.numel(), float(grad_scale)))

    ops.sqnorm, ops.clip_coef, ops.adamw_step = sqnorm, clip_coef, adamw_step
    real_ar = dist.all_reduce

    def counting_all_reduce(t, *a, **k):
        collectives.append(t.numel())
        return real_ar(t, *a, **k)

    def emulate_backward(eng, seed):
        """what a micro-step's backward leaves behind: rank- and micro-step-dependent gradients in the flat buffers, block hooks fired last
        block first (overlap=True; without overlap accumulate() launches every bucket).  -> (matrix, vector) this rank contributed"""
        eng.zero_grad()
        g = torch.Generator().manual_seed(seed)
        lm = torch.randn(eng.n_mat, generator=g).to(torch.bfloat16)
        lv = torch.randn(eng.n_vec, generator=g)
        eng.grad_mat.copy_(lm); eng.grad_vec.copy_(lv)
        if eng.tower.grad_ready_hook is not None:
            for i in range(cfg.depth - 1, -1, -1):
                eng.tower.grad_ready_hook(i)
        return lm, lv

    def over_ranks(t):
        t = t.double().clone()
        real_ar(t)
        return t

    def check_sums(eng, terms, n_terms):
        """the shard / the vector accumulator against the fp64 sum of all (micro-step, rank) terms; bound: first-order error of an fp32 sum
        of n_terms exact inputs in any order, n_terms * 2^-24 * sum |terms|, elementwise"""
        exact_m = sum(over_ranks(lm) for lm, _ in terms)
        abs_m = sum(over_ranks(lm.abs()) for lm, _ in terms)
        exact_v = sum(over_ranks(lv) for _, lv in terms)
        abs_v = sum(over_ranks(lv.abs()) for _, lv in terms)
        worst = 0.0
        for lo, hi in eng.buckets:
            s0, c = eng._shard(lo, hi)
            got = eng.grad_shard32[lo // world:lo // world + c].double()
            err, bound = (got - exact_m[s0:s0 + c]).abs(), n_terms * U * abs_m[s0:s0 + c]
            assert torch.isfinite(got).all() and bool((err <= bound).all()), ("shard sum", float((err - bound).max()))
            worst = max(worst, float((err / bound.clamp_min(1e-30)).max()))
        err, bound = (eng._acc_vec.double() - exact_v).abs(), n_terms * U * abs_v
        assert bool((err <= bound).all()), ("vector accumulator", float((err - bound).max()))
        return worst

    def expect(exc, fn, word):
        try:
            fn()
        except exc as e:
            assert word in str(e), str(e)
            return
        raise AssertionError(f"{fn} did not raise {exc.__name__}")

    worst = 0.0
    for overlap in (True, False):
        ez = IVTrainEngine(fresh(), bucket_bytes=64 * 1024, reduce_mode="zero1", overlap=overlap)
        assert ez.zero1 and ez.world == 2 and len(ez.buckets) >= 2 and (ez.tower.grad_ready_hook is not None) == overlap
        for cycle in range(2):
            if cycle == 1:
                ez.grad_shard32.fill_(float("nan"))          # a second cycle overwrites the shard, it does not add to what the first left
            terms = []
            for k in range(GAS):
                terms.append(emulate_backward(ez, 1000 * cycle + 10 * k + rank))
                ez.accumulate()
                assert ez.reduce_log == ez.buckets, (overlap, cycle, k, ez.reduce_log)
                assert ez._acc_mat is None and ez._acc_n == k + 1
                if cycle == 0 and k == 0:
                    # optimizer_step() in the middle of a cycle would apply this micro-step's buffers and leave the sums behind
                    expect(RuntimeError, ez.optimizer_step, "accumulated=True")
                    assert ez.step_count == 0 and ez._acc_n == 1
                    # a graph that captured its collectives froze the overwrite / accumulate argument of the shard sums
                    ez._capture_comm = True
                    expect(RuntimeError, ez.accumulate, "capture_comm")
                    ez._capture_comm = False
                    assert ez._acc_n == 1
            worst = max(worst, check_sums(ez, terms, GAS * world))
            # the boundary: no gradient collective (only the scalar of the shard norms crosses the ranks, and the bf16 all-gather), AdamW reads
            # grad_shard32 and _acc_vec; average=True divides by the number of micro-steps
            del adamw_calls[:], collectives[:]
            dist.all_reduce = counting_all_reduce
            try:
                ez.optimizer_step(accumulated=True, average=(cycle == 1))
            finally:
                dist.all_reduce = real_ar
            assert collectives == [1], collectives
            assert ez._acc_n == 0 and ez._acc_mat is None and not bool(ez._acc_vec.any()) and ez.step_count == cycle + 1
            assert len(adamw_calls) == len(ez.buckets) + 1
            for (lo, hi), (p, n, gs) in zip(ez.buckets, adamw_calls):
                assert p == ez.grad_shard32[lo // world:].data_ptr() and n == (hi - lo) // world
            assert adamw_calls[-1][:2] == (ez._acc_vec.data_ptr(), ez.n_vec)
            want_gs = 1.0 / world / (GAS if cycle == 1 else 1)
            assert all(abs(c[2] - want_gs) < 1e-12 for c in adamw_calls), (adamw_calls, want_gs)
        expect(RuntimeError, lambda: ez.optimizer_step(accumulated=True), "without a preceding accumulate")

    # replicated mode: accumulate() after a bucket of this micro-step went to the wire would count it `world` times at the boundary
    er = IVTrainEngine(fresh(), bucket_bytes=64 * 1024)
    emulate_backward(er, 7 + rank)
    assert er._next_bucket > 0
    expect(RuntimeError, er.accumulate, "already been reduced")
    assert er._acc_n == 0 and er._acc_mat is None
    # ... and without overlap it accumulates as before: full-size fp32 accumulators, nothing on the wire
    eo = IVTrainEngine(fresh(), bucket_bytes=64 * 1024, overlap=False)
    lm, lv = emulate_backward(eo, 9 + rank)
    eo.accumulate()
    assert eo.reduce_log == [] and torch.equal(eo._acc_mat, lm.float()) and torch.equal(eo._acc_vec, lv) and eo._acc_n == 1

    # ---- the script seam: --zero_stage 1 --update_freq 2 ------------------------------------------------------------------------------
    args = SimpleNamespace(lr=1e-3, weight_decay=0.05, opt_betas=[0.9, 0.98], opt_eps=1e-6, clip_grad=3.0, update_freq=2, zero_stage=1)
    dse, optimizer, _, _ = ds_compat.initialize(args=args, model=fresh(), model_parameters=None, dist_init_required=False, bucket_bytes=64 * 1024)
    eng = dse.engine
    assert eng.zero1 and eng.overlap and dse.gradient_accumulation_steps() == 2
    reached = []
    real_step = eng.optimizer_step

    def spy(*a, **k):
        reached.append(k)
        return real_step(*a, **k)
    eng.optimizer_step = spy
    terms = []
    for k in range(2):
        terms.append(emulate_backward(eng, 500 + 10 * k + rank))      # (the forward has no CPU path; dse(...) would zero the buffers first)
        dse._stepped = False
        dse.backward(torch.zeros((), requires_grad=True) * 1.0)        # engine.backward + accumulate()
        if k == 0:
            expect(RuntimeError, lambda: dse.save_checkpoint(os.path.join(tempfile.gettempdir(), "ivh_zero1_accum_never_written")), "accumulation cycle")
            assert not dse.is_gradient_accumulation_boundary()
            dse.step()                                                   # between boundaries: nothing is applied
            assert reached == [] and eng._acc_n == 1
        else:
            check_sums(eng, terms, 2 * world)
            dse.step()
    assert len(reached) == 1 and reached[0].get("accumulated") is True and not reached[0].get("average", False)
    assert dse.global_steps == 1 and dse.micro_steps == 2 and eng._acc_n == 0 and eng._acc_mat is None
    sys.stdout.write("RANK %d OK worst error / bound %.3f\n" % (rank, worst))      # one write: the ranks share the pipe
    sys.stdout.flush()
    dist.destroy_process_group()


# ---- GPU: batches and micro-steps ----------------------------------------------------------------------------------------------------------
def _micro_step(eng, v, m, tg, gas, vis_inv=None):
    """one eager micro-step the way ds_compat drives the engine: fresh per-micro-step buffers, backward of loss / gas, accumulate()"""
    eng.zero_grad()
    eng._begin_step_on_device()
    loss, _ = eng.model.forward_loss(v, m, tg, eng.clip_loss_ratio, eng.mae_loss_ratio, vis_inv=vis_inv)
    eng.backward(loss / float(gas))
    eng.accumulate()
    return loss.detach()


def rccl1():
    import faulthandler
    faulthandler.enable()
    from internvideo_amd.engine import IVTrainEngine
    from oracle import internvideo2_oracle as O
    from tests.test_model_gpu import build
    DEV, GAS, STEPS = "cuda", 2, 2
    cfg = O.named_config("tiny88")
    params = O.synthetic_params(cfg, seed=1)
    batches = []
    for seed in range(1, 1 + GAS * STEPS):
        video, mask, targets = O.synthetic_batch(cfg, 2, 5, seed=seed)
        batches.append((video.to(DEV), torch.from_numpy(mask).to(DEV).to(torch.uint8), tuple(t.to(DEV) for t in targets)))
    L = int((~torch.from_numpy(mask)[0]).sum())
    kw = dict(lr=1e-3, bucket_bytes=1 << 18)

    def run_eager(eng, want_acc):
        losses, accs = [], []
        for s in range(STEPS):
            for k in range(GAS):
                losses.append(_micro_step(eng, *batches[s * GAS + k], GAS).item())
            accs.append(want_acc(eng).clone())
            eng.optimizer_step(accumulated=True)
        torch.cuda.synchronize()
        return losses, accs

    base = IVTrainEngine(build(cfg, params), **kw)            # no process group: today's replicated accumulate()
    ref, ref_acc = run_eager(base, lambda e: e._acc_mat)
    print("STEP ref done", flush=True)
    _one_rank_rccl()
    print("STEP group up", flush=True)
    relm = lambda e: ((e.master[:base.n_mat].double() - base.master[:base.n_mat].double()).norm() / base.master[:base.n_mat].double().norm()).item()   # noqa: E731
    res = dict(ref=ref)
    e = IVTrainEngine(build(cfg, params), force_comm=True, reduce_mode="zero1", **kw)
    assert e.zero1 and e.overlap and e.n_mat == base.n_mat
    res["eager"], acc = run_eager(e, lambda e_: e_.grad_shard32)
    res["buckets"] = len(e.reduce_log)
    res["acc_mat_is_none"] = e._acc_mat is None
    res["shard_bitwise"] = [bool(torch.equal(a.view(torch.int32), b.view(torch.int32))) for a, b in zip(acc, ref_acc)]
    res["eager_master_rel"] = relm(e)
    print("STEP eager done", flush=True)
    # the same cycles as replayed graph segments: the captured loss is not divided by gas, the boundary averages
    g = IVTrainEngine(build(cfg, params), force_comm=True, reduce_mode="zero1", **kw)
    sv, sm, stg = batches[0][0].clone(), batches[0][1].clone(), tuple(t.clone() for t in batches[0][2])
    g.capture_step(sv, sm, stg, L=L, segmented=True)
    print("STEP captured", flush=True)
    res["segments"] = len(g._segments)
    seg = []
    for s in range(STEPS):
        for k in range(GAS):
            v, m, tg = batches[s * GAS + k]
            sv.copy_(v); sm.copy_(m)
            for dst, src in zip(stg, tg):
                dst.copy_(src)
            seg.append(g.replay_micro_step()[0].item())
            assert g._acc_n == k + 1 and g._acc_mat is None
        g.optimizer_step(accumulated=True, average=True)
    torch.cuda.synchronize()
    res["seg"], res["seg_master_rel"] = seg, relm(g)
    res["seg_reduce_log_ok"] = [list(b) for b in g.reduce_log] == [list(b) for b in g.buckets]
    _finish(res)


def dp(a):
    import datetime
    import importlib.util
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    if world > 1:
        assert a.share_gpu, "several ranks: --share-gpu (every rank on cuda:0, collectives over gloo staged through host memory)"
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=180))
        spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
        bench = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(bench)
        bench._host_staged_collectives()
    from internvideo_amd import internvideo2_pretrain as M
    from internvideo_amd.engine import IVTrainEngine
    from oracle import internvideo2_oracle as O
    cfg = O.named_config("S14")
    GAS, CLIPS, BATCH, STEPS = 2, 2, 8, 3
    torch.manual_seed(0)
    model = _student(cfg, dev)
    model.load_state_dict({k: v.to(dev) for k, v in O.synthetic_params(cfg, seed=3).items()}, strict=True)
    model.train()
    kw = dict(reduce_mode="zero1") if world > 1 else {}
    eng = IVTrainEngine(model, lr=1.5e-4, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.05, max_grad_norm=3.0, bucket_bytes=4 << 20, **kw)
    T, h, w = cfg.grid
    n_vis = max(1, (h * w) // 5)
    video, mask, targets = O.synthetic_batch(cfg, BATCH, n_vis, seed=7)
    L = 1 + T * n_vis

    def clips(b0, b1):
        return (video[b0:b1].to(dev).to(torch.bfloat16), torch.from_numpy(mask[b0:b1]).to(dev).to(torch.uint8),
                (targets[0][:, b0:b1].to(dev).to(torch.bfloat16).contiguous(), targets[1][b0:b1].to(dev).to(torch.bfloat16).contiguous(),
                 targets[2][:, b0:b1].to(dev).to(torch.bfloat16).contiguous()))
    if world > 1:
        assert world * GAS * CLIPS == BATCH and eng.zero1 and eng.overlap
        micro = [clips(rank * GAS * CLIPS + k * CLIPS, rank * GAS * CLIPS + (k + 1) * CLIPS) for k in range(GAS)]
    else:
        whole = clips(0, BATCH)
    losses, norms = [], []
    for _ in range(STEPS):
        if world > 1:
            # equal-sized micro-batches: the mean of the W x gas local losses IS the loss of the concatenated batch
            lv = torch.zeros(1, dtype=torch.float64, device=dev)
            for v, m, tg in micro:
                lv += _micro_step(eng, v, m, tg, GAS, vis_inv=M.build_gather_indices(m, dev, L=L, check=False)).double() / GAS
            assert eng._acc_mat is None
            eng.optimizer_step(accumulated=True)
            dist.all_reduce(lv)
            lv /= world
        else:
            v, m, tg = whole
            loss, _ = eng.train_step(v, m, tg, vis_inv=M.build_gather_indices(m, dev, L=L, check=False))
            lv = loss.detach().reshape(1).double()
        losses.append(float(lv.item()))
        norms.append(float(eng.grad_norm.item()))
    torch.cuda.synchronize()
    if rank == 0:
        print(json.dumps({"world": world, "gas": GAS if world > 1 else 1, "global_batch": BATCH, "losses": losses, "grad_norms": norms,
                          "buckets": len(eng.buckets), "reduce": f"{eng.reduce_mode}/{eng.reduce_dtype}"}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def protocol():
    import faulthandler
    faulthandler.enable()
    import numpy as np
    from types import SimpleNamespace
    from internvideo_amd import ds_compat, masking
    from oracle import internvideo2_oracle as O
    from tests.test_model_gpu import build
    from tests.test_step_protocol import FIX2, teacher_features
    DEV = "cuda"
    cfg = O.named_config(FIX2["config"])
    B, TD = FIX2["batch"], FIX2["td_ratio"]
    T, h, w = cfg.grid
    params = O.synthetic_params(cfg, seed=FIX2["param_seed"])
    _one_rank_rccl()
    print("STEP group up", flush=True)
    args = SimpleNamespace(lr=FIX2["lr"], weight_decay=FIX2["weight_decay"], opt_betas=FIX2["betas"], opt_eps=FIX2["eps"], clip_grad=FIX2["clip"],
                           update_freq=2, zero_stage=1)
    model, optimizer, _, _ = ds_compat.initialize(args=args, model=build(cfg, params), model_parameters=None, dist_init_required=False, force_comm=True,
                                                  bucket_bytes=1 << 18)
    eng = model.engine
    assert model.gradient_accumulation_steps() == 2 and eng.zero1 and eng.overlap
    gv = torch.Generator().manual_seed(FIX2["video_seed"])
    loader = [torch.rand(B, 3, T * TD, cfg.img_size, cfg.img_size, generator=gv) for _ in range(FIX2["steps"])]
    steps, cur = [], None
    for e in FIX2["trace"]:
        if e["call"] == "clip_teacher":
            cur = {}
            steps.append(cur)
        if cur is not None:
            cur[e["call"]] = e
    model.train(); model.zero_grad(); model.micro_steps = 0
    got, gn, buckets = [], [], []
    for it, st in enumerate(steps):
        for group in optimizer.param_groups:                                             # E:56-61, every iteration
            group["lr"] = FIX2["lr_schedule"][it] * group["lr_scale"]
            if group["weight_decay"] > 0:
                group["weight_decay"] = FIX2["wd_schedule"][it]
        videos = loader[it].to(DEV)[:, :, ::TD]
        clip_mid, clip_fin, _, mae = (t.to(DEV) for t in teacher_features(it, cfg, B))
        e = st["model.__call__"]
        mask = torch.from_numpy(np.unpackbits(np.array(e["mask"]["packed"], dtype=np.uint8), axis=1)[:, :e["mask"]["shape"][1]].astype(bool)).to(DEV)
        tg_mid = masking.gather_visible(clip_mid, mask)
        tg_mae = masking.gather_visible(mae, mask, drop_cls=True)
        oc, of, om = model(videos.bfloat16(), mask)
        loss = (2 - 2 * (oc * tg_mid).sum(dim=-1)).mean() + (2 - 2 * (of * clip_fin).sum(dim=-1)).mean() + (2 - 2 * (om * tg_mae).sum(dim=-1)).mean()
        model.backward(loss)
        buckets.append(len(eng.reduce_log))
        model.step()
        got.append(loss.item())
        if st["model.step"]["boundary"]:
            gn.append(float(model.optimizer._global_grad_norm))
    _finish(dict(losses=got, grad_norms=gn, want_losses=[s["model.backward"]["loss"] for s in steps],
                 want_grad_norms=[s["model.step"]["grad_norm"] for s in steps if s["model.step"]["boundary"]],
                 buckets_per_micro_step=buckets, n_buckets=len(eng.buckets), acc_mat_is_none=eng._acc_mat is None,
                 micro_steps=model.micro_steps, global_steps=model.global_steps))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["host", "rccl1", "dp", "protocol"])
    ap.add_argument("--share-gpu", action="store_true")
    a = ap.parse_args()
    {"host": host, "rccl1": rccl1, "dp": lambda: dp(a), "protocol": protocol}[a.mode]()
