"""Linear-probing regime (scripts/finetuning/linear_probing/1B_lp_k400_f16.sh: InternVideo2-1B, 16 x 224^2 clips -> L = 4097 tokens, batch 64,
every block frozen): the time of one probe step on the native engine, and a same-box A/B of the frozen-prefix trunk against the existing
classifier with the same parameters frozen.  GPU box only.

    python tools/bench_probe.py [--steps 5] [--warmup 2] [--rounds 3] [--max-batch 64] [--skip-full] [--skip-ab] [--kernels] [--md FILE]

Part 1 (`probe_step`): internvideo2_cat_1B_patch14_224 after probe.freeze_for_probing, heads `proj` and `cls_avgN` / `kaiming_BN`, 16 frames,
the largest batch of (64, 48, 32, 16, 8), from --max-batch down, that runs without an out-of-memory error; one step = IVTrainEngine.train_step_fn(forward_loss).
Part 2 (`probe_ab`): 1B, 8 frames, batch 8, open_block_num 0 and 1.  A = internvideo2_cat_1B_patch14_224 (`proj`) with `frozen_prefix` set
by freeze_for_probing; B = internvideo2_1B_patch14_224 with the same names frozen and no `frozen_prefix`, i.e. every block through
BlockStackFn as before.  Both models live side by side and are timed in alternating rounds (A B A B ...), each round `steps` steps after
`warmup`; reported: the median step of every round, and peak memory of a step of each (measured in a round of its own).
Part 3 (`pool_call`, --kernels): the pooling pass alone, see pool_calls.
One JSON line per measurement; --md writes the same numbers as a markdown table.  Random-init weights, synthetic clips, drop_path 0."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from internvideo_amd import internvideo2 as FT, internvideo2_cat as CAT  # noqa: E402
from internvideo_amd.engine import IVTrainEngine  # noqa: E402
from internvideo_amd.probe import freeze_for_probing  # noqa: E402

DEV = "cuda"
CLASSES = 400


def build(kind, frames, open_block_num, **extra):
    with torch.device(DEV):
        if kind == "parent":
            m = FT.internvideo2_1B_patch14_224(num_frames=frames, num_classes=CLASSES, drop_path_rate=0.0)
        else:
            m = CAT.internvideo2_cat_1B_patch14_224(num_frames=frames, num_classes=CLASSES, drop_path_rate=0.0, **extra)
    m.train()
    freeze_for_probing(m, open_block_num=open_block_num)
    if kind == "parent":
        del m.frozen_prefix                                   # the existing classifier's path: every block through BlockStackFn
    return m


class Stepper:
    def __init__(self, model, batch, frames):
        self.model, self.batch = model, batch
        self.engine = IVTrainEngine(model, lr=1e-4)
        self.video = torch.rand((batch, 3, frames, 224, 224), device=DEV).to(torch.bfloat16)
        self.labels = torch.randint(0, CLASSES, (batch,), device=DEV, dtype=torch.int32)

    def step(self):
        return self.engine.train_step_fn(lambda: self.model.forward_loss(self.video, self.labels, smoothing=0.1))

    def timed(self, warmup, steps):
        ms = []
        for it in range(warmup + steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.step()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms.append(e0.elapsed_time(e1))
        return ms

    def close(self):
        self.engine.close()


def probe_step(a, rows):
    for method, norm in (("proj", "kaiming_BN"), ("cls_avgN", "kaiming_BN")):
        done = False
        for batch in (b for b in (64, 48, 32, 16, 8) if b <= a.max_batch):
            st = None
            try:
                st = Stepper(build("cat", 16, 0, merge_method=method, merge_norm=norm), batch, 16)
                torch.cuda.reset_peak_memory_stats()
                ms = st.timed(a.warmup, a.steps)
                r = dict(measurement="probe_step", model="internvideo2_cat_1B_patch14_224", merge_method=method, merge_norm=norm, frames=16,
                         seq_len=4097, batch=batch, open_block_num=0, step_ms_median=round(float(np.median(ms)), 2), step_ms_min=round(min(ms), 2),
                         step_ms_max=round(max(ms), 2), clips_per_s=round(batch / float(np.median(ms)) * 1e3, 2),
                         peak_mem_gb=round(torch.cuda.max_memory_allocated() / 1e9, 1), steps=a.steps, warmup=a.warmup)
                print(json.dumps(r), flush=True)
                rows.append(r)
                done = True
            except torch.cuda.OutOfMemoryError:
                print(json.dumps(dict(measurement="probe_step", merge_method=method, batch=batch, result="out of memory")), flush=True)
            finally:
                if st is not None:
                    st.close()
                del st
                torch.cuda.empty_cache()
            if done:
                break


def probe_ab(a, rows):
    frames, batch = 8, 8
    for k in (0, 1):
        A = Stepper(build("cat", frames, k, merge_method="proj"), batch, frames)
        B = Stepper(build("parent", frames, k), batch, frames)
        B.model.load_state_dict(A.model.state_dict(), strict=True)       # same weights (the engine's post-hook refreshes its bf16 copies)
        B.video.copy_(A.video); B.labels.copy_(A.labels)
        peak = {}
        for name, st in (("A", A), ("B", B)):
            st.timed(1, 1)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            st.timed(0, 1)
            peak[name] = (torch.cuda.max_memory_allocated() - base) / 1e9
        med = {"A": [], "B": []}
        for _ in range(a.rounds):
            for name, st in (("A", A), ("B", B)):
                med[name].append(float(np.median(st.timed(a.warmup, a.steps))))
        la, lb = float(A.step()[0].detach()), float(B.step()[0].detach())
        r = dict(measurement="probe_ab", frames=frames, seq_len=1 + frames * 256, batch=batch, open_block_num=k,
                 A="internvideo2_cat_1B_patch14_224 proj, frozen_prefix (forward-only trunk)",
                 B="internvideo2_1B_patch14_224, same parameters frozen, BlockStackFn over every block",
                 A_round_medians_ms=[round(v, 2) for v in med["A"]], B_round_medians_ms=[round(v, 2) for v in med["B"]],
                 A_ms=round(float(np.median(med["A"])), 2), B_ms=round(float(np.median(med["B"])), 2),
                 B_over_A=round(float(np.median(med["B"])) / float(np.median(med["A"])), 3),
                 A_step_extra_mem_gb=round(peak["A"], 2), B_step_extra_mem_gb=round(peak["B"], 2), loss_A=round(la, 5), loss_B=round(lb, 5),
                 rounds=a.rounds, steps=a.steps, warmup=a.warmup)
        print(json.dumps(r), flush=True)
        rows.append(r)
        A.close(); B.close()
        del A, B
        torch.cuda.empty_cache()


def pool_calls(a, rows):
    """part 3 (`pool_call`): the stream pass alone at the recipe's shape (64 clips x 4097 tokens x 1408, 1.48 GB in fp32: far beyond the
    last-level cache), time between device events around single calls; ops.token_mean_fwd (the pass AttnPoolFn makes) for comparison"""
    from internvideo_amd import ops
    B, T, S, Cn = 64, 16, 256, 1408
    Lr = 1 + T * S
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn((B * Lr, Cn), device=DEV).to(dtype)
        variants = [("avgN", lambda: ops.cat_pool_fwd(x, B, T, S)), ("avgN + token mean", lambda: ops.cat_pool_fwd(x, B, T, S, want_token_mean=True)),
                    ("avg1 + token mean", lambda: ops.cat_pool_fwd(x, B, T, S, avg1=True, want_token_mean=True))]
        if dtype == torch.float32:
            variants.append(("ops.token_mean_fwd", lambda: ops.token_mean_fwd(x, B, Lr)))
        for name, fn in variants:
            us = []
            for it in range(3 + 20):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if it >= 3:
                    us.append(e0.elapsed_time(e1) * 1e3)
            nbytes = x.numel() * x.element_size()
            r = dict(measurement="pool_call", call=name, stream_dtype=str(dtype).replace("torch.", ""), shape=[B, T, S, Cn], stream_gb=round(nbytes / 1e9, 3),
                     call_us_median=round(float(np.median(us)), 1), call_us_min=round(min(us), 1), call_us_max=round(max(us), 1),
                     gb_per_s=round(nbytes / 1e9 / (float(np.median(us)) * 1e-6), 0))
            print(json.dumps(r), flush=True)
            rows.append(r)
        del x
        torch.cuda.empty_cache()


def write_md(path, rows):
    lines = ["| measurement | configuration | batch | open blocks | result |", "|---|---|---|---|---|"]
    for r in rows:
        if r["measurement"] == "pool_call":
            lines.append(f"| pool call | {r['call']}, {r['stream_dtype']} stream {r['shape']} ({r['stream_gb']} GB) | 64 | - | "
                         f"{r['call_us_median']} us (min {r['call_us_min']}, max {r['call_us_max']}), {r['gb_per_s']:.0f} GB/s |")
        elif r["measurement"] == "probe_step":
            lines.append(f"| probe step | 1B, 16 frames, {r['merge_method']} / {r['merge_norm']} | {r['batch']} | 0 | "
                         f"{r['step_ms_median']} ms (min {r['step_ms_min']}, max {r['step_ms_max']}), {r['clips_per_s']} clips/s, peak {r['peak_mem_gb']} GB |")
        else:
            lines.append(f"| A/B | 1B, 8 frames, proj | {r['batch']} | {r['open_block_num']} | A {r['A_ms']} ms {r['A_round_medians_ms']}, "
                         f"B {r['B_ms']} ms {r['B_round_medians_ms']}, B / A = {r['B_over_A']}; step memory A {r['A_step_extra_mem_gb']} GB, "
                         f"B {r['B_step_extra_mem_gb']} GB |")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-batch", type=int, default=64, help="part 1: start the batch search here")
    ap.add_argument("--skip-full", action="store_true", help="skip part 1 (the 16-frame probe step)")
    ap.add_argument("--skip-ab", action="store_true", help="skip part 2 (the 8-frame A/B)")
    ap.add_argument("--kernels", action="store_true", help="part 3: time the pooling pass alone at the recipe's shape")
    ap.add_argument("--md", default=None, help="also write the results as a markdown table to this file")
    a = ap.parse_args()
    torch.manual_seed(0)
    rows = []
    if not a.skip_ab:
        probe_ab(a, rows)
    if not a.skip_full:
        probe_step(a, rows)
    if a.kernels:
        pool_calls(a, rows)
    if a.md:
        write_md(a.md, rows)


if __name__ == "__main__":
    main()
