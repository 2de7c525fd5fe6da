"""Test-time forward of the classifier and the multi-view test (internvideo_amd.evaluate).  GPU box only.

    python tools/bench_eval.py [--batch 8] [--frames 8] [--reps 6] [--warmup 2] [--out profiles/eval_forward_ab.md]

Three measurements, written to one markdown file:
  1. the InternVideo2-1B classifier's forward on `--batch` clips of `--frames` x 224^2 (L = 2049 tokens at 8 frames) through the two
     paths a test pass can take: BlockStackFn under torch.no_grad() (what the model did before internvideo_amd.evaluate existed) and
     `forward_only` (the forward-only block loop).  The two alternate in one process, `--reps` times each after `--warmup` untimed rounds;
     per path the device-event times and `torch.cuda.max_memory_allocated` (the peak is reset before every run; the weights are in both);
     and the largest difference between the two paths' logits on the same clips;
  2. `final_test` + `ViewTable.finalize` on synthetic bf16 logits at the Kinetics-400 test shape (19,796 videos x 12 views x 400
     classes) with a stub model, i.e. the cost of everything but the model: the row pass, the table, the host loop, finalize;
  3. the deviation of the finalized mean probabilities from an fp64 recomputation on the rows of tests/golden/eval_views.npz, next to the
     reference's own fp32-vs-fp64 error recorded there.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from internvideo_amd import evaluate as E, internvideo2 as FT, ops  # noqa: E402

DEV = "cuda"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), torch.cuda.max_memory_allocated(), out


def forward_ab(a, lines):
    torch.manual_seed(0)
    with torch.device(DEV):
        model = FT.internvideo2_1B_patch14_224(num_frames=a.frames, num_classes=400, drop_path_rate=0.0)
    model.eval()
    clips = torch.rand((a.batch, 3, a.frames, 224, 224), device=DEV).to(torch.bfloat16)
    weights = torch.cuda.memory_allocated()

    def stack():
        with torch.no_grad():
            return model(clips)

    def fwd_only():
        with E.forward_only(model):
            return model(clips)

    paths = (("BlockStackFn under no_grad", stack), ("forward_only", fwd_only))
    ms = {n: [] for n, _ in paths}
    peak = {n: 0 for n, _ in paths}
    outs = {}
    for r in range(a.warmup + a.reps):
        for name, fn in paths:                                  # alternating, same process, same clips
            t, p, o = timed(fn)
            if r >= a.warmup:
                ms[name].append(t); peak[name] = max(peak[name], p)
            outs[name] = o.float()
            del o
    diff = (outs[paths[0][0]] - outs[paths[1][0]]).abs().max().item()
    scale = outs[paths[0][0]].abs().max().item()
    L = 1 + a.frames * 256
    lines += [f"## 1. Test-time forward, InternVideo2-1B, {a.frames} x 224^2 (L = {L}), batch {a.batch}, bf16", "",
              f"Alternating runs in one process, {a.reps} timed after {a.warmup} warm-up rounds; device events around `model(clips)`; "
              f"`torch.cuda.max_memory_allocated` with the peak reset before every run.  Allocated before the first forward (weights, clips): "
              f"{weights / 2**30:.2f} GiB.", "",
              "| path | ms min | ms median | ms max | clips/s (median) | peak allocated GiB | peak above weights GiB |", "|---|---|---|---|---|---|---|"]
    for name, _ in paths:
        v = sorted(ms[name]); med = v[len(v) // 2]
        lines.append(f"| {name} | {v[0]:.1f} | {med:.1f} | {v[-1]:.1f} | {a.batch / med * 1e3:.1f} | {peak[name] / 2**30:.2f} | {(peak[name] - weights) / 2**30:.2f} |")
    lines += ["", f"Largest |difference| between the two paths' logits on the same clips: {diff:.3g} (largest |logit| {scale:.3g}).", ""]
    del model, clips
    torch.cuda.empty_cache()


class Stub:
    def __init__(self, pool):
        self.pool, self.i = pool, 0

    def eval(self):
        return self

    def __call__(self, clips):
        self.i += 1
        return self.pool[self.i % len(self.pool)][:clips.shape[0]]


def table_pass(a, lines):
    n_videos, n_views, V, B = 19796, 12, 400, a.test_batch
    names = [f"v{i:05d}" for i in range(n_videos)]
    g = torch.Generator().manual_seed(1)
    order = torch.randperm(n_videos * n_views, generator=g)
    labels = torch.randint(0, V, (n_videos,), generator=g)
    pool = [(torch.randn((B, V), generator=g) * 2.5).to(DEV).to(torch.bfloat16) for _ in range(16)]

    def loader():
        for at in range(0, order.numel(), B):
            idx = order[at:at + B]
            vid = idx // n_views
            view = idx % n_views
            yield torch.zeros((idx.numel(), 1)), labels[vid], [names[v] for v in vid.tolist()], view // 3, view % 3

    rows = []
    for r in range(1 + a.table_reps):
        table = E.ViewTable(names, n_views, V, device=DEV)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        E.final_test(loader(), Stub(pool), DEV, None, ds=True, bf16=True, table=table)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        scores = table.finalize()
        t2 = time.perf_counter()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.view_finalize(table.table, table.owner, table.labels, n_views, V)
        e1.record()
        torch.cuda.synchronize()
        if r:
            rows.append((t1 - t0, t2 - t1, e0.elapsed_time(e1)))
        assert int(scores.count.min()) == n_views
    nb = (order.numel() + B - 1) // B
    tbytes = table.table.numel() * 2
    lines += [f"## 2. `final_test(table=...)` + `finalize`, synthetic logits, {n_videos} videos x {n_views} views x {V} classes", "",
              f"A stub model hands out bf16 logits that are already on the device, so this is the cost of everything but the model: {nb} batches "
              f"of {B} rows (host loop, name lookup, one row pass per batch), then finalize.  Host clock around work that ends in a device "
              f"synchronise; the finalize kernel alone by device events.  Table: {tbytes / 1e6:.0f} MB of bf16 logits.", "",
              "| run | final_test s | per batch us | finalize (kernel + one host copy) ms | finalize kernel ms | kernel GB/s (table read once) |", "|---|---|---|---|---|---|"]
    for i, (a_, b_, k_) in enumerate(rows):
        lines.append(f"| {i} | {a_:.3f} | {a_ / nb * 1e6:.0f} | {b_ * 1e3:.2f} | {k_:.3f} | {tbytes / k_ / 1e6:.0f} |")
    lines.append("")


def deviation(lines):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "eval_views.npz"))
    names = [str(n) for n in gold["video_names"]]
    lines += ["## 3. Finalized mean probabilities against fp64, rows of tests/golden/eval_views.npz", "",
              "| case | max abs deviation (device, fp32) | reference's own fp32-vs-fp64 error | 16 x that (the test's bound) |", "|---|---|---|---|"]
    for pre in (str(c) for c in gold["cases"]):
        V = int(pre[1:pre.index(":")]); nv = int(pre[pre.index(":s") + 2]) * 3
        table = E.ViewTable(names, nv, V, device=DEV)
        p64 = np.zeros((len(names), V)); count = np.zeros(len(names)); seen = set()
        for k in (0, 1):
            r = pre + f"r{k}:"
            x = (gold[r + "bits"].astype(np.uint32) << 16).view(np.float32)
            at = 0
            for n in gold[r + "sizes"]:
                s = slice(at, at + int(n)); at += int(n)
                table.add(torch.from_numpy(x[s]).to(DEV).to(torch.bfloat16), torch.from_numpy(gold[r + "labels"][s].astype(np.int64)),
                          [names[v] for v in gold[r + "video"][s]], gold[r + "chunk"][s].tolist(), gold[r + "split"][s].tolist(), rank=k)
            for i in range(x.shape[0]):
                key = (int(gold[r + "video"][i]), int(gold[r + "chunk"][i]) * 3 + int(gold[r + "split"][i]))
                if key not in seen:
                    seen.add(key)
                    e = np.exp(x[i].astype(np.float64) - x[i].max())
                    p64[key[0]] += e / e.sum(); count[key[0]] += 1
        p64[count > 0] /= count[count > 0, None]
        probs = table.finalize(want_probs=True).probs.cpu().numpy().astype(np.float64)
        f32err = float(gold[pre + "f32err"][0])
        lines.append(f"| {pre[:-1]} | {np.abs(probs - p64).max():.3g} | {f32err:.3g} | {16 * f32err:.3g} |")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--test-batch", type=int, default=64)
    ap.add_argument("--table-reps", type=int, default=2)
    ap.add_argument("--skip-forward", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_forward_ab.md"))
    a = ap.parse_args()
    ops._L.require_gpu()
    lines = ["# Validation and multi-view test: forward paths, table pass, probability deviation", "",
             f"`python tools/bench_eval.py --batch {a.batch} --frames {a.frames} --reps {a.reps} --warmup {a.warmup} --test-batch {a.test_batch}` on "
             f"{torch.cuda.get_device_name(0)}.", ""]
    if not a.skip_forward:
        forward_ab(a, lines)
    table_pass(a, lines)
    deviation(lines)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
