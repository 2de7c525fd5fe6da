"""Fine-tuning / inference regime: InternVideo2-1B classifier, 8 x 224^2 clips, NO masking -> L = 2049 tokens per clip, the
long-sequence attention regime (attention is 19 % of the FLOPs instead of 4 %).  Forward + cross-entropy + backward in plain autograd (the
reference's engine_for_finetuning.py drives the model that way), and forward only (inference).  GPU box only.

    python tools/bench_finetune.py [--batch 16] [--steps 5] [--warmup 2] [--frames 8] [--mixup [--torch-loss]]

--mixup puts the recipe's step into the timed region (run_finetuning.py:116-148: Mixup 0.8 / CutMix 1.0 / smoothing 0.1, batch mode, on fp32
clips, then the soft-target loss): natively through internvideo_amd.finetune (ivh_mix_clips + ivh_soft_ce_rows, the draw in a device-side
table), or with --torch-loss as the torch ops the reference runs (flip / mul_ / add_ / .bfloat16(), dense one-hot target, log_softmax), on the
same seeded draws -- the A/B of profiles/finetune_native_step_ab.md.
The JSON line carries `step_form`, `train_ms_min` / `train_ms_max` and `mix_and_cast_ms` (null without --mixup) in every mode.

One JSON line: clips/s and ms for training-mode forward + backward and for inference forward, the algorithmic TFLOP per clip, the fraction of
the dense bf16 MFMA peak, peak memory.  Random-init weights, synthetic clips, drop_path 0 in the timing (the recipe's 0.3 changes no shape)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from internvideo_amd import internvideo2 as FT  # noqa: E402

PEAK = 2500.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--classes", type=int, default=400)
    ap.add_argument("--mixup", action="store_true", help="Mixup / CutMix + soft-target loss inside the timed step")
    ap.add_argument("--torch-loss", action="store_true", help="with --mixup: the torch-op form of the mixing and the loss (A/B)")
    a = ap.parse_args()
    torch.manual_seed(0)
    dev = "cuda"
    with torch.device(dev):
        model = FT.internvideo2_1B_patch14_224(num_frames=a.frames, num_classes=a.classes, drop_path_rate=0.0)
    model.train()
    B, T = a.batch, a.frames
    L = 1 + T * 256
    D, Hm, depth = 1408, 6144, 40
    fwd_flop = depth * (2.0 * L * D * (3 * D + D + 2 * Hm) + 4.0 * L * L * D) + 2.0 * T * 256 * 588 * D
    video = torch.rand((B, 3, T, 224, 224), device=dev).to(torch.bfloat16)
    labels = torch.randint(0, a.classes, (B,), device=dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    train_ms, fwd_ms, bwd_ms, infer_ms, mix_ms = [], [], [], [], []
    if a.mixup:
        from internvideo_amd import finetune
        np.random.seed(0)
        mixer = finetune.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode="batch", label_smoothing=0.1, num_classes=a.classes)
        clips32 = torch.rand((B, 3, T, 224, 224), device=dev)                      # the loader's fp32 batch
        work = torch.empty_like(clips32)                                           # --torch-loss mixes in place, as the reference does
        labels32 = labels.to(torch.int32)
        static = mixer.draw(B, clips32.shape).to(dev)

    def torch_form(params):
        """datasets/mixup.py _mix_batch + mixup_target + SoftTargetCrossEntropy as torch ops, on the draw `params`"""
        kind, yl, yh, xl, xh = (int(v) for v in params.table[0, 1:6])
        lam, oml = (float(v) for v in params.target_mix[0])
        if kind == 1:
            flipped = work.flip(0).mul_(oml)
            work.mul_(lam).add_(flipped)
        elif kind == 2:
            work[..., yl:yh, xl:xh] = work.flip(0)[..., yl:yh, xl:xh]
        x = work.bfloat16()
        off = 0.1 / a.classes
        y1 = torch.full((B, a.classes), off, device=dev).scatter_(1, labels.view(-1, 1), 1.0 - 0.1 + off)
        y2 = torch.full((B, a.classes), off, device=dev).scatter_(1, labels.flip(0).view(-1, 1), 1.0 - 0.1 + off)
        return x, y1 * lam + y2 * oml

    for it in range(a.warmup + a.steps):
        model.zero_grad(set_to_none=True)
        e0, em, e1, e2 = ev(), ev(), ev(), ev()
        if a.mixup:
            params = mixer.draw(B, clips32.shape)                                   # host side, outside the timed region in both forms
            if a.torch_loss:
                work.copy_(clips32)
            else:
                static.copy_(params)
        e0.record()
        if a.mixup and a.torch_loss:
            x, target = torch_form(params)
            em.record()
            logits = model(x)
            loss = torch.sum(-target * torch.nn.functional.log_softmax(logits.float(), dim=-1), dim=-1).mean()
        elif a.mixup:
            x, la, lb, mix = mixer.apply(clips32, labels32, static)
            em.record()
            loss, logits = model.forward_loss(x, la, lb, mix, smoothing=0.1)
        else:
            em.record()
            logits = model(video)
            loss = torch.nn.functional.cross_entropy(logits.float(), labels)
        e1.record()
        loss.backward()
        e2.record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            train_ms.append(e0.elapsed_time(e2)); fwd_ms.append(e0.elapsed_time(e1)); bwd_ms.append(e1.elapsed_time(e2))
            mix_ms.append(e0.elapsed_time(em))
    peak_train = torch.cuda.max_memory_allocated() / 1e9
    model.zero_grad(set_to_none=True)
    model.eval()
    with torch.no_grad():
        for it in range(a.warmup + a.steps):
            e0, e1 = ev(), ev()
            e0.record()
            model(video)
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                infer_ms.append(e0.elapsed_time(e1))
    t_tr, t_inf = float(np.median(train_ms)), float(np.median(infer_ms))
    print(json.dumps(dict(metric="clips/sec, InternVideo2-1B classifier (fine-tuning regime, no masking), 8x224^2 -> L=2049, bf16, 1 GPU",
                          train_clips_per_s=round(B / t_tr * 1e3, 2), train_ms=round(t_tr, 2), forward_ms=round(float(np.median(fwd_ms)), 2),
                          backward_ms=round(float(np.median(bwd_ms)), 2), train_mfma_frac=round(3 * fwd_flop * B / (t_tr * 1e-3) / 1e12 / PEAK, 4),
                          infer_clips_per_s=round(B / t_inf * 1e3, 2), infer_ms=round(t_inf, 2),
                          infer_mfma_frac=round(fwd_flop * B / (t_inf * 1e-3) / 1e12 / PEAK, 4), batch=B, seq_len=L,
                          tflop_per_clip_fwd=round(fwd_flop / 1e12, 3), attention_share_of_flops=round(depth * 4.0 * L * L * D / fwd_flop, 3),
                          peak_mem_gb_train=round(peak_train, 1), loss=round(float(loss), 4), dtype="bf16", data="synthetic",
                          launch_mode="eager autograd (no HIP graph, no fused optimizer)",
                          step_form=("torch-op mixup + soft-target loss" if a.torch_loss else "native mixup + soft-target loss") if a.mixup else "plain cross entropy",
                          train_ms_min=round(min(train_ms), 2), train_ms_max=round(max(train_ms), 2),
                          mix_and_cast_ms=round(float(np.median(mix_ms)), 3) if a.mixup else None)), flush=True)


if __name__ == "__main__":
    main()
