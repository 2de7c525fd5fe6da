"""The fine-tuning step of InternVideo2/single_modality/run_finetuning.py on the MI355X: Mixup / CutMix of the clip batch, the soft-target
cross entropy and top-k accuracy, in the kernels of csrc/finetune.hip.

    mixup_fn = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch',
                     label_smoothing=0.1, num_classes=400)                                   # run_finetuning.py:349-352, unchanged
    criterion = SoftTargetCrossEntropy()                                                     # run_finetuning.py:593-597

    samples, targets = mixup_fn(samples, targets)        # drop-in: (bf16 clips, dense fp32 target), engine_for_finetuning.py:63-67
    loss = criterion(model(samples), targets)

    x, a, b, mix = mixup_fn.apply(samples, labels, params)       # native: the draw is a table in HBM, so the step can be captured
    loss, logits = model.forward_loss(x, a, b, mix, smoothing=0.1)

`Mixup` is a TABLE BUILDER: `draw()` consumes numpy's global RNG in exactly the order of datasets/mixup.py (so a seeded run draws the
reference's lambda, mixup / cutmix switch and boxes) and returns host arrays; the mixing itself is ivh_mix_clips reading that table from
device memory.  Which (lam, oml) pair goes into the table is decided here and differs by mode, because the reference multiplies by a
Python double in 'batch' mode and by fp32 scalars in 'elem' mode:
    batch:  (f32(lam), f32(1.0 - lam)), lam a double             elem:  (f32(lam), f32(1) - f32(lam))
and after CutMix the target uses the box-corrected lambda.  With those pairs the kernels reproduce the reference's clips and targets bit
for bit (tests/golden/finetune_mixup.npz).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch
from torch import nn

from . import ops

BF16, F32 = torch.bfloat16, torch.float32
KIND_NONE, KIND_MIXUP, KIND_CUTMIX = 0, 1, 2


class DeviceMixParams(NamedTuple):
    """a draw in HBM: what a captured step reads.  Refresh with `copy_` between replays."""
    table: torch.Tensor        # int32 (B, 8)
    target_mix: torch.Tensor   # fp32 (B, 2)

    def copy_(self, params: "MixParams") -> "DeviceMixParams":
        self.table.copy_(torch.from_numpy(params.table))              # 40 bytes per sample from pageable memory: a plain blocking copy
        self.target_mix.copy_(torch.from_numpy(params.target_mix))
        return self


class MixParams(NamedTuple):
    """a draw on the host.  table[i] = (src, kind, yl, yh, xl, xh, bits(lam), bits(oml)): how ivh_mix_clips makes clip i;
    target_mix[i] = (lam, oml): the weights of label i and label B-1-i in the target of row i."""
    table: np.ndarray          # int32 (B, 8)
    target_mix: np.ndarray     # float32 (B, 2)

    def to(self, device) -> DeviceMixParams:
        return DeviceMixParams(torch.from_numpy(self.table).to(device), torch.from_numpy(self.target_mix).to(device))


def _bits(v) -> int:
    return int(np.float32(v).view(np.int32))


class Mixup:
    """datasets/mixup.py:90-119: same constructor, attributes and `mixup_enabled` switch; `mode` 'batch' or 'elem'."""

    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch', correct_lam=True,
                 label_smoothing=0.1, num_classes=1000):
        self.mixup_alpha = mixup_alpha
        self.cutmix_alpha = cutmix_alpha
        self.cutmix_minmax = cutmix_minmax
        if cutmix_minmax is not None:
            if len(cutmix_minmax) != 2:
                raise ValueError("cutmix_minmax is a (min, max) pair")
            self.cutmix_alpha = 1.0                            # the box comes from min / max; the alpha only has to switch CutMix on
        self.mix_prob = prob
        self.switch_prob = switch_prob
        self.label_smoothing = label_smoothing
        self.num_classes = num_classes
        self.mode = mode
        self.correct_lam = correct_lam
        self.mixup_enabled = True                              # the training loop may switch mixing off (all samples pass through)
        if mode == 'pair':
            raise NotImplementedError(
                "Mixup(mode='pair') is not supported: the reference's _mix_pair cuts a 4-D video sample as x[i][:, yl:yh, xl:xh], i.e. it "
                "applies a box drawn for (H, W) to (T, H); reproducing that is not wanted and no shipped script selects the mode")
        if mode not in ('batch', 'elem'):
            raise ValueError(f"unknown mixup mode {mode!r}")

    # ---- the draws, in the reference's RNG order -------------------------------------------------------------------------------------
    def _lam_mix(self, size=None):
        """(lambda, use_cutmix) before the mix_prob decision: scalars for 'batch', arrays of `size` for 'elem'"""
        if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
            if size is None:
                use_cutmix = bool(np.random.rand() < self.switch_prob)
                alpha = self.cutmix_alpha if use_cutmix else self.mixup_alpha
                return np.random.beta(alpha, alpha), use_cutmix
            use_cutmix = np.random.rand(size) < self.switch_prob
            lam_cut = np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=size)      # both are drawn for every sample
            lam_mix = np.random.beta(self.mixup_alpha, self.mixup_alpha, size=size)
            return np.where(use_cutmix, lam_cut, lam_mix), use_cutmix
        if self.mixup_alpha > 0.:
            return np.random.beta(self.mixup_alpha, self.mixup_alpha, size=size), (False if size is None else np.zeros(size, dtype=bool))
        if self.cutmix_alpha > 0.:
            return np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=size), (True if size is None else np.ones(size, dtype=bool))
        raise ValueError("one of mixup_alpha > 0, cutmix_alpha > 0, cutmix_minmax is needed")

    def _box(self, H: int, W: int, lam, f32: bool):
        """one CutMix box and the lambda that goes with it.  `f32`: lambda is an fp32 scalar ('elem' mode) and the cut size is computed in
        fp32, as numpy does for `int * float32`."""
        if self.cutmix_minmax is not None:
            lo, hi = self.cutmix_minmax
            cut_h = np.random.randint(int(H * lo), int(H * hi))
            cut_w = np.random.randint(int(W * lo), int(W * hi))
            yl = np.random.randint(0, H - cut_h)
            xl = np.random.randint(0, W - cut_w)
            yl, yh, xl, xh = int(yl), int(yl + cut_h), int(xl), int(xl + cut_w)
        else:
            if f32:
                ratio = np.sqrt(np.float32(1) - np.float32(lam))
                cut_h, cut_w = int(np.float32(H) * ratio), int(np.float32(W) * ratio)
            else:
                ratio = np.sqrt(1 - float(lam))
                cut_h, cut_w = int(H * ratio), int(W * ratio)
            cy = int(np.random.randint(0, H))
            cx = int(np.random.randint(0, W))
            yl, yh = min(max(cy - cut_h // 2, 0), H), min(max(cy + cut_h // 2, 0), H)
            xl, xh = min(max(cx - cut_w // 2, 0), W), min(max(cx + cut_w // 2, 0), W)
        if self.correct_lam or self.cutmix_minmax is not None:
            lam = 1. - ((yh - yl) * (xh - xl)) / float(H * W)
        return (yl, yh, xl, xh), lam

    def draw(self, batch_size: int, clip_shape) -> MixParams:
        """one step's draw for `batch_size` clips whose last two dimensions are (H, W)"""
        if batch_size % 2:
            raise ValueError("Mixup: the batch size must be even (sample i is mixed with sample B-1-i)")
        H, W = int(clip_shape[-2]), int(clip_shape[-1])
        B = int(batch_size)
        table = np.zeros((B, 8), dtype=np.int32)
        table[:, 0] = B - 1 - np.arange(B)
        table[:, 6] = _bits(1.0)
        tmix = np.zeros((B, 2), dtype=np.float32)
        tmix[:, 0] = 1.0
        if self.mode == 'elem':
            if not self.mixup_enabled:
                return MixParams(table, tmix)
            lam_mix, use_cutmix = self._lam_mix(B)
            lam_batch = np.where(np.random.rand(B) < self.mix_prob, lam_mix.astype(np.float32), np.ones(B, dtype=np.float32))
            for i in range(B):
                lam = lam_batch[i]
                if lam == 1.:
                    continue
                if use_cutmix[i]:
                    box, lam = self._box(H, W, lam, f32=True)
                    table[i, 1] = KIND_CUTMIX
                    table[i, 2:6] = box
                else:
                    table[i, 1] = KIND_MIXUP
                lam = np.float32(lam)
                oml = np.float32(1) - lam
                table[i, 6], table[i, 7] = _bits(lam), _bits(oml)
                tmix[i] = (lam, oml)
            return MixParams(table, tmix)
        # 'batch': one draw for all samples
        if not (self.mixup_enabled and np.random.rand() < self.mix_prob):
            return MixParams(table, tmix)
        lam, use_cutmix = self._lam_mix(None)
        lam = float(lam)
        if lam == 1.:
            return MixParams(table, tmix)
        if use_cutmix:
            box, lam = self._box(H, W, lam, f32=False)
            table[:, 1] = KIND_CUTMIX
            table[:, 2:6] = box
        else:
            table[:, 1] = KIND_MIXUP
        lam, oml = np.float32(lam), np.float32(1. - lam)
        table[:, 6], table[:, 7] = _bits(lam), _bits(oml)
        tmix[:] = (lam, oml)
        return MixParams(table, tmix)

    # ---- device side -------------------------------------------------------------------------------------------------------------------
    def __call__(self, x: torch.Tensor, target: torch.Tensor):
        """drop-in for the reference's loop (engine_for_finetuning.py:63-67): x fp32|bf16 (B, C, T, H, W), target integer labels (B,)
        -> (mixed clips bf16 -- the loop's `.bfloat16()` is then a no-op --, dense fp32 (B, num_classes) target)"""
        assert len(x) % 2 == 0, 'Batch size should be even when using this'
        params = self.draw(len(x), x.shape).to(x.device)
        mixed = ops.mix_clips(x.contiguous(), params.table, BF16)
        return mixed, ops.mixup_target(target, params.target_mix, float(self.label_smoothing), int(self.num_classes))

    def apply(self, x: torch.Tensor, labels: torch.Tensor, params=None):
        """native form -> (mixed clips bf16, label_a int32 (B,), label_b int32 (B,), mix fp32 (B, 2)), the arguments of
        InternVideo2.forward_loss / ops.soft_ce_rows.  params: None (draw now), a MixParams (uploaded now) or a DeviceMixParams; with the
        latter nothing here touches the host, so the call can sit in a captured step whose table is refreshed by `copy_` between replays."""
        if params is None:
            params = self.draw(len(x), x.shape)
        if isinstance(params, MixParams):
            params = params.to(x.device)
        label_a = labels if labels.dtype == torch.int32 else labels.to(torch.int32)
        return ops.mix_clips(x.contiguous(), params.table, BF16), label_a, label_a.flip(0), params.target_mix


# ---- losses ------------------------------------------------------------------------------------------------------------------------------
def _kernel_rows(logits: torch.Tensor):
    """(matrix the row kernel accepts, V): the classifier's `[:, :n]` view of its zero-padded head GEMM passes as it is (the kernel
    ignores columns >= V); any other (M, V) matrix is copied into rows padded to a multiple of 8 columns"""
    M, V = logits.shape
    if logits.dtype not in (BF16, F32):
        logits = logits.float()
    if logits.stride(1) == 1 and logits.stride(0) % 8 == 0 and logits.stride(0) >= V and logits.data_ptr() % 16 == 0:
        return logits, V
    buf = logits.new_zeros((M, (V + 7) // 8 * 8))
    buf[:, :V].copy_(logits)
    return buf[:, :V], V


class SoftCrossEntropyFn(torch.autograd.Function):
    """mean over rows of -sum_c t_c log_softmax(logits)_c for a factored or a dense target (ops.soft_ce_rows).  The backward runs the row
    kernel again with the upstream gradient as a device scalar (no host visit, as xbert.LinearCrossEntropyFn) and writes the gradient
    into a NEW tensor: the logits are tiny and callers read them after the backward."""

    @staticmethod
    def forward(ctx, logits, label_a, label_b, mix, smoothing, target):
        lg, V = _kernel_rows(logits.detach())
        loss, _, _ = ops.soft_ce_rows(lg, label_a, label_b, mix, smoothing, V=V, target=target, want_grad=False)
        ctx.save_for_backward(lg, label_a, label_b, mix, target)
        ctx.smoothing, ctx.V, ctx.dtype = smoothing, V, logits.dtype
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        lg, label_a, label_b, mix, target = ctx.saved_tensors
        _, dl, _ = ops.soft_ce_rows(lg, label_a, label_b, mix, ctx.smoothing, V=ctx.V, target=target, want_grad=True,
                                    dscale_dev=g.reshape(1).float().contiguous())
        return dl[:, :ctx.V].to(ctx.dtype), None, None, None, None, None


def soft_cross_entropy(logits, label_a=None, label_b=None, mix=None, smoothing: float = 0.0, target=None) -> torch.Tensor:
    if target is not None:
        target = (target if target.dtype == F32 else target.float()).contiguous()
    return SoftCrossEntropyFn.apply(logits, label_a, label_b, mix, float(smoothing), target)


class SoftTargetCrossEntropy(nn.Module):
    """timm.loss.SoftTargetCrossEntropy: `torch.sum(-target * F.log_softmax(x, dim=-1), dim=-1).mean()` (run_finetuning.py:593-595)"""

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return soft_cross_entropy(x, target=target)


class LabelSmoothingCrossEntropy(nn.Module):
    """timm.loss.LabelSmoothingCrossEntropy(smoothing): (1 - s) nll + s mean_c(-log_softmax) (run_finetuning.py:596-597)"""

    def __init__(self, smoothing: float = 0.1):
        super().__init__()
        assert smoothing < 1.0
        self.smoothing = smoothing
        self.confidence = 1. - smoothing

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return soft_cross_entropy(x, target, smoothing=self.smoothing)


def accuracy(output: torch.Tensor, target: torch.Tensor, topk=(1,)):
    """timm.utils.accuracy (engine_for_finetuning.py:173,225): top-k accuracies in percent, one device scalar per k.  The rank of the label
    in its row comes out of the loss kernel's pass (ties: the lower column ranks first)."""
    lg, V = _kernel_rows(output.detach())
    rank = ops.soft_ce_rows(lg, target, V=V, want_grad=False, want_rank=True)[2]
    maxk = min(max(topk), V)
    return [(rank < min(k, maxk)).float().sum() * (100.0 / output.shape[0]) for k in topk]
