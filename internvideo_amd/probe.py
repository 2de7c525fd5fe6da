"""Linear / attentive probing (InternVideo2/single_modality/run_linear_probing.py, scripts/finetuning/{linear,attentive}_probing): the
freezing loop of the recipe and the autograd seams of the probing heads (csrc/probe.hip).

    from internvideo_amd import internvideo2_cat, internvideo2_ap          # registers internvideo2_{cat,ap}_*_patch14_224
    from internvideo_amd.probe import freeze_for_probing
    model = create_model("internvideo2_cat_1B_patch14_224", merge_method="cls_avgN", merge_norm="kaiming_BN", num_frames=16, ...)
    freeze_for_probing(model, open_block_num=0)                            # run_linear_probing.py:556-581

A frozen trunk runs forward-only (`InternVideo2._final_stream`): BlockStackFn saves ~42 bytes per token and channel per block whether or not
anything needs a gradient, the forward-only loop saves nothing.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import functional as Fn
from . import ops

BF16, F32 = torch.bfloat16, torch.float32


def freeze_for_probing(model, open_block_num: int = 0, open_clip_projector: bool = False, depth: Optional[int] = None):
    """run_linear_probing.py:556-581 by parameter name: `patch_embed*`, `pos_embed*`, `cls_token` frozen; every block frozen except the last
    `open_block_num`; `clip_projector*` frozen unless `open_clip_projector`; everything else (fc_norm, head, down, down_norm, extra_mlp) stays
    trainable.  Sets `model.frozen_prefix = depth - open_block_num`, which the classifiers honour by running those blocks forward-only.
    -> (frozen names, trainable names).

    Two differences from the reference loop: `depth` defaults to `len(model.blocks)` where the reference hard-codes 40 (48 for "6B" model
    names), so that the smaller registry entries open their LAST blocks too; and a block is matched by its index, where the reference's
    `name.startswith(f"blocks.{num}")` would also open blocks 30-39 when block 3 is opened (open_block_num >= 37)."""
    depth = len(model.blocks) if depth is None else int(depth)
    open_block_num = int(open_block_num)
    if not 0 <= open_block_num <= depth:
        raise ValueError(f"open_block_num={open_block_num} outside 0..{depth}")
    opened = {depth - i - 1 for i in range(open_block_num)}
    frozen, trainable = [], []
    for name, p in model.named_parameters():
        if name.startswith("patch_embed") or name.startswith("pos_embed") or name.startswith("cls_token"):
            freeze = True
        elif name.startswith("blocks"):
            freeze = int(name.split(".")[1]) not in opened
        elif name.startswith("clip_projector") and not open_clip_projector:
            freeze = True
        else:
            freeze = False
        if freeze:
            p.requires_grad = False
            frozen.append(name)
        else:
            trainable.append(name)
    model.frozen_prefix = max(min(depth - open_block_num, len(model.blocks)), 0)
    return frozen, trainable


class ProbePoolFn(torch.autograd.Function):
    """cls row + per-frame (avgN) or all-patch (avg1) means of the final stream (internvideo2_cat.py:583-587) -> (fp32 (B, G, C), the
    all-token mean fp32 (B, C) when `want_token_mean` -- the query AttentionPoolingBlock builds, from the same pass -- else None)"""

    @staticmethod
    def forward(ctx, x, B, T, S, avg1, want_token_mean):
        out, tok = ops.cat_pool_fwd(x.contiguous(), B, T, S, avg1=avg1, want_token_mean=want_token_mean)
        ctx.meta = (B, T, S, bool(avg1), x.dtype)
        return out, tok

    @staticmethod
    def backward(ctx, dout, dtok):
        B, T, S, avg1, xdtype = ctx.meta
        dout = dout.contiguous().float() if dout is not None else None
        dtok = dtok.contiguous().float() if dtok is not None else None
        dx = ops.cat_pool_bwd(dout, dtok, B, T, S, avg1=avg1)
        return (dx if xdtype == F32 else dx.to(xdtype)), None, None, None, None, None


class BatchNormColsFn(torch.autograd.Function):
    """`bn(x.permute(0, 2, 1)).reshape(B, -1)` for bn = BatchNorm1d(C) on x (B, G, C) (internvideo2_cat.py:589-590) -> bf16 (B, C * G),
    channel-major.  In training mode the module's running buffers and `num_batches_tracked` are updated by the kernel, on the device.
    dact (bf16 (B, G, C), optional): multiplied into dx -- the GELU derivative that the `down` projection's GEMM stored."""

    @staticmethod
    def forward(ctx, x, w, b, bn, training, dact):
        x = x.contiguous()
        if x.dtype not in (F32, BF16):
            x = x.float()
        y, mean, rstd = ops.batchnorm_cols_fwd(x, Fn.vec(w) if w is not None else None, Fn.vec(b) if b is not None else None, bn.eps,
                                               training or bn.running_mean is None,
                                               momentum=(0.1 if bn.momentum is None else bn.momentum), running_mean=bn.running_mean,
                                               running_var=bn.running_var, num_batches_tracked=bn.num_batches_tracked)
        ctx.save_for_backward(x, mean, rstd, dact)
        ctx.p, ctx.training = (w, b), bool(training or bn.running_mean is None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, dact = ctx.saved_tensors
        w, b = ctx.p
        dy = dy if dy.dtype == BF16 else dy.to(BF16)
        if dy.stride(-1) != 1:
            dy = dy.contiguous()
        affine = w is not None and (Fn._wants_grad(ctx, 1, w) or Fn._wants_grad(ctx, 2, b))
        dx, dw, db = ops.batchnorm_cols_bwd(x, Fn.vec(w) if w is not None else None, mean, rstd, dy, training=ctx.training, dact=dact,
                                            dx_dtype=x.dtype, want_affine_grads=affine, dw_out=Fn._mg(w), db_out=Fn._mg(b))
        if not ctx.needs_input_grad[0]:
            dx = None
        return dx, (Fn._ret_grad(w, dw) if affine else None), (Fn._ret_grad(b, db) if affine else None), None, None, None


class LinearGeluFn(torch.autograd.Function):
    """gelu(x W^T + b) (the `down` projection, internvideo2_cat.py:457-460) -> (g bf16, gelu'(pre-activation) bf16): the GEMM's epilogue
    stores the derivative, the consumer's backward (BatchNormColsFn `dact`) multiplies it in, so this backward receives d(pre-activation)."""

    @staticmethod
    def forward(ctx, x, w, b):
        x2 = x.reshape(-1, x.shape[-1])
        x2 = (x2 if x2.dtype == BF16 else x2.to(BF16)).contiguous()
        g, u = ops.gemm(x2, Fn.mat(w), bias=Fn.vec(b), act="gelu_erf_d", want_preact=True)
        ctx.save_for_backward(x2)
        ctx.p, ctx.xshape, ctx.xdtype = (w, b), x.shape, x.dtype
        ctx.mark_non_differentiable(u)
        return g.reshape(*x.shape[:-1], w.shape[0]), u.reshape(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, du, _):
        (x2,) = ctx.saved_tensors
        w, b = ctx.p
        du2 = du.reshape(-1, du.shape[-1])
        du2 = (du2 if du2.dtype == BF16 else du2.to(BF16)).contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.gemm(du2, Fn.mat(w), a_kc=True, b_kc=False).reshape(ctx.xshape).to(ctx.xdtype)
        db = Fn._ret_grad(b, ops.colsum_bf16(du2)) if Fn._wants_grad(ctx, 2, b) else None
        dw = None
        if Fn._wants_grad(ctx, 1, w):
            if du2.shape[0] % 8:                         # B * G rows: the transposing GEMM reads 8-row groups -> zero-pad a ragged count
                pad = 8 - du2.shape[0] % 8
                du2, x2 = torch.nn.functional.pad(du2, (0, 0, 0, pad)), torch.nn.functional.pad(x2, (0, 0, 0, pad))
            dw = Fn._wgrad_defer(du2, x2, w)
        return dx, dw, db
