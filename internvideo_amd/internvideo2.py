"""MI355X-native mirror of InternVideo2/single_modality/models/internvideo2.py ("F:"): the fine-tuning / inference classifier
 -- the student trunk at FULL sequence length (no mask: L = 1 + T*H*W = 2049 tokens for 8 x 224^2, the
regime where the attention kernels dominate), the attention-pool projector, `fc_norm` and the classification `head`.

    InternVideo2.forward(x (B, C, T, H, W)) -> logits (B, num_classes)                           (F:500-543)

Same class / registry names (`internvideo2_{small,base,large,1B,6B}_patch14_224`), constructor kwargs and state_dict keys / shapes
as the reference, so fine-tuning checkpoints load with strict=True and `run_finetuning.py` + `optim_factory.py` (layer-wise lr decay
reads `get_num_layers()` and the parameter names) run unchanged.  Forward and backward run in the same gfx950 kernels as pre-training.
"""
from __future__ import annotations

from functools import partial

import torch
import torch.nn.functional as F
from torch import nn

from . import functional as Fn
from .internvideo2_pretrain import AttentionPoolingBlock, Block, PatchEmbed, PretrainInternVideo2, RMSNorm, _residual_is_bf16, _trunc_normal_, register_model


class PaddedHeadFn(torch.autograd.Function):
    """y = x W^T + b for a head whose width n is not a multiple of 8: the GEMM runs on W / b zero-padded to the next multiple (as
    xbert.LinearCrossEntropyFn does) and the result is the `[:, :n]` view of the padded logits, whose row pitch the loss kernels accept as
    it is.  The padding happens INSIDE the function, so the gradients are delivered to the head's own parameters (`_ret_grad`: into the
    training engine's buffers, overwriting like every other matrix gradient) instead of arriving through autograd's pad backward."""

    @staticmethod
    def forward(ctx, x, w, b):
        x2 = x.reshape(-1, x.shape[-1])
        x2 = (x2 if x2.dtype == torch.bfloat16 else x2.to(torch.bfloat16)).contiguous()
        n = w.shape[0]
        pad = 8 - n % 8
        W, bias = F.pad(Fn.mat(w), (0, 0, 0, pad)), F.pad(Fn.vec(b), (0, pad))
        y = Fn.ops.gemm(x2, W, bias=bias)
        ctx.save_for_backward(x2, W)
        ctx.p, ctx.n, ctx.xshape, ctx.xdtype = (w, b), n, x.shape, x.dtype
        return y.reshape(*x.shape[:-1], n + pad)[..., :n]

    @staticmethod
    def backward(ctx, dy):
        x2, W = ctx.saved_tensors
        w, b = ctx.p
        n = ctx.n
        dl = x2.new_zeros((x2.shape[0], W.shape[0]))
        dl[:, :n].copy_(dy.reshape(-1, n))
        dx = Fn.ops.gemm(dl, W, a_kc=True, b_kc=False).reshape(ctx.xshape).to(ctx.xdtype) if ctx.needs_input_grad[0] else None
        M = dl.shape[0]
        dlp, xp = (dl, x2) if M % 8 == 0 else (F.pad(dl, (0, 0, 0, 8 - M % 8)), F.pad(x2, (0, 0, 0, 8 - M % 8)))   # the transposing GEMM reads 8-row groups
        dW = Fn._ret_grad(w, Fn.ops.gemm(dlp, xp, a_kc=False, b_kc=False)[:n])
        db = Fn._ret_grad(b, Fn.ops.colsum_bf16(dl)[:n])
        return dx, dW, db


class InternVideo2(PretrainInternVideo2):
    """F:337-543.  Inherits the token / block machinery of the pre-training student (forward_features with mask=None)."""

    def __init__(
            self, in_chans: int = 3, patch_size: int = 14, img_size: int = 224, qkv_bias: bool = False,
            drop_path_rate: float = 0.25, embed_dim: int = 1408, head_drop_path_rate: float = 0., num_heads: int = 16,
            mlp_ratio: float = 4.3637, init_values: float = 1e-5, qk_normalization: bool = True, depth: int = 40,
            use_flash_attn: bool = True, use_fused_rmsnorm: bool = True, use_fused_mlp: bool = True,
            fused_mlp_heuristic: int = 1, attn_pool_num_heads: int = 16, clip_embed_dim: int = 768,
            layerscale_no_force_fp32: bool = False, num_frames: int = 8, tubelet_size: int = 1,
            sep_pos_embed: bool = False, use_checkpoint: bool = False, checkpoint_num: int = 0,
            fc_drop_rate: float = 0., num_classes: int = 1000, init_scale: float = 0.001, fused_mlp_act: str = "erf",
    ):
        nn.Module.__init__(self)
        assert use_flash_attn == use_fused_rmsnorm == use_fused_mlp, \
            'use_flash_attn, use_fused_rmsnorm and use_fused_mlp should be consistent'
        self.use_flash_attn = use_flash_attn
        self.embed_dim, self.depth, self.num_heads = embed_dim, depth, num_heads
        self.fused_mlp_act = {"erf": "gelu_erf", "tanh": "gelu_tanh"}[fused_mlp_act]
        self.clip_return_index, self.mae_return_index = [], []
        self.norm_layer_for_blocks = partial(RMSNorm, eps=1e-6)
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim, num_frames=num_frames, tubelet_size=tubelet_size)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.sep_pos_embed = bool(sep_pos_embed)
        if self.sep_pos_embed:                                 # F:390-397: spatial + temporal + cls tables, joined on the fly in forward (F:510-525)
            grid = self.patch_embed.grid_size
            self.grid_size = grid
            self.pos_embed_spatial = nn.Parameter(torch.zeros(1, grid[1] * grid[2], embed_dim))
            self.pos_embed_temporal = nn.Parameter(torch.zeros(1, grid[0], embed_dim))
            self.pos_embed_cls = nn.Parameter(torch.zeros(1, 1, embed_dim))
        else:
            self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches + 1, embed_dim))
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth, device="cpu")]
        self.drop_path_rates = dpr
        with_cp_list = [use_checkpoint and idx < checkpoint_num for idx in range(depth)]
        self.blocks = nn.ModuleList([
            Block(embed_dim, num_heads, mlp_ratio, qkv_bias=qkv_bias, drop_path=dpr[i], init_values=init_values, attn_drop=0.,
                  use_flash_attn=use_flash_attn, use_fused_mlp=use_fused_mlp, fused_mlp_heuristic=fused_mlp_heuristic,
                  with_cp=with_cp_list[i], qk_normalization=qk_normalization,
                  layerscale_no_force_fp32=layerscale_no_force_fp32, use_fused_rmsnorm=use_fused_rmsnorm)
            for i in range(depth)])
        self.clip_projector = AttentionPoolingBlock(dim=embed_dim, num_heads=attn_pool_num_heads, qkv_bias=True,
                                                    norm_layer=partial(nn.LayerNorm, eps=1e-5), out_dim=clip_embed_dim)
        self.fc_norm = nn.LayerNorm(clip_embed_dim)
        self.fc_dropout = nn.Dropout(p=fc_drop_rate) if fc_drop_rate > 0 else nn.Identity()
        self.head = nn.Linear(clip_embed_dim, num_classes)
        self.init_pos_embed()
        _trunc_normal_(self.cls_token, std=.02)
        self.apply(self._init_weights)
        self.fix_init_weight()
        self.head.weight.data.mul_(init_scale)                                                   # F:449-450
        self.head.bias.data.mul_(init_scale)
        self.grad_ready_hook = None

    def init_pos_embed(self):                                                                    # F:452-475
        from .pos_embed import get_1d_sincos_pos_embed, get_2d_sincos_pos_embed, get_3d_sincos_pos_embed
        if self.sep_pos_embed:                                 # F:454-465 (the cls table stays zero)
            D = self.pos_embed_spatial.shape[-1]
            self.pos_embed_spatial.data.copy_(torch.from_numpy(get_2d_sincos_pos_embed(D, self.patch_embed.grid_size[1])).float().unsqueeze(0))
            self.pos_embed_temporal.data.copy_(torch.from_numpy(get_1d_sincos_pos_embed(D, self.patch_embed.grid_size[0])).float().unsqueeze(0))
            return
        pe = get_3d_sincos_pos_embed(self.pos_embed.shape[-1], self.patch_embed.grid_size[1], self.patch_embed.grid_size[0], cls_token=True)
        self.pos_embed.data.copy_(torch.from_numpy(pe).float().unsqueeze(0))

    @torch.jit.ignore
    def no_weight_decay(self):                                                                   # F:490-498
        return {'pos_embed', 'pos_embed_spatial', 'pos_embed_temporal', 'pos_embed_cls', 'cls_token'}

    def _frozen_prefix(self, x) -> int:
        """how many leading blocks run forward-only (probe.freeze_for_probing sets `frozen_prefix`): 0 without the attribute; every block
        when no gradient is recorded; else the attribute's n, provided the prefix really is frozen -- every parameter of blocks < n and of
        the embedding (patch embed, cls token, positional tables) has requires_grad False and the clip itself needs no gradient.  The
        forward-only loop is the fp32-stream bf16 one: a model with fp8 GEMMs or a bf16 residual stream keeps the autograd stack."""
        n = int(getattr(self, "frozen_prefix", 0) or 0)
        if n <= 0 or getattr(self, "fp8_gemm", False) or _residual_is_bf16(getattr(self, "residual_dtype", "fp32")):
            return 0
        if not torch.is_grad_enabled():
            return self.depth
        n = min(n, self.depth)
        if x.requires_grad:
            return 0
        embed = [p for name, p in self.named_parameters(recurse=False) if name == "cls_token" or name.startswith("pos_embed")]
        embed += list(self.patch_embed.parameters())
        for blk in self.blocks[:n]:
            embed += list(blk.parameters())
        return 0 if any(p.requires_grad for p in embed) else n

    def _final_stream(self, x):
        """-> (the residual stream after the last block and the final `x + residual` (F:527-536), fp32 [B*L, D]; B; L).  With a frozen
        prefix of n blocks (`_frozen_prefix`) the patch embed and blocks 0 .. n-1 run through the forward-only loop (nothing is saved) and
        blocks n .. depth-1 through BlockStackFn, which starts from the prefix's last tap: the same residual-stream value, since the
        first block of a stack reads `res = x0, branch = None`.  DropPath draws are taken for the whole depth either way."""
        n = self._frozen_prefix(x)
        if n == 0:
            taps, _, _, B, L = self.forward_features(x, None)
            return taps[self.depth - 1], B, L
        if not x.is_cuda:
            raise Fn.ops.InternVideoHipError("InternVideo2.forward needs HBM-resident inputs: there is no CPU path")
        if x.dim() != 5:
            raise ValueError(f"expected a (B, C, T, H, W) clip tensor, got {tuple(x.shape)}")
        pe = self.patch_embed
        x0, B, L = Fn.embed_all_tokens(x, pe.proj.weight, pe.proj.bias, self.cls_token, self._pos_table("").detach(), pe.tubelet_size, pe.patch_size[0])
        rs = self._drop_path_scales(B, x.device)
        outs = Fn.block_stack_infer(x0, [blk.flat_params() for blk in self.blocks[:n]], B, L, self.num_heads, 1e-6, self.fused_mlp_act, (),
                                    rowscale=(rs[:n] if rs is not None else None))
        xn = outs[n - 1]
        if n == self.depth:
            return xn, B, L
        n_cp = 0
        for blk in self.blocks[n:]:
            if not getattr(blk, "with_cp", False):
                break
            n_cp += 1
        hook = self.grad_ready_hook                      # the engine counts blocks from the bottom of the model, the suffix stack from its own
        meta = dict(B=B, L=L, H=self.num_heads, eps=1e-6, act=self.fused_mlp_act, taps=[self.depth - 1 - n],
                    grad_ready_hook=(None if hook is None else (lambda i, _h=hook, _n=n: _h(i + _n))), checkpoint_num=n_cp, fp8=False,
                    fp8_hist=None, fp8_wchan=False, res_bf16=False, taps_bf16=False,
                    dp_skip=getattr(self, "drop_path_skip", "auto"), dp_count_acc=None)
        params = [p for blk in self.blocks[n:] for p in blk.flat_params()]
        (final,) = Fn.BlockStackFn.apply(xn, rs[n:].contiguous() if rs is not None else None, meta, *params)
        return final, B, L

    def _pooled_features(self, xf, B, L, token_mean=None):
        """fc_norm(clip_projector(x)) (F:538-539) -> bf16 (B, clip_embed_dim); token_mean: see AttentionPoolingBlock.forward"""
        pooled = self.clip_projector(xf, B, L, token_mean)                                       # F:538
        return Fn.LayerNormFn.apply(pooled, self.fc_norm.weight, self.fc_norm.bias, self.fc_norm.eps)   # F:539

    def _classify(self, h):
        """head(fc_dropout(h)) (F:540-541)"""
        h = self.fc_dropout(h)                                                                   # F:540 (a (B, 768) tensor)
        w, b = self.head.weight, self.head.bias
        n = w.shape[0]
        if n % 8:                                          # class counts like 174 / 339: the GEMM moves 8-column chunks -> zero-pad
            return PaddedHeadFn.apply(h, w, b)
        return Fn.LinearFn.apply(h, w, b)[:, :n]

    def forward(self, x):
        """F:500-543 -> logits (B, num_classes) bf16"""
        xf, B, L = self._final_stream(x)
        return self._classify(self._pooled_features(xf, B, L))

    def forward_loss(self, x, target, target_b=None, mix=None, smoothing: float = 0.0):
        """the fine-tuning step's loss (engines/engine_for_finetuning.py:13-17 with the criterion of run_finetuning.py:593-599) in one
        row kernel: x (B, C, T, H, W), target / target_b integer labels (B,), mix fp32 (B, 2) = (lam, oml) per row -- what
        finetune.Mixup.apply returns; target alone: (label-smoothed) cross entropy -> (loss, logits.detach())"""
        from .finetune import soft_cross_entropy
        logits = self.forward(x)
        return soft_cross_entropy(logits, target, target_b, mix, smoothing), logits.detach()


def _ft(embed_dim, depth, num_heads, mlp_ratio, **kwargs):
    return InternVideo2(img_size=224, patch_size=14, embed_dim=embed_dim, depth=depth, num_heads=num_heads, mlp_ratio=mlp_ratio,
                        attn_pool_num_heads=16, clip_embed_dim=768, **kwargs)


@register_model
def internvideo2_small_patch14_224(pretrained=False, **kwargs):
    """F:546-554"""
    return _ft(384, 12, 6, 4, **kwargs)


@register_model
def internvideo2_base_patch14_224(pretrained=False, **kwargs):
    """F:557-565"""
    return _ft(768, 12, 12, 4, **kwargs)


@register_model
def internvideo2_large_patch14_224(pretrained=False, **kwargs):
    """F:568-576"""
    return _ft(1024, 24, 16, 4, **kwargs)


@register_model
def internvideo2_1B_patch14_224(pretrained=False, **kwargs):
    """F:579-587"""
    return _ft(1408, 40, 16, 48 / 11, **kwargs)


@register_model
def internvideo2_6B_patch14_224(pretrained=False, **kwargs):
    """F:590-598"""
    return _ft(3200, 48, 25, 4, **kwargs)
