"""MI355X-native mirror of InternVideo2/single_modality/models/internvideo2_cat.py ("C:"): the linear-probing classifier of
scripts/finetuning/linear_probing -- the fine-tuning trunk with a head over [cls, patch means] of the final residual stream, optionally
concatenated with the attention-pooled feature.

    InternVideo2.forward(x (B, C, T, H, W)) -> logits (B, num_classes)                           (C:542-603)

Same class / registry names (`internvideo2_cat_{small,base,large,1B,6B}_patch14_224`), constructor kwargs and state_dict keys / shapes as the
reference.  Layout notes (C:581-602): cls and the means are taken AFTER the final `x + residual`; the BatchNorm variants normalise
`final.permute(0, 2, 1)` and flatten that, so the head input is channel-major (c * G + g, G = 1 + T' or 2), while the LayerNorm variant is
group-major (g * C + c); `*_proj` appends fc_norm(clip_projector(x)).  The stream pass and the batch norm are csrc/probe.hip.
"""
from __future__ import annotations

import torch
from torch import nn

from . import functional as Fn
from .internvideo2 import InternVideo2 as _Classifier
from .internvideo2_pretrain import register_model
from .probe import BatchNormColsFn, LinearGeluFn, ProbePoolFn

MERGE_METHODS = ("proj", "cls_avg1", "cls_avgN", "cls_avg1_proj", "cls_avgN_proj")
MERGE_NORMS = ("kaiming_BN", "LN", "BN")


class _GradTimesFn(torch.autograd.Function):
    """identity whose backward multiplies by a saved factor: the GELU derivative of `down` in front of the LayerNorm variant (the
    BatchNorm variants fold it into their own backward kernel)"""

    @staticmethod
    def forward(ctx, g, u):
        ctx.save_for_backward(u)
        return g.view_as(g)

    @staticmethod
    def backward(ctx, dy):
        (u,) = ctx.saved_tensors
        return (dy.float() * u.float()).to(dy.dtype), None


class InternVideo2(_Classifier):
    """C:337-603"""

    def __init__(self, *args, merge_method: str = "proj", merge_norm: str = "kaiming_BN", **kwargs):
        if merge_method not in MERGE_METHODS:                  # C:471-473
            raise ValueError(f"Wrong method: {merge_method!r} (one of {MERGE_METHODS})")
        if merge_method != "proj" and merge_norm not in MERGE_NORMS:      # C:449-451
            raise ValueError(f"Wrong Norm: {merge_norm!r} (one of {MERGE_NORMS})")
        super().__init__(*args, **kwargs)
        self.merge_method, self.merge_norm = merge_method, merge_norm
        if merge_method == "proj":
            return
        embed_dim, clip_embed_dim = self.embed_dim, self.fc_norm.normalized_shape[0]
        num_classes = self.head.out_features
        groups = self.patch_embed.grid_size[0]                 # num_frames // tubelet_size
        init_scale = kwargs.get("init_scale", 0.001)
        del self.head
        norm_dim = embed_dim if "avg1" in merge_method else clip_embed_dim                      # C:442
        if merge_norm == "kaiming_BN":                                                           # C:443-448
            self.down_norm = nn.BatchNorm1d(norm_dim, affine=False, eps=1e-6)
        elif merge_norm == "LN":
            self.down_norm = nn.LayerNorm(norm_dim)
        else:
            self.down_norm = nn.BatchNorm1d(norm_dim)
        if "avg1" in merge_method:                                                               # C:453-470
            self.down = nn.Identity()
            width = embed_dim * 2
        else:
            self.down = nn.Sequential(nn.Linear(embed_dim, clip_embed_dim), nn.GELU())
            width = clip_embed_dim * (groups + 1)
        if merge_method.endswith("_proj"):
            width += clip_embed_dim
        self.head = nn.Linear(width, num_classes)
        for m in (self.down, self.head):
            m.apply(self._init_weights)
        self.head.weight.data.mul_(init_scale)                                                   # C:479-480
        self.head.bias.data.mul_(init_scale)

    def forward(self, x):
        """C:542-603 -> logits (B, num_classes) bf16"""
        xf, B, L = self._final_stream(x)
        if self.merge_method == "proj":
            return self._classify(self._pooled_features(xf, B, L))
        T = x.shape[2] // self.patch_embed.tubelet_size
        S = (L - 1) // T
        avg1 = "avg1" in self.merge_method
        with_proj = self.merge_method.endswith("_proj")
        tok, token_mean = ProbePoolFn.apply(xf, B, T, S, avg1, with_proj)                        # C:583-587: fp32 (B, G, C) [+ the pool's query mean]
        u = None
        if not avg1:
            tok, u = LinearGeluFn.apply(tok, self.down[0].weight, self.down[0].bias)             # C:588: bf16 (B, 1 + T, clip_embed_dim)
        dn = self.down_norm
        if "BN" in self.merge_norm:                                                              # C:589-590: channel-major
            final = BatchNormColsFn.apply(tok, dn.weight, dn.bias, dn, self.training, u)
        else:                                                                                    # C:592: group-major
            if u is not None:
                tok = _GradTimesFn.apply(tok, u)
            final = Fn.LayerNormFn.apply(tok, dn.weight, dn.bias, dn.eps)
            final = (final if final.dtype == torch.bfloat16 else final.to(torch.bfloat16)).reshape(B, -1)
        if with_proj:                                                                            # C:601-602
            final = torch.cat([final, self._pooled_features(xf, B, L, token_mean)], dim=1)
        return self._classify(final)


def _cat(embed_dim, depth, num_heads, mlp_ratio, **kwargs):
    return InternVideo2(img_size=224, patch_size=14, embed_dim=embed_dim, depth=depth, num_heads=num_heads, mlp_ratio=mlp_ratio,
                        attn_pool_num_heads=16, clip_embed_dim=768, **kwargs)


@register_model
def internvideo2_cat_small_patch14_224(pretrained=False, **kwargs):
    """C:606-614"""
    return _cat(384, 12, 6, 4, **kwargs)


@register_model
def internvideo2_cat_base_patch14_224(pretrained=False, **kwargs):
    """C:617-625"""
    return _cat(768, 12, 12, 4, **kwargs)


@register_model
def internvideo2_cat_large_patch14_224(pretrained=False, **kwargs):
    """C:628-636"""
    return _cat(1024, 24, 16, 4, **kwargs)


@register_model
def internvideo2_cat_1B_patch14_224(pretrained=False, **kwargs):
    """C:639-647"""
    return _cat(1408, 40, 16, 48 / 11, **kwargs)


@register_model
def internvideo2_cat_6B_patch14_224(pretrained=False, **kwargs):
    """C:650-658"""
    return _cat(3200, 48, 25, 4, **kwargs)
