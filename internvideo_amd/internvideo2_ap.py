"""MI355X-native mirror of InternVideo2/single_modality/models/internvideo2_ap.py ("A:"): the attentive-probing classifier of
scripts/finetuning/attentive_probing -- the fine-tuning classifier with a zero-initialised residual MLP (as in VideoGLUE) between the
attention-pooling projector and `fc_norm`.

    InternVideo2.forward(x (B, C, T, H, W)) -> logits (B, num_classes)                           (A:513-558)

Same class / registry names (`internvideo2_ap_{small,base,large,1B,6B}_patch14_224`), constructor kwargs and state_dict keys / shapes as the
reference.  The existing kernels suffice: LayerNormFn and the fused MLP.
"""
from __future__ import annotations

from torch import nn

from . import functional as Fn
from .internvideo2 import InternVideo2 as _Classifier
from .internvideo2_pretrain import Mlp, register_model


class InternVideo2(_Classifier):
    """A:330-558"""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        clip_embed_dim = self.fc_norm.normalized_shape[0]
        tail = {n: self._modules.pop(n) for n in ("fc_norm", "fc_dropout", "head")}            # keep the reference's module order
        self.extra_mlp = nn.Sequential(nn.LayerNorm(clip_embed_dim),                             # A:429-436
                                       Mlp(in_features=clip_embed_dim, hidden_features=int(clip_embed_dim * 4.0)))
        for n, m in tail.items():
            self.add_module(n, m)
        self.extra_mlp.apply(self._init_weights)
        nn.init.constant_(self.extra_mlp[1].fc2.weight, 0.)                                      # A:449-451
        nn.init.constant_(self.extra_mlp[1].fc2.bias, 0.)

    def _pooled_features(self, xf, B, L, token_mean=None):
        """fc_norm(p + extra_mlp(p)), p = clip_projector(x) (A:552-556); the sum is taken in fp32"""
        pooled = self.clip_projector(xf, B, L, token_mean)
        ln, mlp = self.extra_mlp[0], self.extra_mlp[1]
        h = Fn.LayerNormFn.apply(pooled, ln.weight, ln.bias, ln.eps)
        h = Fn.MlpFn.apply(h, mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias, "gelu_erf")
        return Fn.LayerNormFn.apply(pooled.float() + h.float(), self.fc_norm.weight, self.fc_norm.bias, self.fc_norm.eps)


def _ap(embed_dim, depth, num_heads, mlp_ratio, **kwargs):
    return InternVideo2(img_size=224, patch_size=14, embed_dim=embed_dim, depth=depth, num_heads=num_heads, mlp_ratio=mlp_ratio,
                        attn_pool_num_heads=16, clip_embed_dim=768, **kwargs)


@register_model
def internvideo2_ap_small_patch14_224(pretrained=False, **kwargs):
    """A:561-569"""
    return _ap(384, 12, 6, 4, **kwargs)


@register_model
def internvideo2_ap_base_patch14_224(pretrained=False, **kwargs):
    """A:572-580"""
    return _ap(768, 12, 12, 4, **kwargs)


@register_model
def internvideo2_ap_large_patch14_224(pretrained=False, **kwargs):
    """A:583-591"""
    return _ap(1024, 24, 16, 4, **kwargs)


@register_model
def internvideo2_ap_1B_patch14_224(pretrained=False, **kwargs):
    """A:594-602"""
    return _ap(1408, 40, 16, 48 / 11, **kwargs)


@register_model
def internvideo2_ap_6B_patch14_224(pretrained=False, **kwargs):
    """A:605-613"""
    return _ap(3200, 48, 25, 4, **kwargs)
