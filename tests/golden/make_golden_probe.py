"""Golden fixture for the probing classifiers: the reference's own models/internvideo2_cat.py ("C:") and models/internvideo2_ap.py ("A:")
under the freezing loop of run_linear_probing.py:556-581.

    python tests/golden/make_golden_probe.py          (authoring container only: needs the reference tree)

RUNS THE REFERENCE'S OWN MODULES on CPU (unfused fp32 path, tests/golden/ref_loader.py) at `tiny88` (D = 176, depth 3, T = 4, S = 16, L = 65),
B = 4, 10 classes, on the deterministic synthetic parameters / clips of oracle.internvideo2_oracle.  Parameters the oracle has no generator
for (`down.*`, `down_norm.*`, `head.*` of the concatenating heads, `extra_mlp.*` with a NON-zero fc2) are seeded here and stored as inputs
(`<case>:in:<name>`).  Per case and open_block_num in {0, 1} (`<case>:o<k>:`): train-mode logits and cross-entropy loss, the gradient of every
trainable parameter outside the blocks (matrices above 4200 elements: norm and 16 x 16 corner) and of a few parameters of the last block when it is open, the BatchNorm buffers after the step, the
eval-mode logits after it, and `bf16err:*`: the reference's own `.bfloat16()` run against its fp32 run (the calibration of the GPU bars).
-> tests/golden/probe.npz, and tests/golden/probe.json: state_dict key / shape lists of every merge_method x merge_norm and of the ap model,
and the frozen / trainable name lists of the freezing loop for (open_block_num, open_clip_projector) in {(0, F), (0, T), (2, T)}."""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_loader  # noqa: E402
from oracle import internvideo2_oracle as O  # noqa: E402

NUM_CLASSES, BATCH = 10, 4
LABELS = [3, 7, 1, 9]
# (case tag, model file, merge_method, merge_norm, open_clip_projector)
CASES = [("cls_avgN_kBN", "cat", "cls_avgN", "kaiming_BN", False),
         ("cls_avg1_kBN", "cat", "cls_avg1", "kaiming_BN", False),
         ("cls_avg1_proj_LN", "cat", "cls_avg1_proj", "LN", False),
         ("cls_avgN_proj_BN", "cat", "cls_avgN_proj", "BN", False),
         ("ap", "ap", None, None, False),
         ("proj_open", "cat", "proj", "kaiming_BN", True)]
LAST_BLOCK = ["norm1.weight", "attn.qkv.weight", "attn.proj.bias", "ls1.gamma", "mlp.fc1.weight", "mlp.fc2.bias", "ls2.gamma"]
METHODS = ["proj", "cls_avg1", "cls_avgN", "cls_avg1_proj", "cls_avgN_proj"]
NORMS = ["kaiming_BN", "LN", "BN"]
FREEZE_SETTINGS = [(0, False), (0, True), (2, True)]
FULL_GRAD_MAX = 4200                                      # gradients with more elements are stored as norm + corner (fixture size)


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def load_module(kind):
    ref_loader.load_sm_pretrain()
    name = {"cat": "internvideo2_cat", "ap": "internvideo2_ap"}[kind]
    return ref_loader._load("_iv_ref_sm_models", name, os.path.join(ref_loader.SM_MODELS, name + ".py"))


def build(cfg, kind, method=None, norm=None):
    mod = load_module(kind)
    extra = {} if kind == "ap" else dict(merge_method=method, merge_norm=norm)
    with contextlib.redirect_stdout(io.StringIO()):
        return mod.InternVideo2(
            in_chans=cfg.in_chans, patch_size=cfg.patch_size, img_size=cfg.img_size, qkv_bias=False, drop_path_rate=0.0,
            embed_dim=cfg.embed_dim, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, init_values=1e-5, qk_normalization=True,
            depth=cfg.depth, use_flash_attn=False, use_fused_rmsnorm=False, use_fused_mlp=False,
            attn_pool_num_heads=cfg.attn_pool_num_heads, clip_embed_dim=cfg.clip_embed_dim, num_frames=cfg.num_frames,
            tubelet_size=cfg.tubelet_size, sep_pos_embed=False, num_classes=NUM_CLASSES, **extra)


def freeze(model, depth, open_block_num, open_clip_projector):
    """what run_linear_probing.py:556-581 does to requires_grad, with the model's own depth in place of the hard-coded 40 / 48
    -> (frozen names, trainable names)"""
    opened = [depth - i - 1 for i in range(open_block_num)]
    frozen, trainable = [], []
    for name, p in model.named_parameters():
        if name.startswith("patch_embed") or name.startswith("pos_embed") or name.startswith("cls_token"):
            hold = True
        elif name.startswith("blocks"):
            hold = not any(name.startswith(f"blocks.{n}") for n in opened)
        elif name.startswith("clip_projector") and not open_clip_projector:
            hold = True
        else:
            hold = False
        p.requires_grad = not hold
        (frozen if hold else trainable).append(name)
    return frozen, trainable


def seeded_inputs(model, params, seed):
    """a full state dict: the oracle's synthetic values where it has them (and the shapes agree), seeded values for the rest of the
    floating-point entries (norm weights around 1, everything else N(0, 0.05)), the module's own defaults for the BatchNorm buffers
    -> (state dict, the seeded entries)"""
    sd = model.state_dict()
    rng = np.random.Generator(np.random.PCG64(seed))
    load, extra = {}, {}
    for k, v in sd.items():
        if k in params and tuple(params[k].shape) == tuple(v.shape):
            load[k] = params[k]
        elif k.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked"):
            load[k] = v.clone()
        else:
            a = rng.standard_normal(tuple(v.shape)).astype(np.float32)
            is_norm_w = k.endswith("weight") and v.dim() == 1
            t = torch.from_numpy((1.0 + 0.1 * a) if is_norm_w else 0.05 * a)
            load[k] = t
            extra[k] = t
    return load, extra


def run(cfg, kind, method, norm, load, k, open_proj, dtype, video, labels):
    m = build(cfg, kind, method, norm)
    m.load_state_dict(load, strict=True)
    m = m.to(dtype).train()
    frozen, trainable = freeze(m, cfg.depth, k, open_proj)
    logits = m(video.to(dtype))
    loss = torch.nn.functional.cross_entropy(logits.float(), labels)
    loss.backward()
    named = dict(m.named_parameters())
    # (cls_avg1 / cls_avgN never use fc_norm(clip_projector(x)), C:599-600: those trainable parameters receive no gradient)
    grads = {n: named[n].grad.detach().float().numpy().copy() for n in trainable if not n.startswith("blocks.") and named[n].grad is not None}
    if k:
        for n in LAST_BLOCK:
            grads[f"blocks.{cfg.depth - 1}.{n}"] = named[f"blocks.{cfg.depth - 1}.{n}"].grad.detach().float().numpy().copy()
    assert all(named[n].grad is None for n in frozen)
    bufs = {n: b.detach().clone().double().numpy() for n, b in m.named_buffers() if n.startswith("down_norm.")}
    m.eval()
    with torch.no_grad():
        ev = m(video.to(dtype)).float().numpy()
    return logits.detach().float().numpy(), float(loss.item()), grads, bufs, ev


def main():
    assert ref_loader.available(), "needs the reference tree (IV_REFERENCE_ROOT)"
    cfg = O.named_config("tiny88")
    d = {}
    labels = torch.tensor(LABELS)
    for ci, (tag, kind, method, norm, open_proj) in enumerate(CASES):
        params = O.synthetic_finetune_params(cfg, NUM_CLASSES, seed=40 + ci)
        video, _, _ = O.synthetic_batch(cfg, BATCH, 5, seed=40 + ci)
        load, extra = seeded_inputs(build(cfg, kind, method, norm), params, 900 + ci)
        for n, t in extra.items():
            d[f"{tag}:in:{n}"] = t.numpy().copy()
        for k in (0, 1):
            pre = f"{tag}:o{k}:"
            lg, loss, grads, bufs, ev = run(cfg, kind, method, norm, load, k, open_proj, torch.float32, video, labels)
            lgb, lossb, gradsb, _, evb = run(cfg, kind, method, norm, load, k, open_proj, torch.bfloat16, video, labels)
            d[pre + "logits"], d[pre + "loss"], d[pre + "eval_logits"] = lg, np.array([loss]), ev
            for n, g in grads.items():
                if g.size <= FULL_GRAD_MAX:
                    d[pre + "grad:" + n] = g
                    d[pre + "bf16err:" + n] = np.array([_rel(gradsb[n], g)])
                    continue
                # a large matrix: its norm and its leading 16 x 16 corner (the `gradnorm:` / `gradcorner:` form of the other fixtures)
                g2, gb2 = g.reshape(-1, g.shape[-1]), gradsb[n].reshape(-1, g.shape[-1])
                d[pre + "gradnorm:" + n] = np.array([float(np.linalg.norm(g.astype(np.float64)))])
                d[pre + "gradcorner:" + n] = g2[:16, :16].copy()
                d[pre + "bf16err:corner:" + n] = np.array([_rel(gb2[:16, :16], g2[:16, :16])])
                d[pre + "bf16err:norm:" + n] = np.array([abs(float(np.linalg.norm(gradsb[n].astype(np.float64))) - d[pre + "gradnorm:" + n][0])
                                                         / d[pre + "gradnorm:" + n][0]])
            for n, b in bufs.items():
                d[pre + "buf:" + n] = b
            d[pre + "bf16err:logits"] = np.array([_rel(lgb, lg)])
            d[pre + "bf16err:loss"] = np.array([abs(lossb - loss) / abs(loss)])
            d[pre + "bf16err:eval_logits"] = np.array([_rel(evb, ev)])
            print(f"{pre:24s} loss {loss:.6f}  {len(grads)} grads  bf16-vs-fp32: logits {d[pre + 'bf16err:logits'][0]:.3g} "
                  f"eval {d[pre + 'bf16err:eval_logits'][0]:.3g} loss {d[pre + 'bf16err:loss'][0]:.3g}")
        d[f"{tag}:bf16err:logits"] = np.maximum(d[f"{tag}:o0:bf16err:logits"], d[f"{tag}:o1:bf16err:logits"])
    path = os.path.join(HERE, "probe.npz")
    np.savez_compressed(path, **d)
    print(f"wrote {path}: {len(d)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")

    meta = {"config": "tiny88", "num_classes": NUM_CLASSES, "state_dict": {}, "freeze": {}}
    for method in METHODS:
        for norm in NORMS:
            m = build(cfg, "cat", method, norm)
            meta["state_dict"][f"cat:{method}:{norm}"] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    meta["state_dict"]["ap"] = [[k, list(v.shape)] for k, v in build(cfg, "ap").state_dict().items()]
    for tag, m in (("cat:cls_avgN_proj:BN", build(cfg, "cat", "cls_avgN_proj", "BN")), ("ap", build(cfg, "ap"))):
        meta["freeze"][tag] = {}
        for k, op in FREEZE_SETTINGS:
            for p in m.parameters():
                p.requires_grad = True
            frozen, trainable = freeze(m, cfg.depth, k, op)
            meta["freeze"][tag][f"{k}:{'T' if op else 'F'}"] = {"frozen": frozen, "trainable": trainable}
    jpath = os.path.join(HERE, "probe.json")
    with open(jpath, "w") as f:
        json.dump(meta, f, indent=1)
    print(f"wrote {jpath}: {os.path.getsize(jpath) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
