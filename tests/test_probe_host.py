"""Linear / attentive probing, CPU side: the registry names of the two probing model families, their state_dict key / shape lists and the
freezing loop against tests/golden/probe.json (written by make_golden_probe.py from the reference's own internvideo2_cat.py /
internvideo2_ap.py and the loop of run_linear_probing.py:556-581), argument errors, the C ABI of csrc/probe.hip (exported, declared, bound,
rejecting bad arguments on the host) and `block_stack_infer`'s signature."""
import ctypes as C
import inspect
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ivh_cat_pool_fwd", "ivh_cat_pool_bwd", "ivh_batchnorm_cols_fwd", "ivh_batchnorm_cols_bwd")
SIZES = ("small", "base", "large", "1B", "6B")
METHODS = ("proj", "cls_avg1", "cls_avgN", "cls_avg1_proj", "cls_avgN_proj")
NORMS = ("kaiming_BN", "LN", "BN")


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(ROOT, "tests", "golden", "probe.json")) as f:
        return json.load(f)


def tiny(kind, **extra):
    from internvideo_amd import internvideo2_ap, internvideo2_cat
    from oracle import internvideo2_oracle as O
    cfg = O.named_config("tiny88")
    mod = {"cat": internvideo2_cat, "ap": internvideo2_ap}[kind]
    return mod.InternVideo2(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio,
                            num_frames=cfg.num_frames, drop_path_rate=0.0, attn_pool_num_heads=cfg.attn_pool_num_heads,
                            clip_embed_dim=cfg.clip_embed_dim, num_classes=10, **extra)


def test_registry_names():
    from internvideo_amd import internvideo2, internvideo2_ap, internvideo2_cat  # noqa: F401
    from internvideo_amd.internvideo2_pretrain import _registry
    for fam in ("cat", "ap"):
        for size in SIZES:
            assert f"internvideo2_{fam}_{size}_patch14_224" in _registry
    assert internvideo2_cat.InternVideo2.__name__ == internvideo2_ap.InternVideo2.__name__ == "InternVideo2"
    assert issubclass(internvideo2_cat.InternVideo2, internvideo2.InternVideo2)
    assert issubclass(internvideo2_ap.InternVideo2, internvideo2.InternVideo2)
    # the plain classifier's names are untouched
    assert "internvideo2_1B_patch14_224" in _registry


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("norm", NORMS)
def test_cat_state_dict_matches_the_reference(meta, method, norm):
    m = tiny("cat", merge_method=method, merge_norm=norm)
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert got == meta["state_dict"][f"cat:{method}:{norm}"]


def test_ap_state_dict_and_zero_init(meta):
    m = tiny("ap")
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == meta["state_dict"]["ap"]
    fc2 = m.extra_mlp[1].fc2
    assert float(fc2.weight.detach().abs().max()) == 0.0 and float(fc2.bias.detach().abs().max()) == 0.0          # internvideo2_ap.py:449-451
    assert float(m.extra_mlp[1].fc1.weight.detach().abs().max()) > 0.0


@pytest.mark.parametrize("tag", ["cat:cls_avgN_proj:BN", "ap"])
def test_freeze_for_probing_reproduces_the_reference_loop(meta, tag):
    from internvideo_amd.probe import freeze_for_probing
    for key, want in meta["freeze"][tag].items():
        k, op = key.split(":")
        m = tiny("ap") if tag == "ap" else tiny("cat", merge_method=tag.split(":")[1], merge_norm=tag.split(":")[2])
        frozen, trainable = freeze_for_probing(m, open_block_num=int(k), open_clip_projector=(op == "T"))
        assert frozen == want["frozen"] and trainable == want["trainable"], key
        named = dict(m.named_parameters())
        assert all(not named[n].requires_grad for n in frozen) and all(named[n].requires_grad for n in trainable)
        assert m.frozen_prefix == len(m.blocks) - int(k)


def test_freeze_for_probing_depth_and_bounds():
    from internvideo_amd.probe import freeze_for_probing
    m = tiny("cat")
    with pytest.raises(ValueError):
        freeze_for_probing(m, open_block_num=4)
    # an explicit depth beyond the model's (the reference's hard-coded 40 on a smaller model) opens nothing
    frozen, _ = freeze_for_probing(m, open_block_num=1, depth=40)
    assert all(n in frozen for n, _ in m.named_parameters() if n.startswith("blocks."))
    assert m.frozen_prefix == len(m.blocks)


def test_default_model_has_no_frozen_prefix():
    m = tiny("cat")
    assert not hasattr(m, "frozen_prefix")
    assert m._frozen_prefix(torch.zeros(1)) == 0


def test_unknown_method_or_norm_raises():
    with pytest.raises(ValueError):
        tiny("cat", merge_method="cls_avg2")
    with pytest.raises(ValueError):
        tiny("cat", merge_method="cls_avg1", merge_norm="GN")


def test_block_stack_infer_signature():
    from internvideo_amd import functional as Fn
    names = list(inspect.signature(Fn.block_stack_infer).parameters)
    assert names[:9] == ["x0", "block_params", "S", "L", "H", "eps", "act", "taps", "fp8"]         # today's positional call
    p = inspect.signature(Fn.block_stack_infer).parameters
    assert p["fp8"].default is False and p["rowscale"].default is None


def test_entry_points_are_exported_declared_and_bound():
    from internvideo_amd import lib as L, ops
    from internvideo_amd.csrc import build as B
    assert "probe.hip" in B.SOURCES
    B.build()
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "internvideo_hip.h")).read()
    assert re.search(r"#define IVH_ABI_VERSION 2\b", header) and lib.ivh_abi_version() == 2       # additions only: no ABI step
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S | re.M)
        assert m, f"{name} is not declared in include/internvideo_hip.h"
        decls = [a for a in m.group(1).split(",") if a.strip()]
        assert len(decls) == len(L.SIGNATURES[name]), (name, len(decls), len(L.SIGNATURES[name]))
        for decl, ty in zip(decls, L.SIGNATURES[name]):
            want = C.c_void_p if "*" in decl else C.c_int64 if "int64_t" in decl else C.c_float if "float" in decl else C.c_int32
            assert ty is want, (name, decl.strip(), ty)
    for fn in ("cat_pool_fwd", "cat_pool_bwd", "batchnorm_cols_fwd", "batchnorm_cols_bwd"):
        assert callable(getattr(ops, fn))


def test_entry_points_reject_bad_arguments_without_launching():
    """host-side validation returns < 0 (no device is touched: this runs without a GPU)"""
    from internvideo_amd import lib as L
    lib = L.load()
    p = C.c_void_p(64)                                      # never dereferenced: every call below is rejected on the host
    assert lib.ivh_cat_pool_fwd(None, 1, 2, 4, 16, 176, 0, p, None, None, None) < 0
    assert lib.ivh_cat_pool_fwd(p, 1, 2, 4, 16, 180, 0, p, None, None, None) < 0            # C % 8
    assert lib.ivh_cat_pool_fwd(p, 1, 2, 4, 16, 176, 2, p, None, None, None) < 0            # mode
    assert lib.ivh_cat_pool_fwd(p, 1, 2, 4, 16, 176, 1, p, None, None, None) < 0            # avg1 without its workspace
    assert lib.ivh_cat_pool_fwd(C.c_void_p(68), 1, 2, 4, 16, 176, 0, p, None, None, None) < 0   # alignment
    assert lib.ivh_cat_pool_fwd(p, 1, 0, 4, 16, 176, 0, p, None, None, None) < 0
    assert "cat_pool_fwd" in L.last_error()
    assert lib.ivh_cat_pool_bwd(None, None, 2, 4, 16, 176, 0, 0, p, None) < 0               # neither gradient
    assert lib.ivh_cat_pool_bwd(p, None, 2, 4, 16, 178, 0, 0, p, None) < 0                  # C % 4
    assert lib.ivh_cat_pool_bwd(p, None, 2, 4, 16, 176, 0, 0, None, None) < 0
    assert lib.ivh_batchnorm_cols_fwd(p, 1, 1, 1, 64, None, None, 1e-5, 1, 0.1, p, p, p, p, 64, p, p, None) < 0     # one value per channel
    assert lib.ivh_batchnorm_cols_fwd(p, 1, 2, 5, 64, None, None, 1e-5, 1, 0.1, p, p, p, p, 319, p, p, None) < 0    # ld_y < C * G
    assert lib.ivh_batchnorm_cols_fwd(p, 1, 2, 5, 64, None, None, 1e-5, 1, 0.1, p, None, p, p, 320, p, p, None) < 0  # half a buffer pair
    assert lib.ivh_batchnorm_cols_fwd(p, 1, 2, 5, 64, None, None, 1e-5, 0, 0.1, None, None, None, p, 320, p, p, None) < 0   # eval without buffers
    assert lib.ivh_batchnorm_cols_fwd(p, 1, 2, 5, 64, None, None, 0.0, 1, 0.1, p, p, p, p, 320, p, p, None) < 0     # eps
    assert "batchnorm_cols_fwd" in L.last_error()
    assert lib.ivh_batchnorm_cols_bwd(p, 1, 2, 5, 64, None, None, p, 1, p, 320, None, p, 1, None, None, None) < 0   # no mean
    assert lib.ivh_batchnorm_cols_bwd(p, 1, 2, 5, 64, None, p, p, 1, p, 100, None, p, 1, None, None, None) < 0      # ld_dy
    assert "batchnorm_cols_bwd" in L.last_error()
