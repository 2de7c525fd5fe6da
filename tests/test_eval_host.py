"""Validation / multi-view test, CPU side: the C ABI of csrc/evaluate.hip (exported, declared, bound, rejecting bad arguments on the host),
the rank-file parser and writer against the text the REFERENCE's final_test wrote (tests/golden/eval_views.npz, made by
make_golden_eval.py), `forward_only`'s attribute handling, and the argument errors of internvideo_amd.evaluate."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "eval_views.npz")
ENTRY_POINTS = ("ivh_eval_rows", "ivh_view_finalize", "ivh_view_mask_owned")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def bits_to_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def tiny(kind="ft"):
    from internvideo_amd import internvideo2, internvideo2_ap, internvideo2_cat
    from oracle import internvideo2_oracle as O
    cfg = O.named_config("tiny88")
    mod = {"ft": internvideo2, "cat": internvideo2_cat, "ap": internvideo2_ap}[kind]
    return mod.InternVideo2(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio,
                            num_frames=cfg.num_frames, drop_path_rate=0.0, attn_pool_num_heads=cfg.attn_pool_num_heads,
                            clip_embed_dim=cfg.clip_embed_dim, num_classes=10)


def test_entry_points_are_exported_declared_and_bound():
    from internvideo_amd import lib as L, ops
    from internvideo_amd.csrc import build as B
    assert "evaluate.hip" in B.SOURCES
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
    for fn in ("eval_rows", "view_finalize", "view_mask_owned"):
        assert callable(getattr(ops, fn))


def test_operators_are_registered_with_meta_kernels():
    import internvideo_amd.torch_ops as T
    ns = torch.ops.internvideo_hip
    for name in ("eval_rows_", "view_finalize", "view_mask_owned_"):
        assert name in T.OPERATORS and hasattr(ns, name)
    lg = torch.empty((5, 174), dtype=torch.bfloat16, device="meta")
    loss, rank = ns.eval_rows_(lg, torch.empty((5,), dtype=torch.int64, device="meta"))
    assert loss.shape == (5,) and loss.dtype == torch.float32 and rank.shape == (5,) and rank.dtype == torch.int32
    table = torch.empty((7 * 12, 176), dtype=torch.bfloat16, device="meta")
    out, probs = ns.view_finalize(table, torch.empty((84,), dtype=torch.int64, device="meta"), torch.empty((84,), dtype=torch.int32, device="meta"), 12, 174)
    assert out.shape == (7, 4) and out.dtype == torch.int32 and probs.shape == (7, 174) and probs.dtype == torch.float32


def test_entry_points_reject_bad_arguments_without_launching():
    """host-side validation returns < 0 (no device is touched: this runs without a GPU)"""
    from internvideo_amd import lib as L
    lib = L.load()
    p = C.c_void_p(64)                                      # never dereferenced: every call below is rejected on the host
    ok = (p, 0, 176, 5, 174, p, p, p, 0, 7, 12, p, 0, 176, p, p, p, p, p, None)

    def rows(**kw):
        names = ("logits", "fp32", "ld", "M", "V", "label", "video", "view", "seq", "nvid", "nview", "table", "tfp32", "ldt", "owner", "tlabel",
                 "loss", "rank", "meters", "stream")
        a = dict(zip(names, ok)); a.update(kw)
        return lib.ivh_eval_rows(*[a[n] for n in names])

    assert rows(logits=None) < 0 and rows(label=None) < 0 and rows(loss=None) < 0 and rows(rank=None) < 0
    assert rows(M=0) < 0 and rows(V=0) < 0
    assert rows(ld=173) < 0                                                        # ld < V
    assert rows(table=None) < 0 and rows(owner=None) < 0 and rows(video=None) < 0  # half a view table
    assert rows(ldt=172) < 0 and rows(ldt=168) < 0                                 # pitch % 8, pitch < V
    assert rows(table=C.c_void_p(72)) < 0                                          # table alignment
    assert rows(nvid=0) < 0 and rows(nview=0) < 0
    assert rows(seq=-1) < 0 and rows(seq=(1 << 40) - 3) < 0 and rows(seq=(1 << 62)) < 0      # the counter would run into the rank field / rank >= 2^22
    assert rows(meters=C.c_void_p(68)) < 0
    assert "eval_rows" in L.last_error()
    assert lib.ivh_view_finalize(None, 0, 176, 174, 7, 12, p, p, p, None, 0, None) < 0
    assert lib.ivh_view_finalize(p, 0, 172, 174, 7, 12, p, p, p, None, 0, None) < 0             # pitch
    assert lib.ivh_view_finalize(p, 0, 176, 174, 0, 12, p, p, p, None, 0, None) < 0
    assert lib.ivh_view_finalize(p, 0, 176, 174, 7, 12, p, p, None, None, 0, None) < 0          # no output
    assert lib.ivh_view_finalize(p, 0, 176, 174, 7, 12, p, p, p, p, 173, None) < 0              # probs pitch < V
    assert lib.ivh_view_finalize(p, 1, 16000, 15999, 7, 12, p, p, p, None, 0, None) < 0         # wider than the LDS accumulator
    assert "view_finalize" in L.last_error()
    assert lib.ivh_view_mask_owned(None, 0, 176, p, p, 84, 0, None) < 0
    assert lib.ivh_view_mask_owned(p, 0, 174, p, p, 84, 0, None) < 0
    assert lib.ivh_view_mask_owned(p, 0, 176, p, p, 0, 0, None) < 0
    assert lib.ivh_view_mask_owned(p, 0, 176, p, p, 84, -1, None) < 0 and lib.ivh_view_mask_owned(p, 0, 176, p, p, 84, 1 << 22, None) < 0
    assert "view_mask_owned" in L.last_error()


def test_parser_reproduces_the_reference_files(gold, tmp_path):
    from internvideo_amd import evaluate as E
    names = [str(n) for n in gold["video_names"]]
    n_text = 0
    for pre in (str(c) for c in gold["cases"]):
        if pre + "r0:text" not in gold.files:
            continue
        for k in (0, 1):
            text = bytes(gold[pre + f"r{k}:text"]).decode()
            (tmp_path / f"{k}.txt").write_text("the first line is skipped\n" + text)
        files = E.read_rank_files(str(tmp_path), 2)
        for k, (ids, labels, chunks, splits, logits) in enumerate(files):
            r = pre + f"r{k}:"
            assert ids == [names[v] for v in gold[r + "video"]]
            assert labels.tolist() == gold[r + "labels"].tolist() and chunks.tolist() == gold[r + "chunk"].tolist()
            assert splits.tolist() == gold[r + "split"].tolist()
            want = bits_to_f32(gold[r + "bits"])
            assert logits.dtype == np.float32 and logits.shape == want.shape and logits.tobytes() == want.tobytes()       # bit-exact fp32
            n_text += 1
    assert n_text == 8                                        # V = 10 and 174, two geometries, two ranks


def test_writer_reproduces_the_reference_lines_byte_for_byte(gold):
    from internvideo_amd import evaluate as E
    names = [str(n) for n in gold["video_names"]]
    for pre in (str(c) for c in gold["cases"]):
        for k in (0, 1):
            r = pre + f"r{k}:"
            logits = torch.from_numpy(bits_to_f32(gold[r + "bits"])).to(torch.bfloat16)        # what the model hands over
            lines = E.format_lines([names[v] for v in gold[r + "video"]], logits, gold[r + "labels"], gold[r + "chunk"], gold[r + "split"])
            text = "".join(lines).encode()
            if r + "text" in gold.files:
                assert text == bytes(gold[r + "text"]), r
            assert hashlib.sha256(text).digest() == gold[r + "text_sha"].tobytes(), r
            name, label, chunk, split, data = E.parse_line(lines[-1])                              # and back
            assert (name, label, chunk, split) == (names[gold[r + "video"][-1]], gold[r + "labels"][-1], gold[r + "chunk"][-1], gold[r + "split"][-1])
            assert data.tobytes() == bits_to_f32(gold[r + "bits"][-1]).tobytes()


@pytest.mark.parametrize("kind", ["ft", "cat", "ap"])
def test_forward_only_restores_the_attribute_state(kind):
    from internvideo_amd.evaluate import forward_only
    m = tiny(kind)
    x = torch.zeros(1)
    assert not hasattr(m, "frozen_prefix") and m._frozen_prefix(x) == 0
    with forward_only(m) as inner:
        assert inner is m and not torch.is_grad_enabled()
        assert m.frozen_prefix == m.depth and m._frozen_prefix(x) == m.depth
    assert not hasattr(m, "frozen_prefix") and torch.is_grad_enabled() and m._frozen_prefix(x) == 0      # absence is restored
    with pytest.raises(RuntimeError, match="boom"):
        with forward_only(m):
            raise RuntimeError("boom")
    assert not hasattr(m, "frozen_prefix") and torch.is_grad_enabled()
    m.frozen_prefix = 2                                      # a probing model keeps its own value
    with forward_only(m):
        assert m.frozen_prefix == m.depth
    assert m.frozen_prefix == 2
    with pytest.raises(RuntimeError):
        with forward_only(m):
            raise RuntimeError("boom")
    assert m.frozen_prefix == 2
    m.fp8_gemm = True                                        # not eligible: the existing rule keeps the autograd stack
    with forward_only(m):
        assert m._frozen_prefix(x) == 0
    del m.fp8_gemm


def test_forward_only_on_a_wrapper_and_on_a_foreign_module():
    from internvideo_amd.evaluate import forward_only
    m = tiny("ft")

    class Wrapper(torch.nn.Module):
        def __init__(self, module):
            super().__init__()
            self.module = module

    w = Wrapper(m)
    with forward_only(w):
        assert m.frozen_prefix == m.depth and not hasattr(w, "frozen_prefix")
    assert not hasattr(m, "frozen_prefix")
    lin = torch.nn.Linear(2, 2)
    with forward_only(lin):
        assert not torch.is_grad_enabled() and not hasattr(lin, "frozen_prefix")
    assert not hasattr(lin, "frozen_prefix")


def test_argument_errors():
    from internvideo_amd import evaluate as E
    from internvideo_amd.lib import InternVideoHipError
    model = torch.nn.Linear(2, 2)
    for fn, extra in ((E.validation_one_epoch, ()), (E.final_test, ("out.txt",))):
        with pytest.raises(NotImplementedError):
            fn([], model, "cpu", *extra, ds=True, bf16=False)
        with pytest.raises(ValueError, match="empty"):
            fn([], model, "cpu", *extra, ds=True, bf16=True)
    with pytest.raises(ValueError, match="file"):
        E.final_test([], model, "cpu", None)
    names = ["a", "b", "c"]
    for bad in (dict(names=["a", "a"]), dict(names=[]), dict(num_views=0), dict(num_views=4), dict(num_classes=0), dict(dtype=torch.float16)):
        kw = dict(names=names, num_views=6, num_classes=10, device="cpu"); kw.update(bad)
        with pytest.raises(ValueError):
            E.ViewTable(**kw)
    t = E.ViewTable(names, 6, 10, device="cpu")
    assert t.table.shape == (18, 16) and t.table.dtype == torch.bfloat16 and bool((t.owner == E.NO_OWNER).all())
    lg, lab = torch.zeros((2, 10), dtype=torch.bfloat16), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="not in the table"):
        t.add(lg, lab, ["a", "zzz"], [0, 0], [0, 1])
    with pytest.raises(ValueError, match="chunk_nb"):
        t.add(lg, lab, ["a", "b"], [0, 2], [0, 1])            # 6 views = 2 chunks x 3 crops
    with pytest.raises(ValueError, match="chunk_nb"):
        t.add(lg, lab, ["a", "b"], torch.tensor([0, 1]), torch.tensor([0, 3]))
    with pytest.raises(ValueError):
        t.add(torch.zeros((2, 11), dtype=torch.bfloat16), lab, ["a", "b"], [0, 0], [0, 1])
    with pytest.raises(ValueError):
        t.add(lg, lab, ["a"], [0, 0], [0, 1])
    with pytest.raises(InternVideoHipError):                 # valid arguments, but there is no CPU path
        t.add(lg, lab, ["a", "b"], [0, 1], [0, 1])
    with pytest.raises(ValueError):
        E.merge(os.path.join(ROOT, "tests", "golden", "no_such_dir"), 0)
