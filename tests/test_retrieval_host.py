"""Stage-2 retrieval evaluation, CPU side: the C ABI of csrc/retrieval.hip is exported and bound consistently, `itm_eval`'s host glue and the
`num_prompts` reshape reproduce the reference's metric dicts (tests/golden/retrieval.npz, written by make_golden_retrieval.py from the
reference's own `evaluation` / `itm_eval`) when fed through a numpy restatement of the rank rule, and unsupported configurations raise."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "retrieval.npz")
ENTRY_POINTS = ("ivh_topk_rows_f32", "ivh_softmax_axis_f32", "ivh_rerank_lists", "ivh_scatter_pair_scores", "ivh_retrieval_ranks")
OUT_NAMES = ("i2t_match", "t2i_match", "i2t_sim", "t2i_sim", "i2t_dsl", "t2i_dsl")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(G))


def numpy_ranks(scores, gt_ptr, gt_idx):
    """the rank rule of ivh_retrieval_ranks restated: min over the row's ground truths g of #{c: x_c > x_g} + #{c < g: x_c == x_g}"""
    out = np.empty(scores.shape[0], dtype=np.int32)
    for r in range(scores.shape[0]):
        row, best = scores[r], scores.shape[1]
        for g in gt_idx[gt_ptr[r]:gt_ptr[r + 1]]:
            best = min(best, int((row > row[g]).sum() + (row[:g] == row[g]).sum()))
        out[r] = best
    return out


def ground_truth(gold):
    ptr = gold["img2txt_ptr"]
    img2txt = {i: list(range(int(ptr[i]), int(ptr[i + 1]))) for i in range(len(ptr) - 1)}
    txt2img = {j: int(v) for j, v in enumerate(gold["txt2img"])}
    return txt2img, img2txt


def metric_dict(gold, key):
    return {str(k): float(v) for k, v in zip(gold["metric_keys"], gold[key])}


def test_entry_points_are_exported_declared_and_bound():
    from internvideo_amd import lib as L, ops
    from internvideo_amd.csrc import build as B
    assert "retrieval.hip" in B.SOURCES
    B.build()
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "internvideo_hip.h")).read()
    assert re.search(r"#define IVH_ABI_VERSION 2\b", header) and lib.ivh_abi_version() == 2
    for name in ENTRY_POINTS + ("ivh_rerank_lists_workspace_bytes",):
        assert hasattr(lib, name), name
        m = re.search(r"^(?:int|int64_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S | re.M)
        assert m, f"{name} is not declared in include/internvideo_hip.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert n_args == len(L.SIGNATURES[name]), (name, n_args, len(L.SIGNATURES[name]))
        # pointers are void*, strides / capacities 64-bit, everything else 32-bit: the binding's types follow the declaration
        for decl, ty in zip(m.group(1).split(","), L.SIGNATURES[name]):
            want = C.c_void_p if "*" in decl else C.c_int64 if "int64_t" in decl else C.c_int32
            assert ty is want, (name, decl.strip(), ty)
    assert L._RESTYPES["ivh_rerank_lists_workspace_bytes"] is C.c_int64
    assert lib.ivh_rerank_lists_workspace_bytes(13, 29) == 13 * 29 + 3 + 13 * 4          # 377 pair bytes rounded to 380, 13 counts
    for fn in ("topk_rows", "softmax_axis", "rerank_lists", "scatter_pair_scores", "retrieval_ranks"):
        assert callable(getattr(ops, fn))


def test_entry_points_reject_bad_arguments_without_launching():
    """host-side validation returns < 0 (no device is touched: this runs without a GPU)"""
    from internvideo_amd import lib as L
    lib = L.load()
    p = C.c_void_p(64)                                      # never dereferenced: every call below is rejected on the host
    assert lib.ivh_topk_rows_f32(p, 4, 10, 10, 1, 0, p, p, None) < 0             # k = 0
    assert lib.ivh_topk_rows_f32(p, 4, 10, 10, 1, 11, p, p, None) < 0            # k > n_cols
    assert lib.ivh_topk_rows_f32(p, 4, 2000, 2000, 1, 1025, p, p, None) < 0      # k > 1024
    assert lib.ivh_topk_rows_f32(None, 4, 10, 10, 1, 3, p, p, None) < 0
    assert "topk_rows" in L.last_error()
    assert lib.ivh_softmax_axis_f32(p, 4, 10, 10, 1, p, 5, 1, 0, None) < 0       # output rows would overlap
    assert lib.ivh_softmax_axis_f32(p, 4, 10, -10, 1, p, 10, 1, 0, None) < 0
    assert lib.ivh_rerank_lists(p, 13, 5, p, 29, 5, 7, 14, p, p, p, p, None) < 0          # v_end > nv
    assert lib.ivh_rerank_lists(p, 13, 30, p, 29, 5, 0, 13, p, p, p, p, None) < 0         # kv > nt
    assert lib.ivh_scatter_pair_scores(p, p, p, p, 10, 10, 4, 13, 29, p, 29, 1, p, 13, 1, None) < 0     # videos [10, 14) of 13
    assert lib.ivh_scatter_pair_scores(p, p, p, p, 10, 0, 4, 13, 29, p, 20, 1, p, 13, 1, None) < 0      # x_v2t rows overlap
    assert lib.ivh_retrieval_ranks(p, 0, 10, 10, 1, p, p, p, None) < 0
    assert lib.ivh_rerank_lists_workspace_bytes(-1, 5) < 0


@pytest.mark.parametrize("k_test", [29, 5])
def test_itm_eval_host_glue_reproduces_the_reference_dicts(gold, k_test, monkeypatch):
    from internvideo_amd import retrieval as Rv
    monkeypatch.setattr(Rv, "_device_ranks", numpy_ranks)
    txt2img, img2txt = ground_truth(gold)
    for name, a, b in (("sim", "i2t_sim", "t2i_sim"), ("dsl", "i2t_dsl", "t2i_dsl"), ("match", "i2t_match", "t2i_match")):
        got = Rv.itm_eval(gold[f"k{k_test}:{a}"], gold[f"k{k_test}:{b}"], txt2img, img2txt)
        assert got == metric_dict(gold, f"k{k_test}:metrics_{name}"), name
    # sequences instead of dicts, ints and lists mixed
    got = Rv.itm_eval(gold["k29:i2t_sim"], gold["k29:t2i_sim"], [txt2img[j] for j in range(len(txt2img))], [img2txt[i] for i in range(len(img2txt))])
    assert got == metric_dict(gold, "k29:metrics_sim")


def test_gt_csr_and_rank_rows():
    from internvideo_amd import retrieval as Rv
    ptr, idx = Rv._gt_csr({0: 3, 1: [4, 1], 2: np.int64(0)}, 3)
    assert ptr.dtype == np.int32 and idx.dtype == np.int32
    assert ptr.tolist() == [0, 1, 3, 4] and idx.tolist() == [3, 4, 1, 0]
    # retrieval_utils.py:377-379: step = n // world + 1
    assert Rv.rank_rows(13, 0, 1) == (0, 13)
    assert [Rv.rank_rows(13, r, 2) for r in range(2)] == [(0, 7), (7, 13)]
    assert [Rv.rank_rows(4, r, 4) for r in range(4)] == [(0, 2), (2, 4), (4, 4), (4, 4)]


class _Loader(list):
    pass


def _wrapper_setup(gold, monkeypatch, n_prompts=None, model_cls="InternVideo2_Stage2_visual"):
    from internvideo_amd import retrieval as Rv
    txt2img, img2txt = ground_truth(gold)
    outs = [gold["k5:" + n] for n in OUT_NAMES]
    ds = SimpleNamespace(txt2img=txt2img, img2txt=img2txt, media_type="video")
    if n_prompts:
        # every caption appears n_prompts times in a row with scores spread around the stored one: the mean restores the stored matrices
        off = np.linspace(-1.0, 1.0, n_prompts).astype(np.float64) * 1e-3
        outs = [np.repeat(o.astype(np.float64), n_prompts, axis=1 if i % 2 == 0 else 0) for i, o in enumerate(outs)]
        for i, o in enumerate(outs):
            o += np.tile(off, o.shape[1] // n_prompts)[None, :] if i % 2 == 0 else np.tile(off, o.shape[0] // n_prompts)[:, None]
        ds.num_prompts = n_prompts
        ds.text = list(range(outs[0].shape[1]))
    loader = _Loader()
    loader.dataset = ds
    monkeypatch.setattr(Rv, "evaluation", lambda *a, **k: tuple(outs))
    monkeypatch.setattr(Rv, "_device_ranks", numpy_ranks)
    config = dict(model=dict(model_cls=model_cls), evaluation=dict(k_test=5))
    return Rv, loader, config


def test_evaluation_wrapper_names_and_dicts(gold, monkeypatch):
    Rv, loader, config = _wrapper_setup(gold, monkeypatch)
    res = Rv.evaluation_wrapper(None, loader, None, "cpu", config, prefix="val")
    assert sorted(res) == ["val_dsl", "val_match", "val_sim"]
    for name in ("sim", "dsl", "match"):
        assert res["val_" + name] == metric_dict(gold, "k5:metrics_" + name)
    config["evaluation"]["use_dsl_for_match"] = True
    assert "val_match (use_dsl)" in Rv.evaluation_wrapper(None, loader, None, "cpu", config, prefix="val")


def test_evaluation_wrapper_averages_prompts(gold, monkeypatch):
    Rv, loader, config = _wrapper_setup(gold, monkeypatch, n_prompts=3)
    res = Rv.evaluation_wrapper(None, loader, None, "cpu", config)
    for name in ("sim", "dsl", "match"):
        assert res["_" + name] == metric_dict(gold, "k5:metrics_" + name)
    m = np.arange(24, dtype=np.float64).reshape(2, 12)
    assert np.array_equal(Rv.mean_over_prompts(m, 3, 1), m.reshape(2, 4, 3).mean(-1))
    assert np.array_equal(Rv.mean_over_prompts(m.T.copy(), 3, 0), m.T.reshape(4, 3, 2).mean(1))
    assert Rv.mean_over_prompts(None, 3, 1) is None


@pytest.mark.parametrize("model_cls", ["InternVideo2_Stage2_qformer", "BLIP_x", "InternVideo2_CLIP", "CoCa"])
def test_other_model_families_raise(gold, monkeypatch, model_cls):
    Rv, loader, config = _wrapper_setup(gold, monkeypatch, model_cls=model_cls)
    with pytest.raises(NotImplementedError):
        Rv.evaluation_wrapper(None, loader, None, "cpu", config)


def test_unsupported_configurations_raise():
    from internvideo_amd import retrieval as Rv

    class Model(torch.nn.Module):
        pass

    def loader(**kw):
        ld = _Loader()
        ld.dataset = SimpleNamespace(media_type="video", text=["a"], max_txt_l=4, **kw)
        return ld
    base = dict(evaluation=dict(eval_frame_ensemble="concat", k_test=4), deep_fusion=False)
    for media_type in ("audio", "audio_video", "image"):
        ld = loader()
        ld.dataset.media_type = media_type
        with pytest.raises(NotImplementedError):
            Rv.evaluation(Model(), ld, None, "cpu", base)
    with pytest.raises(NotImplementedError):
        Rv.evaluation(Model(), loader(use_subtitle=True, subtitle=["s"]), None, "cpu", base)
    with pytest.raises(NotImplementedError):
        Rv.evaluation(Model(), loader(), None, "cpu", dict(base, deep_fusion=True))
    with pytest.raises(NotImplementedError):
        Rv.evaluation(Model(), loader(), None, "cpu", dict(base, evaluation=dict(eval_frame_ensemble="mean", k_test=4)))
    t, a = torch.zeros(3, 4, 8), torch.ones(3, 4, dtype=torch.long)
    with pytest.raises(NotImplementedError):                                    # two clips per video
        Rv.rerank_and_score(Model(), t, a, torch.zeros(2, 2, 5, 8), torch.zeros(2, 1, 8), base)
    with pytest.raises(NotImplementedError):
        Rv.rerank_and_score(Model(), t, a, torch.zeros(2, 1, 5, 8), torch.zeros(2, 1, 8), dict(base, deep_fusion=True))


def test_shared_cross_attention_is_inference_only():
    """the shared-encoder-state form refuses to run where a backward could follow (checked before any kernel is called)"""
    from internvideo_amd import xbert
    from internvideo_amd.lib import InternVideoHipError
    cfg = xbert.BertConfig(vocab_size=32, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256,
                           max_position_embeddings=16, fusion_layer=0, encoder_width=64)
    att = xbert.BertSelfAttention(cfg, is_cross_attention=True).eval()
    with pytest.raises(InternVideoHipError, match="inference"):
        att(torch.zeros(3, 4, 128), None, torch.zeros(1, 5, 64), None)
