"""Golden fixture for the stage-2 zero-shot retrieval evaluation: the reference's own `evaluation` and `itm_eval`
(InternVideo2/multi_modality/tasks/retrieval_utils.py:226-613, :1243-1303) on a stand-in model.

    python tests/golden/make_golden_retrieval.py          (authoring container only: needs /root/reference; CPU, fp32)

retrieval_utils.py is imported UNMODIFIED under module stand-ins, as ref_loader does for criterions.py: `models.criterions` is the reference's
criterions.py, `utils.basic_utils.MetricLogger.log_every` passes its iterable through, `utils.distributed` reports rank 0 of 1.  The model the
reference's `evaluation` drives is a stand-in: `encode_text` / `encode_vision` hand out seeded features, `vision_proj`, `text_proj` and `itm_head`
are real nn.Linear layers, `get_text_encoder()` is the reference's own BertModel at the bert_tiny size with the weights of
`oracle.synthetic_bert_params(cfg, seed=0)` (generated, not stored).

Sizes: nv = 13 videos of 9 tokens x 176, nt = 29 captions of 12 tokens x 128 (right-padded, lengths 1 .. 12, both ends present), `img2txt` lists
of 2 or 3 captions, `txt2img` ints.  The features carry a signal: the projected [CLS] feature of a caption is the projected pooled feature of its
video plus noise, so that the dual-encoder ranking is neither trivial nor hopeless (a purely random ranking would leave the ground truth of most
rows among the not re-ranked -100 entries, which are tied, at k_test = 5).

Stored: the inputs, the raw similarities, the reference's six outputs at k_test = 29 (every pair re-ranked: the match matrices are the row softmax
of the full pair-score matrix) and at k_test = 5, the three metric dicts of both runs, and `bf16_err`: the relative l2 error of the k_test = 29 match
matrices (both directions, concatenated) of the same reference run with `.bfloat16()` weights and features against the fp32 run.

The inputs' seed is the first of 0, 1, 2, ... whose fixture passes every check below (stored as `seed`).  For a seed the generator refuses to
write unless
  * in every row of every output the best ground-truth entry is unique in its row and, in the match matrices, was re-ranked (not a fill entry), and
    the row's ten largest entries are pairwise distinct (the k_test = 5 match matrices: the five re-ranked ones; the fill entries below them are
    tied by construction) -- R@1 / R@5 / R@10 then do not depend on how a sort breaks ties;
  * the reference's own bf16 run reproduces, row by row, whether the best ground truth ranks below 1, 5 and 10 in the match matrices (over all
    columns and over the columns selected at k_test = 5): the match metrics then do not hinge on differences of the size of bf16 rounding;
  * at k_test = 5 the 5th and 6th largest similarity of every row, in both directions, are more than 1e-3 apart (cosines; fp32 summation-order
    error over 512 terms is ~1e-6), so the selected set does not depend on rounding.
-> tests/golden/retrieval.npz"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_loader  # noqa: E402
from oracle import internvideo2_oracle as O  # noqa: E402

NV, NT, LV, DV, LT, DT, E = 13, 29, 9, 176, 12, 128, 32
MAX_SEEDS = 400               # the inputs' seed is the first one whose fixture passes both checks below (recorded in the file)
OUT_NAMES = ("i2t_match", "t2i_match", "i2t_sim", "t2i_sim", "i2t_dsl", "t2i_dsl")


def load_retrieval_utils():
    crit = ref_loader.load_mm_criterions()
    models = types.ModuleType("models"); models.__path__ = []
    mc = types.ModuleType("models.criterions"); mc.get_sim = crit.get_sim
    utils = types.ModuleType("utils"); utils.__path__ = []
    ub = types.ModuleType("utils.basic_utils")

    class MetricLogger:
        def __init__(self, delimiter=" "):
            pass

        def log_every(self, iterable, print_freq, header=None):
            yield from iterable
    ub.MetricLogger = MetricLogger
    ud = types.ModuleType("utils.distributed"); ud.get_rank = lambda: 0; ud.get_world_size = lambda: 1
    saved = {k: sys.modules.get(k) for k in ("models", "models.criterions", "utils", "utils.basic_utils", "utils.distributed")}
    sys.modules.update({"models": models, "models.criterions": mc, "utils": utils, "utils.basic_utils": ub, "utils.distributed": ud})
    try:
        spec = importlib.util.spec_from_file_location(
            "_iv_ref_retrieval_utils", os.path.join(ref_loader.REF_ROOT, "InternVideo2", "multi_modality", "tasks", "retrieval_utils.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return m


class Cfg(dict):
    __getattr__ = dict.__getitem__


class TextBatch:
    def __init__(self, rows, atts):
        self.rows, self.attention_mask, self.input_ids = rows, atts, rows

    def to(self, device):
        return self


class StandIn(nn.Module):
    def __init__(self, bert, heads, text_feats, media_feats, pooled):
        super().__init__()
        self.text_encoder = bert
        self.vision_proj, self.text_proj, self.itm_head = nn.Linear(DV, E), nn.Linear(DT, E), nn.Linear(DT, 2)
        with torch.no_grad():
            for lin, (w, b) in zip((self.vision_proj, self.text_proj, self.itm_head), heads):
                lin.weight.copy_(torch.from_numpy(w)); lin.bias.copy_(torch.from_numpy(b))
        self.register_buffer("text_feats", text_feats)
        self.register_buffer("media_feats", media_feats)
        self.register_buffer("pooled", pooled)

    def get_text_encoder(self):
        return self.text_encoder

    def encode_text(self, text):
        f = self.text_feats[text.rows]
        return f, f[:, 0]

    def encode_vision(self, image, test=False):
        rows = image.long()
        return self.media_feats[rows], self.pooled[rows]


def make_inputs(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    d = {}
    d["head_vision_w"] = (rng.standard_normal((E, DV)) / np.sqrt(DV)).astype(np.float32)
    d["head_vision_b"] = (0.1 * rng.standard_normal(E)).astype(np.float32)
    d["head_text_w"] = (rng.standard_normal((E, DT)) / np.sqrt(DT)).astype(np.float32)
    d["head_text_b"] = (0.1 * rng.standard_normal(E)).astype(np.float32)
    d["head_itm_w"] = (rng.standard_normal((2, DT)) / np.sqrt(DT)).astype(np.float32)
    d["head_itm_b"] = (0.1 * rng.standard_normal(2)).astype(np.float32)
    d["media_feats"] = rng.standard_normal((NV, 1, LV, DV)).astype(np.float32)
    d["pooled_media_feats"] = rng.standard_normal((NV, 1, DV)).astype(np.float32)
    # captions: 2 or 3 per video, consecutive (13 videos -> 3 + 12 * 2 + 2 extra = 29)
    per = [3 if i in (0, 4, 9) else 2 for i in range(NV)]
    assert sum(per) == NT
    txt2img = np.repeat(np.arange(NV), per).astype(np.int64)
    d["txt2img"] = txt2img
    d["img2txt_ptr"] = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    text = rng.standard_normal((NT, LT, DT)).astype(np.float32)
    # [CLS] rows: text_proj(cls_j) = vision_proj(pooled_i) + noise for the caption's video i (minimum-norm preimage + a null-space part)
    pv = d["pooled_media_feats"][:, 0] @ d["head_vision_w"].T + d["head_vision_b"]
    target = pv[txt2img] + 1.5 * rng.standard_normal((NT, E)).astype(np.float32) * pv.std()
    pinv = np.linalg.pinv(d["head_text_w"].astype(np.float64))                       # (DT, E)
    cls = (target - d["head_text_b"]).astype(np.float64) @ pinv.T
    null = text[:, 0].astype(np.float64)
    null = null - (null @ d["head_text_w"].astype(np.float64).T) @ pinv.T           # remove the part text_proj sees
    text[:, 0] = (cls + 0.5 * null).astype(np.float32)
    d["text_feats"] = text
    lengths = np.array([1, 12] + [int(x) for x in rng.integers(2, LT + 1, size=NT - 2)], dtype=np.int64)
    d["text_lengths"] = lengths
    d["text_atts"] = (np.arange(LT)[None, :] < lengths[:, None]).astype(np.int64)
    return d


def run_reference(R, d, k_test, use_dsl=False, bf16=False):
    cfg = O.named_bert_config("bert_tiny")
    ref = ref_loader.build_reference_bert(cfg)
    ref.load_state_dict(O.synthetic_bert_params(cfg, seed=0), strict=False)
    heads = [(d["head_vision_w"], d["head_vision_b"]), (d["head_text_w"], d["head_text_b"]), (d["head_itm_w"], d["head_itm_b"])]
    model = StandIn(ref.bert, heads, torch.from_numpy(d["text_feats"]), torch.from_numpy(d["media_feats"][:, 0]),
                    torch.from_numpy(d["pooled_media_feats"][:, 0]))
    if bf16:
        model = model.bfloat16()
    model.eval()
    atts = torch.from_numpy(d["text_atts"])
    tokenizer = lambda text, **kw: TextBatch(torch.tensor(list(text), dtype=torch.long), atts[list(text)])      # noqa: E731
    dataset = types.SimpleNamespace(text=list(range(NT)), max_txt_l=LT, media_type="video", image=list(range(NV)),
                                    txt2img={j: int(v) for j, v in enumerate(d["txt2img"])},
                                    img2txt={i: list(range(int(d["img2txt_ptr"][i]), int(d["img2txt_ptr"][i + 1]))) for i in range(NV)})

    class Loader(list):
        pass
    loader = Loader([(torch.arange(a, min(NV, a + 5)).float(), list(range(a, min(NV, a + 5)))) for a in range(0, NV, 5)])
    loader.dataset = dataset
    config = Cfg(use_half_precision=False, deep_fusion=False, distributed=False,
                 evaluation=Cfg(eval_frame_ensemble="concat", eval_offload=False, k_test=k_test, use_dsl_for_match=use_dsl),
                 model=Cfg(model_cls="InternVideo2_Stage2_visual"))
    outs = R.evaluation(model, loader, tokenizer, "cpu", config)
    return [np.asarray(o, dtype=np.float32) for o in outs], dataset


def check_rows(name, m, gts, selected=None):
    """the best ground-truth entry of every row is unique in the row (and re-ranked), and the ten largest entries are pairwise distinct"""
    for r in range(m.shape[0]):
        row = m[r]
        g = max(gts[r], key=lambda c: row[c])
        assert (row == row[g]).sum() == 1, f"{name} row {r}: the best ground truth is tied"
        cols = np.arange(row.size) if selected is None else np.flatnonzero(selected[r])
        if selected is not None:
            assert selected[r][g], f"{name} row {r}: the best ground truth was not re-ranked"
        top = np.sort(row[cols])[::-1][:10]
        assert len(np.unique(top)) == len(top), f"{name} row {r}: tie among the largest entries"


def recall_flags(m, gts, selected=None):
    """per row: (rank < 1, rank < 5, rank < 10) of the best ground truth among the (selected) columns"""
    out = []
    for r in range(m.shape[0]):
        cols = np.arange(m.shape[1]) if selected is None else np.flatnonzero(selected[r])
        rank = min(int((m[r, cols] > m[r, g]).sum()) for g in gts[r] if selected is None or selected[r][g])
        out.append((rank < 1, rank < 5, rank < 10))
    return np.array(out)


def main():
    assert ref_loader.available(), "needs the reference tree (IV_REFERENCE_ROOT)"
    torch.manual_seed(0)
    R = load_retrieval_utils()
    for seed in range(MAX_SEEDS):
        try:
            d = build(R, seed)
            break
        except AssertionError as e:
            print(f"seed {seed}: refused ({e})")
    else:
        raise SystemExit("no seed passed the checks: no fixture written")
    path = os.path.join(HERE, "retrieval.npz")
    np.savez_compressed(path, **d)
    print(f"seed {seed}: wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB")


def build(R, seed):
    d = make_inputs(seed)
    d["seed"] = np.array(seed)
    get_sim = ref_loader.load_mm_criterions().get_sim
    with torch.no_grad():
        pv = torch.from_numpy(d["pooled_media_feats"]) @ torch.from_numpy(d["head_vision_w"]).T + torch.from_numpy(d["head_vision_b"])
        pt = torch.from_numpy(d["text_feats"][:, 0]) @ torch.from_numpy(d["head_text_w"]).T + torch.from_numpy(d["head_text_b"])
        s1, s2 = get_sim(pv, pt)
    d["sim_v2t"], d["sim_t2v"] = s1.numpy(), s2.numpy()
    for tag, s in (("v2t", d["sim_v2t"]), ("t2v", d["sim_t2v"])):
        srt = np.sort(s, axis=1)[:, ::-1]
        gap = (srt[:, 4] - srt[:, 5]).min()
        assert gap > 1e-3, f"{tag}: 5th / 6th similarity only {gap:.2e} apart"
        print(f"{tag}: smallest 5th / 6th gap {gap:.3e}")
    gt_v = {i: list(range(int(d["img2txt_ptr"][i]), int(d["img2txt_ptr"][i + 1]))) for i in range(NV)}
    gt_t = {j: [int(v)] for j, v in enumerate(d["txt2img"])}
    for k_test in (29, 5):
        outs, dataset = run_reference(R, d, k_test)
        for name, o in zip(OUT_NAMES, outs):
            d[f"k{k_test}:{name}"] = o
            sel = None
            if name.endswith("match") and k_test < max(NV, NT):
                srt = np.sort(d["sim_v2t" if name[0] == "i" else "sim_t2v"], axis=1)[:, ::-1]
                sel = d["sim_v2t" if name[0] == "i" else "sim_t2v"] >= srt[:, k_test - 1:k_test]
            check_rows(f"k{k_test}:{name}", o, gt_v if name[0] == "i" else gt_t, sel)
        for mname, (a, b) in (("sim", (outs[2], outs[3])), ("dsl", (outs[4], outs[5])), ("match", (outs[0], outs[1]))):
            res = R.itm_eval(a, b, dataset.txt2img, dataset.img2txt)
            d[f"k{k_test}:metrics_{mname}"] = np.array([res[k] for k in sorted(res)], dtype=np.float64)
            d["metric_keys"] = np.array(sorted(res))
            print(f"k_test {k_test} {mname}: {res}")
    b16, _ = run_reference(R, d, 29, bf16=True)
    ref = np.concatenate([d["k29:i2t_match"].ravel(), d["k29:t2i_match"].ravel()]).astype(np.float64)
    got = np.concatenate([b16[0].ravel(), b16[1].ravel()]).astype(np.float64)
    d["bf16_err"] = np.array(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    print(f"bf16_err {float(d['bf16_err']):.4e}")
    # the match metrics must not hinge on differences of the size of bf16 rounding: the reference's own bf16 run reproduces the recall flags
    # of every row, over all columns (k_test = 29) and over the columns selected at k_test = 5
    for i, (name, gts, sim) in enumerate((("i2t_match", gt_v, d["sim_v2t"]), ("t2i_match", gt_t, d["sim_t2v"]))):
        srt = np.sort(sim, axis=1)[:, ::-1]
        for sel in (None, sim >= srt[:, 4:5]):
            same = recall_flags(b16[i], gts, sel) == recall_flags(d["k29:" + name], gts, sel)
            assert same.all(), f"{name}: the bf16 run of the reference changes R@k of {int((~same).any(1).sum())} rows"
    return d


if __name__ == "__main__":
    main()
