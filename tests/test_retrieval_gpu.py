"""Stage-2 retrieval evaluation on the GPU: the five kernels of csrc/retrieval.hip against torch / numpy restatements (exact where the work is
integer or a selection), cross-attention against shared encoder states (bitwise against the expanded form), and `rerank_and_score` /
`evaluation` / `itm_eval` against the reference's own outputs (tests/golden/retrieval.npz, make_golden_retrieval.py).

Tolerances.  Match matrices: 2 * `bf16_err`, where `bf16_err` is the relative l2 error of the REFERENCE's own run with bf16 weights and features
against its fp32 run (stored in the fixture); the factor 2 because the native tower also rounds activations to bf16 between kernels.
Similarities: 1e-4 absolute (cosines from fp32 projections; fp32 summation-order error is ~1e-6).  Softmax: 4 x the error of torch's own fp32
evaluation of the same expression against fp64, measured inside the test (a different summation order, nothing else)."""
import dataclasses
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import internvideo2_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = os.path.join(os.path.dirname(__file__), "golden", "retrieval.npz")
OUT_NAMES = ("i2t_match", "t2i_match", "i2t_sim", "t2i_sim", "i2t_dsl", "t2i_dsl")
PAD = 64


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(G))


# ---- ivh_topk_rows_f32 -----------------------------------------------------------------------------------------------------------------------
def topk_guarded(x, k):
    """the entry point on outputs that sit inside a canary border; the border must come back untouched"""
    from internvideo_amd.lib import call, ptr, stream_ptr
    R, Cn = x.shape
    val = torch.full((R * k + 2 * PAD,), -777.0, dtype=torch.float32, device=DEV)
    idx = torch.full((R * k + 2 * PAD,), -777, dtype=torch.int32, device=DEV)
    call("ivh_topk_rows_f32", ptr(x), R, Cn, x.stride(0), x.stride(1), k, ptr(val[PAD:]), ptr(idx[PAD:]), stream_ptr())
    torch.cuda.synchronize()
    for buf in (val, idx):
        assert bool((buf[:PAD] == -777).all()) and bool((buf[PAD + R * k:] == -777).all()), "write outside the output"
    return val[PAD:PAD + R * k].view(R, k).clone(), idx[PAD:PAD + R * k].view(R, k).clone()


def distinct_rows(n_rows, n_cols, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.linspace(-3.0, 3.0, n_cols) if n_cols > 1 else torch.tensor([0.25])
    return torch.stack([base[torch.randperm(n_cols, generator=g)] for _ in range(n_rows)])


def stable_order(row):
    """columns by descending value, equal values (-0.0 == +0.0) by ascending column"""
    return sorted(range(len(row)), key=lambda c: (-float(row[c]) if row[c] != 0 else 0.0, c))


@pytest.mark.parametrize("n_rows,n_cols,k", [(3, 1, 1), (5, 63, 63), (4, 333, 128), (2, 4099, 128), (2, 1500, 1024)])
def test_topk_rows_matches_torch_topk(n_rows, n_cols, k):
    x = distinct_rows(n_rows, n_cols, seed=n_cols + k).to(DEV)
    val, idx = topk_guarded(x, k)
    rv, ri = torch.topk(x, k, dim=1)
    assert torch.equal(val, rv)
    assert torch.equal(idx.long(), ri)


def test_topk_rows_transposed_strides():
    buf = distinct_rows(70, 333, seed=5).T.contiguous().to(DEV)      # a (333, 70) buffer whose COLUMNS are the rows to select from
    xt = buf.T                                                       # (70, 333) behind strides (1, 70): no transposed copy is made
    assert buf.shape == (333, 70) and xt.stride() == (1, 70)
    val, idx = topk_guarded(xt, 50)
    rv, ri = torch.topk(xt, 50, dim=1)
    assert torch.equal(val, rv) and torch.equal(idx.long(), ri)


def test_topk_rows_zeros_infinities_and_negatives():
    row = [-0.0, 0.0, float("-inf"), -1.5, 0.0, -0.0, float("-inf"), -2.0, 3.0, -1.5, -1e-30, 1e-30]
    x = torch.tensor([row, row[::-1]], dtype=torch.float32, device=DEV)
    for k in (len(row), 4, 1, 7):
        val, idx = topk_guarded(x, k)
        rv, _ = torch.topk(x, k, dim=1)
        assert torch.equal(val, rv)                            # -0.0 == +0.0 under ==
        for r in range(2):
            want = stable_order(x[r].cpu().tolist())[:k]
            assert idx[r].tolist() == want, (k, r, idx[r].tolist(), want)
            assert torch.equal(val[r].view(torch.int32), x[r][idx[r].long()].view(torch.int32))     # the input's own bits


def test_topk_rows_planted_ties():
    g = torch.Generator().manual_seed(9)
    x = distinct_rows(3, 333, seed=9)
    for r in range(3):                                         # groups of equal values, one of them straddling the k-th position
        cols = torch.randperm(333, generator=g)
        x[r, cols[:40]] = 1.0 + 0.01 * r
        x[r, cols[40:45]] = 2.5
        x[r, cols[45:200]] = float(torch.topk(x[r], 128).values[-1])
    x = x.to(DEV)
    val, idx = topk_guarded(x, 128)
    rv, _ = torch.topk(x, 128, dim=1)
    assert torch.equal(val, rv)
    for r in range(3):
        assert idx[r].tolist() == stable_order(x[r].cpu().tolist())[:128]


# ---- ivh_softmax_axis_f32 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv,nt", [(13, 29), (70, 333)])
def test_softmax_axis_four_uses(nv, nt):
    from internvideo_amd import ops
    g = torch.Generator().manual_seed(nv)
    s = (3.0 * torch.randn(nv, nt, generator=g)).to(DEV)
    dsl = torch.empty(nv, nt, device=DEV)
    dsl_t = torch.empty(nt, nv, device=DEV)
    ops.softmax_axis(s.T, mul_input=True, out=dsl.T)
    ops.softmax_axis(s, mul_input=True, out=dsl_t.T)
    cases = [("softmax(dim=1)", ops.softmax_axis(s), lambda z: z.softmax(dim=1)),
             (".T.softmax(dim=1)", ops.softmax_axis(s.T), lambda z: z.T.softmax(dim=1)),
             ("s * s.softmax(dim=0)", dsl, lambda z: z * z.softmax(dim=0)),
             ("s.T * s.T.softmax(dim=0)", dsl_t, lambda z: z.T * z.T.softmax(dim=0))]
    for name, got, expr in cases:
        ref64 = expr(s.double())
        e_torch, e_got = rel(expr(s), ref64), rel(got, ref64)
        print(f"{name} ({nv}, {nt}): kernel {e_got:.3e}, torch fp32 {e_torch:.3e}")
        assert got.shape == ref64.shape
        assert e_got <= 4 * e_torch, (name, e_got, e_torch)


# ---- ivh_rerank_lists / ivh_scatter_pair_scores ------------------------------------------------------------------------------------------------
def lists_numpy(idx_v2t, idx_t2v, v_begin, v_end):
    ptr, cand, flags = [0], [], []
    for i in range(v_begin, v_end):
        d = {}
        for j in idx_v2t[i]:
            d[int(j)] = d.get(int(j), 0) | 1
        for j in range(idx_t2v.shape[0]):
            if (idx_t2v[j] == i).any():
                d[j] = d.get(j, 0) | 2
        for j in sorted(d):
            cand.append(j); flags.append(d[j])
        ptr.append(len(cand))
    return np.array(ptr, dtype=np.int32), np.array(cand, dtype=np.int32), np.array(flags, dtype=np.uint8)


def check_lists_and_scatter(idx_v2t, idx_t2v, v_begin, v_end, transposed_target=False):
    from internvideo_amd import ops
    (nv, kv), (nt, kt) = idx_v2t.shape, idx_t2v.shape
    a, b = torch.from_numpy(idx_v2t).to(DEV), torch.from_numpy(idx_t2v).to(DEV)
    ptr_, cand, flags = ops.rerank_lists(a, b, v_begin, v_end)
    rp, rc, rf = lists_numpy(idx_v2t, idx_t2v, v_begin, v_end)
    assert cand.numel() == flags.numel() == (v_end - v_begin) * kv + nt * kt
    assert np.array_equal(ptr_.cpu().numpy(), rp)
    total = int(rp[-1])
    assert np.array_equal(cand[:total].cpu().numpy(), rc) and np.array_equal(flags[:total].cpu().numpy(), rf)
    g = torch.Generator().manual_seed(nv * 1000 + nt)
    scores = torch.randn(cand.numel(), generator=g).to(DEV)
    prior_v = torch.randn(nv, nt, generator=g)
    prior_t = torch.randn(nt, nv, generator=g)
    x_v2t = prior_v.to(DEV)
    x_t2v = prior_t.T.contiguous().to(DEV).T if transposed_target else prior_t.to(DEV)      # column-major target: same values, other strides
    ops.scatter_pair_scores(ptr_, cand, flags, scores, v_begin, x_v2t, x_t2v)
    want_v, want_t, sc = prior_v.numpy().copy(), prior_t.numpy().copy(), scores.cpu().numpy()
    for n in range(v_end - v_begin):
        for e in range(rp[n], rp[n + 1]):
            if rf[e] & 1:
                want_v[v_begin + n, rc[e]] = sc[e]
            if rf[e] & 2:
                want_t[rc[e], v_begin + n] = sc[e]
    assert np.array_equal(x_v2t.cpu().numpy(), want_v)           # candidates hold their score, everything else its prior contents
    assert np.array_equal(x_t2v.cpu().numpy(), want_t)


def random_topk_indices(nv, nt, kv, kt, seed):
    rng = np.random.default_rng(seed)
    idx_v2t = np.stack([rng.permutation(nt)[:kv] for _ in range(nv)]).astype(np.int32)
    idx_t2v = np.stack([rng.permutation(nv)[:kt] for _ in range(nt)]).astype(np.int32)
    return idx_v2t, idx_t2v


@pytest.mark.parametrize("nv,nt,kv,kt", [(13, 29, 5, 5), (7, 300, 128, 3), (1, 1, 1, 1)])
def test_rerank_lists_and_scatter_match_numpy(nv, nt, kv, kt):
    a, b = random_topk_indices(nv, nt, kv, kt, seed=nv + nt)
    check_lists_and_scatter(a, b, 0, nv, transposed_target=(nt == 300))


def test_rerank_lists_every_text_chooses_one_video():
    a, b = random_topk_indices(13, 29, 5, 1, seed=3)
    b[:, 0] = 2                                                 # the longest possible list for video 2, no t2v contribution anywhere else
    check_lists_and_scatter(a, b, 0, 13)


def test_rerank_lists_sub_range():
    a, b = random_topk_indices(13, 29, 5, 5, seed=4)
    check_lists_and_scatter(a, b, 3, 9)
    check_lists_and_scatter(a, b, 12, 13, transposed_target=True)


# ---- ivh_retrieval_ranks / itm_eval ---------------------------------------------------------------------------------------------------------------
def numpy_ranks(scores, gt_ptr, gt_idx):
    out = np.empty(scores.shape[0], dtype=np.int32)
    for r in range(scores.shape[0]):
        row, best = scores[r], scores.shape[1]
        for g in gt_idx[gt_ptr[r]:gt_ptr[r + 1]]:
            best = min(best, int((row > row[g]).sum() + (row[:g] == row[g]).sum()))
        out[r] = best
    return out


def ground_truth(gold):
    ptr = gold["img2txt_ptr"]
    return ({j: int(v) for j, v in enumerate(gold["txt2img"])},
            {i: list(range(int(ptr[i]), int(ptr[i + 1]))) for i in range(len(ptr) - 1)})


def metric_dict(gold, key):
    return {str(k): float(v) for k, v in zip(gold["metric_keys"], gold[key])}


@pytest.mark.parametrize("n_cols", [29, 333])
def test_retrieval_ranks_matches_the_rule(n_cols):
    from internvideo_amd import ops
    x = distinct_rows(6, n_cols, seed=n_cols)
    x[4, ::3] = x[4, 0]                                         # planted ties: lower columns first
    x[5, :] = 0.5
    gts = [[0], [n_cols - 1], [3, n_cols - 1, 0], [n_cols // 2], [6, 9], [7]]          # first column, last column, lists
    ptr = np.cumsum([0] + [len(g) for g in gts]).astype(np.int32)
    idx = np.concatenate(gts).astype(np.int32)
    want = numpy_ranks(x.numpy(), ptr, idx)
    got = ops.retrieval_ranks(x.to(DEV), torch.from_numpy(ptr).to(DEV), torch.from_numpy(idx).to(DEV))
    assert got.cpu().numpy().tolist() == want.tolist()
    assert want[5] == 7
    # argsort-based ranks of the reference on the tie-free rows
    for r in range(4):
        order = np.argsort(x[r].numpy())[::-1]
        assert want[r] == min(int(np.where(order == g)[0][0]) for g in gts[r])
    xt = x.T.contiguous().to(DEV).T                             # column-major scores
    assert ops.retrieval_ranks(xt, torch.from_numpy(ptr).to(DEV), torch.from_numpy(idx).to(DEV)).cpu().numpy().tolist() == want.tolist()


@pytest.mark.parametrize("k_test", [29, 5])
def test_itm_eval_equals_the_reference_dicts(gold, k_test):
    from internvideo_amd import retrieval as Rv
    txt2img, img2txt = ground_truth(gold)
    for name, a, b in (("sim", "i2t_sim", "t2i_sim"), ("dsl", "i2t_dsl", "t2i_dsl"), ("match", "i2t_match", "t2i_match")):
        got = Rv.itm_eval(gold[f"k{k_test}:{a}"], gold[f"k{k_test}:{b}"], txt2img, img2txt)
        assert got == metric_dict(gold, f"k{k_test}:metrics_{name}"), (name, got)


# ---- cross-attention against shared encoder states ------------------------------------------------------------------------------------------------
def native_bert(encoder_width=None):
    from internvideo_amd import xbert
    bcfg = O.named_bert_config("bert_tiny")
    if encoder_width is not None:
        bcfg = dataclasses.replace(bcfg, encoder_width=encoder_width)
    pc = xbert.BertConfig(vocab_size=bcfg.vocab_size, hidden_size=bcfg.hidden_size, num_hidden_layers=bcfg.num_hidden_layers,
                          num_attention_heads=bcfg.num_attention_heads, intermediate_size=bcfg.intermediate_size,
                          max_position_embeddings=bcfg.max_position_embeddings, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                          fusion_layer=bcfg.fusion_layer, encoder_width=bcfg.encoder_width)
    m = xbert.BertForMaskedLM(pc)
    m.load_state_dict(O.synthetic_bert_params(bcfg, seed=0), strict=False)
    return m.to(DEV).eval(), bcfg


def test_shared_cross_attention_is_bitwise_the_expanded_pass(gold):
    bert, _ = native_bert()
    text = torch.from_numpy(gold["text_feats"][:7]).to(DEV)
    atts = torch.from_numpy(gold["text_atts"][:7]).to(DEV)
    video = torch.from_numpy(gold["media_feats"][4]).to(DEV)                 # (1, 9, 176)
    with torch.no_grad():
        shared = bert.bert(encoder_embeds=text, attention_mask=atts, encoder_hidden_states=video, encoder_attention_mask=None,
                           return_dict=True, mode="fusion").last_hidden_state
        atts2 = torch.from_numpy(gold["text_atts"][:7]).to(DEV)
        expanded = bert.bert(encoder_embeds=text, attention_mask=atts2, encoder_hidden_states=video.expand(7, -1, -1).contiguous(),
                             encoder_attention_mask=None, return_dict=True, mode="fusion").last_hidden_state
    assert shared.shape == expanded.shape == (7, 12, 128)
    assert torch.equal(shared.view(torch.int16), expanded.view(torch.int16))
    from internvideo_amd.lib import InternVideoHipError
    with pytest.raises(InternVideoHipError, match="inference"):              # a backward could follow: refused
        bert.bert(encoder_embeds=text, attention_mask=atts, encoder_hidden_states=video, return_dict=True, mode="fusion")


# ---- rerank_and_score against the reference --------------------------------------------------------------------------------------------------------
class Heads(torch.nn.Module):
    """what `rerank_and_score` reads of the model: the two projections, the matching head, the fusion tower"""

    def __init__(self, gold, bert):
        super().__init__()
        self.text_encoder = bert
        for name, key in (("vision_proj", "vision"), ("text_proj", "text"), ("itm_head", "itm")):
            w, b = torch.from_numpy(gold[f"head_{key}_w"]), torch.from_numpy(gold[f"head_{key}_b"])
            lin = torch.nn.Linear(w.shape[1], w.shape[0])
            with torch.no_grad():
                lin.weight.copy_(w); lin.bias.copy_(b)
            setattr(self, name, lin)

    def get_text_encoder(self):
        return self.text_encoder.bert


@pytest.fixture(scope="module")
def scored(gold):
    """the fixture's features through `rerank_and_score` once per configuration, shared by the tests below (never modified)"""
    from internvideo_amd import retrieval as Rv
    bert, _ = native_bert()
    model = Heads(gold, bert).to(DEV).eval()
    feats = (torch.from_numpy(gold["text_feats"]).to(DEV), torch.from_numpy(gold["text_atts"]).to(DEV),
             torch.from_numpy(gold["media_feats"]).to(DEV), torch.from_numpy(gold["pooled_media_feats"]).to(DEV))

    def run(k_test, **kw):
        cfg = dict(evaluation=dict(k_test=k_test, eval_frame_ensemble="concat", eval_offload=False), deep_fusion=False)
        return Rv.rerank_and_score(model, *feats, cfg, **kw)
    out = {"k29": run(29), "k5": run(5), "k5_raw": run(5, merge=False),
           "k5_r0": run(5, rank=0, world_size=2, merge=False), "k5_r1": run(5, rank=1, world_size=2, merge=False)}
    out["k29_np"], out["k5_np"] = Rv.softmax_outputs(out["k29"]), Rv.softmax_outputs(out["k5"])
    return out


def test_rerank_and_score_all_pairs_matches_the_reference(gold, scored):
    raw, outs = scored["k29"], scored["k29_np"]
    bound = 2 * float(gold["bf16_err"])
    e_sim = max(float((raw[2].cpu() - torch.from_numpy(gold["sim_v2t"])).abs().max()), float((raw[3].cpu() - torch.from_numpy(gold["sim_t2v"])).abs().max()))
    e_match = [rel(outs[i], gold["k29:" + OUT_NAMES[i]]) for i in range(2)]
    print(f"sims max abs err {e_sim:.3e} (bound 1e-4); match rel l2 {e_match[0]:.3e} / {e_match[1]:.3e} (bound {bound:.3e})")
    assert e_sim < 1e-4
    assert e_match[0] < bound and e_match[1] < bound
    for i in range(2, 6):
        assert outs[i].dtype == np.float32 and outs[i].shape == gold["k29:" + OUT_NAMES[i]].shape
        assert rel(outs[i], gold["k29:" + OUT_NAMES[i]]) < 1e-4, OUT_NAMES[i]
    assert bool((raw[0] != -100.0).all()) and bool((raw[1] != -100.0).all())          # every pair was re-ranked


def test_rerank_and_score_top5_matches_the_reference(gold, scored):
    from internvideo_amd import retrieval as Rv
    raw, outs = scored["k5"], scored["k5_np"]
    bound = 2 * float(gold["bf16_err"])
    for i in range(2):
        ref5, ref29 = gold["k5:" + OUT_NAMES[i]], gold["k29:" + OUT_NAMES[i]].astype(np.float64)
        sel_ref = ref5 > 1e-20                                  # the reference's fill entries are softmax(-100 - max) ~ 1e-44
        assert (sel_ref.sum(1) == 5).all()
        mine = raw[i].cpu().numpy()
        assert np.array_equal(mine != -100.0, sel_ref), OUT_NAMES[i]              # the top-k set of every row; everything else is exactly -100.0
        # the selected scores against the reference's all-pairs matrix: softmax over the selected columns of both
        got = torch.from_numpy(np.where(sel_ref, mine, -np.inf)).double().softmax(dim=1).numpy()
        want = np.where(sel_ref, ref29, 0.0)
        want = want / want.sum(1, keepdims=True)
        e = rel(got, want)
        print(f"{OUT_NAMES[i]}: selected scores rel l2 {e:.3e} (bound {bound:.3e})")
        assert e < bound
        assert rel(outs[i], ref5) < bound
    txt2img, img2txt = ground_truth(gold)
    for name, a, b in (("match", 0, 1), ("sim", 2, 3), ("dsl", 4, 5)):
        got = Rv.itm_eval(outs[a], outs[b], txt2img, img2txt)
        assert got == metric_dict(gold, "k5:metrics_" + name), (name, got)


def test_rerank_and_score_rank_split_is_bitwise(scored):
    full, r0, r1 = scored["k5_raw"], scored["k5_r0"], scored["k5_r1"]
    for i in range(2):
        assert bool(torch.isinf(r0[i]).any()) and bool(torch.isinf(r1[i]).any())          # each rank holds a part
        merged = torch.maximum(r0[i], r1[i])
        assert torch.equal(merged.view(torch.int32), full[i].view(torch.int32))
        done = merged.masked_fill(merged == float("-inf"), -100.0)
        assert torch.equal(done.view(torch.int32), scored["k5"][i].view(torch.int32))
    # videos 0 .. 6 belong to rank 0, 7 .. 12 to rank 1 (step = 13 // 2 + 1): rank 0 wrote nothing into the rows / columns of rank 1's videos
    assert bool(torch.isinf(r0[0][7:]).all()) and bool(torch.isinf(r0[1][:, 7:]).all())
    assert bool(torch.isinf(r1[0][:7]).all()) and bool(torch.isinf(r1[1][:, :7]).all())


def test_rerank_chunks_and_offload_do_not_change_scores(gold, scored):
    """a long candidate list cut into chunks, and token features kept on the host, give the same scores: every text row is computed on its own"""
    from internvideo_amd import retrieval as Rv
    bert, _ = native_bert()
    model = Heads(gold, bert).to(DEV).eval()
    cfg = dict(evaluation=dict(k_test=5, eval_frame_ensemble="concat", eval_offload=True, rerank_chunk_rows=3), deep_fusion=False)
    raw = Rv.rerank_and_score(model, torch.from_numpy(gold["text_feats"]).to(DEV), torch.from_numpy(gold["text_atts"]).to(DEV),
                              torch.from_numpy(gold["media_feats"]), torch.from_numpy(gold["pooled_media_feats"]), cfg)
    for i in range(2):
        assert torch.equal(raw[i] == -100.0, scored["k5"][i] == -100.0)
        assert rel(raw[i], scored["k5"][i]) < 2 * float(gold["bf16_err"])


# ---- evaluation end to end on the assembled stage-2 model ---------------------------------------------------------------------------------------
class TextInput:
    def __init__(self, ids, mask):
        self.input_ids, self.attention_mask = ids, mask

    def to(self, device):
        return TextInput(self.input_ids.to(device), self.attention_mask.to(device))


class Loader(list):
    pass


def tiny_stage2_eval():
    """bert_tiny + the mm88 vision tower (the smallest configuration the stage-2 tests use), 5 videos and 7 captions"""
    from internvideo_amd import mm_internvideo2 as mm
    from internvideo_amd.stage2 import InternVideo2_Stage2_visual
    scfg = O.named_config("mm88")
    bert, bcfg = native_bert(encoder_width=scfg.embed_dim)
    torch.manual_seed(0)
    vision = mm.PretrainInternVideo2(img_size=scfg.img_size, embed_dim=scfg.embed_dim, depth=scfg.depth, num_heads=scfg.num_heads,
                                     mlp_ratio=scfg.mlp_ratio, num_frames=scfg.num_frames, drop_path_rate=0.0,
                                     attn_pool_num_heads=scfg.attn_pool_num_heads, clip_embed_dim=scfg.clip_embed_dim,
                                     clip_teacher_embed_dim=scfg.clip_teacher_embed_dim, clip_teacher_final_dim=scfg.clip_teacher_final_dim,
                                     clip_return_layer=scfg.clip_return_layer, sep_image_video_pos_embed=scfg.sep_image_video_pos_embed)
    vision.load_state_dict(O.synthetic_params(scfg, seed=1), strict=True)
    config = dict(model=dict(model_cls="InternVideo2_Stage2_visual",
                             vision_encoder=dict(clip_embed_dim=scfg.clip_embed_dim, img_size=scfg.img_size, num_frames=scfg.num_frames,
                                                 tubelet_size=1, patch_size=scfg.patch_size, video_mask_type="random", video_mask_ratio=0.5,
                                                 image_mask_type="random", image_mask_ratio=0.5, only_mask=True),
                             text_encoder=dict(d_model=bcfg.hidden_size), embed_dim=32, temp=0.07),
                  criterion=dict(loss_weight=dict(uta=0.0, vtc=1.0, vtm=1.0, mlm=1.0), vtm_hard_neg=True, mlm_masking_prob=0.5),
                  evaluation=dict(k_test=3, eval_frame_ensemble="concat", eval_offload=False), deep_fusion=False, use_half_precision=False)
    tok_ids = SimpleNamespace(pad_token_id=bcfg.pad_token_id, cls_token_id=bcfg.cls_token_id, mask_token_id=bcfg.mask_token_id)
    model = InternVideo2_Stage2_visual(config, tok_ids, True, vision_encoder=vision, text_encoder=bert).to(DEV).eval()
    nv, nt, L = 5, 7, 12
    ids, mask = O.synthetic_text_batch(bcfg, nt, L, seed=2)
    table = {f"caption {j}": (torch.from_numpy(ids[j]), torch.from_numpy(mask[j])) for j in range(nt)}

    def tokenizer(text, padding=None, truncation=None, max_length=None, return_tensors=None):
        assert padding == "max_length" and truncation and max_length == L and return_tensors == "pt"
        return TextInput(torch.stack([table[t][0] for t in text]), torch.stack([table[t][1] for t in text]))
    g = torch.Generator().manual_seed(4)
    videos = torch.randn(nv, scfg.num_frames, 3, scfg.img_size, scfg.img_size, generator=g)
    loader = Loader([(videos[:3], [0, 1, 2]), (videos[3:], [3, 4])])
    loader.dataset = SimpleNamespace(media_type="video", text=list(table), max_txt_l=L, image=list(range(nv)),
                                     txt2img={j: j % nv for j in range(nt)}, img2txt={i: [j for j in range(nt) if j % nv == i] for i in range(nv)})
    return model, loader, tokenizer, config


def test_evaluation_end_to_end_equals_rerank_and_score_on_its_features():
    from internvideo_amd import retrieval as Rv
    model, loader, tokenizer, config = tiny_stage2_eval()
    outs = Rv.evaluation(model, loader, tokenizer, DEV, config)
    with torch.no_grad():
        tf, ta = Rv.extract_text_feats(loader.dataset.text, loader.dataset.max_txt_l, tokenizer, model, DEV)
        vf, pf = Rv.extract_vision_feats(loader, model, DEV, config)
    assert tf.shape[:2] == (7, 12) and ta.shape == (7, 12) and vf.dim() == 4 and vf.shape[:2] == (5, 1) and pf.shape[:2] == (5, 1)
    want = Rv.softmax_outputs(Rv.rerank_and_score(model, tf, ta, vf, pf, config))
    shapes = [(5, 7), (7, 5)] * 3
    for o, w, shp in zip(outs, want, shapes):
        assert isinstance(o, np.ndarray) and o.dtype == np.float32 and o.shape == shp       # the reference's `.cpu().float().numpy()`
        assert np.array_equal(o, w)
        assert np.allclose(o.sum(1), 1.0, atol=1e-5)
    assert ((outs[0] > 1e-20).sum(1) >= 3).all() and ((outs[1] > 1e-20).sum(1) >= 3).all()    # k_test = 3 candidates per query at least
    res = Rv.evaluation_wrapper(model, loader, tokenizer, DEV, config, prefix="tiny")
    assert sorted(res) == ["tiny_dsl", "tiny_match", "tiny_sim"]
    assert all(sorted(v) == sorted(["v2t_r1", "v2t_r5", "v2t_r10", "v2t_r_mean", "t2v_r1", "t2v_r5", "t2v_r10", "t2v_r_mean", "r_mean"]) for v in res.values())
    model.itm_head = None                                                             # a model without a matching head: sims only
    outs = Rv.evaluation(model, loader, tokenizer, DEV, config)
    assert outs[0] is None and outs[1] is None and all(np.array_equal(a, b) for a, b in zip(outs[2:], want[2:]))
