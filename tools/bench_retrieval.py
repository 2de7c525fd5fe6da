"""Stage-2 retrieval evaluation, the part after feature extraction, at the MSRVTT-1k-A shape of the 1B model: 1000 videos of 1025 tokens x 1408,
1000 captions of 32 tokens x 1024, the five fusion layers of BERT-large, k_test = 128.  GPU box only.

    python tools/bench_retrieval.py [--nv 1000] [--nt 1000] [--k 128] [--reps 2] [--ref-queries 0]

Two forms, alternated in one process on the same synthetic features (random-init weights, random features; the JSON line reports how many
distinct pairs the two top-k directions ask for):
  (a) internvideo_amd.retrieval.rerank_and_score: every (video, text) pair once, grouped by video, the video's tokens given once per pass;
  (b) the loop structure of the reference (multi_modality/tasks/retrieval_utils.py:396-566) on the SAME native modules: per video the tokens
      repeated 32 times in front of batches of 32 texts, then per text batches of 32 gathered videos -- the two directions kept separate.
Times are host clocks around work that ends in a device synchronise; every shape of the timed windows is warmed up first.
--ref-queries N (0 = all) runs (b) over the first N videos and the first N texts only and scales its time by the number of queries: every
query of (b) does the same work (k / 32 passes over 32 x 1025 video rows), so the scaling is exact up to launch jitter; the JSON line says when
it was used.  The scores of the two forms are compared on the rows (b) computed.  One JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from internvideo_amd import ops, retrieval as Rv, xbert  # noqa: E402
from internvideo_amd.stage2 import get_sim  # noqa: E402

DEV = "cuda"


class Model(torch.nn.Module):
    def __init__(self, bert, clip_dim, text_width, embed_dim):
        super().__init__()
        self.text_encoder = bert
        self.vision_proj = torch.nn.Linear(clip_dim, embed_dim)
        self.text_proj = torch.nn.Linear(text_width, embed_dim)
        self.itm_head = torch.nn.Linear(text_width, 2)

    def get_text_encoder(self):
        return self.text_encoder


@torch.no_grad()
def reference_structure(model, text_feats, text_atts, lengths, media_feats, pooled, k, n_queries):
    """retrieval_utils.py:366-566 with the native modules: same selection, same batches of 32, the video repeated / gathered per batch"""
    nv, nt = media_feats.shape[0], text_feats.shape[0]
    enc_model = model.get_text_encoder()
    v_proj = Rv._linear_f32(pooled.reshape(nv, -1), model.vision_proj).reshape(nv, 1, -1)
    t_proj = Rv._linear_f32(text_feats[:, 0], model.text_proj)
    sim = get_sim(v_proj, t_proj)[0].contiguous()
    _, idx_v2t = ops.topk_rows(sim, min(nt, k))
    _, idx_t2v = ops.topk_rows(sim.T, min(nv, k))
    x_v2t = torch.full((nv, nt), Rv.FILL, device=DEV)
    x_t2v = torch.full((nt, nv), Rv.FILL, device=DEV)
    bs = 32

    def fuse(t, a, n, enc):
        a._ivh_kv_len = n
        out = enc_model(encoder_embeds=t, attention_mask=a, encoder_hidden_states=enc, encoder_attention_mask=None, return_dict=True, mode="fusion")
        return out.last_hidden_state[:, 0]
    for i in range(min(nv, n_queries)):
        topk_idx = idx_v2t[i].long()
        enc = media_feats[i, 0].repeat(bs, 1, 1)
        embeds = []
        for j in range(0, topk_idx.numel(), bs):
            sel = topk_idx[j:j + bs]
            embeds.append(fuse(text_feats[sel], text_atts[sel], lengths[sel].contiguous(), enc[:sel.numel()]))
        x_v2t[i, topk_idx] = Rv._linear_f32(torch.cat(embeds, dim=0), model.itm_head)[:, 1]
    for j in range(min(nt, n_queries)):
        topk_idx = idx_t2v[j].long()
        embeds = []
        for b in range(0, topk_idx.numel(), bs):
            sel = topk_idx[b:b + bs]
            n = sel.numel()
            embeds.append(fuse(text_feats[j].repeat(n, 1, 1), text_atts[j].repeat(n, 1), lengths[j].repeat(n).contiguous(), media_feats[sel, 0]))
        x_t2v[j, topk_idx] = Rv._linear_f32(torch.cat(embeds, dim=0), model.itm_head)[:, 1]
    return x_v2t, x_t2v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nv", type=int, default=1000)
    ap.add_argument("--nt", type=int, default=1000)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--ref-queries", type=int, default=0, help="time form (b) on the first N videos and N texts and scale (0 = all)")
    ap.add_argument("--tokens", type=int, default=1025)
    ap.add_argument("--text-len", type=int, default=32)
    ap.add_argument("--tiny", action="store_true", help="bert_tiny-sized tower (rehearsal of the script itself; not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_retrieval needs the GPU: there is no CPU path and no CPU figure")
    torch.manual_seed(0)
    if a.tiny:
        cfg = xbert.BertConfig(vocab_size=210, hidden_size=128, num_hidden_layers=4, num_attention_heads=2, intermediate_size=256,
                               max_position_embeddings=40, fusion_layer=2, encoder_width=176, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        clip_dim = 64
    else:
        cfg = xbert.BertConfig(fusion_layer=19, encoder_width=1408)                 # config_bert_large.json + the 1B stage-2 config
        clip_dim = 768
    with torch.device(DEV):
        bert = xbert.BertModel(cfg)
        model = Model(bert, clip_dim, cfg.hidden_size, 512)
    model.eval()
    nv, nt = a.nv, a.nt
    g = torch.Generator(device=DEV).manual_seed(1)
    text_feats = torch.randn((nt, a.text_len, cfg.hidden_size), device=DEV, generator=g).bfloat16()
    lengths = torch.randint(4, a.text_len + 1, (nt,), device=DEV, generator=g, dtype=torch.int32)
    text_atts = (torch.arange(a.text_len, device=DEV)[None, :] < lengths[:, None]).long()
    media_feats = torch.randn((nv, 1, a.tokens, cfg.encoder_width), device=DEV, generator=g).bfloat16()
    pooled = torch.randn((nv, 1, clip_dim), device=DEV, generator=g)
    config = dict(evaluation=dict(k_test=a.k, eval_frame_ensemble="concat", eval_offload=False), deep_fusion=False)
    nq = a.ref_queries if a.ref_queries > 0 else max(nv, nt)

    def form_a(**kw):
        return Rv.rerank_and_score(model, text_feats, text_atts, media_feats, pooled, config, **kw)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    # warm-up: both forms on a few queries (every kernel and every GEMM shape class of the timed windows)
    form_a(rank=0, world_size=max(1, nv // 8), merge=False)
    reference_structure(model, text_feats, text_atts, lengths, media_feats, pooled, a.k, 4)
    ta, tb = [], []
    for _ in range(a.reps):
        t, out_a = timed(form_a)
        ta.append(t)
        t, out_b = timed(lambda: reference_structure(model, text_feats, text_atts, lengths, media_feats, pooled, a.k, nq))
        tb.append(t)
    scale = max(nv, nt) / min(nq, max(nv, nt))
    rows_v, rows_t = min(nv, nq), min(nt, nq)
    same_sel = bool(((out_a[0][:rows_v] != Rv.FILL) == (out_b[0][:rows_v] != Rv.FILL)).all()) and \
        bool(((out_a[1][:rows_t] != Rv.FILL) == (out_b[1][:rows_t] != Rv.FILL)).all())

    def rel_selected(x, y):                                     # over the re-ranked positions only: the fill entries agree trivially
        m = y != Rv.FILL
        return float((x[m] - y[m]).norm() / y[m].norm())
    err = max(rel_selected(out_a[0][:rows_v], out_b[0][:rows_v]), rel_selected(out_a[1][:rows_t], out_b[1][:rows_t]))
    _, idx_v2t = ops.topk_rows(out_a[2], min(nt, a.k))
    _, idx_t2v = ops.topk_rows(out_a[3], min(nv, a.k))
    ptr_, _, _ = ops.rerank_lists(idx_v2t, idx_t2v)
    pairs_a = int(ptr_[-1])
    print(json.dumps(dict(metric="seconds, stage-2 retrieval re-ranking after feature extraction (MSRVTT-1k-A shape, 1B model), 1 GPU",
                          nv=nv, nt=nt, k_test=a.k, video_tokens=a.tokens, text_len=a.text_len, fusion_layers=cfg.num_hidden_layers - cfg.fusion_layer,
                          grouped_s=[round(t, 3) for t in ta], reference_structure_s=[round(t * scale, 3) for t in tb],
                          reference_structure_measured_s=[round(t, 3) for t in tb], reference_queries_timed=min(nq, max(nv, nt)),
                          reference_time_scaled_by=round(scale, 3), speedup_min=round(min(tb) * scale / max(ta), 2),
                          speedup_max=round(max(tb) * scale / min(ta), 2), pairs_scored_grouped=pairs_a,
                          pair_passes_reference=nv * min(nt, a.k) + nt * min(nv, a.k), mean_list_len=round(pairs_a / nv, 1),
                          same_selected_positions=same_sel, scores_rel_l2_between_forms=round(err, 5), dtype="bf16 tower, fp32 similarities",
                          data="synthetic (random features, random-init weights)",
                          tiny_rehearsal=bool(a.tiny))), flush=True)


if __name__ == "__main__":
    main()
