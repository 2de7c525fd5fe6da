"""Stage-2 zero-shot video<->text retrieval evaluation on the MI355X kernels.

Mirrors InternVideo2/multi_modality/tasks/retrieval_utils.py for the path an `InternVideo2_Stage2_visual` checkpoint is measured by
(`evaluation_wrapper` :173-223 -> `evaluation` :226-613 -> `itm_eval` :1243-1303): the same names, arguments and return values, so
tasks/pretrain.py and tasks/retrieval.py change one import.  Feature extraction runs the native towers (`encode_text`,
`encode_vision(test=True)`); everything after it is `rerank_and_score`:

  similarities    `vision_proj` / `text_proj` on the fp32 A B^T kernel (ivh_vtc_abt), then `get_sim` on the frame-level features
  dual softmax    ivh_softmax_axis_f32 through transposed strides (`s * s.softmax(dim=0)`, `s.T * s.T.softmax(dim=0)`)
  selection       ivh_topk_rows_f32 in both directions on the same buffer
  bookkeeping     ivh_rerank_lists: the (video, text) pairs both directions ask for, grouped by video, each pair once
  re-ranking      ONE fusion pass per video over its candidate texts (cut into chunks of `rerank_chunk_rows`), the video's tokens given
                  once (xbert.py: cross-attention against shared encoder states), `itm_head` on the [CLS] rows
  placement       ivh_scatter_pair_scores into both match matrices; ivh_retrieval_ranks for R@1 / R@5 / R@10

The reference scores the pair (video i, text j) once per direction that selects it: video -> text with video i repeated 32 times in
front of batches of 32 texts, text -> video with 128 different videos projected per text.  The score is the same function of
(video i, text j) in both directions, so here every pair is scored once, grouped by video, and each video's keys and values are
projected once per fusion layer and chunk.

Supported: `media_type == "video"`, `eval_frame_ensemble == "concat"`, one clip per video, no subtitles, no `deep_fusion`; anything
else raises NotImplementedError (the reference itself asserts against `deep_fusion` and several clips, :390).
"""
from __future__ import annotations

import logging

import numpy as np
import torch
import torch.distributed as dist

from . import ops
from .stage2 import _cfg, get_sim

logger = logging.getLogger(__name__)

FILL = -100.0                 # retrieval_utils.py:367 / :487: the score of a pair that was not re-ranked
DEFAULT_CHUNK_ROWS = 256      # texts per fusion pass (config.evaluation.rerank_chunk_rows)


# ---- feature extraction (retrieval_utils.py:18-87) ---------------------------------------------------------------------------------------
def extract_text_feats(texts, max_txt_l, tokenizer, model, device, return_ids=False):
    """:18-49 -> (text_feats (n, Lt, d), text_atts (n, Lt)[, text_ids])"""
    num_text = len(texts)
    text_bs = 256
    text_feats, text_atts, text_ids = [], [], []
    for i in range(0, num_text, text_bs):
        text = texts[i: min(num_text, i + text_bs)]
        text_input = tokenizer(text, padding="max_length", truncation=True, max_length=max_txt_l, return_tensors="pt").to(device)
        text_feats.append(model.encode_text(text_input)[0])
        text_atts.append(text_input.attention_mask)
        if return_ids:
            text_ids.append(text_input.input_ids)
    text_feats, text_atts = torch.cat(text_feats, dim=0), torch.cat(text_atts, dim=0)
    if return_ids:
        return text_feats, text_atts, torch.cat(text_ids, dim=0)
    return text_feats, text_atts


def _check_ensemble(config):
    ens = _cfg(config, "evaluation.eval_frame_ensemble", "concat")
    if ens != "concat":
        raise NotImplementedError(f"eval_frame_ensemble={ens!r}: only \"concat\" is implemented")


def extract_vision_feats(data_loader, model, device, config):
    """:51-87 -> (image_feats (n, 1, #frm*L, d), pooled_image_feats (n, 1, d)); `eval_offload` keeps both on the host.  The native tower
    reads fp32 or bf16 frames and computes in bf16 either way: `use_half_precision` uploads bf16 frames."""
    _check_ensemble(config)
    cast_dtype = torch.bfloat16 if _cfg(config, "use_half_precision", False) else None
    offload = bool(_cfg(config, "evaluation.eval_offload", False))
    image_feats_all, pooled_image_feats_all = [], []
    for image, _img_id in data_loader:
        image = image.to(device, dtype=cast_dtype, non_blocking=True)
        image_feat, pooled_image_feat = model.encode_vision(image, test=True)
        if pooled_image_feat.dim() == 2:
            pooled_image_feat = pooled_image_feat.unsqueeze(1)
        if image_feat.dim() == 4:
            image_feat = image_feat.reshape(image_feat.shape[0], -1, image_feat.shape[-1]).contiguous()      # "b t l c -> b (t l) c"
        image_feat = image_feat.unsqueeze(1)
        if offload:
            image_feat, pooled_image_feat = image_feat.cpu(), pooled_image_feat.cpu()
        image_feats_all.append(image_feat)
        pooled_image_feats_all.append(pooled_image_feat)
    return torch.cat(image_feats_all, dim=0), torch.cat(pooled_image_feats_all, dim=0)


# ---- everything after feature extraction (retrieval_utils.py:275-613) -----------------------------------------------------------------------
def _linear_f32(x: torch.Tensor, lin) -> torch.Tensor:
    """nn.Linear in fp32 on the A B^T kernel: the similarities decide which pairs are re-ranked, so the projections keep fp32"""
    y = ops.abt_f32(x.float().contiguous(), lin.weight.detach().float().contiguous())
    return y + lin.bias.detach().float() if lin.bias is not None else y


def rank_rows(n: int, rank: int, world_size: int):
    """:377-379: the rows rank `rank` of `world_size` owns -> (start, end), possibly empty"""
    step = n // world_size + 1
    start = rank * step
    return min(start, n), min(n, start + step)


def _check_supported(media_feats, config):
    if _cfg(config, "deep_fusion", False):
        raise NotImplementedError("deep_fusion evaluation is not implemented")
    _check_ensemble(config)
    if media_feats.dim() != 4:
        raise ValueError(f"media_feats must be (n, clips, tokens, d), got {tuple(media_feats.shape)}")
    if media_feats.shape[1] != 1:
        raise NotImplementedError(f"n_clip_per_video={media_feats.shape[1]}: one clip per video is implemented")


@torch.no_grad()
def rerank_and_score(model, text_feats, text_atts, media_feats, pooled_media_feats, config, rank=0, world_size=1, merge=True):
    """text_feats (nt, Lt, d) and text_atts (nt, Lt) in HBM; media_feats (nv, 1, Lv, dv) in HBM or on the host (`eval_offload`: one video's
    tokens are uploaded per pass); pooled_media_feats (nv, 1, dv).  -> the six RAW score matrices of :596-613 before their final softmax,
    fp32 in HBM: (v2t_match, t2v_match, v2t_sim, t2v_sim, v2t_dsl, t2v_dsl); the first two are None for a model without `itm_head`.
    Pairs that were not re-ranked hold -100.0.  This rank scores the videos `rank_rows(nv, rank, world_size)`; with torch.distributed
    initialised the match matrices are merged by all_reduce(MAX).  merge=False returns this rank's part with -inf everywhere else."""
    _check_supported(media_feats, config)
    nv, nt = media_feats.shape[0], text_feats.shape[0]
    dev = text_feats.device
    k_test = int(_cfg(config, "evaluation.k_test", 128))
    kv, kt = min(nt, k_test), min(nv, k_test)
    if max(kv, kt) > 1024:
        raise NotImplementedError(f"k_test={k_test}: the selection kernel holds up to 1024 candidates per row")
    chunk = int(_cfg(config, "evaluation.rerank_chunk_rows", DEFAULT_CHUNK_ROWS))
    if chunk < 1:
        raise ValueError("evaluation.rerank_chunk_rows must be positive")

    pooled = pooled_media_feats.to(dev)
    v_proj = _linear_f32(pooled.reshape(-1, pooled.shape[-1]), model.vision_proj).reshape(pooled.shape[0], pooled.shape[1], -1)
    t_proj = _linear_f32(text_feats[:, 0], model.text_proj)
    sim = get_sim(v_proj, t_proj)[0].contiguous()                     # (nv, nt); the text -> video direction is its transpose
    dsl_v2t = torch.empty((nv, nt), dtype=torch.float32, device=dev)  # s * s.softmax(dim=0)
    ops.softmax_axis(sim.T, mul_input=True, out=dsl_v2t.T)
    dsl_t2v = torch.empty((nt, nv), dtype=torch.float32, device=dev)  # s.T * s.T.softmax(dim=0)
    ops.softmax_axis(sim, mul_input=True, out=dsl_t2v.T)
    if not hasattr(model, "itm_head") or model.itm_head is None:
        return None, None, sim, sim.T, dsl_v2t, dsl_t2v

    use_dsl = bool(_cfg(config, "evaluation.use_dsl_for_match", False))               # :283-287
    _, idx_v2t = ops.topk_rows(dsl_v2t if use_dsl else sim, kv)
    _, idx_t2v = ops.topk_rows(dsl_t2v if use_dsl else sim.T, kt)
    x_v2t = torch.full((nv, nt), float("-inf"), dtype=torch.float32, device=dev)
    x_t2v = torch.full((nt, nv), float("-inf"), dtype=torch.float32, device=dev)
    v_begin, v_end = rank_rows(nv, int(rank), int(world_size))
    if v_end > v_begin:
        ptr_, cand, flags = ops.rerank_lists(idx_v2t, idx_t2v, v_begin, v_end)
        bounds = ptr_.tolist()                                        # the one host read: list lengths drive the loop
        total = bounds[-1]
        from .xbert import right_padded_lengths
        lengths = right_padded_lengths(text_atts, "attention_mask")
        text_encoder = model.get_text_encoder()
        cand64 = cand[:total].long()
        cls = torch.empty((total, text_feats.shape[-1]), dtype=torch.bfloat16, device=dev)        # the tower's output format
        for n in range(v_end - v_begin):
            lo, hi = bounds[n], bounds[n + 1]
            if hi == lo:
                continue
            enc = media_feats[v_begin + n, 0].to(dev, non_blocking=True).unsqueeze(0)              # (1, Lv, dv): given once
            for a in range(lo, hi, chunk):
                b = min(hi, a + chunk)
                sel = cand64[a:b]
                atts = text_atts[sel]
                atts._ivh_kv_len = None if lengths is None else lengths[sel].contiguous()          # rows of a checked mask
                out = text_encoder(encoder_embeds=text_feats[sel], attention_mask=atts, encoder_hidden_states=enc,
                                   encoder_attention_mask=None, return_dict=True, mode="fusion")
                cls[a:b] = out.last_hidden_state[:, 0]
        scores = torch.zeros((cand.numel(),), dtype=torch.float32, device=dev)
        if total:
            scores[:total] = _linear_f32(cls, model.itm_head)[:, 1]                                # :475 `match_head(itm_embeds)[:, 1]`
        ops.scatter_pair_scores(ptr_, cand, flags, scores, v_begin, x_v2t, x_t2v)
    if merge:
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(x_v2t, op=dist.ReduceOp.MAX)
            dist.all_reduce(x_t2v, op=dist.ReduceOp.MAX)
        x_v2t.masked_fill_(x_v2t == float("-inf"), FILL)
        x_t2v.masked_fill_(x_t2v == float("-inf"), FILL)
    return x_v2t, x_t2v, sim, sim.T, dsl_v2t, dsl_t2v


def softmax_outputs(raw):
    """:596-613: `.softmax(dim=1).cpu().float().numpy()` of every matrix of `rerank_and_score` (None stays None)"""
    return tuple(None if m is None else ops.softmax_axis(m).cpu().numpy() for m in raw)


@torch.no_grad()
def evaluation(model, data_loader, tokenizer, device, config):
    """:226-613 -> (i2t_match, t2i_match, i2t_sim, t2i_sim, i2t_dsl, t2i_dsl), softmaxed numpy fp32; the first two are None for a model
    without `itm_head`"""
    model.eval()
    dataset = data_loader.dataset
    media_type = dataset.media_type
    if media_type != "video":
        raise NotImplementedError(f"media_type={media_type!r}: video retrieval is implemented")
    if getattr(dataset, "use_subtitle", False):
        raise NotImplementedError("subtitle fusion (vs_fusion / vstm_head) is not implemented")
    if _cfg(config, "deep_fusion", False):
        raise NotImplementedError("deep_fusion evaluation is not implemented")
    _check_ensemble(config)
    text_feats, text_atts = extract_text_feats(dataset.text, dataset.max_txt_l, tokenizer, model, device)
    image_feats, pooled_image_feats = extract_vision_feats(data_loader, model, device, config)
    rank, world = (dist.get_rank(), dist.get_world_size()) if (dist.is_available() and dist.is_initialized()) else (0, 1)
    return softmax_outputs(rerank_and_score(model, text_feats, text_atts, image_feats, pooled_image_feats, config, rank, world))


# ---- metrics (retrieval_utils.py:1243-1303) ------------------------------------------------------------------------------------------------
def _gt_csr(gt, n_rows: int):
    """`img2txt` / `txt2img` (dict or sequence: row -> int or list of ints) -> (gt_ptr int32 [n_rows + 1], gt_idx int32)"""
    ptr_, idx = [0], []
    for r in range(n_rows):
        g = gt[r]
        idx.extend([int(g)] if isinstance(g, (int, np.integer)) else [int(i) for i in g])
        ptr_.append(len(idx))
    return np.asarray(ptr_, dtype=np.int32), np.asarray(idx, dtype=np.int32)


def _device_ranks(scores: np.ndarray, gt_ptr: np.ndarray, gt_idx: np.ndarray) -> np.ndarray:
    """best position of a ground-truth column in every row's descending order (ivh_retrieval_ranks)"""
    if gt_idx.size == 0:
        return np.full((scores.shape[0],), scores.shape[1], dtype=np.int32)
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cuda"
    s = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).to(dev)
    r = ops.retrieval_ranks(s, torch.from_numpy(gt_ptr).to(dev), torch.from_numpy(gt_idx).to(dev))
    return r.cpu().numpy()


def _recalls(ranks: np.ndarray):
    n = len(ranks)
    return tuple(100.0 * int((ranks < k).sum()) / n for k in (1, 5, 10))


def itm_eval(scores_i2t, scores_t2i, txt2img, img2txt):
    """:1243-1303: R@1 / R@5 / R@10 in both directions and their means, rounded to two decimals"""
    scores_i2t, scores_t2i = np.asarray(scores_i2t), np.asarray(scores_t2i)
    tr1, tr5, tr10 = _recalls(_device_ranks(scores_i2t, *_gt_csr(img2txt, scores_i2t.shape[0])))
    ir1, ir5, ir10 = _recalls(_device_ranks(scores_t2i, *_gt_csr(txt2img, scores_t2i.shape[0])))
    tr_mean = (tr1 + tr5 + tr10) / 3
    ir_mean = (ir1 + ir5 + ir10) / 3
    r_mean = (tr_mean + ir_mean) / 2
    eval_result = {"v2t_r1": tr1, "v2t_r5": tr5, "v2t_r10": tr10, "v2t_r_mean": tr_mean,
                   "t2v_r1": ir1, "t2v_r5": ir5, "t2v_r10": ir10, "t2v_r_mean": ir_mean, "r_mean": r_mean}
    return {k: round(v, 2) for k, v in eval_result.items()}


def mean_over_prompts(scores, n_prompts: int, axis: int):
    """:199-205: the text axis holds `n_prompts` consecutive prompts per caption; average them (axis 1 of a video x text matrix, axis 0 of
    a text x video matrix)"""
    if scores is None:
        return None
    if axis == 1:
        return scores.reshape((scores.shape[0], scores.shape[1] // n_prompts, n_prompts)).mean(axis=-1)
    return scores.reshape((scores.shape[0] // n_prompts, n_prompts, scores.shape[1])).mean(axis=1)


@torch.no_grad()
def evaluation_wrapper(model, data_loader, tokenizer, device, config, prefix=""):
    """:173-223 -> {prefix + "_sim": ..., prefix + "_dsl": ..., prefix + "_match"[" (use_dsl)"]: ...}, each an `itm_eval` dict"""
    model_cls = str(_cfg(config, "model.model_cls", "")).lower()
    for other in ("qformer", "blip", "clip", "coca"):
        if other in model_cls:
            raise NotImplementedError(f"model_cls {model_cls!r}: retrieval evaluation is implemented for InternVideo2_Stage2_visual")
    i2t_match, t2i_match, i2t_sim, t2i_sim, i2t_dsl, t2i_dsl = evaluation(model, data_loader, tokenizer, device, config)
    dataset = data_loader.dataset
    if hasattr(dataset, "num_prompts"):
        n = dataset.num_prompts
        logger.info(f"Using {n} prompts, we need reshape and mean!!!")
        i2t_match, i2t_sim, i2t_dsl = (mean_over_prompts(m, n, 1) for m in (i2t_match, i2t_sim, i2t_dsl))
        t2i_match, t2i_sim, t2i_dsl = (mean_over_prompts(m, n, 0) for m in (t2i_match, t2i_sim, t2i_dsl))
    score_pairs = [(prefix + "_sim", i2t_sim, t2i_sim), (prefix + "_dsl", i2t_dsl, t2i_dsl)]
    if i2t_match is not None:
        name = "_match (use_dsl)" if _cfg(config, "evaluation.use_dsl_for_match", False) else "_match"
        score_pairs.append((prefix + name, i2t_match, t2i_match))
    return {name: itm_eval(i2t, t2i, dataset.txt2img, dataset.img2txt) for name, i2t, t2i in score_pairs if i2t is not None}
