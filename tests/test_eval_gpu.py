"""Validation / multi-view test on a real MI355X (csrc/evaluate.hip, internvideo_amd.evaluate) against what the REFERENCE's own final_test,
merge and compute_video produced on the same rows (tests/golden/eval_views.npz, make_golden_eval.py): the per-batch meters, the view table's
first-row-wins rule, finalize, the multi-rank merge and the whole path from a classifier to the merged accuracies.

Bars.  acc1 / acc5, pred, count, top-1 / top-5 flags, merge's two numbers: exact -- the generator asserted that no decision in the fixture
hangs on a tie or on a gap below 1e-4.  loss: 1e-6 relative to an fp64 recomputation from the same logits (fp32 logsumexp with expf / logf
over <= 710 terms, a double sum over <= 8 rows), and 2^-8 relative to the reference's value, which is rounded to bf16.  Mean
probabilities: 16 x the fixture's f32err (the reference's own fp32-vs-fp64 error on these rows) and never above 1e-5, a tenth of the
guaranteed decision gap.  All shapes are the fixture's: at most 8 rows per launch, 7 videos."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from internvideo_amd import evaluate as E, ops  # noqa: E402
from oracle import internvideo2_oracle as O  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
CASES = [f"V{V}:s{s}c3:" for V in (10, 174, 400, 710) for s in (4, 2)]
NAN = float("nan")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "eval_views.npz"))


def bits_to_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


_CASE = {}


def case(gold, pre):
    """the rows of a case and their fp64 recomputation, made once and shared (read-only)"""
    if pre in _CASE:
        return _CASE[pre]
    V = int(pre[1:pre.index(":")]); seg = int(pre[pre.index(":s") + 2]); crop = 3
    names = [str(n) for n in gold["video_names"]]
    ranks = []
    for k in (0, 1):
        r = pre + f"r{k}:"
        ranks.append(dict(logits=bits_to_f32(gold[r + "bits"]), labels=gold[r + "labels"], video=gold[r + "video"], chunk=gold[r + "chunk"],
                          split=gold[r + "split"], sizes=[int(n) for n in gold[r + "sizes"]], stats=gold[r + "stats"]))
    kept = {}                                                 # first in reading order: rank file by rank file, row by row
    for k, r in enumerate(ranks):
        for i in range(len(r["video"])):
            kept.setdefault((int(r["video"][i]), int(r["chunk"][i]) * crop + int(r["split"][i])), (k, i))
    p64 = np.zeros((len(names), V)); count = np.zeros(len(names), dtype=np.int64)
    for (v, w), (k, i) in sorted(kept.items()):
        x = ranks[k]["logits"][i].astype(np.float64)
        e = np.exp(x - x.max())
        p64[v] += e / e.sum(); count[v] += 1
    p64[count > 0] /= count[count > 0, None]
    for r in ranks:
        at, tot = 0, []
        for n in r["sizes"]:
            x = r["logits"][at:at + n].astype(np.float64); lab = r["labels"][at:at + n]
            m = x.max(axis=1, keepdims=True)
            tot.append(float(np.mean((m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0] - x[np.arange(n), lab])))
            at += n
        r["loss64"] = float(np.mean(tot))
    c = dict(V=V, nv=seg * crop, crop=crop, names=names, ranks=ranks, kept=kept, p64=p64, count=count, order=[int(v) for v in gold[pre + "names"]],
             pred=gold[pre + "pred"], top1=gold[pre + "top1"], top5=gold[pre + "top5"], label=gold[pre + "label"], merge=gold[pre + "merge"],
             f32err=float(gold[pre + "f32err"][0]), dups=gold[pre + "dups"])
    _CASE[pre] = c
    return c


def batches(c, k, dtype=BF16, pad=False):
    """the batches of rank k on the device -> (logits, labels, ids, chunk, split); pad: rows of pitch ceil8(V) + 8 whose columns >= V hold
    +inf, which no kernel may read"""
    r = c["ranks"][k]
    at = 0
    for n in r["sizes"]:
        x = torch.from_numpy(r["logits"][at:at + n]).to(DEV).to(dtype)
        if pad:
            buf = torch.full((n, (c["V"] + 7) // 8 * 8 + 8), float("inf"), dtype=dtype, device=DEV)
            buf[:, :c["V"]].copy_(x)
            x = buf[:, :c["V"]]
        yield (x, torch.from_numpy(r["labels"][at:at + n].astype(np.int64)), [c["names"][v] for v in r["video"][at:at + n]],
               torch.from_numpy(r["chunk"][at:at + n].astype(np.int64)), torch.from_numpy(r["split"][at:at + n].astype(np.int64)))
        at += n


def new_table(c, dtype=BF16):
    t = E.ViewTable(c["names"], c["nv"], c["V"], dtype=dtype, device=DEV, num_crop=c["crop"])
    t.table.fill_(NAN)                                        # a slot that was never written must not be read
    t.labels.fill_(-12345)
    return t


def fill(c, t, ranks=(0, 1), dtype=BF16, pad=False, meters=None):
    for k in ranks:
        for x, lab, ids, ch, sp in batches(c, k, dtype, pad):
            t.add(x, lab, ids, ch, sp, rank=k, meters=None if meters is None else meters[k])
    return t


def raw(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32) if t.dtype == F32 else t


class StubModel:
    """hands out the fixture's logits batch by batch, as the generator's stub did"""

    def __init__(self, outs):
        self.outs = list(outs)

    def eval(self):
        return self

    def __call__(self, clips):
        assert clips.dtype == BF16 and clips.is_cuda
        return self.outs.pop(0)


def loader(c, k):
    for x, lab, ids, ch, sp in batches(c, k):
        yield torch.zeros((x.shape[0], 1)), lab, ids, ch, sp


# ---- 1. the per-batch meters ---------------------------------------------------------------------------------------------------------------
def check_stats(c, k, stats, tag):
    ref = c["ranks"][k]["stats"]
    l64 = c["ranks"][k]["loss64"]
    print(f"{tag} rank {k}: loss {stats['loss']!r} fp64 {l64!r} (rel {abs(stats['loss'] - l64) / l64:.3g}) reference {ref[0]!r} "
          f"(rel {abs(stats['loss'] - ref[0]) / ref[0]:.3g}) acc1 {stats['acc1']!r} acc5 {stats['acc5']!r}")
    assert stats["acc1"] == ref[1] and stats["acc5"] == ref[2], (tag, stats, ref.tolist())
    assert abs(stats["loss"] - l64) <= 1e-6 * l64, (tag, stats["loss"], l64)
    assert abs(stats["loss"] - ref[0]) <= 2.0 ** -8 * ref[0], (tag, stats["loss"], ref[0])


@pytest.mark.parametrize("pre", CASES)
def test_validation_meters_match_the_reference(gold, pre):
    c = case(gold, pre)
    for k in (0, 1):
        outs = [x for x, *_ in batches(c, k)]
        stats = E.validation_one_epoch(loader(c, k), StubModel(outs), DEV, ds=True, bf16=True)
        check_stats(c, k, stats, pre + " validation_one_epoch bf16")


@pytest.mark.parametrize("pre", CASES)
@pytest.mark.parametrize("dtype,pad", [(BF16, True), (F32, False), (F32, True)])
def test_row_pass_dtypes_and_padded_rows(gold, pre, dtype, pad):
    """fp32 logits, and rows whose pitch exceeds V with +inf in the padding (V = 174 in rows of 184, V = 10 in rows of 24)"""
    c = case(gold, pre)
    for k in (0, 1):
        m = E.Meters(DEV)
        at = 0
        for x, lab, *_ in batches(c, k, dtype, pad):
            loss, rank = ops.eval_rows(x, lab.to(DEV), V=c["V"], meters=m.block)
            xr = c["ranks"][k]["logits"][at:at + x.shape[0]]; lr = c["ranks"][k]["labels"][at:at + x.shape[0]]
            want = [(int((r > r[l]).sum()) + int((r[:l] == r[l]).sum())) for r, l in zip(xr, lr)]
            assert rank.tolist() == want and bool(torch.isfinite(loss).all())
            at += x.shape[0]
        check_stats(c, k, m.read(), f"{pre} eval_rows {dtype} pad={pad}")
        tot, _ = m.totals()
        assert tot[3] == len(c["ranks"][k]["sizes"]) and tot[6] == at and tot[7] == 0
        assert tot[4] == sum(1 for r, l in zip(c["ranks"][k]["logits"], c["ranks"][k]["labels"]) if (r > r[l]).sum() == 0)


# ---- 2. finalize ------------------------------------------------------------------------------------------------------------------------------
def check_scores(c, out, probs, tag):
    out = out.cpu().numpy()
    for j, v in enumerate(c["order"]):                       # every video the reference scored, none excluded
        cnt, pred, rank, lab = (int(a) for a in out[v])
        assert cnt == c["count"][v] and pred == c["pred"][j] and lab == c["label"][j], (tag, v, out[v].tolist())
        assert int(rank < 1) == c["top1"][j] and int(rank < 5) == c["top5"][j], (tag, v, rank)
    absent = [v for v in range(len(c["names"])) if v not in c["order"]]
    assert absent and all(out[v].tolist() == [0, -1, -1, -1] for v in absent)
    if probs is not None:
        p = probs.cpu().numpy().astype(np.float64)
        dev = float(np.abs(p - c["p64"]).max())
        bound = min(16 * c["f32err"], 1e-5)
        print(f"{tag}: max |mean probability - fp64| = {dev:.3g} (bound {bound:.3g}, reference's own {c['f32err']:.3g})")
        assert dev <= bound, (tag, dev, bound)
        assert all(not p[v].any() for v in absent)


@pytest.mark.parametrize("pre", CASES)
@pytest.mark.parametrize("tdtype,ldtype,pad", [(BF16, BF16, False), (F32, BF16, True), (BF16, F32, True), (F32, F32, False)])
def test_finalize_matches_the_reference(gold, pre, tdtype, ldtype, pad):
    c = case(gold, pre)
    t = fill(c, new_table(c, tdtype), dtype=ldtype, pad=pad)
    n, V = len(c["names"]), c["V"]
    obuf = torch.full((n + 2, 4), 777, dtype=torch.int32, device=DEV)
    pbuf = torch.full((n + 2, V), NAN, dtype=F32, device=DEV)
    pbuf[0].fill_(-3.0); pbuf[-1].fill_(-3.0)                  # canaries in front and behind
    out, probs = ops.view_finalize(t.table, t.owner, t.labels, c["nv"], V, out=obuf[1:-1], probs=pbuf[1:-1])
    assert out.data_ptr() == obuf[1].data_ptr() and probs.data_ptr() == pbuf[1].data_ptr()
    assert bool((obuf[0] == 777).all()) and bool((obuf[-1] == 777).all()) and bool((pbuf[0] == -3.0).all()) and bool((pbuf[-1] == -3.0).all())
    assert bool(torch.isfinite(probs).all())                  # NaN from a slot nobody wrote would show here
    tag = f"{pre} table {tdtype} logits {ldtype} pad={pad}"
    check_scores(c, out, probs, tag)
    scores = t.finalize(want_probs=True)
    assert (scores.top1 * 100, scores.top5 * 100) == tuple(c["merge"].tolist()), (tag, scores.top1, scores.top5, c["merge"])
    assert torch.equal(scores.probs, probs) and scores.count.tolist() == c["count"].tolist()
    # the table itself: exactly the first row in reading order per slot, bit for bit; every other slot still holds its NaN fill
    tb = t.table.cpu(); own = t.owner.cpu(); labs = t.labels.cpu()
    for slot in range(n * c["nv"]):
        key = (slot // c["nv"], slot % c["nv"])
        if key in c["kept"]:
            k, i = c["kept"][key]
            want = torch.from_numpy(c["ranks"][k]["logits"][i]).to(tdtype)
            assert torch.equal(raw(tb[slot, :V]), raw(want)) and not tb[slot, V:].float().any(), (tag, key)
            assert labs[slot] == c["ranks"][k]["labels"][i]
            assert own[slot] >> 40 == k and (int(own[slot]) & ((1 << 40) - 1)) == i
        else:
            assert own[slot] == E.NO_OWNER and bool(torch.isnan(tb[slot].float()).all()) and labs[slot] == -12345, (tag, key)


def test_table_canaries_and_bad_rows(gold):
    """raw entry point on a table with canary slots in front and behind; a view index outside the table that only the device sees is skipped
    and counted"""
    c = case(gold, "V174:s2c3:")
    n_slots, ldt, V = len(c["names"]) * c["nv"], 176, c["V"]
    tbuf = torch.full((n_slots + 2, ldt), NAN, dtype=BF16, device=DEV); tbuf[0].fill_(5.0); tbuf[-1].fill_(5.0)
    obuf = torch.full((n_slots + 2,), E.NO_OWNER, dtype=torch.int64, device=DEV); obuf[0] = 42; obuf[-1] = 42
    lbuf = torch.full((n_slots + 2,), -7, dtype=torch.int32, device=DEV)
    x, lab, ids, ch, sp = next(batches(c, 0))
    video = torch.tensor([c["names"].index(i) for i in ids], dtype=torch.int32, device=DEV)
    view = (ch * 3 + sp).to(torch.int32).to(DEV)
    video[1] = len(c["names"]); view[2] = c["nv"]; view[3] = -1; video[4] = -1        # three bad rows and one meters-only row
    m = E.Meters(DEV)
    loss, rank = ops.eval_rows(x, lab.to(DEV), V=V, meters=m.block, video=video, view=view, seq_base=0, n_views=c["nv"], table=tbuf[1:-1],
                               owner=obuf[1:-1], table_label=lbuf[1:-1])
    assert (rank < 0).tolist() == [False, True, True, True, False]
    assert bool((tbuf[0] == 5.0).all()) and bool((tbuf[-1] == 5.0).all()) and obuf[0] == 42 and obuf[-1] == 42 and lbuf[0] == -7 and lbuf[-1] == -7
    written = (obuf[1:-1] != E.NO_OWNER).nonzero().flatten().tolist()
    assert written == [int(video[0]) * c["nv"] + int(view[0])]
    assert int(torch.isnan(tbuf[1:-1].float()).all(dim=1).sum()) == n_slots - 1
    tot, _ = m.totals()
    assert tot[7] == 3 and tot[6] == 5
    with pytest.raises(ValueError, match="3 rows"):
        E.Meters.stats(tot)
    t = new_table(c)
    with pytest.raises(ValueError, match="1 rows"):
        t.add(x, lab, ids, ch.to(DEV), torch.where(torch.arange(5) == 2, 3, sp).to(DEV))       # split 3 of 3 crops, on the device
        t.finalize()


# ---- 3. duplicates, determinism, world size ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", CASES)
def test_duplicates_keep_the_first_row_read(gold, pre):
    c = case(gold, pre)
    t = fill(c, new_table(c))
    V = c["V"]
    kinds = set()
    for rk, row, orig in c["dups"].tolist():
        r = c["ranks"][rk]
        key = (int(r["video"][row]), int(r["chunk"][row]) * c["crop"] + int(r["split"][row]))
        r0 = c["ranks"][0]
        assert key == (int(r0["video"][orig]), int(r0["chunk"][orig]) * c["crop"] + int(r0["split"][orig]))
        assert r["logits"][row].tobytes() != r0["logits"][orig].tobytes()       # the copy carries other logits: the bits tell which was kept
        slot = key[0] * c["nv"] + key[1]
        assert torch.equal(raw(t.table[slot, :V].cpu()), raw(torch.from_numpy(r0["logits"][orig]).to(BF16))), (pre, rk, row, orig)
        assert int(t.owner[slot]) == orig
        sizes = np.cumsum([0] + r["sizes"])
        same_batch = rk == 0 and np.searchsorted(sizes, row, "right") == np.searchsorted(sizes, orig, "right")
        kinds.add("rank" if rk == 1 else "batch" if same_batch else "batches")
    assert kinds == {"rank", "batch", "batches"}
    before = (t.table.clone(), t.owner.clone(), t.labels.clone())
    fill(c, t, ranks=(0,)); fill(c, t, ranks=(1,))            # the same batches once more: later sequence numbers, nothing moves
    assert torch.equal(raw(before[0]), raw(t.table)) and torch.equal(before[1], t.owner) and torch.equal(before[2], t.labels)


@pytest.mark.parametrize("pre", ["V10:s4c3:", "V710:s2c3:"])
def test_two_passes_are_bit_identical(gold, pre):
    c = case(gold, pre)
    res = []
    for _ in range(2):
        meters = [E.Meters(DEV), E.Meters(DEV)]
        t = fill(c, new_table(c), meters=meters)
        out, probs = ops.view_finalize(t.table, t.owner, t.labels, c["nv"], c["V"], want_probs=True)
        res.append((meters[0].block.clone(), meters[1].block.clone(), raw(t.table).clone(), t.owner.clone(), t.labels.clone(), out, probs.view(torch.int32)))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert int(res[0][0][3]) == len(c["ranks"][0]["sizes"])


@pytest.mark.parametrize("pre", CASES)
def test_result_does_not_depend_on_the_world_size(gold, pre):
    """two tables filled as rank 0 and rank 1, combined by the code path `finalize` runs under a process group (reduce_over_ranks) with the
    collectives replaced by a local minimum / add, against one table filled with all rows in rank-major order"""
    c = case(gold, pre)
    single = fill(c, new_table(c))
    a, b = fill(c, new_table(c), ranks=(0,)), fill(c, new_table(c), ranks=(1,))
    omin = torch.minimum(a.owner, b.owner)
    theirs = {}

    def reduce_b(t, op, what):
        if op == "min":
            t.copy_(omin)
        else:
            theirs[what] = t.clone()                          # rank 1's contribution to the sums

    def reduce_a(t, op, what):
        if op == "min":
            t.copy_(omin)
        else:
            t.add_(theirs[what])

    b.reduce_over_ranks(reduce_b, rank=1)
    a.reduce_over_ranks(reduce_a, rank=0)
    assert sorted(theirs) == ["bad", "labels", "table"]
    assert torch.equal(a.owner, single.owner)
    owned = single.owner != E.NO_OWNER
    assert torch.equal(raw(a.table)[owned], raw(single.table)[owned]) and torch.equal(a.labels[owned], single.labels[owned])
    assert not a.table[~owned].float().any() and not a.labels[~owned].any()                     # finite everywhere after the merge
    assert bool(((b.owner >> 40) == 1).sum() > 0) and not theirs["table"][(omin >> 40) != 1].float().any()
    o1, p1 = ops.view_finalize(a.table, a.owner, a.labels, c["nv"], c["V"], want_probs=True)
    o2, p2 = ops.view_finalize(single.table, single.owner, single.labels, c["nv"], c["V"], want_probs=True)
    assert torch.equal(o1, o2) and torch.equal(p1.view(torch.int32), p2.view(torch.int32))
    check_scores(c, o1, p1, pre + " two ranks merged")


# ---- 4. files and the whole path ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", ["V10:s4c3:", "V174:s2c3:", "V400:s4c3:"])
def test_final_test_files_and_merge_match_the_reference(gold, pre, tmp_path):
    """final_test on the fixture's rows writes the reference's rank files byte for byte (but for the first line), returns its stats, and
    merge on those files gives the reference's two numbers"""
    c = case(gold, pre)
    for k in (0, 1):
        outs = [x for x, *_ in batches(c, k)]
        stats = E.final_test(loader(c, k), StubModel(outs), DEV, str(tmp_path / f"{k}.txt"), ds=True, bf16=True)
        check_stats(c, k, stats, pre + " final_test")
        lines = open(tmp_path / f"{k}.txt").readlines()
        last = c["ranks"][k]["sizes"][-1]
        xr, lr = c["ranks"][k]["logits"][-last:], c["ranks"][k]["labels"][-last:]
        rk = np.array([int((r > r[l]).sum()) for r, l in zip(xr, lr)])
        assert lines[0] == "{}, {}\n".format(float((rk < 1).sum() * 100.0 / last), float((rk < 5).sum() * 100.0 / last))
        if pre + f"r{k}:text" in gold.files:
            assert "".join(lines[1:]).encode() == bytes(gold[pre + f"r{k}:text"])
    top1, top5, scores = E.merge(str(tmp_path), 2, return_scores=True)
    assert (top1, top5) == tuple(c["merge"].tolist())
    assert [scores.pred[i].item() for i in range(len(c["order"]))] == c["pred"].tolist()      # merge numbers the videos in the order it met them


def test_end_to_end_on_the_tiny_classifier(gold, tmp_path):
    """final_test over a three-batch loader on the `tiny88` classifier (10 classes) with forward_only on: files + table in one pass; merge on
    the files equals ViewTable.finalize on the same run; the forward-only logits agree with the ordinary no_grad forward to the reference's
    bf16 calibration (tests/golden/finetune_mixup.npz, step:*:bf16err:logits)"""
    from internvideo_amd import internvideo2 as FT
    cfg = O.named_config("tiny88")
    model = FT.InternVideo2(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio,
                            num_frames=cfg.num_frames, drop_path_rate=0.0, attn_pool_num_heads=cfg.attn_pool_num_heads,
                            clip_embed_dim=cfg.clip_embed_dim, num_classes=10)
    model.load_state_dict(O.synthetic_finetune_params(cfg, 10, seed=12), strict=True)
    model = model.to(DEV)
    names = ["clip_a", "clip_b", "clip_c", "never_seen"]
    g = torch.Generator().manual_seed(5)
    rows = [(v, w) for v in range(3) for w in range(6)]
    rows = [rows[i] for i in torch.randperm(len(rows), generator=g).tolist()]
    clips = torch.randn((len(rows), 3, cfg.num_frames, cfg.img_size, cfg.img_size), generator=g)
    labels = torch.tensor([3, 7, 1])

    def loader():
        at = 0
        for n in (5, 8, 5):
            part = rows[at:at + n]
            yield (clips[at:at + n], labels[[v for v, _ in part]], [names[v] for v, _ in part], torch.tensor([w // 3 for _, w in part]),
                   torch.tensor([w % 3 for _, w in part]))
            at += n

    table = E.ViewTable(names, 6, 10, device=DEV)
    stats = E.final_test(loader(), model, DEV, str(tmp_path / "0.txt"), ds=True, bf16=True, table=table)
    assert not hasattr(model, "frozen_prefix") and torch.is_grad_enabled()
    scores = table.finalize()
    top1, top5, merged = E.merge(str(tmp_path), 1, return_scores=True)
    assert (top1, top5) == (scores.top1 * 100, scores.top5 * 100)
    assert scores.count.tolist() == [6, 6, 6, 0] and scores.label.tolist() == [3, 7, 1, -1]
    first_seen = list(dict.fromkeys(v for v, _ in rows))
    assert merged.pred.tolist() == [int(scores.pred[v]) for v in first_seen] and merged.count.tolist() == [6, 6, 6]
    assert E.validation_one_epoch(loader(), model, DEV, ds=True, bf16=True) == stats
    # the forward-only pass against the ordinary no_grad forward (BlockStackFn)
    _, _, _, _, logits = E.read_rank_files(str(tmp_path), 1)[0]
    with torch.no_grad():
        plain = torch.cat([model(b[0].to(DEV).bfloat16()).float() for b in loader()]).cpu().numpy()
    cal = np.load(os.path.join(GOLDEN, "finetune_mixup.npz"))
    bound = min(float(cal["step:mixup:bf16err:logits"][0]), float(cal["step:cutmix:bf16err:logits"][0]))
    err = float(np.linalg.norm(logits.astype(np.float64) - plain) / np.linalg.norm(plain))
    print(f"forward_only vs no_grad BlockStackFn logits: rel-L2 {err:.3g} (bound {bound:.3g})")
    assert np.abs(plain).max() > 0.05 and err <= bound
