"""Validation and the multi-view test of the classifiers (InternVideo2/single_modality/engines/engine_for_finetuning.py:147-295, called
from run_finetuning.py / run_linear_probing.py with `--test_num_segment 4 --test_num_crop 3`): from a checkpoint to the reported
Acc@1 / Acc@5 without going back to the reference's loop.

    from internvideo_amd.evaluate import validation_one_epoch, final_test, merge, ViewTable
    stats = validation_one_epoch(val_loader, model, device, ds=True, bf16=True)          # {"loss", "acc1", "acc5"}
    # the reference's form: one text file per rank, scored by merge
    final_test(test_loader, model, device, os.path.join(out, f"{rank}.txt"), ds=True, bf16=True)
    top1, top5 = merge(out, world_size)
    # the native form: nothing is written, the logits never leave the device
    table = ViewTable(video_ids, num_views=12, num_classes=400, device=device)
    stats = final_test(test_loader, model, device, None, ds=True, bf16=True, table=table)
    scores = table.finalize(process_group)                                               # ViewScores: top1, top5, pred, label, count

What runs where (csrc/evaluate.hip): per batch one row pass (`ops.eval_rows`) computes the cross entropy and the label's rank of every row,
adds them to a meter block in DEVICE memory and stores the row's logits into the (video, view) table; `ops.view_finalize` is the softmax,
view mean and ranking of `merge` / `compute_video` as one kernel.  The batch loop never reads the device: the only host reads are one copy
of the meter block at the end of a pass, and one copy of the logits when `final_test` writes a file (of the per-video scores in `finalize`).
The model runs forward-only (`forward_only`), so a test pass holds no saved activation.

Reference semantics that are kept:
  * `loss` is the mean over BATCHES of the batch-mean cross entropy (`MetricLogger.update(loss=...)` counts n = 1 per batch), `acc1` /
    `acc5` are weighted by the batch size (`update(acc.item(), n=batch_size)` of timm's fp32 `hits * 100 / batch`);
  * with an initialised process group the totals and counts are summed over the ranks (`synchronize_between_processes`);
  * of several rows that name the same (video, chunk, split) the FIRST in reading order -- rank file by rank file, row by row -- counts;
  * the rank files have the reference's format, so either `merge` reads the other's files.
Differences, all documented at their place: the loss is computed in fp32 from the model's bf16 logits and not rounded (the reference's
`CrossEntropyLoss` returns a bf16 scalar on the DeepSpeed path: one bf16 rounding of the loss apart); the duplicate key is the PAIR (chunk,
split), where the reference's string `chunk_nb + split_nb` makes (1, 12) and (11, 2) collide (the two agree while both numbers are below
10: every shipped recipe); a video's label is the one stored with its lowest present view, the reference keeps the one it read last (they
differ only where a dataset labels one video inconsistently).  `ModelEma` is not part of this module.
"""
from __future__ import annotations

import contextlib
import os
import time
from dataclasses import dataclass
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

BF16, F32 = torch.bfloat16, torch.float32
NO_OWNER = (1 << 63) - 1
_MISSING = object()


# ---- forward-only test pass ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def forward_only(model):
    """`with forward_only(model): logits = model(clips)`: torch.no_grad(), and an `InternVideo2` / `internvideo2_cat` / `internvideo2_ap`
    classifier (or such a model behind a `.module` wrapper) runs ALL its blocks through the forward-only loop instead of BlockStackFn, which
    computes and holds the training forward's saved activations whether or not a gradient is recorded.  Done by setting `frozen_prefix =
    depth` for the duration: `InternVideo2._frozen_prefix` decides eligibility as for probing (a model with fp8 GEMMs or a bf16 residual
    stream keeps the autograd stack).  The attribute's previous state, its absence included, is restored on exit, also when the body raises;
    nothing changes for a model called outside the context."""
    from .internvideo2 import InternVideo2
    target = model
    if not isinstance(target, InternVideo2) and isinstance(getattr(model, "module", None), InternVideo2):
        target = model.module
    native = isinstance(target, InternVideo2)
    prev = target.__dict__.get("frozen_prefix", _MISSING) if native else _MISSING
    if native:
        target.frozen_prefix = target.depth
    try:
        with torch.no_grad():
            yield model
    finally:
        if native:
            if prev is _MISSING:
                target.__dict__.pop("frozen_prefix", None)
            else:
                target.frozen_prefix = prev


# ---- meters ---------------------------------------------------------------------------------------------------------------------------------
def _group(process_group=None):
    """(use collectives?, group): an explicit group, else the default group when torch.distributed is initialised"""
    import torch.distributed as dist
    if process_group is not None:
        return True, process_group
    return (dist.is_available() and dist.is_initialized()), None


class Meters:
    """the meter block of `ops.eval_rows` in device memory: int64 [8] = (float64 bits of: sum of batch-mean losses, acc1 total, acc5 total;
    batches, top-1 hits, top-5 hits, samples, bad rows).  Nothing is read before `read()`."""

    def __init__(self, device):
        self.block = torch.zeros((ops.METER_SLOTS,), dtype=torch.int64, device=device)

    def reset(self) -> None:
        self.block.zero_()

    def totals(self, process_group=None, extra: Optional[torch.Tensor] = None):
        """ONE host copy -> (float64 [8] totals, summed over the ranks of the process group when there is one; `extra` as it is on this rank)"""
        t = torch.cat([self.block[:3].view(torch.float64), self.block[3:].to(torch.float64)])
        use, group = _group(process_group)
        if use:
            import torch.distributed as dist
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        if extra is not None:
            t = torch.cat([t, extra.reshape(-1).to(torch.float64)])
        t = t.cpu()
        return t[:ops.METER_SLOTS], t[ops.METER_SLOTS:]

    @staticmethod
    def stats(totals) -> Dict[str, float]:
        loss, a1, a5, batches, _, _, samples, bad = (float(v) for v in totals)
        if bad:
            raise ValueError(f"{int(bad)} rows had a label outside [0, num_classes) or a video / view index outside the table")
        return {"loss": loss / batches, "acc1": a1 / samples, "acc5": a5 / samples}

    def read(self, process_group=None) -> Dict[str, float]:
        return self.stats(self.totals(process_group)[0])


# ---- the view table ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class ViewScores:
    """top1 / top5: fractions over the videos that have at least one view; pred, label, count, rank: int32 [n_videos] on the host (-1 and
    count 0 for a video without a view; rank = position of the label in the mean); probs: fp32 [n_videos, V] on the device, or None"""
    top1: float
    top5: float
    pred: torch.Tensor
    label: torch.Tensor
    count: torch.Tensor
    probs: Optional[torch.Tensor] = None
    rank: Optional[torch.Tensor] = None


def _host_ints(x) -> Optional[np.ndarray]:
    """the values of a host-side index list / array / CPU tensor, or None when they live on the device"""
    if isinstance(x, torch.Tensor):
        return None if x.is_cuda else x.reshape(-1).numpy().astype(np.int64)
    return np.asarray([int(v) for v in x], dtype=np.int64).reshape(-1)


class ViewTable:
    """The logits of every (video, view) of a test set in device memory, view = chunk * num_crop + split, filled by `add` under the
    reference's rule that the first row read for a slot wins (engine_for_finetuning.py:267-268; here the key is the pair (chunk, split),
    the reference's is the string chunk + split).  `names`: the test video ids, which every rank has from the annotation file; the host
    keeps name -> index.  Memory: n_videos * num_views * ceil8(num_classes) elements of `dtype` (K400 test: 19,796 x 12 x 400 bf16 = 190 MB)
    plus 12 bytes per slot.  `num_crop` (default 3, `--test_num_crop 3` of every shipped recipe) must divide num_views."""

    def __init__(self, names: Sequence[str], num_views: int, num_classes: int, dtype=BF16, device="cuda", num_crop: int = 3, rank: Optional[int] = None):
        names = [str(n) for n in names]
        self.index = {n: i for i, n in enumerate(names)}
        if len(self.index) != len(names) or not names:
            raise ValueError("ViewTable: names must be a non-empty list of distinct video ids")
        if num_views <= 0 or num_crop <= 0 or num_views % num_crop:
            raise ValueError(f"ViewTable: num_views = {num_views} is not a positive multiple of num_crop = {num_crop}")
        if num_classes <= 0 or dtype not in (BF16, F32):
            raise ValueError("ViewTable: num_classes > 0 and dtype bf16 / fp32")
        self.names, self.num_views, self.num_crop, self.num_classes = names, int(num_views), int(num_crop), int(num_classes)
        self.rank = rank
        n_slots = len(names) * self.num_views
        self.table = torch.empty((n_slots, (self.num_classes + 7) // 8 * 8), dtype=dtype, device=device)
        self.owner = torch.empty((n_slots,), dtype=torch.int64, device=device)
        self.labels = torch.empty((n_slots,), dtype=torch.int32, device=device)
        self.bad = torch.zeros((1,), dtype=torch.int64, device=device)
        self.reset()

    @property
    def device(self):
        return self.table.device

    def reset(self) -> None:
        """empty every slot (the logits are left as they are: a slot without an owner is never read)"""
        self.owner.fill_(NO_OWNER)
        self.bad.zero_()
        self._rows_added: Dict[int, int] = {}

    def _rank(self, rank: Optional[int]) -> int:
        if rank is not None:
            return int(rank)
        if self.rank is not None:
            return int(self.rank)
        use, _ = _group(None)
        if use:
            import torch.distributed as dist
            return dist.get_rank()
        return 0

    def add(self, logits: torch.Tensor, labels, ids: Optional[Sequence[str]], chunk_nb=None, split_nb=None, meters: Optional[Meters] = None,
            rank: Optional[int] = None):
        """one batch: logits (M, num_classes) bf16 / fp32 on the device (any row pitch), labels (M,), ids M video names (None: the rows
        update `meters` only), chunk_nb / split_nb (M,) -> (per-row loss fp32 [M], rank int32 [M]), both on the device.  Rows are numbered
        (rank << 40) | rows this rank added before; `rank` defaults to the table's / the process group's.  An unknown id, or a chunk / split
        outside the table that the host can see (lists, CPU tensors), raises ValueError; on device tensors such a row is skipped and counted,
        and `finalize` raises."""
        dev = self.device
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError(f"ViewTable.add: logits must be (M, {self.num_classes}), got {tuple(logits.shape)}")
        M = logits.shape[0]
        if logits.dtype not in (BF16, F32):
            logits = logits.float()
        if logits.stride(1) != 1:
            logits = logits.contiguous()
        labels = torch.as_tensor(labels).to(dev, non_blocking=True)
        if ids is None:
            return ops.eval_rows(logits, labels, V=self.num_classes, meters=None if meters is None else meters.block)
        if len(ids) != M:
            raise ValueError("ViewTable.add: one id per row")
        try:
            video = torch.tensor([self.index[str(n)] for n in ids], dtype=torch.int32)
        except KeyError as e:
            raise ValueError(f"ViewTable.add: video id {e.args[0]!r} is not in the table's names") from None
        n_chunk = self.num_views // self.num_crop
        ch, sp = _host_ints(chunk_nb), _host_ints(split_nb)
        if ch is not None and sp is not None:
            if ch.size != M or sp.size != M:
                raise ValueError("ViewTable.add: one chunk_nb and one split_nb per row")
            if ((ch < 0) | (ch >= n_chunk) | (sp < 0) | (sp >= self.num_crop)).any():
                raise ValueError(f"ViewTable.add: chunk_nb outside [0, {n_chunk}) or split_nb outside [0, {self.num_crop})")
            view = torch.from_numpy((ch * self.num_crop + sp).astype(np.int32)).to(dev, non_blocking=True)
        else:                                                          # indices that live on the device: checked by the kernel
            chd = torch.as_tensor(chunk_nb).to(dev).reshape(-1).to(torch.int64)
            spd = torch.as_tensor(split_nb).to(dev).reshape(-1).to(torch.int64)
            ok = (chd >= 0) & (chd < n_chunk) & (spd >= 0) & (spd < self.num_crop)
            view = torch.where(ok, chd * self.num_crop + spd, torch.full_like(chd, -1)).to(torch.int32)
        r = self._rank(rank)
        done = self._rows_added.get(r, 0)
        self._rows_added[r] = done + M
        loss, rk = ops.eval_rows(logits, labels, V=self.num_classes, meters=None if meters is None else meters.block,
                                 video=video.to(dev, non_blocking=True), view=view, seq_base=(r << 40) | done, n_views=self.num_views,
                                 table=self.table, owner=self.owner, table_label=self.labels)
        self.bad.add_((rk < 0).sum())
        return loss, rk

    def reduce_over_ranks(self, all_reduce: Callable[[torch.Tensor, str, str], None], rank: Optional[int] = None) -> None:
        """the multi-rank merge, IN PLACE: owner <- min over the ranks; every slot this rank does not own is zeroed (ops.view_mask_owned);
        table, labels and the bad-row count <- sum over the ranks, exact because a slot has at most one non-zero contributor.  Afterwards
        every rank holds the table a single process would have built from all rows in rank-major order.  all_reduce(tensor, "min" | "sum",
        "owner" | "table" | "labels" | "bad") reduces in place."""
        all_reduce(self.owner, "min", "owner")
        ops.view_mask_owned(self.table, self.owner, self.labels, self._rank(rank))
        all_reduce(self.table, "sum", "table")
        all_reduce(self.labels, "sum", "labels")
        all_reduce(self.bad, "sum", "bad")

    def finalize(self, process_group=None, want_probs: bool = False, local: bool = False) -> ViewScores:
        """softmax per present view, mean over the views, argmax and the label's rank per video, on the device (ops.view_finalize); with a
        process group (or an initialised default group) the ranks' tables are merged first (`reduce_over_ranks`), so the result does not
        depend on the world size; `local=True` never communicates (a table that already holds every rank's rows: `merge`).  One host copy:
        the per-video (count, pred, rank, label) and the bad-row count.  Videos without a view are left out of top1 / top5, as the reference
        never sees them."""
        use, group = (False, None) if local else _group(process_group)
        if use:
            import torch.distributed as dist
            ops_ = {"min": dist.ReduceOp.MIN, "sum": dist.ReduceOp.SUM}
            self.reduce_over_ranks(lambda t, op, what: dist.all_reduce(t, op=ops_[op], group=group), rank=dist.get_rank(group))
        out, probs = ops.view_finalize(self.table, self.owner, self.labels, self.num_views, self.num_classes, want_probs=want_probs)
        host = torch.cat([out.reshape(-1).to(torch.int64), self.bad]).cpu()
        if int(host[-1]):
            raise ValueError(f"ViewTable: {int(host[-1])} rows had a label outside [0, num_classes) or a video / view index outside the table")
        res = host[:-1].reshape(-1, 4).to(torch.int32)
        count, pred, rank, label = res[:, 0], res[:, 1], res[:, 2], res[:, 3]
        present = count > 0
        n = int(present.sum())
        if n == 0:
            raise ValueError("ViewTable.finalize: the table is empty")
        return ViewScores(int(((rank < 1) & present).sum()) / n, int(((rank < 5) & present).sum()) / n, pred, label, count, probs, rank)


# ---- the reference's rank files -------------------------------------------------------------------------------------------------------------
def format_lines(ids: Sequence[str], logits, labels, chunk_nb, split_nb) -> List[str]:
    """the per-sample lines of final_test (:217-223): "{id} {logits as a Python list} {label} {chunk} {split}\\n", the logits as the exact
    decimal `repr` of their fp32 values (`.float().cpu().numpy().tolist()`)"""
    lg = torch.as_tensor(logits).detach().float().cpu().numpy()
    lab, ch, sp = (np.asarray(torch.as_tensor(v).cpu()).reshape(-1) for v in (labels, chunk_nb, split_nb))
    return ["{} {} {} {} {}\n".format(ids[i], str(lg[i].tolist()), str(int(lab[i])), str(int(ch[i])), str(int(sp[i]))) for i in range(len(ids))]


def parse_line(line: str) -> Tuple[str, int, int, int, np.ndarray]:
    """one per-sample line with merge's own string handling (:256-261) -> (name, label, chunk_nb, split_nb, fp32 logits)"""
    line = line.strip()
    name = line.split(' ')[0]
    tail = line.split(']')[-1].split(' ')
    body = ' '.join(line.split(' ')[1:]).split('[')[1].split(']')[0]
    data = np.array([float(t) for t in body.split(',')], dtype=np.float64).astype(np.float32)
    return name, int(tail[1]), int(tail[2]), int(tail[3]), data


def read_rank_files(eval_path: str, num_tasks: int):
    """`{eval_path}/{x}.txt` for x in range(num_tasks), first line skipped (:252-254) -> per file (names, labels, chunks, splits, logits)"""
    files = []
    for x in range(num_tasks):
        with open(os.path.join(eval_path, str(x) + '.txt'), 'r') as f:
            rows = [parse_line(line) for line in f.readlines()[1:]]
        files.append(([r[0] for r in rows], np.array([r[1] for r in rows], dtype=np.int64), np.array([r[2] for r in rows], dtype=np.int64),
                      np.array([r[3] for r in rows], dtype=np.int64), np.stack([r[4] for r in rows]) if rows else np.zeros((0, 0), np.float32)))
    return files


def merge(eval_path, num_tasks, device="cuda", return_scores: bool = False):
    """engine_for_finetuning.py:246-286 -> (top1 * 100, top5 * 100) (and the ViewScores with `return_scores`).  The files are parsed on the
    host with the reference's string handling; their rows fill an fp32 ViewTable in file order (file x as rank x), which is finalized on the
    device: no text re-scoring, no process pool.  The table's geometry comes from the files: num_crop = largest split_nb + 1, views =
    (largest chunk_nb + 1) * num_crop.  Differences from the reference: see the module docstring (duplicate key, a video's label)."""
    print("Reading individual output files")
    files = [f for f in read_rank_files(eval_path, num_tasks) if f[0]]
    if not files:
        raise ValueError(f"merge: no sample lines under {eval_path}")
    names = list(dict.fromkeys(n for f in files for n in f[0]))
    num_crop = max(int(f[3].max()) for f in files) + 1
    n_chunk = max(int(f[2].max()) for f in files) + 1
    V = files[0][4].shape[1]
    print("Computing final results")
    print(len(names))
    table = ViewTable(names, n_chunk * num_crop, V, dtype=F32, device=device, num_crop=num_crop)
    for x, (ids, labels, chunks, splits, logits) in enumerate(files):
        table.add(torch.from_numpy(logits).to(device), torch.from_numpy(labels), ids, chunks, splits, rank=x)
    scores = table.finalize(local=True)
    res = (scores.top1 * 100, scores.top5 * 100)
    return res + (scores,) if return_scores else res


# ---- the two passes ---------------------------------------------------------------------------------------------------------------------------
def _check_mode(ds: bool, bf16: bool) -> None:
    if ds and not bf16:
        raise NotImplementedError("ds=True with bf16=False is the reference's fp16 path; the models of this package compute in bf16")


def _clips(videos, device, ds: bool, bf16: bool):
    videos = videos.to(device, non_blocking=True)
    return videos.bfloat16() if ds and bf16 else videos               # :164-166; without ds the reference autocasts, the native models cast inside


def _progress(header: str, i: int, t0: float, samples: int) -> None:
    if i % 10 == 0:
        print(f"{header} [{i}] samples {samples} time {time.time() - t0:.1f}s")          # counts and time only: no meter is read here


def validation_one_epoch(data_loader: Iterable, model, device, ds=False, bf16=False):
    """engine_for_finetuning.py:147-184 -> {"loss", "acc1", "acc5"}: `loss` the mean over batches of the batch-mean cross entropy (fp32 from
    the model's logits, not rounded to bf16 as the reference's DeepSpeed path does), `acc1` / `acc5` in percent weighted by batch size,
    totals and counts summed over an initialised process group.  The model runs under `forward_only`; the meters live on the device and
    are read ONCE, after the last batch.  ds=True with bf16=False raises NotImplementedError, an empty loader ValueError (the reference
    fails with a NameError there)."""
    _check_mode(ds, bf16)
    model.eval()
    meters = Meters(device)
    n, samples, t0 = 0, 0, time.time()
    with forward_only(model):
        for batch in data_loader:
            target = batch[1].to(device, non_blocking=True)
            output = model(_clips(batch[0], device, ds, bf16))
            _row_pass(output, target, meters)
            samples += int(target.shape[0])
            _progress("Val:", n, t0, samples)
            n += 1
    if n == 0:
        raise ValueError("validation_one_epoch: the data loader is empty")
    stats = meters.read()
    print('* Acc@1 {acc1:.3f} Acc@5 {acc5:.3f} loss {loss:.3f}'.format(**stats))
    return stats


def _row_pass(output, target, meters: Meters):
    if output.dtype not in (BF16, F32):
        output = output.float()
    if output.stride(1) != 1:
        output = output.contiguous()
    return ops.eval_rows(output, target, V=output.shape[1], meters=meters.block)


def final_test(data_loader: Iterable, model, device, file, ds=False, bf16=False, table: Optional[ViewTable] = None):
    """engine_for_finetuning.py:187-243 -> the same dict as validation_one_epoch, over batches (videos, target, ids, chunk_nb, split_nb).
    `file=path` writes the reference's rank file: a first line that `merge` skips (here the last batch's two accuracies as plain numbers,
    the reference prints two tensors), then one line per sample, duplicates included, in the reference's format (`format_lines`) -- the
    batches' logits stay on the device and are copied ONCE, after the last batch.  `file=None` with `table=ViewTable(...)` is the native
    form: every row goes into the table on the device and nothing is written; both may be given.  Same argument errors as
    validation_one_epoch, plus ValueError when neither a file nor a table is given."""
    _check_mode(ds, bf16)
    if file is None and table is None:
        raise ValueError("final_test: give a file to write, a ViewTable to fill, or both")
    model.eval()
    meters = Meters(device)
    kept = []
    n, samples, t0 = 0, 0, time.time()
    rank = None
    with forward_only(model):
        for batch in data_loader:
            target, ids, chunk_nb, split_nb = batch[1], batch[2], batch[3], batch[4]
            target_dev = target.to(device, non_blocking=True)
            output = model(_clips(batch[0], device, ds, bf16))
            if table is not None:
                _, rank = table.add(output, target_dev, ids, chunk_nb, split_nb, meters=meters)
            else:
                _, rank = _row_pass(output, target_dev, meters)
            if file is not None:
                kept.append((output, target, list(ids), chunk_nb, split_nb))
            samples += int(target.shape[0])
            _progress("Test:", n, t0, samples)
            n += 1
    if n == 0:
        raise ValueError("final_test: the data loader is empty")
    totals, last = meters.totals(extra=rank)
    if file is not None:
        k = np.where(last.numpy() < 0, -1 - last.numpy(), last.numpy())
        acc1, acc5 = float((k < 1).sum() * 100.0 / k.size), float((k < 5).sum() * 100.0 / k.size)
        logits = torch.cat([o.float() for o, _, _, _, _ in kept]).cpu()
        lines, at = [], 0
        for o, tg, ids, ch, sp in kept:
            lines += format_lines(ids, logits[at:at + o.shape[0]], tg, ch, sp)
            at += o.shape[0]
        with open(file, 'w') as f:
            f.write("{}, {}\n".format(acc1, acc5))
            f.writelines(lines)
    stats = Meters.stats(totals)
    print('* Acc@1 {acc1:.3f} Acc@5 {acc5:.3f} loss {loss:.3f}'.format(**stats))
    return stats
