"""Golden fixture of validation / the multi-view test, made by RUNNING THE REFERENCE'S OWN `final_test`, `merge` and `compute_video` on CPU:

    python tests/golden/make_golden_eval.py          (needs the reference tree: IV_REFERENCE_ROOT)

single_modality/engines/engine_for_finetuning.py is loaded by file path, with this generator's own stubs in sys.modules for what it imports
besides torch, numpy and scipy: `timm.utils` (`accuracy` restated from timm: `correct[:k].reshape(-1).float().sum(0) * 100. /
batch_size`), `utils` (a MetricLogger whose SmoothedValue keeps `total += value * n; count += n; global_avg = total / count`, as the
reference's) and `datasets.mixup`.  `multiprocessing.Pool` is replaced by an in-process stand-in whose `map` records the inputs and outputs
of `compute_video`.  The model is a stub that returns seeded logits already rounded to bf16 (a bf16 tensor: the DeepSpeed path, ds=True,
bf16=True, on which the reference's CrossEntropyLoss returns a bf16 scalar); the loader yields (videos, target, ids, chunk_nb, split_nb).

Cases: V in {10, 174, 400, 710} x (num_segment, num_crop) in {(4, 3), (2, 3)}, 7 videos on two "ranks".  Every case holds: one video with
only 5 of its views, one video absent altogether, one duplicate inside a batch, one across batches of the same rank, one (for 6 views:
three) across the two rank files -- the DistributedSampler padding case --, batch sizes 5, 8 and a last batch of 3.  A duplicate carries
OTHER logits than the row it repeats, so which one was kept shows in the bits.

tests/golden/eval_views.npz, per case under "V<V>:s<seg>c<crop>:" --
  r<k>:bits / labels / video / chunk / split / sizes   the rows of rank k in loader order (logits as bf16 bit patterns) and the batch sizes
  r<k>:text (V = 10, 174) / r<k>:text_sha   the rank file the reference wrote, without its first line (which prints two tensors)
  r<k>:stats                  the dict the reference's final_test returned: (loss, acc1, acc5)
  names                       the videos in the order merge met them (index into NAMES)
  probs (V = 10, 174) / probs_sha   the per-video mean probability compute_video ranks, recomputed from its recorded inputs as it does
  pred, top1, top5, label     compute_video's recorded outputs
  merge                       merge's two numbers
  f32err                      max |that mean - the same recomputed in fp64 from the same logits|
  loss64                      per rank: the mean over batches of the batch-mean cross entropy in fp64
The generator ASSERTS the conditions under which a test may demand exact decisions with no case left out, and picks the first seed at
which they hold: for every video the fp64 gaps between the 1st / 2nd and the 5th / 6th mean probability are >= 1e-4; for every row the
label's logit is not tied across rank positions 1 and 5; the reference's (bf16-rounded) loss is within 0.75 * 2^-8 relative of fp64.
The file is written with fixed zip time stamps: it regenerates bit for bit.
"""
from __future__ import annotations

import hashlib
import importlib.util
import io
import multiprocessing
import os
import sys
import tempfile
import types
import zipfile
from collections import defaultdict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_loader  # noqa: E402

CLASSES = (10, 174, 400, 710)
GEOMETRIES = ((4, 3), (2, 3))
NAMES = tuple(f"video_{i:03d}" for i in range(7))
ABSENT, PARTIAL, PARTIAL_VIEWS = 6, 5, 5
# batch sizes per rank; with 6 views the second rank carries two more rows of sampler padding
PLANS = {12: ((5, 8, 5, 8, 5, 3), (5, 8, 5, 8, 5, 3)), 6: ((5, 8, 3), (5, 8, 8, 3))}
FULL_TEXT = (10, 174)
SCALE = 2.5                                    # logits ~ N(0, SCALE^2); a share P_BOOST[video] of a video's rows get their label raised by SCALE sqrt(2 ln V)
P_BOOST = (0.9, 0.8, 0.3, 0.15, 0.6, 0.2, 0.0)
MIN_GAP, LOSS_TOL = 1e-4, 0.75 * 2.0 ** -8


def case_key(V, seg, crop):
    return f"V{V}:s{seg}c{crop}:"


def to_bf16_bits(x: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def from_bf16_bits(b: np.ndarray) -> np.ndarray:
    return (b.astype(np.uint32) << 16).view(np.float32)


# ---- the stubs ------------------------------------------------------------------------------------------------------------------------------
class SmoothedValue:
    def __init__(self):
        self.total, self.count = 0.0, 0

    def update(self, value, n=1):
        self.count += n
        self.total += value * n

    @property
    def global_avg(self):
        return self.total / self.count


class MetricLogger:
    def __init__(self, delimiter="\t"):
        self.meters = defaultdict(SmoothedValue)

    def update(self, **kwargs):
        for k, v in kwargs.items():
            if v is None:
                continue
            if isinstance(v, torch.Tensor):
                v = v.item()
            self.meters[k].update(v)

    def __getattr__(self, attr):
        if attr in self.meters:
            return self.meters[attr]
        raise AttributeError(attr)

    def log_every(self, iterable, print_freq, header=None):
        yield from iterable

    def synchronize_between_processes(self):
        pass


def timm_accuracy(output, target, topk=(1,)):
    maxk = min(max(topk), output.size()[1])
    batch_size = target.size(0)
    _, pred = output.topk(maxk, 1, True, True)
    pred = pred.t()
    correct = pred.eq(target.reshape(1, -1).expand_as(pred))
    return [correct[:min(k, maxk)].reshape(-1).float().sum(0) * 100. / batch_size for k in topk]


def load_reference_engine():
    stubs = {"timm": types.ModuleType("timm"), "timm.utils": types.ModuleType("timm.utils"), "utils": types.ModuleType("utils"),
             "datasets": types.ModuleType("datasets"), "datasets.mixup": types.ModuleType("datasets.mixup")}
    stubs["timm.utils"].accuracy, stubs["timm.utils"].ModelEma = timm_accuracy, type("ModelEma", (), {})
    stubs["timm"].utils = stubs["timm.utils"]
    stubs["utils"].MetricLogger = MetricLogger
    stubs["datasets.mixup"].Mixup = type("Mixup", (), {})
    stubs["datasets"].mixup = stubs["datasets.mixup"]
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        path = os.path.join(ref_loader.REF_ROOT, "InternVideo2", "single_modality", "engines", "engine_for_finetuning.py")
        spec = importlib.util.spec_from_file_location("_iv_ref_engine_ft", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


class StubModel:
    """returns the next batch's seeded bf16 logits"""

    def __init__(self, batches):
        self.batches = list(batches)

    def eval(self):
        return self

    def __call__(self, videos):
        out = self.batches.pop(0)
        assert out.shape[0] == videos.shape[0] and videos.dtype == torch.bfloat16
        return out


class RecordingPool:
    calls = []

    def __init__(self, n):
        pass

    def map(self, fn, lst):
        out = [fn(item) for item in lst]
        RecordingPool.calls.append((lst, out))
        return out


# ---- the rows of a case ---------------------------------------------------------------------------------------------------------------------
def build_rows(V, seg, crop, seed):
    """-> per rank (video, chunk, split, label, logits bf16-valued fp32, batch sizes) and the positions of the planted duplicates"""
    nv = seg * crop
    rs = np.random.RandomState(seed)
    video_label = rs.randint(0, V, size=len(NAMES))
    base = [(v, w) for v in range(len(NAMES)) if v not in (ABSENT, PARTIAL) for w in range(nv)]
    base += [(PARTIAL, int(w)) for w in sorted(rs.choice(nv, PARTIAL_VIEWS, replace=False))]
    base = [base[i] for i in rs.permutation(len(base))]
    plan0, plan1 = PLANS[nv]
    n0, n1 = sum(plan0), sum(plan1)
    n_cross = n0 + n1 - len(base) - 2
    assert n_cross >= 1
    r0 = base[:n0 - 2]
    r1 = base[n0 - 2:]
    # in-batch duplicate: a copy of the first row of rank 0's second batch, two places later in that batch
    a = plan0[0]
    r0.insert(a + 2, r0[a])
    # cross-batch duplicate: a copy of rank 0's row 1 (first batch) inside its third batch
    b = plan0[0] + plan0[1]
    r0.insert(b + 1, r0[1])
    # cross-rank duplicates: the sampler's padding repeats rank 0's first rows at the end of rank 1
    r1 = r1 + [r0[i] for i in range(n_cross)]
    assert len(r0) == n0 and len(r1) == n1
    dups = dict(in_batch=(0, a + 2, a), cross_batch=(0, b + 1, 1), cross_rank=[(1, n1 - n_cross + i, i) for i in range(n_cross)])
    ranks = []
    for rows, plan in ((r0, plan0), (r1, plan1)):
        n = len(rows)
        x = rs.standard_normal((n, V)).astype(np.float32) * SCALE
        vid = np.array([r[0] for r in rows]); view = np.array([r[1] for r in rows])
        lab = video_label[vid]
        boost = rs.rand(n) < np.array(P_BOOST)[vid]
        x[np.arange(n), lab] += np.where(boost, SCALE * np.sqrt(2 * np.log(V)), 0.0).astype(np.float32)
        x = from_bf16_bits(to_bf16_bits(x))
        ranks.append(dict(video=vid.astype(np.int32), chunk=(view // crop).astype(np.int32), split=(view % crop).astype(np.int32),
                          labels=lab.astype(np.int32), logits=x, sizes=np.array(plan, dtype=np.int32)))
    return ranks, dups


def loader(rank):
    at = 0
    for n in rank["sizes"]:
        s = slice(at, at + int(n))
        yield (torch.zeros((int(n), 1)), torch.from_numpy(rank["labels"][s].astype(np.int64)), [NAMES[v] for v in rank["video"][s]],
               torch.from_numpy(rank["chunk"][s].astype(np.int64)), torch.from_numpy(rank["split"][s].astype(np.int64)))
        at += int(n)


def winners(ranks, nv, crop):
    """the row kept per (video, view): the first in reading order, rank file by rank file -> {(video, view): (rank, row)}"""
    kept = {}
    for k, r in enumerate(ranks):
        for i in range(len(r["video"])):
            kept.setdefault((int(r["video"][i]), int(r["chunk"][i]) * crop + int(r["split"][i])), (k, i))
    return kept


def softmax64(x):
    x = x.astype(np.float64)
    e = np.exp(x - x.max())
    return e / e.sum()


def mean_probs64(ranks, nv, crop, V):
    kept = winners(ranks, nv, crop)
    out = {}
    for v in range(len(NAMES)):
        views = [kept[(v, w)] for w in range(nv) if (v, w) in kept]
        if views:
            out[v] = np.mean([softmax64(ranks[k]["logits"][i]) for k, i in views], axis=0)
    return out


def loss64(rank):
    at, tot = 0, []
    for n in rank["sizes"]:
        x = rank["logits"][at:at + int(n)].astype(np.float64); lab = rank["labels"][at:at + int(n)]
        m = x.max(axis=1, keepdims=True)
        lse = (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]
        tot.append(float(np.mean(lse - x[np.arange(int(n)), lab])))
        at += int(n)
    return float(np.mean(tot))


def rows_undecided(rank):
    """rows whose top-1 / top-5 flag depends on how a tie is broken: the label's value tied across position k"""
    bad = 0
    for x, lab in zip(rank["logits"], rank["labels"]):
        g, e = int((x > x[lab]).sum()), int((x == x[lab]).sum())
        bad += any(g < k < g + e for k in (1, 5))
    return bad


def run_case(engine, V, seg, crop, seed):
    """-> the case's arrays, or the reason this seed is rejected"""
    nv = seg * crop
    ranks, dups = build_rows(V, seg, crop, seed)
    if any(rows_undecided(r) for r in ranks):
        return None, "a label tied across rank 1 / 5"
    p64 = mean_probs64(ranks, nv, crop, V)
    for v, p in p64.items():
        s = np.sort(p)[::-1]
        if s[0] - s[1] < MIN_GAP or s[4] - s[5] < MIN_GAP:
            return None, f"video {v}: gaps {s[0] - s[1]:.3g} / {s[4] - s[5]:.3g}"
    d = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, r in enumerate(ranks):
            at, batches = 0, []
            for n in r["sizes"]:
                batches.append(torch.from_numpy(r["logits"][at:at + int(n)]).to(torch.bfloat16)); at += int(n)
            stats = engine.final_test(loader(r), StubModel(batches), "cpu", os.path.join(tmp, f"{k}.txt"), ds=True, bf16=True)
            l64 = loss64(r)
            if abs(stats["loss"] - l64) > LOSS_TOL * l64:
                return None, f"rank {k}: the reference's bf16 loss {stats['loss']} is {abs(stats['loss'] - l64) / l64:.3g} from fp64"
            text = "".join(open(os.path.join(tmp, f"{k}.txt")).readlines()[1:])
            pre = f"r{k}:"
            d[pre + "bits"] = to_bf16_bits(r["logits"])
            for name in ("labels", "video", "chunk", "split", "sizes"):
                d[pre + name] = r[name]
            if V in FULL_TEXT:
                d[pre + "text"] = np.frombuffer(text.encode(), dtype=np.uint8).copy()
            d[pre + "text_sha"] = np.frombuffer(hashlib.sha256(text.encode()).digest(), dtype=np.uint8).copy()
            d[pre + "stats"] = np.array([stats["loss"], stats["acc1"], stats["acc5"]], dtype=np.float64)
            d[pre + "loss64"] = np.array([l64])
        RecordingPool.calls.clear()
        orig = multiprocessing.Pool
        multiprocessing.Pool = RecordingPool
        try:
            top1, top5 = engine.merge(tmp, 2)
        finally:
            multiprocessing.Pool = orig
    (inputs, outputs), = RecordingPool.calls
    order = [NAMES.index(item[1]) for item in inputs]
    assert sorted(order) == sorted(p64), "the reference saw other videos than the first-wins emulation"
    probs = np.stack([np.mean([x for x in item[2]], axis=0) for item in inputs])          # compute_video's `feat`
    assert probs.dtype == np.float32
    f32err = max(float(np.abs(probs[j].astype(np.float64) - p64[v]).max()) for j, v in enumerate(order))
    for j, v in enumerate(order):                                                         # the decisions are those of fp64: no case to leave out
        assert int(outputs[j][0]) == int(np.argmax(p64[v])) and len(inputs[j][2]) == (PARTIAL_VIEWS if v == PARTIAL else nv)
    d["names"] = np.array(order, dtype=np.int32)
    if V in FULL_TEXT:
        d["probs"] = probs
    d["probs_sha"] = np.frombuffer(hashlib.sha256(probs.tobytes()).digest(), dtype=np.uint8).copy()
    d["pred"] = np.array([int(o[0]) for o in outputs], dtype=np.int32)
    d["top1"] = np.array([int(o[1]) for o in outputs], dtype=np.int32)
    d["top5"] = np.array([int(o[2]) for o in outputs], dtype=np.int32)
    d["label"] = np.array([int(o[3]) for o in outputs], dtype=np.int32)
    d["merge"] = np.array([top1, top5], dtype=np.float64)
    d["f32err"] = np.array([f32err])
    d["seed"] = np.array([seed])
    d["dups"] = np.array([dups["in_batch"], dups["cross_batch"]] + dups["cross_rank"], dtype=np.int32)      # (rank, row, the row it repeats on rank 0)
    return d, None


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps, so that the file regenerates bit for bit"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    assert ref_loader.available(), "reference tree not found"
    torch.set_num_threads(1)
    engine = load_reference_engine()
    out = {}
    for V in CLASSES:
        for seg, crop in GEOMETRIES:
            for seed in range(3000, 3400):
                d, why = run_case(engine, V, seg, crop, seed)
                if d is not None:
                    break
                print(f"  V={V} ({seg}, {crop}) seed {seed} rejected: {why}")
            else:
                raise AssertionError(f"no seed for V={V} ({seg}, {crop})")
            pre = case_key(V, seg, crop)
            out.update({pre + k: v for k, v in d.items()})
            print(f"{pre} seed {seed} merge {d['merge'].tolist()} f32err {d['f32err'][0]:.3g} "
                  f"stats r0 {d['r0:stats'].tolist()} r1 {d['r1:stats'].tolist()}")
    out["cases"] = np.array([case_key(V, s, c) for V in CLASSES for s, c in GEOMETRIES])
    out["video_names"] = np.array(NAMES)
    path = os.path.join(HERE, "eval_views.npz")
    write_npz(path, out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
