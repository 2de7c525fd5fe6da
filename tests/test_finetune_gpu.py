"""The fine-tuning step on a real MI355X (csrc/finetune.hip, internvideo_amd.finetune): Mixup / CutMix of the clips and the dense target
bit for bit against what the REFERENCE's datasets/mixup.py produced (tests/golden/finetune_mixup.npz), the soft-target cross entropy
against fp64 restatements of its formulas, the rank / accuracy output, the registered operator, the model step against the reference
classifier, and the captured step reading its draw from device memory.

Bars.  Clips and targets: bitwise.  Loss / gradient of the row kernel: those of tests/test_bert_gpu.py::test_ce_rows (|loss - ref| <
2e-5 |ref| + 1e-6 -- fp32 sums of <= 2050 terms with __expf / __logf --, gradient rel-L2 < 5e-3 -- one bf16 rounding per element is
<= 2^-9 = 2e-3 relative --, padding columns exactly 0).  Model step: the bars of test_finetune_classifier_matches_reference_golden."""
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from internvideo_amd import finetune, ops  # noqa: E402
from oracle import internvideo2_oracle as O  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "finetune_mixup.npz")
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
NUM_CLASSES = 10


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def clips(shape, seed):                                          # the generator's seeded inputs (make_golden_finetune_mixup.py)
    return np.random.RandomState(1000 + seed).standard_normal(shape).astype(np.float32)


def labels_of(batch, seed):
    return np.random.RandomState(2000 + seed).randint(0, NUM_CLASSES, size=batch).astype(np.int64)


def draws(gold, cfg=None, mode=None, si=None):
    for key in gold["draws"]:
        c, m, s, seed = str(key).split(":")
        if (cfg is None or c == cfg) and (mode is None or m == mode) and (si is None or int(s) == si):
            yield str(key) + ":", c, m, tuple(int(v) for v in gold["shapes"][int(s)]), int(seed)


def sha(t: torch.Tensor) -> bytes:
    t = t.detach().cpu().contiguous()
    a = t.view(torch.int16).numpy() if t.dtype == BF16 else t.numpy()
    return hashlib.sha256(a.tobytes()).digest()


def emulate_mix(x: np.ndarray, table: np.ndarray) -> np.ndarray:
    """the table semantics in numpy: two separately rounded fp32 products and a rounded sum; CutMix is a select"""
    out = np.empty_like(x)
    for i in range(x.shape[0]):
        src, kind, yl, yh, xl, xh = (int(v) for v in table[i, :6])
        lam, oml = table[i, 6:8].copy().view(np.float32)
        if kind == 1:
            out[i] = (x[i] * lam).astype(np.float32) + (x[src] * oml).astype(np.float32)
        else:
            out[i] = x[i]
            if kind == 2:
                out[i][..., yl:yh, xl:xh] = x[src][..., yl:yh, xl:xh]
    return out


def rel(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# ---- 1. mix_clips ---------------------------------------------------------------------------------------------------------------------
def test_mix_clips_reproduces_the_reference_clips_bit_for_bit(gold):
    n, kinds, full = 0, set(), 0
    for pre, cfg, mode, shape, seed in draws(gold):
        x = clips(shape, seed)
        table = gold[pre + "table"]
        xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(table).to(DEV)
        o32 = ops.mix_clips(xd, td, F32)
        assert o32.dtype == F32 and o32.shape == xd.shape and torch.equal(xd.cpu(), torch.from_numpy(x)), "the input must stay untouched"
        if pre + "mixed" in gold.files:                          # the full reference clips: a mismatch is located, not just detected
            want = torch.from_numpy(gold[pre + "mixed"])
            bad = (o32.cpu().view(torch.int32) != want.view(torch.int32)).nonzero()
            assert bad.numel() == 0, (pre, "first mismatches (b, c, t, y, x)", bad[:4].tolist(), table.tolist())
            full += 1
        assert sha(o32) == gold[pre + "sha_f32"].tobytes(), (pre, "fp32 -> fp32", table.tolist())
        o16 = ops.mix_clips(xd, td, BF16)
        assert o16.dtype == BF16 and sha(o16) == gold[pre + "sha_bf16"].tobytes(), (pre, "fp32 -> bf16")
        assert torch.equal(o16, o32.to(BF16))
        # bf16 -> bf16: the same formula on the up-cast input, then rounded
        xb = xd.to(BF16)
        want_b = torch.from_numpy(emulate_mix(xb.float().cpu().numpy(), table)).to(BF16)
        assert torch.equal(ops.mix_clips(xb, td, BF16).cpu(), want_b), (pre, "bf16 -> bf16")
        kinds |= set(int(k) for k in table[:, 1])
        n += 1
    assert n >= 60 and full >= 6 and kinds == {0, 1, 2}, (n, full, kinds)


def test_mix_clips_hand_made_boxes_and_nan_poison():
    """whole-frame box, empty box, one pixel at the last column; NaN in the partner outside the box / in the partner of an unmixed
    sample must not reach the output (CutMix is a select, kind 0 a copy)"""
    shape = (2, 3, 2, 14, 14)
    x = torch.from_numpy(clips(shape, 77)).to(DEV)
    one = int(np.float32(1.0).view(np.int32))

    def table(row0, row1):
        return torch.tensor([row0, row1], dtype=torch.int32, device=DEV)
    for dt in (F32, BF16):
        xin = x.to(dt)
        out = ops.mix_clips(xin, table([1, 2, 0, 14, 0, 14, one, 0], [0, 2, 5, 5, 0, 14, one, 0]), dt)
        assert torch.equal(out[0], xin[1]), "a box over the whole frame takes the partner"
        assert torch.equal(out[1], xin[1]), "an empty box (yl == yh) leaves the sample"
        out = ops.mix_clips(xin, table([1, 2, 5, 6, 13, 14, one, 0], [0, 0, 0, 0, 0, 0, one, 0]), dt)
        want = xin[0].clone(); want[..., 5, 13] = xin[1][..., 5, 13]
        assert torch.equal(out[0], want) and torch.equal(out[1], xin[1]), "one pixel at the last column"
        poison = xin.clone()
        keep = poison[1][..., 5, 13].clone()
        poison[1] = float("nan"); poison[1][..., 5, 13] = keep
        out = ops.mix_clips(poison, table([1, 2, 5, 6, 13, 14, one, 0], [0, 0, 0, 0, 0, 0, one, 0]), dt)
        assert torch.isfinite(out[0]).all() and torch.equal(out[0], want), "NaN outside the box of the partner reached the output"
        poison[1] = float("nan")
        out = ops.mix_clips(poison, table([1, 0, 0, 14, 0, 14, one, 0], [0, 0, 0, 0, 0, 0, one, 0]), dt)
        assert torch.isfinite(out[0]).all() and torch.equal(out[0], xin[0]), "the partner of an unmixed sample was read into the output"
    # a flat sample size that is a multiple of 4 but not of 8 (the 4-element path), CutMix box with odd edges
    shape = (2, 1, 1, 6, 6)
    x = torch.from_numpy(clips(shape, 78)).to(DEV)
    t = np.array([[1, 2, 1, 4, 3, 6, one, 0], [0, 1, 0, 0, 0, 0, int(np.float32(0.3).view(np.int32)), int(np.float32(0.7).view(np.int32))]], dtype=np.int32)
    want = torch.from_numpy(emulate_mix(x.cpu().numpy(), t))
    assert torch.equal(ops.mix_clips(x, torch.from_numpy(t).to(DEV), F32).cpu(), want)
    with pytest.raises(ops.InternVideoHipError, match="multiple of 4"):
        ops.mix_clips(torch.zeros((2, 1, 1, 3, 6), device=DEV), torch.zeros((2, 8), dtype=torch.int32, device=DEV))


# ---- 2. mixup_target ------------------------------------------------------------------------------------------------------------------
def test_mixup_target_is_bitwise_the_reference_target(gold):
    n = 0
    for pre, cfg, mode, shape, seed in draws(gold):
        y = torch.from_numpy(labels_of(shape[0], seed)).to(DEV)
        t = ops.mixup_target(y, torch.from_numpy(gold[pre + "tmix"]).to(DEV), 0.1, NUM_CLASSES)
        assert t.cpu().numpy().tobytes() == gold[pre + "target"].tobytes(), (pre, t.cpu().numpy(), gold[pre + "target"])
        n += 1
    assert n >= 60


# ---- 3. / 4. soft_ce_rows against fp64 -------------------------------------------------------------------------------------------------
def target64(a, b, mix, smoothing, V):
    """datasets/mixup.py:22-27 in fp64"""
    off = smoothing / V
    on = 1.0 - smoothing + off
    ya = torch.full((a.numel(), V), off, dtype=torch.float64).scatter_(1, a.long().view(-1, 1), on)
    yb = torch.full((b.numel(), V), off, dtype=torch.float64).scatter_(1, b.long().view(-1, 1), on)
    return ya * mix[:, :1].double() + yb * mix[:, 1:].double()


def soft_ce64(x, t, upstream=1.0):
    """timm SoftTargetCrossEntropy in fp64 -> (loss, d(upstream * loss) / dx)"""
    x = x.detach().double().cpu().requires_grad_(True)
    loss = torch.sum(-t * torch.nn.functional.log_softmax(x, dim=-1), dim=-1).mean()
    (loss * upstream).backward()
    return loss.item(), x.grad


def ls_ce64(x, a, s):
    """timm LabelSmoothingCrossEntropy in fp64: (1 - s) nll + s mean_c(-logp)"""
    logp = torch.nn.functional.log_softmax(x.detach().double().cpu(), dim=-1)
    nll = -logp.gather(1, a.long().cpu().view(-1, 1)).squeeze(1)
    return ((1.0 - s) * nll + s * (-logp.mean(dim=-1))).mean().item()


def make_logits(M, V, dtype, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    ld = (V + 7) // 8 * 8 + (8 if V % 8 == 0 else 0)            # always at least one padding column
    buf = torch.full((M, ld), 50.0)                              # junk in the padding: must be ignored
    buf[:, :V] = scale * torch.randn(M, V, generator=g)
    return buf.to(DEV).to(dtype)[:, :V], g


def make_rows(M, V, g):
    a = torch.randint(0, V, (M,), generator=g)
    b = torch.randint(0, V, (M,), generator=g)
    a[0], b[0] = 0, V - 1                                        # labels at the first and the last live column
    if M > 2:
        a[1], b[1] = V - 1, 0
        b[2] = a[2]                                              # both labels on one class
    mix = torch.tensor([(1.0, 0.0), (0.0, 1.0), (0.3, 0.7)] * M)[:M]
    if M == 1:
        mix = torch.tensor([(0.3, 0.7)])
    return a.to(torch.int32), b.to(torch.int32), mix.contiguous()


def check_loss_and_grad(loss, dl, V, ref_loss, ref_grad):
    assert abs(loss.item() - ref_loss) < 2e-5 * abs(ref_loss) + 1e-6, (loss.item(), ref_loss)
    assert rel(dl[:, :V], ref_grad) < 5e-3, rel(dl[:, :V], ref_grad)
    assert dl.shape[1] > V and float(dl[:, V:].float().abs().max()) == 0.0, "padding columns of the gradient must be exactly 0"


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("M", [1, 6])
@pytest.mark.parametrize("V", [5, 174, 400, 1000, 2050])
def test_soft_ce_rows_factored_matches_fp64(V, M, smoothing, dtype):
    logits, g = make_logits(M, V, dtype, seed=V + M)
    a, b, mix = make_rows(M, V, g)
    up = torch.tensor([0.37], device=DEV)
    loss, none, _ = ops.soft_ce_rows(logits, a.to(DEV), b.to(DEV), mix.to(DEV), smoothing, want_grad=False)
    assert none is None
    loss2, dl, _ = ops.soft_ce_rows(logits, a.to(DEV), b.to(DEV), mix.to(DEV), smoothing, dscale=2.0, dscale_dev=up)
    assert torch.equal(loss, loss2) and dl.dtype == BF16
    ref_loss, ref_grad = soft_ce64(logits, target64(a, b, mix, smoothing, V), 2.0 * 0.37)
    check_loss_and_grad(loss, dl, V, ref_loss, ref_grad)


def test_soft_ce_rows_survives_logits_of_80():
    """without the max subtraction exp(80) overflows fp32"""
    V, M = 174, 6
    logits, g = make_logits(M, V, F32, seed=9)
    base = logits.clone()
    base = base / base.abs().max() * 80.0
    buf = torch.full((M, 176), 50.0, device=DEV); buf[:, :V] = base
    logits = buf[:, :V]
    a, b, mix = make_rows(M, V, g)
    loss, dl, _ = ops.soft_ce_rows(logits, a.to(DEV), b.to(DEV), mix.to(DEV), 0.1)
    assert torch.isfinite(loss).all() and torch.isfinite(dl.float()).all() and float(logits.abs().max()) == 80.0
    ref_loss, ref_grad = soft_ce64(logits, target64(a, b, mix, 0.1, V))
    check_loss_and_grad(loss, dl, V, ref_loss, ref_grad)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_soft_ce_rows_identities(dtype):
    V, M = 174, 6
    logits, g = make_logits(M, V, dtype, seed=4)
    a, _, _ = make_rows(M, V, g)
    ad = a.to(DEV)
    # smoothing 0, no mix: the plain mean cross entropy of ivh_ce_rows on the same logits
    loss, dl, _ = ops.soft_ce_rows(logits, ad)
    l_ce, dl_ce = ops.ce_rows(logits, ad, V=V)
    assert abs(loss.item() - l_ce.item()) < 2e-5 * abs(l_ce.item()) + 1e-6 and rel(dl[:, :V], dl_ce[:, :V]) < 5e-3
    assert float(dl[:, V:].float().abs().max()) == 0.0
    # lam = 1, smoothing 0.1: timm's LabelSmoothingCrossEntropy
    loss, _, _ = ops.soft_ce_rows(logits, ad, smoothing=0.1, want_grad=False)
    ref = ls_ce64(logits, a, 0.1)
    assert abs(loss.item() - ref) < 2e-5 * abs(ref) + 1e-6, (loss.item(), ref)
    crit = finetune.LabelSmoothingCrossEntropy(0.1)
    assert torch.equal(crit(logits, ad).reshape(1), loss)


def test_soft_ce_rows_dense_targets_from_the_fixture(gold):
    """the reference's dense targets (they sum to 1 +- 1.2e-7, nothing relies on that) and a target that sums to 2.5"""
    n = 0
    for pre, cfg, mode, shape, seed in draws(gold, "std", si=0):
        M, V = shape[0], NUM_CLASSES
        logits, _ = make_logits(M, V, BF16 if seed % 2 else F32, seed=100 + seed)
        t = torch.from_numpy(gold[pre + "target"])
        loss, dl, _ = ops.soft_ce_rows(logits, None, target=t.to(DEV), dscale=2.0, dscale_dev=torch.tensor([0.37], device=DEV))
        ref_loss, ref_grad = soft_ce64(logits, t.double(), 2.0 * 0.37)
        check_loss_and_grad(loss, dl, V, ref_loss, ref_grad)
        # dense form fed with ivh_mixup_target's output == factored form on the same draw
        y = torch.from_numpy(labels_of(M, seed)).to(DEV)
        mix = torch.from_numpy(gold[pre + "tmix"]).to(DEV)
        dense = ops.mixup_target(y, mix, 0.1, V)
        l_d = ops.soft_ce_rows(logits, None, target=dense, want_grad=False)[0].item()
        l_f = ops.soft_ce_rows(logits, y, y.flip(0), mix, 0.1, want_grad=False)[0].item()
        assert abs(l_d - l_f) <= 1e-6 * abs(l_f), (pre, l_d, l_f)
        n += 1
    assert n >= 24
    logits, _ = make_logits(6, 174, F32, seed=3)
    t = torch.rand(6, 174, dtype=torch.float64) * (2.5 / 87.0)
    loss, dl, _ = ops.soft_ce_rows(logits, None, target=t.float().to(DEV))
    ref_loss, ref_grad = soft_ce64(logits, t.float().double())
    check_loss_and_grad(loss, dl, 174, ref_loss, ref_grad)


# ---- 5. rank / accuracy -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [5, 174, 2050])
def test_rank_is_topk_membership_on_tie_free_rows(V):
    M = 6
    logits, g = make_logits(M, V, F32, seed={5: 55, 174: 224, 2050: 2101}[V])      # seeds whose randn rows hold no two equal values
    for r in range(M):
        assert torch.unique(logits[r]).numel() == V, "the test's rows must be tie-free"
    a = torch.randint(0, V, (M,), generator=g).to(DEV)
    a[0] = logits[0].argmax()
    _, _, rank = ops.soft_ce_rows(logits, a, want_grad=False, want_rank=True)
    assert rank.dtype == torch.int32 and int(rank[0]) == 0
    accs = finetune.accuracy(logits, a, topk=(1, 5))
    for k, acc in zip((1, 5), accs):
        member = (torch.topk(logits, min(k, V), dim=-1).indices == a.view(-1, 1)).any(dim=-1)
        assert torch.equal(rank < k, member), (k, rank.tolist())
        assert abs(acc.item() - 100.0 * member.float().mean().item()) < 1e-4
    if V == 5:
        assert bool((rank < 5).all())


def test_rank_tie_rule_equal_values_at_a_lower_index_rank_first():
    row = torch.tensor([1.0, 3.0, 3.0, 2.0, 3.0, 0.0, 4.0, 2.0, -1.0, 2.0])
    buf = torch.full((4, 16), 50.0); buf[:, :10] = row
    logits = buf.to(DEV)[:, :10]
    a = torch.tensor([1, 2, 4, 9], dtype=torch.int32, device=DEV)
    _, _, rank = ops.soft_ce_rows(logits, a, want_grad=False, want_rank=True)
    assert rank.tolist() == [1, 2, 3, 6], rank.tolist()          # one value above the 3s; three above the 2s plus two earlier 2s


# ---- 6. the registered operator ----------------------------------------------------------------------------------------------------------
def test_soft_target_cross_entropy_operator_opcheck_and_equals_the_module(gold):
    import internvideo_amd.torch_ops  # noqa: F401
    K = torch.ops.internvideo_hip
    checks = ("test_schema", "test_autograd_registration", "test_faketensor")
    pre = next(p for p, c, m, s, _ in draws(gold, "std", "elem", 0) if p + "mixed" in gold.files)
    M, V = 6, NUM_CLASSES
    base, _ = make_logits(M, V, BF16, seed=8)
    y = torch.from_numpy(labels_of(M, 1)).to(DEV).to(torch.int32)
    mix = torch.from_numpy(gold[pre + "tmix"]).to(DEV)
    dense = torch.from_numpy(gold[pre + "target"]).to(DEV)
    for make in (lambda: base.detach().clone().requires_grad_(True),                          # contiguous (6, 10): copied into padded rows
                 lambda: base.detach().requires_grad_(True),                                  # the classifier's view: pitch 16
                 lambda: base.detach().float().contiguous().requires_grad_(True)):
        torch.library.opcheck(K.soft_target_cross_entropy.default, (make(), y, y.flip(0), mix, 0.1, None), test_utils=checks)
        torch.library.opcheck(K.soft_target_cross_entropy.default, (make(), None, None, None, 0.0, dense), test_utils=checks)
        x1, x2 = make(), make()
        l1 = K.soft_target_cross_entropy(x1, None, None, None, 0.0, dense)
        l2 = finetune.SoftTargetCrossEntropy()(x2, dense)
        (l1.sum() * 0.5).backward(); (l2 * 0.5).backward()
        assert torch.equal(l1.reshape(()), l2) and torch.equal(x1.grad, x2.grad) and x1.grad.shape == x1.shape
        ref_loss, ref_grad = soft_ce64(x1, dense.double().cpu(), 0.5)
        assert abs(l1.item() - ref_loss) < 2e-5 * abs(ref_loss) + 1e-6 and rel(x1.grad, ref_grad) < 5e-3
    clip = torch.from_numpy(clips((6, 3, 2, 14, 14), 1)).to(DEV)
    table = torch.from_numpy(gold[pre + "table"]).to(DEV)
    torch.library.opcheck(K.mix_clips.default, (clip, table), test_utils=("test_schema", "test_faketensor"))
    assert torch.equal(K.mix_clips(clip, table, True).cpu(), torch.from_numpy(gold[pre + "mixed"]))


# ---- 7. the model step against the reference --------------------------------------------------------------------------------------------
def build_classifier(cfg, drop_path_rate=0.0):
    from internvideo_amd import internvideo2 as FT
    m = FT.InternVideo2(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio,
                        num_frames=cfg.num_frames, drop_path_rate=drop_path_rate, attn_pool_num_heads=cfg.attn_pool_num_heads,
                        clip_embed_dim=cfg.clip_embed_dim, num_classes=NUM_CLASSES)
    m.load_state_dict(O.synthetic_finetune_params(cfg, NUM_CLASSES, seed=12), strict=True)
    return m.to(DEV).train()


@pytest.mark.parametrize("name", ["mixup", "cutmix"])
def test_finetune_step_with_mixing_matches_the_reference(gold, name):
    """Mixup.apply -> forward_loss against the reference's Mixup -> InternVideo2 -> SoftTargetCrossEntropy formula -> backward (fp32, CPU),
    `tiny88`, 10 classes (head padded to 16 columns); the bars of test_finetune_classifier_matches_reference_golden"""
    from tests.test_flavours_gpu import check_grads, rel as rel_l2
    pre = f"step:{name}:"
    cfg = O.named_config("tiny88")
    video, _, _ = O.synthetic_batch(cfg, 2, 5, seed=12)
    video = video.float().to(DEV)
    labels = torch.tensor([3, 7], device=DEV)
    kw = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, label_smoothing=0.1, num_classes=NUM_CLASSES)
    mixer = finetune.Mixup(**kw)
    np.random.seed(int(gold[pre + "seed"][0]))
    params = mixer.draw(2, video.shape)
    assert np.array_equal(params.table, gold[pre + "table"]) and params.target_mix.tobytes() == gold[pre + "tmix"].tobytes()
    assert int(params.table[0, 1]) == {"mixup": 1, "cutmix": 2}[name]
    m = build_classifier(cfg)
    x, a, b, mix = mixer.apply(video, labels, params)
    assert x.dtype == BF16 and a.dtype == torch.int32 and b.tolist() == [7, 3]
    loss, logits = m.forward_loss(x, a, b, mix, smoothing=0.1)
    assert tuple(logits.shape) == (2, NUM_CLASSES) and not logits.requires_grad
    assert rel_l2(logits.float(), gold[pre + "logits"]) < 1e-2, rel_l2(logits.float(), gold[pre + "logits"])
    ref = float(gold[pre + "loss"][0])
    assert abs(loss.item() - ref) / ref < 1e-3, (loss.item(), ref)
    loss.backward()
    assert check_grads(gold, pre, m, pre + "bf16err:") >= 9
    # the drop-in route of the reference's loop: Mixup.__call__ + SoftTargetCrossEntropy()(model(x), target)
    m.zero_grad(set_to_none=True)
    np.random.seed(int(gold[pre + "seed"][0]))
    samples, targets = mixer(video, labels)
    assert samples.dtype == BF16 and targets.cpu().numpy().tobytes() == gold[pre + "target"].tobytes() and torch.equal(samples, x)
    out = m(samples.bfloat16())
    keep = out.detach().clone()
    loss2 = finetune.SoftTargetCrossEntropy()(out, targets)
    assert abs(loss2.item() - loss.item()) <= 1e-6 * abs(loss.item()), (loss2.item(), loss.item())
    loss2.backward()
    assert torch.equal(out, keep), "the logits are read after the backward: the loss must not overwrite them"
    assert check_grads(gold, pre, m, pre + "bf16err:") >= 9


# ---- 8. the captured step reads its draw from device memory -------------------------------------------------------------------------------
def test_captured_finetune_step_follows_the_table_in_device_memory():
    """two engines over the same classifier: eager train_step_fn against capture_fn + train_step_graphed, three steps with three different
    draws (none, mixup, cutmix) copied into the static table and labels between replays: losses and final weights bit for bit"""
    from internvideo_amd.engine import IVTrainEngine
    cfg = O.named_config("tiny88")
    video, _, _ = O.synthetic_batch(cfg, 2, 5, seed=12)
    video = video.float().to(DEV)
    H, W = video.shape[-2:]
    one = int(np.float32(1.0).view(np.int32))
    l3, l7 = int(np.float32(0.3).view(np.int32)), int(np.float32(0.7).view(np.int32))
    steps = [
        (finetune.MixParams(np.array([[1, 0, 0, 0, 0, 0, one, 0], [0, 0, 0, 0, 0, 0, one, 0]], dtype=np.int32),
                            np.array([[1, 0], [1, 0]], dtype=np.float32)), [3, 7]),
        (finetune.MixParams(np.array([[1, 1, 0, 0, 0, 0, l3, l7], [0, 1, 0, 0, 0, 0, l3, l7]], dtype=np.int32),
                            np.array([[0.3, 0.7], [0.3, 0.7]], dtype=np.float32)), [1, 9]),
        (finetune.MixParams(np.array([[1, 2, 3, H - 5, 7, W, one, 0], [0, 2, 3, H - 5, 7, W, one, 0]], dtype=np.int32),
                            np.array([[0.6, 0.4], [0.6, 0.4]], dtype=np.float32)), [0, 4]),
    ]
    mixer = finetune.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=NUM_CLASSES)
    traj = {}
    for tag in ("eager", "graph"):
        m = build_classifier(cfg)
        eng = IVTrainEngine(m, lr=1e-3, layer_decay=0.75)
        static = steps[0][0].to(DEV)
        labels = torch.tensor(steps[0][1], dtype=torch.int32, device=DEV)

        def loss_fn():
            x, a, b, mix = mixer.apply(video, labels, static)
            return m.forward_loss(x, a, b, mix, smoothing=0.1)
        if tag == "graph":
            eng.capture_fn(loss_fn)                              # (the capture's warm-up passes run no optimizer: the weights stand)
        losses = []
        for params, lab in steps:
            static.copy_(params)
            labels.copy_(torch.tensor(lab, dtype=torch.int32))
            out = eng.train_step_graphed() if tag == "graph" else eng.train_step_fn(loss_fn)
            losses.append(out[0].detach().clone())
        torch.cuda.synchronize()
        traj[tag] = (torch.stack([l.reshape(()) for l in losses]).cpu(), eng.master.clone())
        eng.close()
        del eng, m
    assert torch.equal(traj["eager"][0], traj["graph"][0]), (traj["eager"][0].tolist(), traj["graph"][0].tolist())
    assert torch.equal(traj["eager"][1], traj["graph"][1])
    assert len(set(traj["eager"][0].tolist())) == 3, "three different draws must give three different losses"


# ---- 9. sizes at which a thread makes more than one grid-stride trip; the remaining dtype instantiations -----------------------------------
def test_mixup_target_past_one_grid_pass_is_still_separately_rounded():
    """M * V = 2^21 > 4096 workgroups x 256 threads: the kernel's loop runs twice per thread (an unrolled loop body is where a compiler
    contracts the products into an FMA if it is allowed to); against the numpy statement of rn(rn(v1 lam) + rn(v2 oml))"""
    M, V = 2048, 1024
    rs = np.random.RandomState(5)
    y = rs.randint(0, V, size=M)
    lam = rs.beta(0.8, 0.8, size=M).astype(np.float32)
    mix = np.stack([lam, np.float32(1) - lam], axis=1).astype(np.float32)
    off, on = np.float32(0.1 / V), np.float32(1.0 - 0.1 + 0.1 / V)
    cols = np.arange(V)[None, :]
    v1 = np.where(cols == y[:, None], on, off).astype(np.float32)
    v2 = np.where(cols == y[::-1][:, None], on, off).astype(np.float32)
    want = (v1 * mix[:, :1]).astype(np.float32) + (v2 * mix[:, 1:]).astype(np.float32)
    got = ops.mixup_target(torch.from_numpy(y).to(DEV), torch.from_numpy(mix).to(DEV), 0.1, V).cpu().numpy()
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, (len(bad), bad[:4].tolist())


def test_mix_clips_past_one_grid_pass_and_from_bf16_to_fp32():
    """a sample of 8.5 M elements (> 4096 workgroups x 256 threads x 8): every thread makes a second trip; W = 1190 is no multiple of 4 and
    the CutMix box has odd edges.  fp32 -> fp32 and bf16 -> fp32 (the instantiations the fixture draws do not reach) bitwise against numpy."""
    shape = (2, 3, 2, 1190, 1190)
    assert shape[1] * shape[2] * shape[3] * shape[4] > 4096 * 256 * 8
    x = np.random.RandomState(6).standard_normal(shape).astype(np.float32)
    b3, b7, one = (int(np.float32(v).view(np.int32)) for v in (0.3, 0.7, 1.0))
    t = np.array([[1, 1, 0, 0, 0, 0, b3, b7], [0, 2, 333, 1001, 5, 1189, one, 0]], dtype=np.int32)
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    want = emulate_mix(x, t)
    got = ops.mix_clips(xd, td, F32).cpu().numpy()
    assert got.tobytes() == want.tobytes(), np.argwhere(got.view(np.int32) != want.view(np.int32))[:4].tolist()
    xb = xd.to(BF16)
    want = emulate_mix(xb.float().cpu().numpy(), t)
    got = ops.mix_clips(xb, td, F32).cpu().numpy()
    assert got.tobytes() == want.tobytes(), np.argwhere(got.view(np.int32) != want.view(np.int32))[:4].tolist()


@pytest.mark.parametrize("din,dout", [(F32, BF16), (BF16, F32), (BF16, BF16)])
def test_mix_clips_four_element_path_in_every_dtype_pair(din, dout):
    """C*T*H*W = 36: a multiple of 4 but not of 8"""
    shape = (2, 1, 1, 6, 6)
    x = torch.from_numpy(clips(shape, 78)).to(DEV).to(din)
    b3, b7, one = (int(np.float32(v).view(np.int32)) for v in (0.3, 0.7, 1.0))
    t = np.array([[1, 2, 1, 4, 3, 6, one, 0], [0, 1, 0, 0, 0, 0, b3, b7]], dtype=np.int32)
    want = torch.from_numpy(emulate_mix(x.float().cpu().numpy(), t)).to(dout)
    assert torch.equal(ops.mix_clips(x, torch.from_numpy(t).to(DEV), dout).cpu(), want)


# ---- 10. a head whose width is no multiple of 8 under the training engine --------------------------------------------------------------
def test_padded_head_gradient_is_overwritten_not_accumulated_across_engine_steps():
    """10 classes: the head GEMM runs zero-padded to 16 columns.  The engine never zeroes its matrix-gradient buffer (every matrix gradient is
    overwritten), so the head's gradient after a second backward must be that backward's alone: equal to what a fresh engine computes for
    the second batch, bit for bit, and different from the first batch's."""
    from internvideo_amd.engine import IVTrainEngine
    cfg = O.named_config("tiny88")
    video, _, _ = O.synthetic_batch(cfg, 2, 5, seed=12)
    video = video.to(DEV).to(BF16)
    batches = [(video, torch.tensor([3, 7], dtype=torch.int32, device=DEV)), (video.flip(0).contiguous(), torch.tensor([1, 9], dtype=torch.int32, device=DEV))]

    def backward_only(eng, m, batch):
        eng.zero_grad()
        eng._begin_step_on_device()
        loss, _ = m.forward_loss(batch[0], batch[1], smoothing=0.1)
        eng.backward(loss)
        eng._finish_reduce()
        p = dict(m.named_parameters())
        return p["head.weight"].main_grad.clone(), p["head.bias"].main_grad.clone()
    m = build_classifier(cfg)
    eng = IVTrainEngine(m, lr=1e-3)
    first = backward_only(eng, m, batches[0])
    second = backward_only(eng, m, batches[1])
    eng.close()
    m2 = build_classifier(cfg)
    eng2 = IVTrainEngine(m2, lr=1e-3)
    fresh = backward_only(eng2, m2, batches[1])
    eng2.close()
    assert float(second[0].float().abs().max()) > 0 and not torch.equal(first[0], second[0])
    assert torch.equal(second[0], fresh[0]) and torch.equal(second[1], fresh[1])
