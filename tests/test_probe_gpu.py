"""Linear / attentive probing on the GPU: the kernels of csrc/probe.hip against fp64 statements computed from the same inputs, the two
probing model families against the reference's own run (tests/golden/probe.npz, written by make_golden_probe.py), the frozen-prefix trunk
against the whole autograd stack, and the training engine (eager, captured) around a frozen model.

Bars.  Pool and batch-norm statistics: the project's row-sum bar, 2e-5 |ref| + 1e-6 per element.  Batch-norm output and input gradient:
rel-L2 < 5e-3 (one bf16 rounding).  Batch-norm affine gradients (fp32 sums of N <= 1088 products): rel-L2 < 1e-4, the N * 2^-24 worst case
of a sequential fp32 sum.  Model logits, loss, BatchNorm buffers and eval logits: rel < max(1e-2, 1.5 x the reference's own bf16-vs-fp32
deviation of that case's logits); gradients: tests.test_flavours_gpu.check_grads."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from internvideo_amd import functional as Fn, lib as L, ops  # noqa: E402
from internvideo_amd.probe import freeze_for_probing  # noqa: E402
from oracle import internvideo2_oracle as O  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probe.npz")
DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NUM_CLASSES = 10
LABELS = [3, 7, 1, 9]
# case tag -> (position in make_golden_probe.CASES, model family, merge_method, merge_norm, open_clip_projector)
CASES = {"cls_avgN_kBN": (0, "cat", "cls_avgN", "kaiming_BN", False), "cls_avg1_kBN": (1, "cat", "cls_avg1", "kaiming_BN", False),
         "cls_avg1_proj_LN": (2, "cat", "cls_avg1_proj", "LN", False), "cls_avgN_proj_BN": (3, "cat", "cls_avgN_proj", "BN", False),
         "ap": (4, "ap", None, None, False), "proj_open": (5, "cat", "proj", "kaiming_BN", True)}


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def rel(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def assert_rowsum_bar(got, ref, what):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    over = (got - ref).abs() - (2e-5 * ref.abs() + 1e-6)
    assert bool(torch.isfinite(got).all()) and float(over.max()) <= 0, (what, float(over.max()), int((over > 0).sum()))


# ---- 1. pool ---------------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(2, 1, 1, 8), (3, 4, 16, 176), (2, 16, 256, 1408)]
GUARD = 3


def guarded_stream(B, T, S, Cn, dtype, seed):
    """the stream [B * (1 + T*S), C] as the middle of a buffer whose rows before and after it are NaN"""
    Lr = 1 + T * S
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((B * Lr, Cn), generator=g, dtype=F32).to(DEV).to(dtype)
    buf = torch.full(((B * Lr + 2 * GUARD), Cn), float("nan"), dtype=dtype, device=DEV)
    buf[GUARD:GUARD + B * Lr] = x
    view = buf[GUARD:GUARD + B * Lr]
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return view


def pool_reference(x, B, T, S, avg1):
    Cn = x.shape[1]
    xd = x.double().view(B, 1 + T * S, Cn)
    cls, patches = xd[:, :1], xd[:, 1:]
    avg = patches.mean(1, keepdim=True) if avg1 else patches.reshape(B, T, S, Cn).mean(2)
    return torch.cat([cls, avg], dim=1), xd.mean(1)


def raw_pool_fwd(x, B, T, S, avg1, sentinel=777.0):
    """ivh_cat_pool_fwd into buffers with two sentinel rows behind each output"""
    Cn = x.shape[1]
    G = 2 if avg1 else 1 + T
    out = torch.full((B * G + 2, Cn), sentinel, dtype=F32, device=DEV)
    tok = torch.full((B + 2, Cn), sentinel, dtype=F32, device=DEV)
    ws = torch.full((B * T + 2, Cn), sentinel, dtype=F32, device=DEV)
    L.call("ivh_cat_pool_fwd", L.ptr(x), int(x.dtype == F32), B, T, S, Cn, int(avg1), L.ptr(out), L.ptr(tok), L.ptr(ws), L.stream_ptr())
    return out, tok, ws


@pytest.mark.parametrize("avg1", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_pool_forward_against_fp64(shape, dtype, avg1):
    B, T, S, Cn = shape
    G = 2 if avg1 else 1 + T
    x = guarded_stream(B, T, S, Cn, dtype, seed=sum(shape))
    ref, ref_tok = pool_reference(x, B, T, S, avg1)
    out, tok, ws = raw_pool_fwd(x, B, T, S, avg1)
    assert_rowsum_bar(out[:B * G].view(B, G, Cn), ref, "pool")                  # (finite: the NaN guard rows were not read)
    assert_rowsum_bar(tok[:B], ref_tok, "token mean")
    assert bool((out[B * G:] == 777.0).all()) and bool((tok[B:] == 777.0).all()) and bool((ws[B * T:] == 777.0).all()), "sentinel rows written"
    out2, tok2, _ = raw_pool_fwd(x, B, T, S, avg1)
    assert torch.equal(out, out2) and torch.equal(tok, tok2), "two runs differ"
    # the wrapper, without the token mean
    o3, t3 = ops.cat_pool_fwd(x, B, T, S, avg1=avg1)
    assert t3 is None and torch.equal(o3.view(B * G, Cn), out[:B * G])


def pool_bwd_reference(dout, dtok, B, T, S, avg1):
    Cn = dout.shape[-1]
    Lr = 1 + T * S
    dx = torch.zeros((B, Lr, Cn), dtype=F64, device=dout.device)
    d = dout.double()
    dx[:, 0] += d[:, 0]
    if avg1:
        dx[:, 1:] += (d[:, 1] / (T * S)).unsqueeze(1)
    else:
        dx[:, 1:] += (d[:, 1:] / S).repeat_interleave(S, dim=1)
    if dtok is not None:
        dx += (dtok.double() / Lr).unsqueeze(1)
    return dx.view(B * Lr, Cn)


@pytest.mark.parametrize("avg1", [False, True])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_pool_backward_against_fp64_overwrite_and_accumulate(shape, avg1):
    B, T, S, Cn = shape
    G = 2 if avg1 else 1 + T
    Lr = 1 + T * S
    g = torch.Generator(device="cpu").manual_seed(7 + sum(shape))
    dout = torch.randn((B, G, Cn), generator=g).to(DEV)
    dtok = torch.randn((B, Cn), generator=g).to(DEV)
    base = torch.randn((B * Lr, Cn), generator=g).to(DEV)
    for dt in (None, dtok):
        ref = pool_bwd_reference(dout, dt, B, T, S, avg1)
        buf = torch.full((B * Lr + 2, Cn), float("nan"), dtype=F32, device=DEV)          # overwrite: what was there must not matter
        buf[B * Lr:] = 777.0
        dx = ops.cat_pool_bwd(dout, dt, B, T, S, avg1=avg1, dx=buf[:B * Lr], accumulate=False)
        assert_rowsum_bar(dx, ref, "pool bwd overwrite")
        assert bool((buf[B * Lr:] == 777.0).all())
        acc = base.clone()
        ops.cat_pool_bwd(dout, dt, B, T, S, avg1=avg1, dx=acc, accumulate=True)
        assert_rowsum_bar(acc, base.double() + ref, "pool bwd accumulate")
    ref = pool_bwd_reference(torch.zeros_like(dout), dtok, B, T, S, avg1)                 # the token mean's gradient alone
    assert_rowsum_bar(ops.cat_pool_bwd(None, dtok, B, T, S, avg1=avg1), ref, "pool bwd token mean only")


# ---- 2. batch norm -----------------------------------------------------------------------------------------------------------------------
BN_SHAPES = [(1, 2, 64), (2, 5, 176), (64, 17, 768)]


def bn_reference(x, w, b, eps):
    """fp64 -> (y [B, G, C], mean, biased var, unbiased var)"""
    xd = x.double()
    N = xd.shape[0] * xd.shape[1]
    mean = xd.mean(dim=(0, 1))
    var = ((xd - mean) ** 2).mean(dim=(0, 1))
    y = (xd - mean) / torch.sqrt(var + eps)
    if w is not None:
        y = y * w.double() + b.double()
    return y, mean, var, var * N / (N - 1)


def flatten_channel_major(y):
    """[B, G, C] -> [B, C * G] with out[b, c * G + g] = y[b, g, c], written index by index"""
    B, G, Cn = y.shape
    out = torch.empty((B, Cn * G), dtype=y.dtype, device=y.device)
    bi, gi, ci = torch.meshgrid(torch.arange(B, device=y.device), torch.arange(G, device=y.device), torch.arange(Cn, device=y.device), indexing="ij")
    out[bi.reshape(-1), (ci * G + gi).reshape(-1)] = y.reshape(-1)
    return out


def bn_inputs(shape, dtype, affine, seed, offset=0.0, scale=1.0):
    B, G, Cn = shape
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (offset + scale * torch.randn(shape, generator=g)).to(DEV).to(dtype)
    w = (1.0 + 0.2 * torch.randn(Cn, generator=g)).to(DEV) if affine else None
    b = (0.1 * torch.randn(Cn, generator=g)).to(DEV) if affine else None
    dy = torch.randn((B, Cn * G), generator=g).to(DEV).to(BF16)
    return x, w, b, dy


def check_bn_train(shape, dtype, affine, seed, eps, offset=0.0, scale=1.0):
    B, G, Cn = shape
    N = B * G
    x, w, b, dy = bn_inputs(shape, dtype, affine, seed, offset, scale)
    rm = torch.full((Cn,), 0.25, dtype=F32, device=DEV)
    rv = torch.full((Cn,), 1.5, dtype=F32, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    y, mean, rstd = ops.batchnorm_cols_fwd(x, w, b, eps, True, 0.1, rm, rv, nbt)
    yr, mr, vr, vur = bn_reference(x, w, b, eps)
    assert y.dtype == BF16 and tuple(y.shape) == (B, Cn * G)
    e = rel(y.float(), flatten_channel_major(yr))
    assert e < 5e-3, ("bn output", e)
    assert_rowsum_bar(mean, mr, "save_mean")
    assert_rowsum_bar(rstd, 1.0 / torch.sqrt(vr + eps), "save_rstd")
    assert_rowsum_bar(rm, 0.9 * 0.25 + 0.1 * mr, "running_mean")
    assert_rowsum_bar(rv, 0.9 * 1.5 + 0.1 * vur, "running_var")
    assert int(nbt.item()) == 1
    # backward: fp64 from the same x and the same bf16 dy
    xd = x.double()
    xh = (xd - mr) / torch.sqrt(vr + eps)
    dyd = dy.double().view(B, Cn, G).permute(0, 2, 1)                                     # [B, G, C]
    dyw = dyd * (w.double() if affine else 1.0)
    dxr = (dyw - dyw.mean(dim=(0, 1)) - xh * (dyw * xh).mean(dim=(0, 1))) / torch.sqrt(vr + eps)
    for dxt in (F32, BF16):
        dx, dw, db = ops.batchnorm_cols_bwd(x, w, mean, rstd, dy, training=True, dx_dtype=dxt, want_affine_grads=affine)
        assert dx.dtype == dxt
        e = rel(dx.float(), dxr)
        assert e < 5e-3, ("bn dx", dxt, e)
        if affine:
            e1, e2 = rel(dw, (dyd * xh).sum(dim=(0, 1))), rel(db, dyd.sum(dim=(0, 1)))
            assert e1 < 1e-4 and e2 < 1e-4, ("bn dw / db", e1, e2)
        else:
            assert dw is None and db is None
    # the derivative factor of the projection in front of the norm rides in the same kernel
    dact = torch.rand(shape, generator=torch.Generator(device="cpu").manual_seed(seed + 1)).to(DEV).to(BF16)
    dx, _, _ = ops.batchnorm_cols_bwd(x, w, mean, rstd, dy, training=True, dact=dact, dx_dtype=F32)
    assert rel(dx, dxr * dact.double()) < 5e-3
    return N


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("shape", BN_SHAPES)
def test_batchnorm_training_against_fp64(shape, dtype, affine):
    check_bn_train(shape, dtype, affine, seed=11 + sum(shape), eps=1e-5 if affine else 1e-6)


def test_batchnorm_statistics_are_centred():
    """inputs 30 + 0.05 N(0, 1): E[x^2] - E[x]^2 in fp32 loses the variance (2.5e-3 against 900) and misses the output bar by an order of
    magnitude; centred fp32 statistics leave the one bf16 rounding of the output"""
    check_bn_train((2, 5, 176), F32, False, seed=5, eps=1e-6, offset=30.0, scale=0.05)
    check_bn_train((64, 17, 768), F32, True, seed=6, eps=1e-5, offset=30.0, scale=0.05)


@pytest.mark.parametrize("affine", [False, True])
def test_batchnorm_eval_after_two_training_calls(affine):
    shape, eps = (2, 5, 176), 1e-5
    B, G, Cn = shape
    rm = torch.zeros((Cn,), dtype=F32, device=DEV)
    rv = torch.ones((Cn,), dtype=F32, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    rm_ref, rv_ref = rm.double(), rv.double()
    for s in (21, 22):
        x, w, b, _ = bn_inputs(shape, BF16, affine, s, offset=0.5, scale=2.0)
        ops.batchnorm_cols_fwd(x, w, b, eps, True, 0.1, rm, rv, nbt)
        _, mr, _, vur = bn_reference(x, None, None, eps)
        rm_ref, rv_ref = 0.9 * rm_ref + 0.1 * mr, 0.9 * rv_ref + 0.1 * vur
    assert int(nbt.item()) == 2
    assert_rowsum_bar(rm, rm_ref, "running_mean after two calls")
    assert_rowsum_bar(rv, rv_ref, "running_var after two calls")
    x, w, b, dy = bn_inputs(shape, BF16, affine, 23, offset=0.5, scale=2.0)
    keep = (rm.clone(), rv.clone())
    y, mean, rstd = ops.batchnorm_cols_fwd(x, w, b, eps, False, 0.1, rm, rv, nbt)
    yr = (x.double() - rm_ref) / torch.sqrt(rv_ref + eps)
    if affine:
        yr = yr * w.double() + b.double()
    assert rel(y.float(), flatten_channel_major(yr)) < 5e-3
    assert torch.equal(rm, keep[0]) and torch.equal(rv, keep[1]) and int(nbt.item()) == 2, "eval mode must leave the buffers alone"
    # eval-mode backward: the statistics are constants
    dx, _, _ = ops.batchnorm_cols_bwd(x, w, mean, rstd, dy, training=False, dx_dtype=F32)
    dyd = dy.double().view(B, Cn, G).permute(0, 2, 1)
    assert rel(dx, dyd * (w.double() if affine else 1.0) / torch.sqrt(rv_ref + eps)) < 5e-3


def test_batchnorm_writes_into_a_wider_row():
    """out with a row pitch beyond C * G (the head input of the `*_proj` variants): only the first C * G columns are written"""
    shape = (2, 5, 176)
    x, _, _, _ = bn_inputs(shape, F32, False, 31)
    wide = torch.full((2, 176 * 5 + 64), 7.0, dtype=BF16, device=DEV)
    rm, rv = torch.zeros(176, device=DEV), torch.ones(176, device=DEV)
    y, _, _ = ops.batchnorm_cols_fwd(x, None, None, 1e-6, True, 0.1, rm, rv, None, out=wide)
    ref, _, _ = ops.batchnorm_cols_fwd(x, None, None, 1e-6, True, 0.1, torch.zeros(176, device=DEV), torch.ones(176, device=DEV), None)
    assert torch.equal(wide[:, :880], ref) and bool((wide[:, 880:] == 7.0).all())


# ---- 3. the models against the reference ----------------------------------------------------------------------------------------------------
def build_case(gold, tag, drop_path_rate=0.0):
    from internvideo_amd import internvideo2_ap, internvideo2_cat
    ci, kind, method, norm, _ = CASES[tag]
    cfg = O.named_config("tiny88")
    extra = {} if kind == "ap" else dict(merge_method=method, merge_norm=norm)
    mod = {"cat": internvideo2_cat, "ap": internvideo2_ap}[kind]
    m = mod.InternVideo2(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio,
                         num_frames=cfg.num_frames, drop_path_rate=drop_path_rate, attn_pool_num_heads=cfg.attn_pool_num_heads,
                         clip_embed_dim=cfg.clip_embed_dim, num_classes=NUM_CLASSES, **extra)
    sd = m.state_dict()
    params = O.synthetic_finetune_params(cfg, NUM_CLASSES, seed=40 + ci)
    load = {k: v for k, v in sd.items() if k.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked")}
    load.update({k: v for k, v in params.items() if k in sd and tuple(v.shape) == tuple(sd[k].shape)})
    pre = f"{tag}:in:"
    load.update({k[len(pre):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(pre)})
    m.load_state_dict(load, strict=True)
    video, _, _ = O.synthetic_batch(cfg, 4, 5, seed=40 + ci)
    return m.to(DEV).train(), video.float().to(DEV), cfg


def case_bar(gold, tag):
    return max(1e-2, 1.5 * float(gold[f"{tag}:bf16err:logits"][0]))


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("tag", list(CASES))
def test_probing_models_match_the_reference(gold, tag, k):
    from tests.test_flavours_gpu import check_grads
    m, video, cfg = build_case(gold, tag)
    frozen, trainable = freeze_for_probing(m, open_block_num=k, open_clip_projector=CASES[tag][4])
    assert m.frozen_prefix == cfg.depth - k and m._frozen_prefix(video) == cfg.depth - k
    pre, bar = f"{tag}:o{k}:", case_bar(gold, tag)
    labels = torch.tensor(LABELS, dtype=torch.int32, device=DEV)
    loss, logits = m.forward_loss(video, labels)
    e = rel(logits.float(), gold[pre + "logits"])
    ref = float(gold[pre + "loss"][0])
    print(f"{pre} logits rel {e:.3g} (bar {bar:.3g}), loss {loss.item():.6f} vs {ref:.6f}")
    assert e < bar, (e, bar)
    assert abs(loss.item() - ref) / abs(ref) < bar, (loss.item(), ref)
    loss.backward()
    n_grads = sum(1 for key in gold.files if key.startswith(pre + "grad:") or key.startswith(pre + "gradnorm:"))
    assert check_grads(gold, pre, m, pre + "bf16err:") >= n_grads > 0
    named = dict(m.named_parameters())
    assert all(named[n].grad is None for n in frozen), [n for n in frozen if named[n].grad is not None]
    bufs = [key for key in gold.files if key.startswith(pre + "buf:")]
    assert bool(bufs) == ("BN" in (CASES[tag][3] or "") and CASES[tag][2] != "proj")
    state = dict(m.named_buffers())
    for key in bufs:
        name = key[len(pre) + 4:]
        if name.endswith("num_batches_tracked"):
            assert int(state[name].item()) == int(gold[key]) == 1
        else:
            eb = rel(state[name], gold[key])
            assert eb < bar, (name, eb, bar)
    m.eval()
    with torch.no_grad():
        ev = m(video)
    ee = rel(ev.float(), gold[pre + "eval_logits"])
    assert ee < bar, ("eval logits", ee, bar)
    assert all(int(b.item()) == 1 for n, b in m.named_buffers() if n.endswith("num_batches_tracked")), "eval mode moved the BatchNorm buffers"


def test_proj_variants_take_the_pool_query_from_the_stream_pass(gold, monkeypatch):
    """`*_proj`: the all-token mean AttentionPoolingBlock uses as its query comes out of the pass that pools the stream for the head, so
    ops.token_mean_fwd (a second read of the whole stream) is not called; the plain `proj` head has no such pass and keeps it"""
    calls = []
    real = ops.token_mean_fwd
    monkeypatch.setattr(ops, "token_mean_fwd", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    labels = torch.tensor(LABELS, dtype=torch.int32, device=DEV)
    for tag, want in (("cls_avgN_proj_BN", 0), ("cls_avg1_proj_LN", 0), ("proj_open", 1)):
        m, video, cfg = build_case(gold, tag)
        freeze_for_probing(m, open_block_num=1)
        calls.clear()
        loss, _ = m.forward_loss(video, labels)
        loss.backward()
        assert len(calls) == want, (tag, len(calls))


# ---- 4. the frozen-prefix path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop_path_rate", [0.0, 0.3])
def test_frozen_prefix_agrees_with_the_whole_autograd_stack(gold, monkeypatch, drop_path_rate):
    """frozen_prefix = depth - 1 against the same frozen model run whole through BlockStackFn (the attribute removed): logits and the open
    block's gradients at the bars of the model tests (not bitwise: the forward-only loop asks fc1 for no gelu' copy).  With DropPath the
    two runs share their draws (`_dp_uniform`): the frozen prefix applies them through block_stack_infer's rowscale."""
    tag = "cls_avgN_proj_BN"
    calls = {"infer": 0, "stack_depth": []}
    infer, fwd = Fn.block_stack_infer, Fn.BlockStackFn.forward

    def spy_infer(*a, **kw):
        calls["infer"] += 1
        return infer(*a, **kw)
    monkeypatch.setattr(Fn, "block_stack_infer", spy_infer)
    labels = torch.tensor(LABELS, dtype=torch.int32, device=DEV)
    out = {}
    for mode in ("prefix", "whole"):
        m, video, cfg = build_case(gold, tag, drop_path_rate=drop_path_rate)
        freeze_for_probing(m, open_block_num=1)
        if mode == "whole":
            del m.frozen_prefix
        if drop_path_rate:
            u = torch.rand((cfg.depth, 2, 4), generator=torch.Generator().manual_seed(3))
            u[0, 0, 1] = 0.0; u[1, 1, 2] = 0.0; u[2, 0, 3] = 0.0          # a dropped sample in the prefix and in the open block
            m._dp_uniform = u
        before = calls["infer"]
        loss, logits = m.forward_loss(video, labels)
        assert (calls["infer"] - before) == (1 if mode == "prefix" else 0)
        loss.backward()
        grads = {n: p.grad.detach().float().clone() for n, p in m.named_parameters() if p.grad is not None}
        out[mode] = (logits.float(), loss.item(), grads)
    bar = case_bar(gold, tag)
    assert rel(out["prefix"][0], out["whole"][0]) < bar
    assert abs(out["prefix"][1] - out["whole"][1]) / abs(out["whole"][1]) < bar
    assert set(out["prefix"][2]) == set(out["whole"][2]) and any(n.startswith(f"blocks.{cfg.depth - 1}.") for n in out["prefix"][2])
    assert not any(n.startswith("blocks.0.") or n.startswith("blocks.1.") for n in out["prefix"][2])
    worst = {n: rel(g, out["whole"][2][n]) for n, g in out["prefix"][2].items()}
    bad = {n: e for n, e in worst.items() if e > 3e-2}
    assert not bad, bad
    if drop_path_rate:                                                   # and the draws did reach the result
        m, video, cfg = build_case(gold, tag, drop_path_rate=0.0)
        freeze_for_probing(m, open_block_num=1)
        _, plain = m.forward_loss(video, labels)
        assert rel(plain.float(), out["prefix"][0]) > 1e-3


def test_frozen_prefix_needs_a_frozen_prefix(gold):
    """the attribute alone is not honoured: one trainable parameter below it, or a clip that needs a gradient, keeps the autograd stack"""
    m, video, cfg = build_case(gold, "proj_open")
    m.frozen_prefix = cfg.depth
    assert m._frozen_prefix(video) == 0
    freeze_for_probing(m)
    assert m._frozen_prefix(video) == cfg.depth
    m.blocks[1].ls1.gamma.requires_grad = True
    assert m._frozen_prefix(video) == 0
    m.blocks[1].ls1.gamma.requires_grad = False
    assert m._frozen_prefix(video.clone().requires_grad_(True)) == 0
    with torch.no_grad():
        m.frozen_prefix = 1
        assert m._frozen_prefix(video) == cfg.depth                     # nothing is recorded: the whole trunk is forward-only


def _forward_footprint(gold, k, whole):
    """-> (bytes still allocated after a forward, peak bytes during it), both relative to the allocation level before it"""
    labels = torch.tensor(LABELS, dtype=torch.int32, device=DEV)
    m, video, cfg = build_case(gold, "cls_avgN_kBN")
    freeze_for_probing(m, open_block_num=k)
    if whole:
        del m.frozen_prefix
    loss, _ = m.forward_loss(video, labels)                              # warm-up: one-time caches (index tables)
    del loss
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss, _ = m.forward_loss(video, labels)
    torch.cuda.synchronize()
    held, peak = torch.cuda.memory_allocated() - before, torch.cuda.max_memory_allocated() - before
    del loss
    return held, peak


def test_frozen_trunk_saves_no_activations(gold):
    """depth 3, B = 4, M = 260 rows of D = 176; one fp32 stream = M D 4 bytes.  A block's saved tuple is ~42 bytes per token and channel
    (BlockStackFn.forward), i.e. 10.5 streams.
    All blocks frozen: what the forward leaves allocated (the head's autograd graph included) is below 3 streams.  The whole stack leaves
    nothing either once it has returned (no input needs a gradient, so autograd drops the context) -- but it HOLDS all three blocks' tuples
    while it runs: its peak is above 30 streams, the forward-only loop's below 12 (residual in and out, the packed qkv, the fc1 output and
    the bf16 rows between them: about 8).
    One open block: the whole stack keeps the three tuples until backward (above 30 streams), the frozen prefix only the open block's
    (10.5 streams plus the head's: below 14)."""
    stream = 4 * 65 * 176 * 4
    held_p, peak_p = _forward_footprint(gold, 0, whole=False)
    held_w, peak_w = _forward_footprint(gold, 0, whole=True)
    print(f"all frozen: held {held_p} / {held_w} B, peak {peak_p} / {peak_w} B (frozen prefix / whole stack), one fp32 stream {stream} B")
    assert held_p <= 3 * stream, (held_p, stream)
    assert peak_p < 12 * stream and peak_w > 30 * stream, (peak_p, peak_w, stream)
    held_p1, _ = _forward_footprint(gold, 1, whole=False)
    held_w1, _ = _forward_footprint(gold, 1, whole=True)
    print(f"one open block: held {held_p1} / {held_w1} B")
    assert held_p1 < 14 * stream and held_w1 > 30 * stream, (held_p1, held_w1, stream)


# ---- 5. the training engine ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1])
def test_engine_step_changes_exactly_the_trainable_parameters(gold, k):
    from internvideo_amd.engine import IVTrainEngine
    m, video, cfg = build_case(gold, "cls_avgN_proj_BN")
    frozen, trainable = freeze_for_probing(m, open_block_num=k)
    eng = IVTrainEngine(m, lr=1e-3)
    assert sorted(n for n, _ in eng.mat_params + eng.vec_params) == sorted(trainable)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    labels = torch.tensor(LABELS, dtype=torch.int32, device=DEV)
    loss, _ = eng.train_step_fn(lambda: m.forward_loss(video.to(BF16), labels, smoothing=0.1))
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()
    after = dict(m.named_parameters())
    changed = sorted(n for n in before if not torch.equal(before[n], after[n].detach()))
    assert changed == sorted(trainable), (sorted(set(trainable) - set(changed)), sorted(set(changed) - set(trainable)))
    assert int(m.down_norm.num_batches_tracked.item()) == 1
    eng.close()


def test_ds_compat_step_on_a_frozen_model(gold):
    from types import SimpleNamespace
    from internvideo_amd import ds_compat
    m, video, cfg = build_case(gold, "ap")
    frozen, trainable = freeze_for_probing(m, open_block_num=1)
    args = SimpleNamespace(lr=1e-3, weight_decay=0.05, opt_betas=(0.9, 0.999), opt_eps=1e-8, clip_grad=None, update_freq=1)
    model, optimizer, _, _ = ds_compat.initialize(args=args, model=m, model_parameters=None, dist_init_required=False)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    model.train(); model.zero_grad()
    logits = model(video.to(BF16))
    loss = torch.nn.functional.cross_entropy(logits.float(), torch.tensor(LABELS, device=DEV))
    model.backward(loss); model.step()
    torch.cuda.synchronize()
    changed = sorted(n for n, p in m.named_parameters() if not torch.equal(before[n], p.detach()))
    assert changed == sorted(trainable), (sorted(set(trainable) - set(changed)), sorted(set(changed) - set(trainable)))


@pytest.mark.parametrize("k,mixed", [(0, True), (1, False)])
def test_captured_probe_step_replays_like_eager_steps(gold, k, mixed):
    """capture_fn + three replays against three eager steps over the same frozen model (k = 0: no block hook ever fires; k = 1: one open block):
    loss trajectory, weights and BatchNorm buffers bit for bit.  The BatchNorm kernel updates its buffers in device memory, so every replay
    counts: num_batches_tracked == 3 + the capture's warm-up passes.  `mixed`: forward_loss reads the finetune.Mixup table."""
    from internvideo_amd import finetune
    from internvideo_amd.engine import IVTrainEngine
    WARMUP = 2
    one = int(np.float32(1.0).view(np.int32))
    l3, l7 = int(np.float32(0.3).view(np.int32)), int(np.float32(0.7).view(np.int32))
    def table(kind, lam, oml):                                           # (src, kind, box, bits(lam), bits(oml)) per clip: finetune.MixParams
        t = np.zeros((4, 8), dtype=np.int32)
        t[:, 0], t[:, 1], t[:, 6], t[:, 7] = 3 - np.arange(4), kind, lam, oml
        return t
    steps = [(table(0, one, 0), np.array([[1, 0]] * 4, dtype=np.float32), [3, 7, 1, 9]),
             (table(1, l3, l7), np.array([[0.3, 0.7]] * 4, dtype=np.float32), [1, 9, 0, 4]),
             (table(0, one, 0), np.array([[1, 0]] * 4, dtype=np.float32), [0, 4, 2, 8])]
    mixer = finetune.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=NUM_CLASSES)
    traj = {}
    for tag in ("eager", "graph"):
        m, video, cfg = build_case(gold, "cls_avgN_proj_BN")
        freeze_for_probing(m, open_block_num=k)
        eng = IVTrainEngine(m, lr=1e-3)
        static = finetune.MixParams(steps[0][0], steps[0][1]).to(DEV)
        labels = torch.tensor(steps[0][2], dtype=torch.int32, device=DEV)
        vb = video.to(BF16)

        def loss_fn():
            if not mixed:
                return m.forward_loss(vb, labels, smoothing=0.1)
            x, a, b, mix = mixer.apply(video, labels, static)
            return m.forward_loss(x, a, b, mix, smoothing=0.1)
        dn = m.down_norm
        if tag == "graph":
            init = (dn.running_mean.clone(), dn.running_var.clone())
            eng.capture_fn(loss_fn, warmup=WARMUP)
            torch.cuda.synchronize()
            assert int(dn.num_batches_tracked.item()) == WARMUP          # the warm-up passes ran eagerly, the capture itself ran nothing
            dn.running_mean.copy_(init[0]); dn.running_var.copy_(init[1])   # the running averages restart; the counter keeps counting
        losses = []
        for table, tmix, lab in steps:
            static.copy_(finetune.MixParams(table, tmix))
            labels.copy_(torch.tensor(lab, dtype=torch.int32))
            out = eng.train_step_graphed() if tag == "graph" else eng.train_step_fn(loss_fn)
            losses.append(out[0].detach().clone())
        torch.cuda.synchronize()
        traj[tag] = (torch.stack([l.reshape(()) for l in losses]).cpu(), eng.master.clone(), dn.running_mean.clone(), dn.running_var.clone(),
                     int(dn.num_batches_tracked.item()))
        eng.close()
        del eng, m
    assert torch.equal(traj["eager"][0], traj["graph"][0]), (traj["eager"][0].tolist(), traj["graph"][0].tolist())
    assert len(set(traj["eager"][0].tolist())) == 3
    assert torch.equal(traj["eager"][1], traj["graph"][1]), "weights after three steps"
    assert torch.equal(traj["eager"][2], traj["graph"][2]) and torch.equal(traj["eager"][3], traj["graph"][3]), "BatchNorm running buffers"
    assert traj["eager"][4] == 3 and traj["graph"][4] == 3 + WARMUP
