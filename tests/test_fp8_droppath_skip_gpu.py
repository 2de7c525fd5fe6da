"""DropPath sample skipping on the fp8 (e4m3) GEMM path -- BASELINE configs[4] with the recipe's drop_path (include/internvideo_hip.h
"fp8 UNDER DropPath SKIPPING", functional.BlockStackFn with meta["fp8"]).  In the style of tests/test_droppath_skip_gpu.py: every kernel that
takes a device-side count is checked against the SAME kernel run on the kept rows alone, with NaN poison (bf16 NaN rows, e4m3 NaN bytes 0x7f)
in everything it must not read and sentinels in everything it must not write; both sides of every bitwise comparison run on the 256^2 e4m3
kernel (ivh_set_gemm_fp8_kernel(2)) with the tail split off.  The block stack is anchored to the non-skipping fp8 run on a draw that keeps
every sample (bitwise), and held to the bars of tests/test_fp8_gpu.py against the bf16 skipping run on random draws -- fp8 skipping is NOT
bitwise the multiply-by-zero run: the per-tensor amax is taken over the kept rows only.  Runs only on a real MI355X (`-m gpu`)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from internvideo_amd import lib as L_  # noqa: E402
from internvideo_amd import ops  # noqa: E402
from internvideo_amd.lib import InternVideoHipError  # noqa: E402
from oracle import internvideo2_oracle as O  # noqa: E402
from tests.test_droppath_skip_gpu import _build, _cfg, _run, cnt, randn, rel  # noqa: E402

DEV = "cuda"
BF16, F32, FP8, U8 = torch.bfloat16, torch.float32, torch.float8_e4m3fn, torch.uint8
LC = 1025                                                                    # tokens per clip of the 6B encoder at 16 x 224^2
NAN8 = 0x7f                                                                  # e4m3fn NaN


def u8(t):
    return t.view(U8)


def nan8(*shape):
    return torch.full(shape, NAN8, dtype=U8, device=DEV).view(FP8)


def kept_rows(M, frac, L=LC):
    """as tests/test_droppath_skip_gpu.py:75-78: whole clips, plus a ragged count"""
    Mk = int(round(M * frac))
    if 0 < Mk < M:
        Mk = Mk // L * L + (5 if frac < 0.5 else 0)
        Mk = max(1, min(Mk, M - 1))
    return Mk


@pytest.fixture
def plain_tiles8():
    """whole 256 x 256 tiles on both GEMM families (no K split of the tail round, no half-width tiles) and the 256^2 e4m3 kernel at every
    size: the reference launch on the kept rows alone then runs the kernel, tile order and K order of the count-carrying launch"""
    lib = L_.load()
    lib.ivh_gemm256_debug_split(0); lib.ivh_gemm256_debug_half(0)
    ops.set_gemm_kernel(2); ops.set_gemm_fp8_kernel(2)
    yield
    ops.set_gemm_kernel(0); ops.set_gemm_fp8_kernel(0)
    lib.ivh_gemm256_debug_split(1); lib.ivh_gemm256_debug_half(1)


FRACS = [0.0, 0.31, 0.875, 1.0]


# ---- 1. quantisation of the kept rows only ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(2 * LC, 3200), (2 * LC, 12800), (LC + 5, 9600), (16 * LC, 3200)])
@pytest.mark.parametrize("frac", FRACS)
def test_fp8_quantize_follows_m_dev(M, K, frac):
    """fp8_quantize(x, want_transposed=True, m_dev=c) with x[c:] = NaN: q[:c], the scale and qt[:, :c] bit-identical to fp8_quantize(x[:c]);
    q[c:] keeps its sentinel, qt holds zeros from c to the next multiple of 16 and its sentinel behind; the scale is finite, the floor for
    c = 0.  Delayed flavour: amax_next is the bit pattern of max|x[:c]|, and an Inf planted behind the count leaves it unchanged."""
    if M > 10000 and frac in (0.0, 0.31):
        pytest.skip("large case: two fractions are enough")
    c = kept_rows(M, frac)
    md = cnt(c)
    x = randn(M, K, seed=M + K, scale=3.0)
    x[c:] = float("nan")
    M16, c16 = (M + 15) // 16 * 16, (c + 15) // 16 * 16
    q, qt = nan8(M, K), nan8(K, M16)
    q, qt, s = ops.fp8_quantize(x, want_transposed=True, m_dev=md, out=(q, qt))
    assert torch.isfinite(s).item()
    assert bool((u8(q[c:]) == NAN8).all()), "rows behind the count were written"
    assert bool((u8(qt[:, c16:]) == NAN8).all()), "columns behind the zero fill were written"
    assert bool((u8(qt[:, c:c16]) == 0).all()), "the weight gradient's K mask needs zeros up to the next multiple of 16"
    if c == 0:
        floor = 1e-12 / 448.0
        assert abs(s.item() - floor) <= 1e-6 * floor, s.item()               # (relative bar of test_fp8_gpu.py::test_fp8_quantize_is_bit_exact)
    else:
        qr, qtr, sr = ops.fp8_quantize(x[:c].contiguous(), want_transposed=True)
        assert torch.equal(s, sr), (s.item(), sr.item())
        assert torch.equal(u8(q[:c]), u8(qr)) and torch.equal(u8(qt[:, :c]), u8(qtr[:, :c]))
    # delayed flavour: quantise with a given amax, collect this call's own over the kept rows only
    amax = (x[:c].float().abs().max() if c else torch.zeros((), device=DEV)).reshape(1)
    prev = amax.clamp_min(1.0)
    nxt = torch.zeros(1, dtype=torch.int32, device=DEV)
    q2, qt2 = nan8(M, K), nan8(K, M16)
    q2, qt2, s2 = ops.fp8_quantize(x, want_transposed=True, amax_prev=prev, amax_next=nxt, m_dev=md, out=(q2, qt2))
    assert torch.equal(nxt, amax.view(torch.int32)), (nxt.view(F32).item(), amax.item())
    assert bool((u8(q2[c:]) == NAN8).all()) and bool((u8(qt2[:, c16:]) == NAN8).all()) and bool((u8(qt2[:, c:c16]) == 0).all())
    if c:
        nr = torch.zeros(1, dtype=torch.int32, device=DEV)
        qr2, qtr2, sr2 = ops.fp8_quantize(x[:c].contiguous(), want_transposed=True, amax_prev=prev, amax_next=nr)
        assert torch.equal(s2, sr2) and torch.equal(u8(q2[:c]), u8(qr2)) and torch.equal(u8(qt2[:, :c]), u8(qtr2[:, :c])) and torch.equal(nxt, nr)
    if c < M:
        x[c, 3] = float("inf")
        ops.fp8_quantize(x, want_transposed=True, amax_prev=prev, amax_next=nxt, m_dev=md)
        assert torch.equal(nxt, amax.view(torch.int32))
        _, _, s3 = ops.fp8_quantize(x, want_transposed=True, m_dev=md)
        assert torch.equal(s3, s)


# ---- 2. / 4. / 5. forward and dgrad GEMMs with m_dev --------------------------------------------------------------------------------------
def _weights(w, channel):
    """(wq, s_fwd, wqt, s_dgrad) per-tensor or per-channel (`_cs` entry point)"""
    if channel:
        wq, wqt, sr, sc = ops.fp8_quantize_weight(w)
        return wq, sr, wqt, sc
    wq, wqt, sw = ops.fp8_quantize(w, want_transposed=True)
    return wq, sw, wqt, sw


@pytest.mark.parametrize("M,N,K", [(2 * LC, 9600, 3200), (3 * LC, 3200, 3200), (2 * LC, 12800, 3200), (2 * LC, 3200, 12800), (834, 1408, 512),
                                   (834, 1408, 256), (16 * LC, 3200, 3200)])
@pytest.mark.parametrize("frac", FRACS)
def test_gemm_fp8_forward_and_dgrad_follow_m_dev(M, N, K, frac, plain_tiles8):
    """forward plain (+ bias), forward GELU + gelu' copy, dgrad plain, dgrad x gelu' with the bias-gradient partials, each with per-tensor and
    per-channel weight scales: the first *m_dev rows equal the same call on the kept rows alone BITWISE, rows behind them keep their
    sentinel; the e4m3 operand rows behind the count are NaN bytes and the gelu' operand rows NaN, never read.  (834, 1408, 512) sits on
    the edge of the size heuristic of a plain launch (M * N >= 512^2 and K >= 512) and (834, 1408, 256) under it in both directions
    (forward: K = 256; dgrad: M * N = 834 x 256 < 512^2): a count-carrying descriptor runs on the 256^2 kernel all the same.
    fc1 bias gradient (the x gelu' launch's column sums, reduced by ivh_colsum_finish_dyn) against the fp32 column sum of the kept rows of
    du: rel-L2 < 4e-3, the bar test_droppath_skip_gpu.py::test_block_stack_skip_equals_multiply_by_zero holds every gradient that is a sum
    over token rows to (mlp.fc1.bias among them)."""
    if M > 10000 and frac in (0.0, 0.31):
        pytest.skip("large case: two fractions are enough")
    L = 417 if M == 834 else LC
    Mk = kept_rows(M, frac, L)
    md = cnt(Mk)
    a = randn(M, K, seed=1)
    a[Mk:] = float("nan")
    dy = randn(M, N, seed=4)
    dy[Mk:] = float("nan")
    w = randn(N, K, seed=2, scale=K ** -0.5)
    bias = randn(N, seed=3, dtype=F32)
    du_in = randn(M, K, seed=5)
    du_in[Mk:] = float("nan")
    aq, _, sa = ops.fp8_quantize(a, m_dev=md, out=(nan8(M, K), None))
    dyq, _, sd = ops.fp8_quantize(dy, m_dev=md, out=(nan8(M, N), None))
    if Mk:
        aqr, _, sar = ops.fp8_quantize(a[:Mk].contiguous())
        dyqr, _, sdr = ops.fp8_quantize(dy[:Mk].contiguous())
        assert torch.equal(sa, sar) and torch.equal(sd, sdr)
    SENT = 7.0
    for channel in (False, True):
        wq, sf, wqt, sg = _weights(w, channel)
        # forward, plain epilogue
        out = torch.full((M, N), SENT, dtype=BF16, device=DEV)
        ops.gemm_fp8(aq, wq, sa, sf, bias=bias, out=out, m_dev=md)
        if Mk:
            assert torch.equal(out[:Mk], ops.gemm_fp8(aqr, wq, sar, sf, bias=bias)), ("fwd", channel)
        assert bool((out[Mk:] == SENT).all())
        # forward, GELU + gelu' copy
        out = torch.full((M, N), SENT, dtype=BF16, device=DEV)
        g, u = ops.gemm_fp8(aq, wq, sa, sf, bias=bias, act="gelu_erf_d", want_preact=True, out=out, m_dev=md)
        if Mk:
            gr, ur = ops.gemm_fp8(aqr, wq, sar, sf, bias=bias, act="gelu_erf_d", want_preact=True)
            assert torch.equal(g[:Mk], gr) and torch.equal(u[:Mk], ur), ("fwd gelu", channel)
        assert bool((out[Mk:] == SENT).all())
        # dgrad: dy [M, N] x W^T copy [K, N]
        out = torch.full((M, K), SENT, dtype=BF16, device=DEV)
        ops.gemm_fp8(dyq, wqt, sd, sg, k=N, out=out, m_dev=md)
        if Mk:
            assert torch.equal(out[:Mk], ops.gemm_fp8(dyqr, wqt, sdr, sg, k=N)), ("dgrad", channel)
        assert bool((out[Mk:] == SENT).all())
        # dgrad x gelu' with the column sums
        out = torch.full((M, K), SENT, dtype=BF16, device=DEV)
        dx, part = ops.gemm_fp8(dyq, wqt, sd, sg, k=N, dact_in=du_in, act="gelu_erf_d", out=out, m_dev=md, want_colsum=True)
        cs = ops.colsum_finish(part, m_dev=md)
        assert bool(torch.isfinite(cs).all())
        if Mk:
            assert torch.equal(dx[:Mk], ops.gemm_fp8(dyqr, wqt, sdr, sg, k=N, dact_in=du_in[:Mk].contiguous(), act="gelu_erf_d")), ("dgrad gelu'", channel)
            want = dx[:Mk].float().sum(0)
            e = rel(cs, want)
            print(f"fc1 bias gradient M={M} N={N} K={K} kept={Mk} channel={channel}: rel-L2 {e:.3e}")
            assert e < 4e-3, e
        else:
            assert bool((cs == 0).all())
        assert bool((out[Mk:] == SENT).all())


def test_gemm_fp8_rejects_what_the_count_carrying_kernel_cannot_do(plain_tiles8):
    M, N, K = 512, 512, 512
    a = randn(M, K, seed=1); w = randn(N, K, seed=2, scale=0.05)
    aq, _, sa = ops.fp8_quantize(a); wq, _, sw = ops.fp8_quantize(w)
    md = cnt(300)
    ops.gemm_fp8(aq, wq, sa, sw, m_dev=md)                                   # the plain launch is fine
    with pytest.raises(InternVideoHipError):
        ops.gemm_fp8(aq, wq, sa, sw, m_dev=md, out_fp32=True)
    with pytest.raises(InternVideoHipError):
        ops.gemm_fp8(aq, wq, sa, sw, m_dev=md, act="gelu_tanh")
    with pytest.raises(InternVideoHipError):
        ops.gemm_fp8(aq, wq, sa, sw, m_dev=md, k_dev=md)
    with pytest.raises(InternVideoHipError):
        ops.gemm_fp8(aq, wq, sa, sw, m_dev=md, act="gelu", want_preact=True)  # a pre-activation copy outside the gelu' exchange
    with pytest.raises(InternVideoHipError):
        ops.gemm_fp8(aq, wq, sa, sw, m_dev=torch.tensor([300], dtype=torch.int64, device=DEV))
    with pytest.raises(InternVideoHipError):
        ops.fp8_quantize(a, m_dev=torch.tensor([300], dtype=torch.int32))     # the count lives in HBM
    ops.set_gemm_fp8_kernel(1)                                                # even with the 128^2 kernel forced: the 256^2 one, rows behind the count untouched
    out = torch.full((M, N), 7.0, dtype=BF16, device=DEV)
    ops.gemm_fp8(aq, wq, sa, sw, m_dev=md, out=out)
    assert bool((out[300:] == 7.0).all()) and bool(torch.isfinite(out[:300]).all())


# ---- 3. weight gradient with k_dev ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,Kf", [(2 * LC, 9600, 3200), (3 * LC, 3200, 3200), (2 * LC, 12800, 3200), (2 * LC, 3200, 12800), (16 * LC, 3200, 3200)])
@pytest.mark.parametrize("frac", FRACS)
def test_fp8_weight_gradient_follows_k_dev(M, N, Kf, frac, plain_tiles8):
    """dW[n, k] = sum_m dy[m, n] x[m, k] on the transposed copies, both K-contiguous with the token rows along K: contraction over the first
    *k_dev token columns, bitwise equal to the product built from quantising the kept rows alone; e4m3 NaN bytes behind the count (from the
    next multiple of 16 on: up to there the quantiser writes the zeros the 16-byte K mask relies on) in both copies are never read; a count
    of 0 writes exact zeros."""
    if M > 10000 and frac in (0.0, 0.31):
        pytest.skip("large case: two fractions are enough")
    c = kept_rows(M, frac)
    md = cnt(c)
    M16, c16 = (M + 15) // 16 * 16, (c + 15) // 16 * 16
    dy = randn(M, N, seed=10, scale=0.1)
    x = randn(M, Kf, seed=20)
    dy[c:] = float("nan"); x[c:] = float("nan")
    _, dyqt, sd = ops.fp8_quantize(dy, want_transposed=True, m_dev=md, out=(nan8(M, N), nan8(N, M16)))
    _, xqt, sx = ops.fp8_quantize(x, want_transposed=True, m_dev=md, out=(nan8(M, Kf), nan8(Kf, M16)))
    assert bool((u8(dyqt[:, c16:]) == NAN8).all()) and bool((u8(xqt[:, c16:]) == NAN8).all())
    out = torch.full((N, Kf), 3.0, dtype=BF16, device=DEV)
    got = ops.gemm_fp8(dyqt, xqt, sd, sx, out=out, k_dev=md)
    assert bool(torch.isfinite(got).all())
    if c == 0:
        assert bool((got == 0).all())
        return
    _, dyqtr, sdr = ops.fp8_quantize(dy[:c].contiguous(), want_transposed=True)
    _, xqtr, sxr = ops.fp8_quantize(x[:c].contiguous(), want_transposed=True)
    ref = ops.gemm_fp8(dyqtr, xqtr, sdr, sxr)
    assert torch.equal(got, ref)
    full = dy[:c].float().t() @ x[:c].float()
    assert rel(got.float(), full) < 6e-2                                     # (e4m3 operands: the bar of test_fp8_gpu.py's Linear test)


# ---- the block stack ------------------------------------------------------------------------------------------------------------------------
def _fp8_run(cfg, params, batch, U, skip, fp8=True, scaling="current", steps=1, **kw):
    video, mask, targets = batch
    model = _build(cfg, params, 0.5, skip, **kw)
    model.fp8_gemm = fp8
    model.fp8_scaling = scaling
    res = []
    for _ in range(steps):
        model.zero_grad(set_to_none=True)
        res.append(_run(model, video, mask, targets, U))
    hist = getattr(model, "_fp8_hist", None)
    return res if steps > 1 else res[0], hist


def _fixture(cfg_name, B=6, seed=5):
    cfg = _cfg(cfg_name)
    return cfg, O.synthetic_params(cfg, seed=seed), O.synthetic_batch(cfg, B, 6, seed=seed)


def _count_plans(fn):
    """run fn() and return (its result, number of ops.droppath_plan calls): proof that the skipping path ran"""
    calls = []
    orig = ops.droppath_plan
    ops.droppath_plan = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        return fn(), len(calls)
    finally:
        ops.droppath_plan = orig


@pytest.mark.parametrize("cfg_name", ["tiny88", "hd128"])
def test_fp8_skip_with_every_sample_kept_equals_the_non_skipping_fp8_run(cfg_name, plain_tiles8):
    """anchor to the existing path: a draw that keeps every sample (U = 0.999 everywhere) -- same rows, same amax -- the skipping fp8 run
    against the fp8 run with drop_path_skip = False on the same forced kernel: loss and outputs bitwise, weight gradients bitwise (tail
    split off); the gradients that are column sums over token rows (the fc1 bias comes out of the dgrad epilogue in fp32 under skipping, from
    the bf16 rows otherwise; the q/k-norm partial sums are split over another number of workgroups) to 4e-3, the bar of
    test_droppath_skip_gpu.py::test_block_stack_skip_equals_multiply_by_zero."""
    cfg, params, batch = _fixture(cfg_name)
    U = torch.full((cfg.depth, 2, 6), 0.999)
    (l0, o0, g0), _ = _fp8_run(cfg, params, batch, U, False)
    ((l1, o1, g1), _), plans = _count_plans(lambda: _fp8_run(cfg, params, batch, U, True))
    assert plans, "the skipping path did not run"
    assert torch.isfinite(l0).item() and torch.equal(l0, l1), (l0.item(), l1.item())
    for a, b in zip(o0, o1):
        assert torch.equal(a, b)
    assert g0.keys() == g1.keys()
    mats = [k for k in g0 if k.startswith("blocks.") and g0[k].dim() == 2]
    assert len(mats) == 4 * cfg.depth
    for k in mats:
        assert torch.equal(g0[k], g1[k]), k
    bad = {k: rel(g1[k], g0[k]) for k in g0 if float(g0[k].abs().max()) > 0 and rel(g1[k], g0[k]) > 4e-3}
    assert not bad, bad


@pytest.mark.parametrize("cfg_name", ["tiny88", "hd128"])
def test_fp8_skip_with_a_fully_dropped_branch(cfg_name, plain_tiles8):
    """block 1's attention branch loses every sample (count 0): scales at their floor, no tile runs, weight gradients written as zeros --
    everything stays finite and the gradients of that branch's parameters are exactly zero"""
    cfg, params, batch = _fixture(cfg_name)
    U = torch.rand((cfg.depth, 2, 6), generator=torch.Generator().manual_seed(3))
    U[1, 0] = 0.0
    U[1, 1] = 0.999
    ((loss, outs, grads), _), plans = _count_plans(lambda: _fp8_run(cfg, params, batch, U, True))
    assert plans
    assert torch.isfinite(loss).item() and all(bool(torch.isfinite(o.float()).all()) for o in outs)
    for k, g in grads.items():
        assert bool(torch.isfinite(g.float()).all()), k
    for name in ("attn.qkv.weight", "attn.proj.weight", "attn.proj.bias", "attn.q_norm.weight", "attn.k_norm.weight", "ls1.gamma"):
        g = grads["blocks.1." + name]
        assert float(g.float().abs().max()) == 0.0, name
    assert float(grads["blocks.1.mlp.fc1.weight"].float().abs().max()) > 0.0   # the MLP branch of the same block kept every sample


@pytest.mark.parametrize("cfg_name", ["tiny88", "hd128"])
def test_fp8_skip_tracks_the_bf16_skip_run_on_random_draws(cfg_name, plain_tiles8):
    """the bars the project holds the fp8 block stack to against its bf16 run (tests/test_fp8_gpu.py::
    test_block_stack_on_fp8_gemms_tracks_the_bf16_run_and_the_oracle: loss 2e-2 relative, gradients 0.25 rel-L2, cosine > 0.97, the same two
    cross-attention key-bias gradients set aside), here with DropPath 0.5 and skipping on both sides, same draws"""
    cfg, params, batch = _fixture(cfg_name)
    U = torch.rand((cfg.depth, 2, 6), generator=torch.Generator().manual_seed(11))
    (lb, _, gb), _ = _fp8_run(cfg, params, batch, U, True, fp8=False)
    ((l8, _, g8), _), plans = _count_plans(lambda: _fp8_run(cfg, params, batch, U, True))
    assert plans
    print(f"{cfg_name}: loss bf16-skip {lb.item():.6f} fp8-skip {l8.item():.6f}")
    assert abs(l8.item() - lb.item()) < 2e-2 * abs(lb.item()), (l8.item(), lb.item())
    worst = {}
    for k, g in gb.items():
        a, b = g.double().flatten().cpu(), g8[k].double().flatten().cpu()
        if float(a.abs().max()) == 0.0 and float(b.abs().max()) == 0.0:       # a branch no sample kept: both sides exactly zero
            continue
        cos = float((a @ b) / (a.norm() * b.norm()).clamp_min(1e-30))
        worst[k] = (rel(g8[k], g), cos)
    worst = {k: v for k, v in worst.items() if not k.startswith("clip_projector.cross_attn.k_bias") and not k.startswith("clip_projector.norm1_k.bias")}
    print(f"{cfg_name}: worst rel-L2 {max(v[0] for v in worst.values()):.4f}, worst cosine {min(v[1] for v in worst.values()):.5f}")
    bad = {k: v for k, v in worst.items() if v[0] > 0.25 or v[1] < 0.97}
    assert not bad, dict(list(bad.items())[:8])


@pytest.mark.parametrize("cfg_name", ["tiny88", "hd128"])
@pytest.mark.parametrize("scaling", ["current", "delayed"])
def test_fp8_skip_recomputation_is_bit_identical(cfg_name, scaling, plain_tiles8):
    """use_checkpoint / checkpoint_num = 2: the recomputed blocks quantise the same kept rows with the same scales -- loss and every gradient
    bit-identical to the run that saved its activations; with delayed scaling over two steps (step 2 quantises with the amax step 1
    recorded over the kept rows), and the history holds no NaN or Inf after either step although the rows behind the counts are stale memory"""
    cfg, params, batch = _fixture(cfg_name)
    U = torch.rand((cfg.depth, 2, 6), generator=torch.Generator().manual_seed(3))
    U[1, 0] = 0.0                                                            # a site that sees no row at all
    steps = 2 if scaling == "delayed" else 1
    plain, h0 = _fp8_run(cfg, params, batch, U, True, scaling=scaling, steps=steps)
    cp, h1 = _fp8_run(cfg, params, batch, U, True, scaling=scaling, steps=steps, use_checkpoint=True, checkpoint_num=2)
    if steps == 1:
        plain, cp = [plain], [cp]
    for (l0, _, g0), (l1, _, g1) in zip(plain, cp):
        assert torch.isfinite(l0).item() and torch.equal(l0, l1), (l0.item(), l1.item())
        assert g0.keys() == g1.keys()
        for k in g0:
            assert torch.equal(g0[k], g1[k]), k
    if scaling == "delayed":
        for h in (h0, h1):
            assert h is not None and len(h.slot) == 8 * cfg.depth
            assert bool(torch.isfinite(h.cur).all()) and bool(torch.isfinite(h.nxt.view(F32)).all())
        assert torch.equal(h0.cur, h1.cur) and torch.equal(h0.nxt, h1.nxt)


def test_fp8_delayed_history_is_clean_after_the_first_step(plain_tiles8):
    """after step 1 of the delayed-scaling fp8-skip run every recorded amax is finite (nothing behind a count reached it), and the site that
    saw no row recorded 0"""
    cfg, params, batch = _fixture("tiny88")
    U = torch.rand((cfg.depth, 2, 6), generator=torch.Generator().manual_seed(3))
    U[1, 0] = 0.0
    _, h = _fp8_run(cfg, params, batch, U, True, scaling="delayed", steps=1)
    n = len(h.slot)
    assert n == 8 * cfg.depth
    rec = h.nxt[:n].view(F32)
    assert bool(torch.isfinite(rec).all()) and bool(torch.isfinite(h.cur).all())
    for name in ("n1", "att", "d:att", "d:n1"):
        assert rec[h.slot[(1, name)]].item() == 0.0, name
    assert rec[h.slot[(1, "n2")]].item() > 0.0


def test_fp8_skip_graph_replay_equals_eager(plain_tiles8):
    """the native training step on fp8 GEMMs with DropPath skipping: eager steps == replays of ONE captured HIP graph, bitwise in the loss,
    over three draws that keep different numbers of samples (one drops a whole branch) -- the kept counts, the scales taken over the kept
    rows and the re-quantised weights are all read from device memory by every replay (patterned on test_fp8_gpu.py::
    test_graph_replayed_fp8_step_requantises_the_weights_every_step and test_droppath_skip_gpu.py::test_skip_in_the_engine_and_under_graph_replay)"""
    from internvideo_amd.engine import IVTrainEngine
    cfg = O.named_config("tiny88")
    params = O.synthetic_params(cfg, seed=9)
    B = 8
    video, mask, targets = O.synthetic_batch(cfg, B, 6, seed=9)
    vd, tg = video.to(DEV).to(BF16), tuple(t.to(DEV).to(BF16) for t in targets)
    mk = torch.from_numpy(mask).to(DEV).to(torch.uint8)
    Lv = int((~mask[0]).sum())
    g = torch.Generator().manual_seed(77)
    draws = [torch.rand((cfg.depth, 2, B), generator=g) for _ in range(3)]
    draws[1][cfg.depth - 1, 0] = 0.0
    keep = 1.0 - torch.linspace(0, 0.4, cfg.depth).view(-1, 1, 1)
    kept = [int(torch.floor(keep + u).sum()) for u in draws]
    assert len(set(kept)) == 3, kept
    traj = {}
    for tag, graph in (("eager", False), ("graph", True)):
        model = _build(cfg, params, 0.4, True)
        model.residual_dtype = "bf16"
        model.fp8_gemm = True
        U = draws[0].clone().to(DEV)
        model._dp_uniform = U
        eng = IVTrainEngine(model, lr=1e-3, weight_decay=0.05, max_grad_norm=1.0)
        start = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in eng.state_dict().items()}
        losses = []

        def steps():
            if graph:
                eng.capture_step(vd, mk, tg, L=Lv)
                eng.load_state_dict(start)                                   # the warm-up steps of the capture do not count
            for k in range(3):
                U.copy_(draws[k])
                losses.append(float((eng.train_step_graphed() if graph else eng.train_step(vd, mk, tg))[0]))
        _, plans = _count_plans(steps)
        assert plans, "the skipping path did not run"
        traj[tag] = (losses, eng.master.clone())
        eng.close()
        del eng, model
    assert traj["eager"][0] == traj["graph"][0], (traj["eager"][0], traj["graph"][0])
    assert torch.equal(traj["eager"][1], traj["graph"][1])
    assert all(x == x and abs(x) < 1e4 for x in traj["eager"][0]) and len(set(traj["eager"][0])) == 3
