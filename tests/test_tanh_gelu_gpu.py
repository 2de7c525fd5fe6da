"""tanh-GELU with the derivative exchanged (ivh_gemm_desc.act = 4, ops.ACT["gelu_tanh_d"]): the activation of the released InternVideo2
checkpoints (flash_attn FusedMLP heuristic 1) on the kernels the erf flavour runs on -- the 256^2 GEMM epilogues in every launch mode
(plain, half-width tiles, tail split, device-side row counts; bf16 and e4m3), the 128^2 kernels, DropPath sample skipping in the block
stack and in the captured training step.  One device function (csrc/common.h gelu_tanh_pair) serves all four GEMM kernels.
Runs only on a real MI355X (`-m gpu`)."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from internvideo_amd import functional as Fn  # noqa: E402
from internvideo_amd import lib as L_  # noqa: E402
from internvideo_amd import ops  # noqa: E402
from oracle import internvideo2_oracle as O  # noqa: E402
# the model builder, the step runner and the small tensor helpers are those of the erf tests of the same feature: the two files build the
# same stacks on the same draws, and a change there is meant to reach the tanh twins
from tests.test_droppath_skip_gpu import _build, _run, cnt, randn, rel  # noqa: E402

DEV = "cuda"
BF16, F32, FP8, U8 = torch.bfloat16, torch.float32, torch.float8_e4m3fn, torch.uint8
ACT = "gelu_tanh_d"
C0, A0 = math.sqrt(2.0 / math.pi), 0.044715


@pytest.fixture
def plain_tiles():
    """whole 256 x 256 tiles on both GEMM families (no K split of the tail round, no half-width tiles), the 256^2 kernels at every size: a
    full-size launch then sums in the order of the launch that carries a device-side count, and the two can be compared BITWISE"""
    lib = L_.load()
    lib.ivh_gemm256_debug_split(0); lib.ivh_gemm256_debug_half(0)
    ops.set_gemm_kernel(2); ops.set_gemm_fp8_kernel(2)
    yield
    ops.set_gemm_kernel(0); ops.set_gemm_fp8_kernel(0)
    lib.ivh_gemm256_debug_split(1); lib.ivh_gemm256_debug_half(1)


def _desc(M, N, K, b_kc=True, act=ACT, **kw):
    d = L_.GemmDesc()
    d.M, d.N, d.K, d.a_kc, d.b_kc, d.batch, d.alpha = M, N, K, 1, int(b_kc), 1, 1.0
    d.lda, d.ldb, d.ldc, d.ldp, d.ldd = K, (K if b_kc else N), N, N, N
    d.act = ops.ACT[act]
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def gelu_tanh_ref64(x):
    """value and derivative of x (1 + tanh u) / 2, u = c (x + a x^3), in fp64"""
    x = x.double()
    u = C0 * (x + A0 * x ** 3)
    t = torch.tanh(u)
    g = 0.5 * x * (1.0 + t)
    d = 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * C0 * (1.0 + 3.0 * A0 * x * x)
    return g, d


# ---- 1. every bf16 input, exact pre-activations -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def every_bf16():
    """W [544][64]: all 33 762 finite bf16 values in [-30, 30], zero-padded; A [300][64] one-hot per row, so that pre[m, n] = W[n, m % 64]
    exactly (one product with 1.0, sixty-three with 0.0); the fp64 value / derivative of every pre-activation, computed once"""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16).view(BF16)
    vals = bits[torch.isfinite(bits.float()) & (bits.float().abs() <= 30.0)]
    assert vals.numel() == 33762
    N, K, M = 544, 64, 300
    W = torch.zeros(N * K, dtype=BF16)
    W[:vals.numel()] = vals
    W = W.view(N, K)
    A = torch.zeros((M, K), dtype=BF16)
    A[torch.arange(M), torch.arange(M) % K] = 1.0
    pre = W.float().t()[torch.arange(M) % K]                                # [M, N]
    g64, d64 = gelu_tanh_ref64(pre)
    return A.to(DEV), W.to(DEV), g64, d64


def _check_every(got, ref, what):
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), what
    err = (got - ref).abs()
    # 2^-8 |ref|: half a bf16 ulp of the stored result.  1e-4 max(|ref|, 1): more than 10x the fp32 evaluation's own error -- __expf's argument
    # error |2u| 2^-23 where the sigmoid is not saturated, plus one ulp of the reciprocal (the fp32 formula on the CPU stays below 2e-6)
    tol = 2.0 ** -8 * ref.abs() + 1e-4 * ref.abs().clamp_min(1.0)
    worst = float((err - tol).max())
    print(f"{what}: max |err| {float(err.max()):.3e}, max (err - tol) {worst:.3e}")
    assert worst <= 0.0, (what, worst)


@pytest.mark.parametrize("kernel", [1, 2])
def test_every_bf16_input(every_bf16, kernel):
    A, W, g64, d64 = every_bf16
    M, N, K = A.shape[0], W.shape[0], A.shape[1]
    ops.set_gemm_kernel(kernel)
    try:
        d = _desc(M, N, K, preact=16)
        sel = L_.load().ivh_gemm_select(C.byref(d))
        assert sel == kernel, sel                                           # kernel 2: the 256^2 kernel really carries the flavour
        g, dv = ops.gemm(A, W, act=ACT, want_preact=True)
        _check_every(g, g64, f"kernel {kernel} g")
        _check_every(dv, d64, f"kernel {kernel} d")
        if kernel == 2:                                                     # forward-only launch: the value alone
            assert L_.load().ivh_gemm_select(C.byref(_desc(M, N, K))) == 2
            g1 = ops.gemm(A, W, act=ACT)
            _check_every(g1, g64, "kernel 2 g (forward only)")
    finally:
        ops.set_gemm_kernel(0)


# ---- 2. random GEMM, both kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [1, 2])
def test_random_gemm_epilogues(kernel):
    """the data recipe and the bars of test_kernels_gpu.py::test_gemm_epilogues for act = 3, with the tanh flavour"""
    M, N, K = 300, 264, 136
    A = randn(M, K, seed=5); W = randn(N, K, seed=6, scale=0.1); bias = randn(N, seed=7, dtype=F32)
    dY = randn(M, 72, seed=9); W2 = randn(72, N, seed=10, scale=0.1)
    pre = (A.float() @ W.float().t() + bias).requires_grad_(True)
    O.gelu(pre, "tanh").sum().backward()
    ops.set_gemm_kernel(kernel)
    try:
        assert L_.load().ivh_gemm_select(C.byref(_desc(M, N, K, preact=16))) == kernel
        g, dv = ops.gemm(A, W, bias=bias, act=ACT, want_preact=True)
        eg, ed = rel(g.float(), O.gelu(pre.detach(), "tanh")), rel(dv.float(), pre.grad)
        print(f"kernel {kernel}: g {eg:.3e} d {ed:.3e}")
        assert eg < 4e-3 and ed < 4e-3, (eg, ed)
        g1 = ops.gemm(A, W, bias=bias, act=ACT)                             # forward only: the same values
        assert torch.equal(g1, g)
        dact = pre.grad.to(BF16)
        want = (dY.float() @ W2.float()) * dact.float()
        got = ops.gemm(dY, W2, a_kc=True, b_kc=False, dact_in=dact, act=ACT)
        e3 = rel(got.float(), want)
        print(f"kernel {kernel}: dgrad x dact_in {e3:.3e}")
        assert e3 < 5e-3, e3
        got2, part = ops.gemm(dY, W2, a_kc=True, b_kc=False, dact_in=dact, act=ACT, want_colsum=True)
        assert torch.equal(got2, got)
        if kernel == 2:
            assert part is not None and rel(part.sum(0), want.sum(0)) < 2e-3
        else:
            assert part is None
    finally:
        ops.set_gemm_kernel(0)


# ---- 3. device-side counts, bf16 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mk", [0, 5, 260, 834])      # no row; a few rows of the first row tile; ragged, past the first row tile; every row
def test_device_side_counts_bf16(Mk, plain_tiles):
    M, N, K = 834, 520, 192
    md = cnt(Mk)
    a = randn(M, K, seed=1)
    a[Mk:] = float("nan")
    w = randn(N, K, seed=2, scale=K ** -0.5)
    bias = randn(N, seed=3, dtype=F32)
    SENT = 7.0
    out = torch.full((M, N), SENT, dtype=BF16, device=DEV)
    assert L_.load().ivh_gemm_select(C.byref(_desc(M, N, K, preact=16, m_dev=16))) == 2
    g, u = ops.gemm(a, w, bias=bias, act=ACT, want_preact=True, out=out, m_dev=md)
    if Mk:
        gr, ur = ops.gemm(a[:Mk].contiguous(), w, bias=bias, act=ACT, want_preact=True)
        assert torch.equal(g[:Mk], gr) and torch.equal(u[:Mk], ur)
        g64, d64 = gelu_tanh_ref64(a[:Mk].float() @ w.float().t() + bias)
        assert rel(gr.float(), g64) < 4e-3 and rel(ur.float(), d64) < 4e-3
    assert bool((out[Mk:] == SENT).all())
    # dgrad x dact_in with the column sums: dy [M, N] x W [N, K] (rows-contiguous B)
    dy = randn(M, N, seed=4)
    dy[Mk:] = float("nan")
    du_in = randn(M, K, seed=5)
    du_in[Mk:] = float("nan")
    out = torch.full((M, K), SENT, dtype=BF16, device=DEV)
    dx, part = ops.gemm(dy, w, a_kc=True, b_kc=False, dact_in=du_in, act=ACT, want_colsum=True, out=out, m_dev=md)
    assert part is not None
    cs = ops.colsum_finish(part, m_dev=md)
    assert bool(torch.isfinite(cs).all())
    if Mk:
        dxr, partr = ops.gemm(dy[:Mk].contiguous(), w, a_kc=True, b_kc=False, dact_in=du_in[:Mk].contiguous(), act=ACT, want_colsum=True)
        assert torch.equal(dx[:Mk], dxr)
        assert torch.equal(cs, ops.colsum_finish(partr))
        # the exchanged flavours share this epilogue: act = 3 gives the same bits
        assert torch.equal(dxr, ops.gemm(dy[:Mk].contiguous(), w, a_kc=True, b_kc=False, dact_in=du_in[:Mk].contiguous(), act="gelu_erf_d"))
    else:
        assert bool((cs == 0).all())
    assert bool((out[Mk:] == SENT).all())


# ---- 4. half-width tiles and the tail split serve the flavour ------------------------------------------------------------------------------
def _half_plan(d, cap):
    out = (C.c_int32 * 4)()
    return L_.load().ivh_gemm256_half_plan(C.byref(d), int(cap), out), list(out)


def test_half_width_tiles_serve_the_flavour():
    M, N, K, cap = 700, 640, 8, 4                                           # the smallest of test_kernels_gpu.py's HALF_CASES
    lib = L_.load()
    lib.ivh_gemm256_debug_max_wg(cap)
    lib.ivh_gemm256_debug_half(1)
    ops.set_gemm_kernel(2)
    try:
        A = randn(M, K, seed=3); W = randn(N, K, seed=4, scale=0.1); bias = randn(N, seed=5, dtype=F32)
        dY = randn(M, K, seed=9); W2 = randn(K, N, seed=10, scale=0.1)
        pre = A.float() @ W.float().t() + bias
        g64, d64 = gelu_tanh_ref64(pre)
        dact = d64.to(BF16)
        assert _half_plan(_desc(M, N, K, preact=16), cap)[0] == 1
        assert _half_plan(_desc(M, N, K), cap)[0] == 1
        assert _half_plan(_desc(M, N, K, b_kc=False, dact_in=dact.data_ptr()), cap)[0] == 1

        def run():
            g, dv = ops.gemm(A, W, bias=bias, act=ACT, want_preact=True)
            g1 = ops.gemm(A, W, bias=bias, act=ACT)
            dd, part = ops.gemm(dY, W2, a_kc=True, b_kc=False, dact_in=dact, act=ACT, want_colsum=True)
            return g, dv, g1, dd, part
        got = run()
        lib.ivh_gemm256_debug_half(0)
        plain = run()
        for x, y in zip(got, plain):
            assert x is not None and torch.equal(x, y)
        assert rel(got[0].float(), g64) < 4e-3 and rel(got[1].float(), d64) < 4e-3
        want = (dY.float() @ W2.float()) * dact.float()
        assert rel(got[3].float(), want) < 5e-3 and rel(got[4].sum(0), want.sum(0)) < 2e-3
    finally:
        ops.set_gemm_kernel(0)
        lib.ivh_gemm256_debug_max_wg(0)
        lib.ivh_gemm256_debug_half(1)
        lib.ivh_gemm256_debug_split(1)


def test_tail_split_serves_the_flavour():
    """five tiles on four workgroups: one whole round and a tail tile cut into four K slices (55 K steps: the shortest K that pays for the
    exchange by the plan's rule, with a K tail; ragged M and N).  Split == unsplit to one bf16 ulp (the bound of
    test_kernels_gpu.py::test_gemm256_tail_split_matches_unsplit), bitwise run to run."""
    M, N, K, cap = 1100, 248, 3464, 4
    lib = L_.load()
    lib.ivh_gemm256_debug_max_wg(cap)
    lib.ivh_gemm256_debug_split(1)
    ops.set_gemm_kernel(2)
    try:
        A = randn(M, K, seed=31); W = randn(N, K, seed=32, scale=0.05); bias = randn(N, seed=33, dtype=F32)
        Wk = W.t().contiguous()
        dact = randn(M, N, seed=36)
        assert lib.ivh_gemm_split_workspace(C.byref(_desc(M, N, K, preact=16))) > 0
        assert lib.ivh_gemm_split_workspace(C.byref(_desc(M, N, K))) > 0
        assert lib.ivh_gemm_split_workspace(C.byref(_desc(M, N, K, b_kc=False, dact_in=dact.data_ptr()))) > 0

        def run():
            g, dv = ops.gemm(A, W, bias=bias, act=ACT, want_preact=True)
            g1 = ops.gemm(A, W, bias=bias, act=ACT)
            dd, part = ops.gemm(A, Wk, a_kc=True, b_kc=False, dact_in=dact, act=ACT, want_colsum=True)
            return g, dv, g1, dd, ops.colsum_finish(part)
        got = run()
        again = run()
        lib.ivh_gemm256_debug_split(0)
        ref = run()
    finally:
        ops.set_gemm_kernel(0)
        lib.ivh_gemm256_debug_max_wg(0)
        lib.ivh_gemm256_debug_split(1)
    for x, y in zip(got, again):
        assert torch.equal(x, y)
    for x, y in zip(got[:4], ref[:4]):
        assert ((x.float() - y.float()).abs() <= 8e-3 * y.float().abs() + 1e-3).all()
    assert rel(got[4], ref[4]) < 1e-4
    g64, d64 = gelu_tanh_ref64(A.float() @ W.float().t() + bias)
    assert rel(got[0].float(), g64) < 4e-3 and rel(got[1].float(), d64) < 4e-3
    assert rel(got[3].float(), (A.float() @ W.float().t()) * dact.float()) < 5e-3

# ---- 5. e4m3 --------------------------------------------------------------------------------------------------------------------------------
def nan8(*shape):
    return torch.full(shape, 0x7f, dtype=U8, device=DEV).view(FP8)


@pytest.mark.parametrize("Mk", [None, 260])                                   # without a count; a ragged count past the first row tile
def test_e4m3(Mk, plain_tiles):
    """forward with the derivative copy and dgrad x dact_in (+ column sums under a count) on the 256^2 e4m3 kernel and on the 128^2 one,
    against the fp64 product of the DEQUANTISED operands (what is left is the fp32 accumulation and the bf16 rounding of the outputs: the
    bf16 bars of test 2).  Under a count: the kept rows equal the launch on them alone bitwise, rows behind keep their sentinel, operand rows
    behind the count are NaN (bytes 0x7f / bf16 NaN) -- the pattern of tests/test_fp8_droppath_skip_gpu.py."""
    M, N, K = 834, 512, 512
    rows = M if Mk is None else Mk
    md = None if Mk is None else cnt(Mk)
    a = randn(M, K, seed=1)
    dy = randn(M, N, seed=4)
    du_in = randn(M, K, seed=5)
    if Mk is not None:
        a[Mk:] = float("nan"); dy[Mk:] = float("nan"); du_in[Mk:] = float("nan")
    w = randn(N, K, seed=2, scale=K ** -0.5)
    bias = randn(N, seed=3, dtype=F32)
    aq, _, sa = ops.fp8_quantize(a, m_dev=md, out=(nan8(M, K), None))
    dyq, _, sd = ops.fp8_quantize(dy, m_dev=md, out=(nan8(M, N), None))
    wq, wqt, sw = ops.fp8_quantize(w, want_transposed=True)
    aqr, _, sar = ops.fp8_quantize(a[:rows].contiguous())
    dyqr, _, sdr = ops.fp8_quantize(dy[:rows].contiguous())
    assert torch.equal(sa, sar) and torch.equal(sd, sdr)
    wd = wq.float().double() * sw.double()
    g64, d64 = gelu_tanh_ref64((aqr.float().double() * sar.double()) @ wd.t() + bias.double())
    want_dx = ((dyqr.float().double() * sdr.double()) @ wd) * du_in[:rows].double()
    SENT = 7.0
    # the 256^2 e4m3 kernel (the fixture forces it at this size)
    out = torch.full((M, N), SENT, dtype=BF16, device=DEV)
    g, u = ops.gemm_fp8(aq, wq, sa, sw, bias=bias, act=ACT, want_preact=True, out=out, m_dev=md)
    gr, ur = ops.gemm_fp8(aqr, wq, sar, sw, bias=bias, act=ACT, want_preact=True)
    assert torch.equal(g[:rows], gr) and torch.equal(u[:rows], ur)
    assert bool((out[rows:] == SENT).all())
    eg, ed = rel(gr.double(), g64), rel(ur.double(), d64)
    print(f"e4m3 256^2: g {eg:.3e} d {ed:.3e}")
    assert eg < 4e-3 and ed < 4e-3, (eg, ed)
    out = torch.full((M, K), SENT, dtype=BF16, device=DEV)
    dxr = ops.gemm_fp8(dyqr, wqt, sdr, sw, k=N, dact_in=du_in[:rows].contiguous(), act=ACT)
    if Mk is None:
        dx = ops.gemm_fp8(dyq, wqt, sd, sw, k=N, dact_in=du_in, act=ACT, out=out)
    else:
        dx, part = ops.gemm_fp8(dyq, wqt, sd, sw, k=N, dact_in=du_in, act=ACT, out=out, m_dev=md, want_colsum=True)
        cs = ops.colsum_finish(part, m_dev=md)
        assert bool(torch.isfinite(cs).all())
        e = rel(cs, dx[:rows].float().sum(0))
        assert e < 4e-3, e
    assert torch.equal(dx[:rows], dxr)
    assert bool((out[rows:] == SENT).all())
    e3 = rel(dxr.double(), want_dx)
    print(f"e4m3 256^2: dgrad x dact_in {e3:.3e}")
    assert e3 < 5e-3, e3
    # the 128^2 e4m3 kernel (it takes no count: the kept rows alone)
    ops.set_gemm_fp8_kernel(1)
    g1, u1 = ops.gemm_fp8(aqr, wq, sar, sw, bias=bias, act=ACT, want_preact=True)
    dx1 = ops.gemm_fp8(dyqr, wqt, sdr, sw, k=N, dact_in=du_in[:rows].contiguous(), act=ACT)
    e1 = (rel(g1.double(), g64), rel(u1.double(), d64), rel(dx1.double(), want_dx))
    print(f"e4m3 128^2: g {e1[0]:.3e} d {e1[1]:.3e} dgrad x dact_in {e1[2]:.3e}")
    assert e1[0] < 4e-3 and e1[1] < 4e-3 and e1[2] < 5e-3, e1

# ---- 6. the block stack ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual,n_cp", [("fp32", 0), ("bf16", 0), ("fp32", 2), ("bf16", 2)])
def test_tanh_block_stack_skip_equals_multiply_by_zero(residual, n_cp, plain_tiles):
    """tests/test_droppath_skip_gpu.py::test_block_stack_skip_equals_multiply_by_zero with fused_mlp_act="tanh": the skipping path really
    runs (ops.droppath_plan is called), loss and outputs are bitwise the multiply-by-zero stack's, gradients as there.  The oracle has no
    DropPath, so the comparison with it (cfg.gelu = "tanh", the bars of tests/test_model_gpu.py) runs the same skipping stack with every
    keep probability set to 1: the plan is made, every kernel carries its device-side count, and every sample is kept at scale 1."""
    cfg = O.named_config("tiny88")
    params = O.synthetic_params(cfg, seed=5)
    B = 6
    video, mask, targets = O.synthetic_batch(cfg, B, 6, seed=5)
    g = torch.Generator().manual_seed(3)
    U = torch.rand((cfg.depth, 2, B), generator=g)
    U[1, 0] = 0.0                                                            # block 1, attention branch: every sample dropped (keep < 1)
    U[1, 1] = 0.999                                                          # block 1, MLP branch: none dropped
    kw = dict(use_checkpoint=True, checkpoint_num=n_cp) if n_cp else {}
    res = {}
    calls = []
    orig = ops.droppath_plan
    for skip in (False, True):
        model = _build(cfg, params, 0.5, skip, fused_mlp_act="tanh", **kw)
        model.residual_dtype = residual
        ops.droppath_plan = lambda *a, **k: (calls.append(skip), orig(*a, **k))[1]
        try:
            res[skip] = _run(model, video, mask, targets, U)
        finally:
            ops.droppath_plan = orig
        del model
    assert calls and all(calls), "the skipping path did not run for the tanh stack"
    keep = 1.0 - torch.linspace(0, 0.5, cfg.depth).view(-1, 1, 1)
    assert int((torch.floor(keep + U) == 0).sum()) >= B + 3
    (l0, o0, g0), (l1, o1, g1) = res[False], res[True]
    assert torch.equal(l0, l1), (l0.item(), l1.item())
    for a, b in zip(o0, o1):
        assert torch.equal(a, b)
    assert g0.keys() == g1.keys()
    worst = {k: rel(g1[k], g0[k]) for k in g0 if float(g0[k].abs().max()) > 0}
    bad = {k: v for k, v in worst.items() if v > 4e-3}
    assert not bad, bad
    exact = [k for k in g0 if k.endswith(("ls1.gamma", "ls2.gamma", "proj.bias", "fc2.bias", "norm1.weight", "norm2.weight")) and k.startswith("blocks.")]
    assert exact
    for k in exact:                                                          # row-kernel column sums: the same rows in the same order
        assert torch.equal(g0[k], g1[k]), k
    # against the oracle's tanh flavour
    cfg_t = O.named_config("tiny88"); cfg_t.gelu = "tanh"
    enc = O.encoder_forward(params, video, mask, cfg_t)
    mae = O.student_forward(params, video, mask, cfg_t)[2]
    model = _build(cfg, params, 0.5, True, fused_mlp_act="tanh", **kw)
    model.residual_dtype = residual
    model._dp_keep = torch.ones((cfg.depth, 1, 1), dtype=F32, device=DEV)    # keep probability 1 everywhere: floor(1 + U) / 1 = 1
    model._dp_uniform = U
    calls.clear()
    ops.droppath_plan = lambda *a, **k: (calls.append(True), orig(*a, **k))[1]
    try:
        out = model(video.to(DEV), torch.from_numpy(mask))
    finally:
        ops.droppath_plan = orig
    assert calls
    e = [rel(out[0].float(), enc["x_clip_align"]), rel(out[1].float(), enc["x_align"]), rel(out[2].float(), mae)]
    print(f"tanh stack vs oracle ({residual}, n_cp {n_cp}): {e}")
    assert max(e) < (2e-2 if residual == "bf16" else 1e-2), e


# ---- 7. the engine under graph replay ----------------------------------------------------------------------------------------------------
def test_tanh_skip_in_the_engine_and_under_graph_replay():
    """the tanh twin of tests/test_droppath_skip_gpu.py::test_skip_in_the_engine_and_under_graph_replay: eager skipping steps == replays of one
    captured HIP graph, bitwise, over three draws with three different kept counts; skipping follows multiply-by-zero"""
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
    draws[1][cfg.depth - 1, 0] = 0.0                                         # second step: a branch with every sample dropped
    keep = 1.0 - torch.linspace(0, 0.4, cfg.depth).view(-1, 1, 1)
    kept = [int(torch.floor(keep + u).sum()) for u in draws]
    assert len(set(kept)) == 3, kept
    traj = {}
    planned = []
    orig = ops.droppath_plan
    ops.droppath_plan = lambda *a, **k: (planned.append(1), orig(*a, **k))[1]
    try:
        for tag, skip, graph in (("zero", False, False), ("skip", True, False), ("skip_graph", True, True)):
            model = _build(cfg, params, 0.4, skip, fused_mlp_act="tanh")
            assert Fn._act_d(model.fused_mlp_act) == ACT
            model.residual_dtype = "bf16"
            U = draws[0].clone().to(DEV)
            model._dp_uniform = U
            eng = IVTrainEngine(model, lr=1e-3, weight_decay=0.05, max_grad_norm=1.0)
            start = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in eng.state_dict().items()}
            losses = []
            if graph:
                eng.capture_step(vd, mk, tg, L=Lv)
                eng.load_state_dict(start)                                   # the warm-up steps of the capture do not count
            n0 = len(planned)
            for k in range(3):
                U.copy_(draws[k])
                if graph:
                    losses.append(float(eng.train_step_graphed()[0]))
                else:
                    losses.append(float(eng.train_step(vd, mk, tg)[0]))
            if tag == "skip":
                assert len(planned) - n0 == 3, "the skipping path did not run for the tanh stack"
            traj[tag] = (losses, eng.master.clone())
            eng.close()
            del eng, model
    finally:
        ops.droppath_plan = orig
    assert traj["skip"][0] == traj["skip_graph"][0], (traj["skip"][0], traj["skip_graph"][0])
    assert torch.equal(traj["skip"][1], traj["skip_graph"][1])
    for a, b in zip(traj["zero"][0], traj["skip"][0]):
        assert abs(a - b) < 2e-3 * abs(a), (traj["zero"][0], traj["skip"][0])
    assert len(set(traj["skip"][0])) == 3
