"""The launch router of the 256x256 GEMM (csrc/gemm256.hip: one table of instantiations, one routing function), seen through
ivh_gemm256_debug_route: the ten template arguments {a_kc, b_kc, epi, grouped, dbg, sched, fp8, split, half, dyn} of the kernel the launchers
would run.  Host logic only, 256 workgroups (what the library assumes without a device, and what an MI355X has).  No device.

The route is held against the queries that existed before it (ivh_gemm256_supported, ivh_gemm_split_workspace, ivh_gemm_fp8_split_workspace,
ivh_gemm256_half_plan) over every combination of layout, activation, epilogue operand, device-side count and output type, on five shapes,
with and without a workspace, with the split / half-width switches on and off.

Where the launcher refuses a descriptor or hands it over there is no route, hence no SPLIT / HALF / DYN bit to compare; which descriptors
those are is asserted separately, from the contract in include/internvideo_hip.h:
  bf16: exactly the descriptors ivh_gemm256_supported rejects, plus the count-carrying ones the header rules out (both counts, m_dev without a
        K-contiguous A, k_dev off the weight-gradient layout or with an epilogue, m_dev with the erf-recomputing dgrad epilogue act = 1);
  e4m3: both operands K-contiguous, bf16 output, no act = 2, x dact_in with act = 3 / 4 and no pre-activation copy, a pre-activation copy with
        act = 3 / 4 only, k_dev with a plain epilogue.  (The e4m3 workspace query looks at layout and size only, so it can be positive for a
        descriptor the launcher hands over; nothing is routed there.)
ivh_gemm256_half_plan describes the bf16 launch; the e4m3 kernels have no half-width flavour and must never route to one."""
import ctypes as C
import itertools

from internvideo_amd import lib

CAP = 256
PTR = 16                                                   # the router looks at which fields are set and at their alignment, never behind them
FIELDS = ("a_kc", "b_kc", "epi", "grouped", "dbg", "sched", "fp8", "split", "half", "dyn")
SHAPES = ((300, 6144, 1408), (13344, 1408, 6144), (13344, 6144, 1408), (53376, 4224, 1408), (1024, 768, 8192))
FLAGS = ("dact_in", "preact", "m_dev", "k_dev", "c_fp32")


def _desc(M, N, K, a_kc=1, b_kc=1, **kw):
    d = lib.GemmDesc()
    d.M, d.N, d.K, d.a_kc, d.b_kc, d.batch, d.alpha = M, N, K, a_kc, b_kc, 1, 1.0
    d.lda, d.ldb, d.ldc, d.ldp, d.ldd = (K if a_kc else M), (K if b_kc else N), N, N, N
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _route(L, d, mode=0, cap=CAP):
    out = (C.c_int32 * 10)(*([-1] * 10))
    rc = L.ivh_gemm256_debug_route(d if isinstance(d, C.Array) else C.byref(d), mode, cap, out)
    assert rc in (0, 1)
    return dict(zip(FIELDS, out)) if rc else None


def _epi(act, dact_in):
    """gemm256.hip g2_epi: x dact_in with the derivative exchanged (act 3 / 4) is EPI 3, with erf recomputed EPI 1; forward tanh EPI 4, GELU EPI 2"""
    if dact_in:
        return 3 if act in (3, 4) else 1
    return 4 if act == 4 else (2 if act else 0)


def _no_route(fp8, a_kc, b_kc, act, f):
    """the descriptors of the grid without a 256x256 launch, from the header's contract (see the module docstring); `f`: the set flags"""
    dyn = f["m_dev"] or f["k_dev"]
    if not fp8:
        if f["m_dev"] and f["k_dev"]:
            return True
        if f["m_dev"] and (not a_kc or _epi(act, f["dact_in"]) == 1):
            return True
        if f["k_dev"] and (a_kc or b_kc or _epi(act, f["dact_in"]) != 0):
            return True
        return False                                       # ... or ivh_gemm256_supported says no: asked of the library
    if not (a_kc and b_kc) or f["c_fp32"] or act == 2 or (f["m_dev"] and f["k_dev"]):
        return True
    if f["dact_in"] and (act not in (3, 4) or f["preact"]):
        return True
    if not f["dact_in"] and f["preact"] and act not in (3, 4):
        return True
    return bool(dyn and f["k_dev"] and (f["dact_in"] or act or f["preact"]))


def _walk(L, split_on=True, half_on=True):
    """grids (a) x (b): every assertion of the module docstring; returns how many routes were seen with each launch mode"""
    seen = dict(split=0, half=0, dyn=0, dyn_split=0, plain=0, none=0)
    out4 = (C.c_int32 * 4)()
    for (M, N, K), fp8, act, bits in itertools.product(SHAPES, (0, 1), range(5), itertools.product((0, 1), repeat=len(FLAGS))):
        f = dict(zip(FLAGS, bits))
        total = -(-M // 256) * -(-N // 256)
        for with_ws in (0, 1):
            keys = {}
            for a_kc, b_kc in itertools.product((0, 1), repeat=2):
                kw = {k: PTR for k in FLAGS[:4] if f[k]}
                d = _desc(M, N, K, a_kc, b_kc, act=act, c_fp32=f["c_fp32"], **kw)
                query = (L.ivh_gemm_fp8_split_workspace if fp8 else L.ivh_gemm_split_workspace)(C.byref(d))
                if with_ws:
                    d.split_ws, d.split_ws_bytes = PTR, query                      # exactly what the query asks for (nothing when it says 0)
                supported = L.ivh_gemm256_supported(C.byref(d))
                r = _route(L, d, fp8)
                what = (M, N, K, fp8, act, a_kc, b_kc, f, with_ws)
                refused = _no_route(fp8, a_kc, b_kc, act, f) or (not fp8 and not supported)
                assert (r is None) == refused, what
                if not fp8 and not (f["m_dev"] or f["k_dev"]):
                    assert (r is None) == (supported == 0), what               # count-free bf16: ivh_gemm256_supported alone decides
                if r is None:
                    seen["none"] += 1
                    continue
                keys[(a_kc, b_kc)] = (r, supported)
                # key fields: layout and epilogue as the descriptor says, no measurement variant, no grouped kernel
                assert (r["a_kc"], r["b_kc"], r["epi"], r["fp8"]) == (a_kc, b_kc, _epi(act, f["dact_in"]), fp8), what
                assert (r["grouped"], r["dbg"], r["sched"]) == (0, 0, 0), what
                assert r["dyn"] == int(f["m_dev"] or f["k_dev"]), what
                want_split = query > 0 and with_ws and (not f["m_dev"] or total >= CAP)
                assert r["split"] == int(want_split), (what, query)
                half = L.ivh_gemm256_half_plan(C.byref(d), CAP, out4)
                assert r["half"] == int(not fp8 and half == 1 and not r["split"]), (what, half)
                if not split_on:
                    assert query == 0 and not r["split"], what
                if not half_on:
                    assert half == 0 and not r["half"], what
                mode = "dyn_split" if r["dyn"] and r["split"] else "dyn" if r["dyn"] else "split" if r["split"] else "half" if r["half"] else "plain"
                seen[mode] += 1
            # layout invariance: with both layouts of B supported and routed, the keys differ in the b_kc field only
            for a_kc in (0, 1):
                if (a_kc, 0) in keys and (a_kc, 1) in keys and keys[(a_kc, 0)][1] and keys[(a_kc, 1)][1]:
                    r0, r1 = dict(keys[(a_kc, 0)][0]), dict(keys[(a_kc, 1)][0])
                    assert (r0.pop("b_kc"), r1.pop("b_kc")) == (0, 1) and r0 == r1, (M, N, K, fp8, act, a_kc, f, with_ws, r0, r1)
    return seen


def test_route_agrees_with_the_capability_queries():
    seen = _walk(lib.load())
    assert all(seen[m] > 0 for m in seen), seen               # the grid reaches every launch mode, and descriptors without a route


def test_route_follows_the_split_and_half_switches():
    L = lib.load()
    try:
        L.ivh_gemm256_debug_split(0)
        seen = _walk(L, split_on=False)
        assert seen["split"] == 0 and seen["dyn_split"] == 0 and seen["half"] > 0, seen
    finally:
        L.ivh_gemm256_debug_split(1)
    try:
        L.ivh_gemm256_debug_half(0)
        seen = _walk(L, half_on=False)
        assert seen["half"] == 0 and seen["split"] > 0, seen
    finally:
        L.ivh_gemm256_debug_half(1)


def test_pinned_rows_of_the_headline_step():
    L = lib.load()
    row = lambda *v: dict(zip(FIELDS, v))
    # fc1 forward at B = 128 under DropPath skipping (m_dev), GELU with the derivative copy: the DYN GELU kernels, tanh (act 4) and erf (act 3)
    for act, epi in ((4, 4), (3, 2)):
        d = _desc(128 * 417, 6144, 1408, act=act, preact=PTR, m_dev=PTR)
        assert _route(L, d) == row(1, 1, epi, 0, 0, 0, 0, 0, 0, 1)
        assert _route(L, d, 1) == row(1, 1, epi, 0, 0, 0, 1, 0, 0, 1)
    # fc2-shaped forward at B = 32, K = 6144: 318 tiles = one round + 62 tail tiles x 4 K slices; SPLIT with the workspace, otherwise not
    d = _desc(32 * 417, 1408, 6144)
    need = L.ivh_gemm_split_workspace(C.byref(d))
    assert need == 4096 + 248 * 262144
    assert _route(L, d)["split"] == 0
    d.split_ws, d.split_ws_bytes = PTR, need
    assert _route(L, d) == row(1, 1, 0, 0, 0, 0, 0, 1, 0, 0)
    d.split_ws_bytes = need - 1
    assert _route(L, d)["split"] == 0
    d.split_ws, d.split_ws_bytes = PTR + 8, need                                   # not 16-byte aligned
    assert _route(L, d)["split"] == 0
    # two weight gradients of a block in one launch, the token count on the device: the grouped DYN kernel; without counts and with one K the
    # grouped kernel; with different K (the decoders' gradients with and without the cls row) the DYN one again
    def pair(k_dev, K2):
        g = (lib.GemmDesc * 2)()
        for q, (M, N, K) in zip(g, ((6144, 1408, 128 * 417), (1408, 6144, K2))):
            q.M, q.N, q.K, q.a_kc, q.b_kc, q.batch, q.alpha = M, N, K, 0, 0, 1, 1.0
            q.lda, q.ldb, q.ldc = M, N, N
            q.k_dev = k_dev
        return g
    assert _route(L, pair(PTR, 128 * 417), 2) == row(0, 0, 0, 1, 0, 0, 0, 0, 0, 1)
    assert _route(L, pair(None, 128 * 417), 2) == row(0, 0, 0, 1, 0, 0, 0, 0, 0, 0)
    assert _route(L, pair(None, 128 * 416), 2) == row(0, 0, 0, 1, 0, 0, 0, 0, 0, 1)
    g = pair(PTR, 128 * 417)
    g[1].act = 1                                                                   # an epilogue: not groupable, launched one by one
    assert _route(L, g, 2) is None
    # a single weight gradient with k_dev: the DYN kernel of the wgrad layout
    assert _route(L, _desc(6144, 1408, 128 * 417, 0, 0, k_dev=PTR)) == row(0, 0, 0, 0, 0, 0, 0, 0, 0, 1)


def test_measurement_variants_route_to_their_own_rows_and_only_for_the_plain_nt_kernel():
    L = lib.load()
    nt, nn = _desc(4096, 4096, 1024), _desc(4096, 4096, 1024, 1, 0)
    try:
        for mode in range(1, 7):
            L.ivh_gemm256_debug_ablate(mode)
            assert (_route(L, nt)["dbg"], _route(L, nt)["sched"]) == (mode, 0)
            assert _route(L, nn)["dbg"] == 0 and _route(L, _desc(4096, 4096, 1024, act=1))["dbg"] == 0
            assert _route(L, _desc(4096, 4096, 1024, m_dev=PTR)) is None               # a count under an ablation: refused
        L.ivh_gemm256_debug_ablate(0)
        L.ivh_gemm256_debug_sched(1)
        assert (_route(L, nt)["dbg"], _route(L, nt)["sched"]) == (0, 1) and _route(L, nn)["sched"] == 0
        assert _route(L, nt, 1)["sched"] == 0                                          # the e4m3 kernels have no variants
    finally:
        L.ivh_gemm256_debug_ablate(0)
        L.ivh_gemm256_debug_sched(0)
    assert (_route(L, nt)["dbg"], _route(L, nt)["sched"]) == (0, 0)
