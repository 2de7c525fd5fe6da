"""tanh-GELU with the derivative exchanged (ivh_gemm_desc.act = 4, ops.ACT["gelu_tanh_d"]), host side: the Python names, DropPath skipping
no longer refusing a tanh stack, and the router (ivh_gemm_select / half-width plan / tail-split workspace: host logic, 256 CUs assumed
without a device) answering for act = 4 what it answers for act = 3.  No device."""
import ctypes as C

import torch

from internvideo_amd import functional as Fn
from internvideo_amd import lib, ops


def test_act_names():
    assert ops.ACT["gelu_tanh_d"] == 4
    assert ops.ACT["gelu_tanh"] == 2 and ops.ACT["tanh"] == 2 and ops.ACT["gelu_erf_d"] == 3      # act = 2 keeps its meaning
    assert Fn._act_d("tanh") == "gelu_tanh_d" and Fn._act_d("gelu_tanh") == "gelu_tanh_d"
    for name in ("gelu", "gelu_erf", "erf"):
        assert Fn._act_d(name) == "gelu_erf_d"
    assert Fn._act_d("gelu_erf_d") == "gelu_erf_d" and Fn._act_d("gelu_tanh_d") == "gelu_tanh_d" and Fn._act_d("none") == "none"


def _params_1b():
    """CPU tensors of the 1B block's parameter shapes, in functional.BLOCK_PARAM_NAMES order"""
    D, F = 1408, 6144
    shapes = [(D,), (3 * D, D), (88,), (88,), (D, D), (D,), (D,), (D,), (F, D), (F,), (D, F), (D,), (D,)]
    assert len(shapes) == Fn.NBP
    return [torch.empty(s) for s in shapes]


def test_dp_skip_applies_to_a_tanh_stack():
    D, H, L = 1408, 16, 417
    M = 128 * L
    meta = dict(act="gelu_tanh", H=H, L=L)
    prm = _params_1b()
    assert Fn.dp_skip_applies(meta, M, D, prm) is True                                   # "auto", bf16
    assert Fn.dp_skip_applies(dict(meta, dp_skip=True), M, D, prm) is True
    assert Fn.dp_skip_applies(dict(meta, fp8=True), M, D, prm) is True
    assert Fn.dp_skip_applies(dict(meta, dp_skip=False), M, D, prm) is False
    assert Fn.dp_skip_applies(dict(meta, dp_skip=False, fp8=True), M, D, prm) is False
    assert Fn.dp_skip_applies(dict(meta, act="gelu_erf"), M, D, prm) is True             # the erf stack as before
    assert Fn.dp_skip_applies(dict(meta, act="none"), M, D, prm) is False                # no exchanged flavour: no count-carrying epilogue


def _desc(M, N, K, b_kc=1, **kw):
    d = lib.GemmDesc()
    d.M, d.N, d.K, d.a_kc, d.b_kc, d.batch = M, N, K, 1, b_kc, 1
    d.lda, d.ldb, d.ldc, d.ldp, d.ldd = K, (K if b_kc else N), N, N, N
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_the_router_does_not_depend_on_the_activation():
    """fc1 forward (+ gelu' copy) and fc2 dgrad x dact_in of the 1B block at B = 128 and B = 32, a small shape, a device-side count:
    ivh_gemm_select, the half-width plan and the tail-split workspace are the same for act = 3 and act = 4; act = 2 stays where it was."""
    L = lib.load()
    PTR = 16                                                                 # the queries look at which fields are set, never behind them
    out3, out4 = (C.c_int32 * 4)(), (C.c_int32 * 4)()
    for M in (128 * 417, 32 * 417, 300):
        for kw in (dict(preact=PTR), dict(), dict(m_dev=PTR, preact=PTR)):                                    # fc1 forward: N = 6144, K = 1408
            d3, d4 = _desc(M, 6144, 1408, act=3, **kw), _desc(M, 6144, 1408, act=4, **kw)
            assert L.ivh_gemm256_supported(C.byref(d4)) == 1
            assert L.ivh_gemm_select(C.byref(d3)) == L.ivh_gemm_select(C.byref(d4)), (M, kw)
            assert L.ivh_gemm256_half_plan(C.byref(d3), 0, out3) == L.ivh_gemm256_half_plan(C.byref(d4), 0, out4) and list(out3) == list(out4)
            assert L.ivh_gemm_split_workspace(C.byref(d3)) == L.ivh_gemm_split_workspace(C.byref(d4))
        for kw in (dict(dact_in=PTR), dict(dact_in=PTR, m_dev=PTR)):                                          # fc2 dgrad: N = 6144, K = 1408
            d3, d4 = _desc(M, 6144, 1408, b_kc=0, act=3, **kw), _desc(M, 6144, 1408, b_kc=0, act=4, **kw)
            assert L.ivh_gemm256_supported(C.byref(d4)) == 1
            assert L.ivh_gemm_select(C.byref(d3)) == L.ivh_gemm_select(C.byref(d4)), (M, kw)
            assert L.ivh_gemm256_half_plan(C.byref(d3), 0, out3) == L.ivh_gemm256_half_plan(C.byref(d4), 0, out4) and list(out3) == list(out4)
            assert L.ivh_gemm_split_workspace(C.byref(d3)) == L.ivh_gemm_split_workspace(C.byref(d4))
    assert L.ivh_gemm_select(C.byref(_desc(128 * 417, 6144, 1408, act=4, preact=PTR))) == 2               # the headline step's fc1: the 256^2 kernel
    assert L.ivh_gemm_select(C.byref(_desc(128 * 417, 6144, 1408, b_kc=0, act=4, dact_in=PTR))) == 2
    assert L.ivh_gemm_select(C.byref(_desc(128 * 417, 6144, 1408, act=2, preact=PTR))) == 1               # act = 2: the 128^2 kernel, as before
    assert L.ivh_gemm256_supported(C.byref(_desc(128 * 417, 6144, 1408, act=2))) == 0
    # the long-K tail split serves the flavour (fc1-shaped forward with K = 6144 at B = 32: 62 tail tiles x 4 slices, as for act = 3)
    need = L.ivh_gemm_split_workspace(C.byref(_desc(13344, 1408, 6144, act=4, preact=PTR)))
    assert need == 4096 + 248 * 262144
    assert L.ivh_gemm_fp8_split_workspace(C.byref(_desc(1024, 768, 8192, act=4, preact=PTR))) == 4096 + 48 * 262144
