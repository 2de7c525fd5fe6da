"""DropPath sample skipping on the fp8 (e4m3) GEMM path, host side: functional.dp_skip_applies no longer refuses `fp8` stacks and applies the
conditions the count-carrying e4m3 kernels really have (widths that are multiples of 16; "auto" also asks for D >= 512).  No device."""
import torch

from internvideo_amd import functional as Fn


def _params(D, hidden):
    p = [None] * Fn.NBP
    p[8] = torch.empty((hidden, D), device="meta")                          # mlp.fc1.weight: its row count is the MLP width
    return p


def test_dp_skip_applies_to_fp8_stacks_at_6B_widths():
    M, D, H = 16 * 1025, 3200, 25                                           # 6B encoder at 16 x 224^2: 16 clips of 1025 tokens, head dim 128
    meta = dict(dp_skip=True, fp8=True, act="gelu", H=H, L=1025)
    assert Fn.dp_skip_applies(meta, M, D, _params(D, 12800)) is True
    assert Fn.dp_skip_applies(dict(meta, dp_skip="auto"), M, D, _params(D, 12800)) is True
    assert Fn.dp_skip_applies(dict(meta, dp_skip=False), M, D, _params(D, 12800)) is False


def test_dp_skip_refuses_fp8_widths_that_are_not_multiples_of_16():
    meta = dict(dp_skip=True, fp8=True, act="gelu", H=5, L=64)                       # head dim 104
    assert Fn.dp_skip_applies(meta, 4096, 520, _params(520, 2080)) is False          # D = 520 = 8 * 65: fine for bf16, not for e4m3 rows
    assert Fn.dp_skip_applies(dict(meta, fp8=False), 4096, 520, _params(520, 2080)) is True
    assert Fn.dp_skip_applies(dict(meta, H=4), 4096, 512, _params(512, 2056)) is False  # MLP width 2056 = 8 * 257
    assert Fn.dp_skip_applies(dict(meta, H=4), 4096, 512, _params(512, 2048)) is True


def test_dp_skip_auto_keeps_narrow_fp8_stacks_on_their_kernel_choice():
    """ "auto" must not move a GEMM from the 128^2 to the 256^2 e4m3 kernel that the fp8 launch's own size heuristic (M * N >= 512^2 and
    K >= 512) would have kept on the 128^2 one: M * D >= 512^2 does not give K >= 512 when D < 512"""
    meta = dict(dp_skip="auto", fp8=True, act="gelu", H=2, L=64)
    assert Fn.dp_skip_applies(meta, 4096, 256, _params(256, 1024)) is False
    assert Fn.dp_skip_applies(dict(meta, fp8=False), 4096, 256, _params(256, 1024)) is True
    assert Fn.dp_skip_applies(dict(meta, dp_skip=True), 4096, 256, _params(256, 1024)) is True
    assert Fn.dp_skip_applies(dict(meta, H=4), 4096, 512, _params(512, 2048)) is True
