"""Host side of the fine-tuning step (internvideo_amd.finetune), no GPU: the Mixup table builder draws what the reference's
datasets/mixup.py draws under the same numpy seed -- kinds, boxes, the (lam, oml) pairs as fp32 bit patterns, the target pairs -- and
leaves numpy's global RNG where the reference leaves it (tests/golden/finetune_mixup.npz, made by make_golden_finetune_mixup.py from the
reference's own code)."""
import inspect
import os

import numpy as np
import pytest
import torch

from internvideo_amd import finetune, ops
from internvideo_amd.lib import InternVideoHipError

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "finetune_mixup.npz")
CONFIGS = {
    "std": dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.7, switch_prob=0.5, label_smoothing=0.1, num_classes=10),
    "minmax": dict(mixup_alpha=0.8, cutmix_alpha=1.0, cutmix_minmax=(0.2, 0.8), prob=0.7, switch_prob=0.5, label_smoothing=0.1, num_classes=10),
}


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _draws(gold, cfg=None, mode=None):
    for key in gold["draws"]:
        c, m, si, seed = str(key).split(":")
        if (cfg is None or c == cfg) and (mode is None or m == mode):
            yield str(key) + ":", c, m, tuple(int(v) for v in gold["shapes"][int(si)]), int(seed)


@pytest.mark.parametrize("cfg,mode", [("std", "batch"), ("std", "elem"), ("minmax", "batch"), ("minmax", "elem")])
def test_draw_reproduces_the_reference_bit_for_bit_and_leaves_its_rng_state(gold, cfg, mode):
    n, kinds = 0, set()
    for pre, c, m, shape, seed in _draws(gold, cfg, mode):
        mix = finetune.Mixup(mode=m, **CONFIGS[c])
        np.random.seed(seed)
        p = mix.draw(shape[0], shape)
        nxt = np.random.rand()
        want = gold[pre + "table"]
        assert p.table.dtype == np.int32 and p.table.shape == (shape[0], 8) and p.target_mix.dtype == np.float32
        assert np.array_equal(p.table[:, :2], want[:, :2]), (pre, "src / kind", p.table[:, :2], want[:, :2])
        assert np.array_equal(p.table[:, 2:6], want[:, 2:6]), (pre, "box")
        assert np.array_equal(p.table[:, 6:], want[:, 6:]), (pre, "lam / oml bit patterns")
        assert p.target_mix.tobytes() == gold[pre + "tmix"].tobytes(), (pre, "target pairs")
        assert nxt == float(gold[pre + "next_rand"][0]), (pre, "RNG state after the draw")
        kinds |= set(int(k) for k in want[:, 1])
        n += 1
    assert n >= (24 if cfg == "std" else 6) and kinds == {0, 1, 2}, (n, kinds)


def test_fixture_holds_the_cases_the_kernels_must_survive(gold):
    """the generator asserts these when it writes the file; they are what the GPU tests lean on"""
    odd = clipped_or_edge = all3 = False
    batch_kinds = set()
    for pre, c, m, shape, seed in _draws(gold, "std"):
        t = gold[pre + "table"]
        cut = t[t[:, 1] == 2]
        odd |= bool(((cut[:, 4] % 2) | (cut[:, 5] % 2)).any())
        clipped_or_edge |= bool(((cut[:, 2] == 0) | (cut[:, 3] == shape[-2]) | (cut[:, 4] == 0) | (cut[:, 5] == shape[-1])).any())
        if m == "batch":
            batch_kinds.add(int(t[0, 1]))
        else:
            all3 |= set(int(k) for k in t[:, 1]) == {0, 1, 2}
    assert odd and clipped_or_edge and all3 and batch_kinds == {0, 1, 2}


def test_mixup_disabled_draws_nothing_and_consumes_no_randomness():
    for mode in ("batch", "elem"):
        mix = finetune.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, num_classes=10)
        mix.mixup_enabled = False
        np.random.seed(5)
        want = np.random.rand()
        np.random.seed(5)
        p = mix.draw(4, (4, 3, 2, 14, 14))
        assert np.random.rand() == want
        assert (p.table[:, 1] == 0).all() and np.array_equal(p.table[:, 0], [3, 2, 1, 0])
        assert np.array_equal(p.target_mix, np.array([[1, 0]] * 4, dtype=np.float32))


def test_pair_mode_is_refused_with_the_reason():
    with pytest.raises(NotImplementedError, match="pair"):
        finetune.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="pair")


def test_odd_batch_raises():
    mix = finetune.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=10)
    with pytest.raises(ValueError, match="even"):
        mix.draw(3, (3, 3, 2, 14, 14))
    with pytest.raises(AssertionError, match="even"):
        mix(torch.zeros(3, 3, 2, 14, 14), torch.zeros(3, dtype=torch.long))


def test_cpu_tensors_are_refused_there_is_no_cpu_path():
    x = torch.zeros(2, 3, 2, 14, 14)
    table = torch.zeros(2, 8, dtype=torch.int32)
    with pytest.raises(InternVideoHipError):
        ops.mix_clips(x, table)
    with pytest.raises(InternVideoHipError):
        ops.soft_ce_rows(torch.zeros(2, 16), torch.zeros(2, dtype=torch.int32), V=10)
    with pytest.raises(InternVideoHipError):
        ops.mixup_target(torch.zeros(2, dtype=torch.int32), torch.zeros(2, 2), 0.1, 10)


def test_constructor_and_attributes_are_the_ones_the_finetuning_script_uses():
    """run_finetuning.py:349-352 passes these keywords; the loop reads / sets `mixup_enabled`"""
    mix = finetune.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode="batch",
                         label_smoothing=0.1, num_classes=400)
    assert list(inspect.signature(finetune.Mixup.__init__).parameters)[1:] == [
        "mixup_alpha", "cutmix_alpha", "cutmix_minmax", "prob", "switch_prob", "mode", "correct_lam", "label_smoothing", "num_classes"]
    assert (mix.mixup_alpha, mix.cutmix_alpha, mix.cutmix_minmax, mix.mix_prob, mix.switch_prob, mix.mode, mix.correct_lam,
            mix.label_smoothing, mix.num_classes, mix.mixup_enabled) == (0.8, 1.0, None, 1.0, 0.5, "batch", True, 0.1, 400, True)
    assert finetune.Mixup(cutmix_minmax=(0.2, 0.8)).cutmix_alpha == 1.0           # min / max switches CutMix on
    assert finetune.LabelSmoothingCrossEntropy(smoothing=0.1).smoothing == 0.1 and isinstance(finetune.SoftTargetCrossEntropy(), torch.nn.Module)


def test_the_three_entry_points_are_declared_and_bound():
    from internvideo_amd import lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "internvideo_hip.h")).read()
    for name in ("ivh_mix_clips", "ivh_soft_ce_rows", "ivh_mixup_target"):
        assert name in lib.SIGNATURES and name + "(" in header, name
    import internvideo_amd.torch_ops as T
    assert "soft_target_cross_entropy" in T.DIFFERENTIABLE and "mix_clips" in T.OPERATORS
    lg = torch.empty((6, 10), dtype=torch.bfloat16, device="meta")
    out = torch.ops.internvideo_hip.soft_target_cross_entropy(lg, torch.empty((6,), dtype=torch.int32, device="meta"))
    assert out.shape == (1,) and out.dtype == torch.float32
    clip = torch.empty((2, 3, 2, 14, 14), dtype=torch.float32, device="meta")
    assert torch.ops.internvideo_hip.mix_clips(clip, torch.empty((2, 8), dtype=torch.int32, device="meta")).dtype == torch.bfloat16
