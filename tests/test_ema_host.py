"""Stage-2 EMA consistency training on the host (no GPU): the decay schedule and the copy / lerp / skip decision of tris_amd.ema.EMA
against tests/oracle_ema.py, what the teacher covers and the modes it keeps, the trainer's argument checks behind cfg.stage2_ema,
the new library symbols and the new ops' refusal of CPU tensors."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))


def _args(extra=()):
    from tris_amd.args import get_parser
    return get_parser().parse_args(["--backbone", "clip-RN50", "--size", "320", "--max_query_len", "20"] + list(extra))


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(3, 2)
        self.bn = torch.nn.BatchNorm1d(2)


@pytest.fixture(scope="module")
def stage2_ema():
    """EMA of a Stage-2 model at the moment train_stage2.main builds it: right after TRIS(args), before model.train()"""
    import warnings
    from tris_amd.CLIP import clip
    from tris_amd.ema import EMA
    from tris_amd.model.model_stage2 import TRIS
    with warnings.catch_warnings(), clip.random_init():
        warnings.simplefilter("ignore")
        m = TRIS(_args())
    return m, EMA(m)


def test_decay_schedule_at_the_defaults():
    import oracle_ema as E
    from tris_amd.ema import EMA
    ema = EMA(_Tiny())
    got = []
    for step in range(401):
        ema.step = step
        got.append(ema.get_current_decay())
        assert got[-1] == E.current_decay(step)
    assert all(d == 0.0 for d in got[:102]) and got[102] > 0.0
    assert got[111] == 1 - 11 ** (-2 / 3)              # the update that READS step 110 evaluates it at 111
    assert all(b > a for a, b in zip(got[102:], got[103:]))
    assert max(got) < 0.9999
    ema.step = 10 ** 9
    assert ema.get_current_decay() == 0.9999            # capped by beta
    assert EMA(_Tiny(), beta=0.5).beta == 0.5
    e2 = EMA(_Tiny(), beta=0.5, min_value=0.3)
    e2.step = 102
    assert e2.get_current_decay() == max(1 - 2 ** (-2 / 3), 0.3)
    e2.step = 1000
    assert e2.get_current_decay() == 0.5


@pytest.mark.parametrize("kw", [{}, dict(update_after_step=2, update_every=1), dict(update_after_step=25, update_every=7)])
def test_copy_lerp_skip_decision_against_the_oracle(kw):
    import oracle_ema as E
    from tris_amd.ema import EMA
    ema = EMA(_Tiny(), **kw)
    seen = []
    ema._launch = seen.append                            # recording stub in place of the launches
    sched = E.Schedule(**kw)
    kinds = set()
    for step in range(131):
        del seen[:]
        assert ema.step == step
        ema.update()
        want = [1.0 if a[0] == "copy" else 1.0 - a[1] for a in sched()]
        assert seen == want, (step, seen, want)
        kinds.add(len(want))
    # skipped (where update_every > 1), one launch, and the copy + lerp of the first averaging update
    assert ema.step == 131 and ema.initted and kinds == ({0, 1, 2} if ema.update_every > 1 else {1, 2})


def test_update_with_an_argument_raises_type_error():
    from tris_amd.ema import EMA
    m = _Tiny()
    ema = EMA(m)
    with pytest.raises(TypeError):
        ema.update(m)
    assert ema.step == 0


def test_covered_tensors_and_grad_flags(stage2_ema):
    m, ema = stage2_ema
    names = ema.covered_names()
    sd = ema.ema_model.state_dict()
    assert not any(k.endswith("num_batches_tracked") for k in names)
    assert sorted(names) == sorted(k for k, v in sd.items() if v.is_floating_point())
    assert len(sd) - len(names) == sum(k.endswith("num_batches_tracked") for k in sd) > 0
    assert "reduced_c1.bn.running_mean" in names and "backbone.logit_scale" in names and "output3.relu.weight" in names
    assert all(not p.requires_grad for p in ema.ema_model.parameters())
    assert any(p.requires_grad for p in m.parameters())                       # the student's flags are untouched
    assert all(a is not b for a, b in zip(m.parameters(), ema.ema_model.parameters()))
    named = dict(ema.ema_model.named_parameters())
    assert getattr(named["backbone.logit_scale"], "_tris_no_grad_path", False)


def test_teacher_modes_after_construction(stage2_ema):
    m, ema = stage2_ema
    t = ema.ema_model
    assert t.training is True and t.backbone.training is False and t.reduced_c1.training is True
    assert t.reduced_c1.bn.training is True and t.final_seg1[0].training is True and t.backbone.visual.bn1.training is False
    m.train()                                             # the student's mode changes do not reach the copy
    assert t.backbone.training is False
    m.eval()
    assert t.training is True and t.reduced_c1.training is True


def test_check_args_behind_the_knob():
    from tris_amd import train_stage2
    from tris_amd.config import cfg
    with cfg.override(stage2_ema=False):
        with pytest.raises(NotImplementedError, match="ema_pytorch"):
            train_stage2._check_args(_args(["--model_ema"]))
        train_stage2._check_args(_args())
    with cfg.override(stage2_ema=True):
        train_stage2._check_args(_args(["--model_ema"]))
        train_stage2._check_args(_args(["--model_ema", "--consistency_type", "mse"]))
        with pytest.raises(ValueError, match="kl_div"):
            train_stage2._check_args(_args(["--model_ema", "--consistency_type", "kl"]))
        train_stage2._check_args(_args(["--consistency_type", "kl"]))      # without EMA the flag is never read
        with pytest.raises(NotImplementedError, match="single GPU"):
            train_stage2._check_args(_args(["--model_ema", "--distributed"]))


def test_train_step_signature():
    import inspect
    from tris_amd import train_stage2
    assert list(inspect.signature(train_stage2.train_step).parameters) == ["model", "optimizer", "img", "word_ids", "pseudo",
                                                                            "model_ema", "consistency"]


def test_new_symbols_are_exported():
    from tris_amd import _lib
    decls, _ = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIBPATH)
    for name in ("tris_lerp_f32", "tris_lerp_table_f32", "tris_seg_loss5_fwd_f32", "tris_seg_loss5_bwd_f32",
                 "tris_seg_loss5_workspace_bytes"):
        assert name in decls and hasattr(lib, name), name
    assert _lib.query("tris_seg_loss5_workspace_bytes", 35) == 8 * 8
    assert _lib.query("tris_seg_loss5_workspace_bytes", 48 * 320 * 320) == 8 * 512 * 8


def test_new_ops_refuse_cpu_tensors():
    from tris_amd import ops
    x = [torch.randn(1, 1, 4, 4) for _ in range(4)]
    with pytest.raises(ops.NoGpuError):
        ops.seg_loss5(x, x, torch.zeros(1, 1, 4, 4, dtype=torch.long))
    with pytest.raises(ops.NoGpuError):
        ops.ema_update([(torch.zeros(8), torch.ones(8))], 0.5)
    with pytest.raises(ops.NoGpuError):
        ops.LerpTable([(torch.zeros(8), torch.ones(8))])
