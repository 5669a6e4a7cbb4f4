"""Training IRNet's heads without a GPU: the torch restatement (tests/oracle_irn_train.py) against what the reference's own
AffinityDisplacementLoss and PolyOptimizer recorded (tests/golden/g17_irn_train.npz, tools/gen_golden_irn_train.py); PolySGD's host
side (schedule, the momentum-slot quirk, state dict); the trainer's parameter groups; the exports; the no-CPU-fallback rule."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import oracle_irn as O
import oracle_irn_train as T

NEW_ENTRY_POINTS = ["tris_irn_stem_batch_f32", "tris_gn_up_bwd_workspace_bytes", "tris_gn_up_bwd_f32",
                    "tris_irn_head_bwd_workspace_bytes", "tris_irn_head_bwd_f32", "tris_sgd_momentum_f32"]


@pytest.fixture(scope="module")
def g17(golden):
    return golden("g17_irn_train.npz")


@pytest.fixture(scope="module")
def filled(g17):
    return O.filled_state_dict(int(g17["weight_seed"]), float(g17["gain"]))


def test_golden_is_what_the_tests_rely_on(g17):
    """the shapes the issue sets; labels from {0, 1, 2, 255}; exact zeros in a padded border; the file within the size limit"""
    assert T.SHAPES == ((2, 65, 97, 10), (3, 72, 50, 5), (2, 64, 96, 10))
    seed = int(g17["seed"])
    for i, (B, H, W, _) in enumerate(T.SHAPES):
        h, w = T.map_size(H, W)
        assert g17[f"a{i}_edge_out"].shape == (B, 1, h, w) and g17[f"a{i}_dp_out"].shape == (B, 2, h, w)
        lab = T.labels(i, seed).numpy()
        assert lab.shape == (B, h, w) and set(np.unique(lab)) <= {0, 1, 2, 255} and len(np.unique(lab)) == 4
        x = T.images(i, seed)
        assert x.dtype == torch.float32 and tuple(x.shape) == (B, 3, H, W)
        assert bool((x[-1, :, H - 9:, :] == 0).all()) and bool((x[-1, :, :, W - 6:] == 0).all()) and bool((x[0] != 0).any())
    assert os.path.getsize(os.path.join(GOLDEN, "g17_irn_train.npz")) < 1_000_000
    assert int(g17["update_ok"]) == 1


def test_restatement_linear_functional_against_the_recording(g17, filled):
    """fp32 restatement with its own masks against the reference's fp32 run: outputs and the gradient of every head parameter,
    1e-5 relative L2 per tensor"""
    seed = int(g17["seed"])
    worst = 0.0
    for i in range(len(T.SHAPES)):
        Ge, Gd = T.cotangents(i, seed)
        r = T.linear_functional(filled, T.images(i, seed), Ge, Gd, torch.float32)
        for name in ("edge_out", "dp_out"):
            d = T.rel_l2(r[name].numpy(), g17[f"a{i}_{name}"])
            worst = max(worst, d)
            assert d < 1e-5, (i, name, d)
        for k, g in r["grads"].items():
            d = T.rel_l2(T.sample(g).numpy(), g17[f"a{i}_grad_{k}"])
            worst = max(worst, d)
            assert d < 1e-5, (i, k, d)
    print(f"worst distance {worst:.3e}")


def test_restatement_three_steps_against_the_recording(g17, filled):
    """the four losses of step 0 and every head parameter after three iterations of the reference's loop with PolyOptimizer"""
    seed = int(g17["seed"])
    B, H, W, radius = T.SHAPES[T.STEP_SHAPE]
    first, after, before = T.train_steps(filled, T.images(T.STEP_SHAPE, seed), T.labels(T.STEP_SHAPE, seed), radius, torch.float32)
    d = T.rel_l2(first.numpy(), g17["b_losses"])
    print(f"losses of step 0: {d:.3e}")
    assert d < 1e-5
    worst = 0.0
    for k, p in after.items():
        d = T.rel_l2(T.sample(p).numpy(), g17[f"b_param_{k}"])
        worst = max(worst, d)
        assert d < 1e-5, (k, d)
        assert not torch.equal(p, before[k]), k
    print(f"worst parameter distance after {T.N_STEPS} steps {worst:.3e}")


def _poly(params=None, **kw):
    from tris_amd.optim import PolySGD
    params = [torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.ones(3, 2))] if params is None else params
    args = dict(lr=T.LR, weight_decay=T.WEIGHT_DECAY, max_step=T.MAX_STEP)
    args.update(kw)
    return PolySGD([{"params": params[:1], "lr": 1 * args["lr"], "weight_decay": args["weight_decay"]},
                    {"params": params[1:], "lr": 10 * args["lr"], "weight_decay": args["weight_decay"]}], **args), params


def test_poly_schedule_is_the_references(g17):
    """the learning rates of MAX_STEP + 2 steps, bit for bit the reference's Python floats, including step >= max_step (the last
    learning rate stays)"""
    opt, _ = _poly()
    want = g17["b_lr_sequence"]
    assert len(want) == T.MAX_STEP + 2
    got = []
    for step in range(len(want)):
        assert opt.global_step == step
        lrs = opt.scheduled_lr()
        for g, lr in zip(opt.param_groups, lrs):   # what step() does on the host, without the launch
            g["lr"] = lr
        opt.global_step += 1
        got.append(lrs)
        assert lrs[1] == 10 * T.LR * ((1 - step / T.MAX_STEP) ** 0.9 if step < T.MAX_STEP else (1 - (T.MAX_STEP - 1) / T.MAX_STEP) ** 0.9)
    assert [g[0] for g in got] == [float(v) for v in want]
    assert want[-1] == want[-2] == want[T.MAX_STEP - 1]
    assert T.poly_lr([T.LR], 2, T.MAX_STEP) == [float(want[2])] and T.poly_lr([T.LR], T.MAX_STEP, T.MAX_STEP) is None


def test_momentum_slot_quirk(g17):
    """PolyOptimizer's super().__init__(params, lr, weight_decay) puts the weight-decay value into torch.optim.SGD's momentum slot:
    pinned against torch.optim.SGD constructed the reference's way, and against what the reference's optimiser recorded"""
    opt, params = _poly()
    ref = torch.optim.SGD([{"params": params[:1], "lr": T.LR, "weight_decay": T.WEIGHT_DECAY},
                           {"params": params[1:], "lr": 10 * T.LR, "weight_decay": T.WEIGHT_DECAY}], T.LR, T.WEIGHT_DECAY)
    for g, r in zip(opt.param_groups, ref.param_groups):
        for key in ("lr", "momentum", "dampening", "weight_decay", "nesterov"):
            assert g[key] == r[key], key
        assert g["momentum"] == T.WEIGHT_DECAY == float(g17["b_momentum"]) and g["momentum"] != 0.9
    assert [g["weight_decay"] for g in opt.param_groups] == [float(v) for v in g17["b_group_wd"]]
    assert opt.power == 0.9
    # a group without a weight decay of its own gets SGD's default 0, not the constructor's argument
    from tris_amd.optim import PolySGD
    bare = PolySGD([torch.nn.Parameter(torch.zeros(4))], lr=0.1, weight_decay=1e-4, max_step=10)
    assert bare.param_groups[0]["weight_decay"] == 0 and bare.param_groups[0]["momentum"] == 1e-4
    assert "deliberate" in PolySGD.__doc__


def test_poly_sgd_state_dict_round_trip():
    """torch.optim.SGD's layout plus global_step, in both directions: a state dict of torch's own SGD (constructed the reference's
    way, stepped once) loads, comes out again unchanged, and torch's SGD loads what PolySGD emits.  Whether the next step reads
    the momentum buffers follows what was loaded, per group, as in torch."""
    opt, params = _poly()
    assert opt.state_dict()["state"] == {} and opt.state_dict()["global_step"] == 0
    mk = lambda: torch.optim.SGD([{"params": params[:1], "lr": T.LR, "weight_decay": T.WEIGHT_DECAY},
                                  {"params": params[1:], "lr": 10 * T.LR, "weight_decay": T.WEIGHT_DECAY}], T.LR, T.WEIGHT_DECAY)
    ref = mk()
    g = torch.Generator().manual_seed(3)
    grads = [torch.randn(p.shape, generator=g) for p in params]
    for p, gr, view in zip(params, grads, [p.grad for p in params]):
        view.copy_(gr)                    # (the arena view stays the parameter's .grad)
    ref.step()
    bufs = [ref.state[p]["momentum_buffer"].clone() for p in params]
    sd_ref = dict(ref.state_dict(), global_step=2)
    sd_ref["param_groups"][0]["lr"] = 0.05
    opt.load_state_dict(sd_ref)
    sd = opt.state_dict()
    assert sorted(sd) == ["global_step", "param_groups", "state"] and sd["global_step"] == 2
    assert [g["initial_lr"] for g in sd["param_groups"]] == [T.LR, 10 * T.LR] and sd["param_groups"][0]["lr"] == 0.05
    assert sorted(sd["state"]) == [0, 1] and [g["params"] for g in sd["param_groups"]] == [[0], [1]]
    assert all(sorted(st) == ["momentum_buffer"] for st in sd["state"].values())
    assert all(torch.equal(sd["state"][j]["momentum_buffer"], bufs[j]) for j in range(2))
    again = mk()
    again.load_state_dict({"state": sd["state"], "param_groups": sd["param_groups"]})      # torch's own SGD accepts the layout
    assert torch.equal(again.state[params[1]]["momentum_buffer"], bufs[1])
    other, _ = _poly()
    other.load_state_dict(sd)
    assert other.global_step == 2 and other.param_groups[0]["lr"] == 0.05 and other.param_groups[0]["initial_lr"] == T.LR
    assert other.scheduled_lr() == opt.scheduled_lr()
    assert all(torch.equal(other.state_dict()["state"][j]["momentum_buffer"], bufs[j]) for j in range(2))
    # a checkpoint without buffers, whatever its step count: the next step creates them (nothing is emitted before it)
    fresh, _ = _poly()
    fresh.load_state_dict({"state": {}, "param_groups": sd["param_groups"], "global_step": 3})
    assert fresh.global_step == 3 and fresh.state_dict()["state"] == {}
    # buffers for one group only: that group reads them, the other creates its own
    half, _ = _poly()
    half.load_state_dict({"state": {1: sd["state"][1]}, "param_groups": sd["param_groups"], "global_step": 1})
    assert sorted(half.state_dict()["state"]) == [1]
    with pytest.raises(ValueError, match="parameter groups"):
        other.load_state_dict({"state": {}, "param_groups": sd["param_groups"][:1]})
    two = [torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(4))]
    part, _ = _poly(two)
    groups = part.state_dict()["param_groups"]
    with pytest.raises(ValueError, match="momentum buffer"):
        part.load_state_dict({"state": {1: {"momentum_buffer": torch.zeros(3)}}, "param_groups": groups, "global_step": 1})


def test_trainer_makes_the_references_groups_trainable():
    """exactly trainable_parameters() of the reference -- edge_layers and dp_layers -- by name against the recorded key list"""
    from tris_amd.irn_net import EdgeDisplacement, canonical_name
    from tris_amd.irn_train import IrnTrainer, head_parameter_names
    with open(os.path.join(GOLDEN, "g15_irn_keys.json")) as f:
        keys = [k for k, _ in json.load(f)]
    net = EdgeDisplacement()
    params = dict(net.named_parameters())
    want = [[canonical_name(k) for k in keys if k.startswith(prefix) and canonical_name(k) in params]
            for prefix in ("edge_layers.", "dp_layers.")]
    assert (len(want[0]), len(want[1])) == (17, 22)
    assert [list(n) for n in head_parameter_names()] == want == [list(n) for n in T.head_names()]
    tr = IrnTrainer(net, lr=0.1, weight_decay=1e-4, max_step=10)
    trainable = [k for k, p in net.named_parameters() if p.requires_grad]
    assert sorted(trainable) == sorted(want[0] + want[1])
    assert all(not p.requires_grad for k, p in net.named_parameters() if k.startswith("resnet50."))
    groups = tr.optimizer.param_groups
    assert [[id(p) for p in g["params"]] for g in groups] == [[id(params[k]) for k in names] for names in want]
    assert [g["lr"] for g in groups] == [0.1, 1.0] and [g["weight_decay"] for g in groups] == [1e-4, 1e-4]
    assert sum(p.numel() for g in groups for p in g["params"]) == 1_394_529
    # the canonical state dict is what a fresh network loads
    fresh = EdgeDisplacement()
    fresh.load_state_dict(tr.state_dict())
    assert all(torch.equal(v, fresh.state_dict()[k]) for k, v in tr.state_dict().items())


def test_c_abi_exports_the_new_entry_points():
    from tris_amd import _lib
    lib = _lib.load()
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.DECLS and hasattr(lib, name), name
    assert _lib.query("tris_gn_up_bwd_workspace_bytes", 2, 9 * 13, 32, 4) > 0
    assert _lib.query("tris_irn_head_bwd_workspace_bytes", 850, 160, 1) > 0
    assert _lib.query("tris_gn_up_bwd_workspace_bytes", 2, 9 * 13, 30, 4) == 0


def test_training_without_a_gpu_raises():
    """no CPU path: train_step, fit_mean_shift and PolySGD.step raise NoGpuError for a network left on the CPU"""
    from tris_amd import ops
    from tris_amd.irn_net import EdgeDisplacement
    from tris_amd.irn_train import IrnTrainer
    tr = IrnTrainer(EdgeDisplacement(), lr=0.1, weight_decay=1e-4, max_step=10)
    x, lab = torch.zeros(1, 3, 64, 96), torch.zeros(1, 16, 24, dtype=torch.uint8)
    with pytest.raises(ops.NoGpuError):
        tr.train_step(x, lab)
    with pytest.raises(ops.NoGpuError):
        tr.fit_mean_shift([x])
    with pytest.raises(ops.NoGpuError):
        tr.optimizer.step()
    with pytest.raises(ValueError, match="float32"):
        tr.train_step(x.to(torch.uint8), lab)
