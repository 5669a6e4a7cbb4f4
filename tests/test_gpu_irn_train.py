"""Training IRNet's edge / displacement heads on the MI355X (csrc/irntrain.hip, tris_amd/irn_train.py, tris_amd.optim.PolySGD).

The ground rule of tests/test_gpu_irn_net.py and tests/test_gpu_irn_loss.py: a GPU result is compared against the fp64 restatement
(tests/oracle_irn_train.py) and must lie within 8 x the distance of the fp32 CPU computation of the same thing from fp64, floored
at 4 fp32 ulps (relative L2 per tensor).  Gradients are taken under the GPU's own ReLU masks, imposed on the restatement; the masks
themselves are compared separately."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle_irn as O
import oracle_irn_loss as L
import oracle_irn_train as T

pytestmark = pytest.mark.gpu
FLOOR = 4 * 2.0 ** -23


@pytest.fixture(params=["x3", "h2"])
def arith(request):
    """both arithmetics of the dense products, as tests/test_gpu_irn_net.py: for every test that runs one (a test of a kernel
    that has no product in it runs once)"""
    from tris_amd import ops
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(request.param)
    yield request.param
    ops.set_gemm_mode(prev)


def _d(a, b):
    cpu = lambda t: t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)
    return T.rel_l2(cpu(a), cpu(b))


def _within(what, got, ref32, ref64):
    """the ground rule; prints the figures before it asserts; returns the ratio"""
    e_ref, e_gpu = _d(ref32, ref64), _d(got, ref64)
    bound = max(8 * e_ref, FLOOR)
    print(f"{what}: e_ref {e_ref:.3e}, gpu {e_gpu:.3e}, ratio {e_gpu / max(e_ref, FLOOR / 8):.2f}")
    assert e_gpu <= bound, (what, e_gpu, e_ref)
    return e_gpu / max(e_ref, FLOOR / 8)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.fixture(scope="module")
def g17(golden):
    return golden("g17_irn_train.npz")


@pytest.fixture(scope="module")
def filled(g17):
    return O.filled_state_dict(int(g17["weight_seed"]), float(g17["gain"]))


def _net(filled):
    from tris_amd.irn_net import EdgeDisplacement
    m = EdgeDisplacement()
    m.load_state_dict(filled)
    return m.cuda()


def _trainer(filled, **kw):
    from tris_amd.irn_train import IrnTrainer
    args = dict(lr=T.LR, weight_decay=T.WEIGHT_DECAY, max_step=T.MAX_STEP)
    args.update(kw)
    return IrnTrainer(_net(filled), **args)


def _head_state(tr):
    return {k: v.detach().clone() for k, v in tr.net.state_dict().items() if k.startswith("fc_")}


# ------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("H,W", [(65, 97), (72, 50)])
def test_float_stem(H, W):
    """fp32 [B,H,W,3] with exact zeros in a padded border against conv2d + frozen BatchNorm + ReLU in fp64; on an image the
    normalisation table can represent, bit for bit the uint8 stem's row 0"""
    from tris_amd import ops
    from tris_amd.irn_net import normalize_table
    from tris_amd.utils.synth import irn_image
    g = torch.Generator().manual_seed(H * W)
    x = torch.stack([O.normalize(irn_image(H, W, seed=H + b)) for b in range(3)])
    x[1, :, H - 11:, :] = 0.0
    x[1, :, :, :7] = 0.0
    w = torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5
    mean, var = 0.1 * torch.randn(64, generator=g), 1 + 0.1 * torch.rand(64, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(64, generator=g), 0.1 * torch.randn(64, generator=g)
    invstd = (1.0 / torch.sqrt(var.double() + 1e-5)).float()

    def ref(dt):
        v = lambda t: t.to(dt).view(1, -1, 1, 1)
        return F.relu((F.conv2d(x.to(dt), w.to(dt), stride=2, padding=3) - v(mean)) * (v(invstd) * v(gamma)) + v(beta))
    d = lambda t: t.cuda()
    wk = d(w.permute(2, 3, 1, 0).contiguous())
    y = ops.irn_stem_batch(d(_nhwc(x)), wk, d(mean), d(invstd), d(gamma), d(beta))
    assert tuple(y.shape) == (3, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64)
    assert torch.equal(y, ops.irn_stem_batch(d(_nhwc(x)), wk, d(mean), d(invstd), d(gamma), d(beta)))
    _within(f"float stem {H}x{W}", _nchw(y), ref(torch.float32), ref(torch.float64))
    img = irn_image(H, W, seed=5)
    lut = normalize_table()
    xf = torch.stack([lut[c][torch.from_numpy(img[..., c]).long()] for c in range(3)], -1)[None]      # [1,H,W,3]
    y8 = ops.irn_stem(d(torch.from_numpy(img)), d(lut), wk, d(mean), d(invstd), d(gamma), d(beta))
    yf = ops.irn_stem_batch(d(xf.contiguous()), wk, d(mean), d(invstd), d(gamma), d(beta))
    assert torch.equal(yf[0], y8[0])


# (channels, groups, upsample factor) of every GroupNorm of the two branches (tris_amd.irn_net EDGE and DP; fc_dp7 is (256, 16, 1))
GN_TABLE = [(32, 4, 1), (32, 4, 2), (32, 4, 4), (64, 8, 1), (128, 16, 1), (256, 16, 1), (256, 16, 2)]


@pytest.mark.parametrize("overhang", [True, False])
@pytest.mark.parametrize("C,G,scale", GN_TABLE)
def test_gn_upsample_backward(C, G, scale, overhang):
    """every (C, G, scale) of the two branches, a 9 x 13 input (two row blocks) whose upsampled map overhangs the crop on both axes
    and one where it does not; the slice sits at channel 32 of a wider buffer whose other channels hold NaN in the gradient.  du,
    dt, dgamma, dbeta against fp64 with the mask of the GPU forward imposed."""
    from tris_amd import ops
    B, hi, wi = 2, 9, 13
    ho, wo = (hi * scale - 1, wi * scale - 1) if overhang else (hi * scale, wi * scale)
    g = torch.Generator().manual_seed(C * scale + int(overhang))
    t = torch.randn(B, C, hi, wi, generator=g) * (1 + torch.rand(1, C, 1, 1, generator=g)) + 0.3 * torch.randn(1, C, 1, 1, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    dy = torch.randn(B, C, ho, wo, generator=g)
    Ct, off = C + 64, 32
    tc = _nhwc(t).cuda()
    st = ops.group_norm_stats(tc, G)
    out = torch.zeros(B, ho, wo, Ct, device="cuda")
    ops.gn_apply_up(tc, st, gamma.cuda(), beta.cuda(), G, scale, (ho, wo), True, out, off)
    mask = _nchw(out[..., off:off + C] > 0).cpu()
    d_out = torch.full((B, ho, wo, Ct), float("nan"), device="cuda")
    d_out[..., off:off + C] = _nhwc(dy).cuda()

    def run():
        return ops.gn_up_bwd(d_out, out, off, tc, st, gamma.cuda(), G, scale, want_du=True)
    got = run()
    assert all(torch.equal(a, b) for a, b in zip(got, run()))        # bitwise repeatable
    dt, dgamma, dbeta, du = got
    assert not any(bool(torch.isnan(v).any()) for v in got)

    def ref(dtype):
        x, ga, be = (v.detach().to(dtype).clone().requires_grad_(True) for v in (t, gamma, beta))
        n = F.group_norm(x, G, ga, be, 1e-5)
        n.retain_grad()
        y = F.interpolate(n, scale_factor=scale, mode="bilinear", align_corners=False) if scale > 1 else n
        (y[..., :ho, :wo] * mask.to(dtype) * dy.to(dtype)).sum().backward()
        return {"du": n.grad, "dt": x.grad, "dgamma": ga.grad, "dbeta": be.grad}
    r32, r64 = ref(torch.float32), ref(torch.float64)
    have = {"du": _nchw(du), "dt": _nchw(dt), "dgamma": dgamma, "dbeta": dbeta}
    for k in have:
        _within(f"gn_up_bwd C{C} G{G} x{scale} overhang={overhang} {k}", have[k], r32[k], r64[k])


@pytest.mark.parametrize("C,N,M,bias", [(160, 1, 2 * 17 * 25, True), (256, 2, 3 * 18 * 13, False)])
def test_narrow_head_backward(C, N, M, bias):
    """dX over the whole buffer, dw and db from fp64 block partials; row counts that are no multiple of 8 (two row blocks)"""
    from tris_amd import ops
    assert M % 8
    gen = torch.Generator().manual_seed(C + N)
    x, w, g = torch.randn(M, C, generator=gen), torch.randn(N, C, generator=gen) / C ** 0.5, torch.randn(M, N, generator=gen)

    def run():
        return ops.irn_head_bwd(g.cuda(), x.cuda(), w.cuda(), want_db=bias)
    dx, dw, db = run()
    again = run()
    assert torch.equal(dx, again[0]) and torch.equal(dw, again[1]) and (db is None or torch.equal(db, again[2]))
    ref = lambda dt: (g.to(dt) @ w.to(dt), g.to(dt).t() @ x.to(dt), g.to(dt).sum(0))
    r32, r64 = ref(torch.float32), ref(torch.float64)
    _within(f"head bwd C{C} N{N} dX", dx, r32[0], r64[0])
    _within(f"head bwd C{C} N{N} dw", dw, r32[1], r64[1])
    if bias:
        _within(f"head bwd C{C} N{N} db", db, r32[2], r64[2])
    else:
        assert db is None


# ------------------------------------------------------------------------------------- the whole head, linear functional
@pytest.fixture(scope="module")
def cpu_runs(g17, filled):
    """per shape: the fp64 and fp32 restatements with their own masks (taps, pre-activations, outputs), computed once"""
    torch.set_num_threads(16)
    seed = int(g17["seed"])
    out = []
    for i in range(len(T.SHAPES)):
        Ge, Gd = T.cotangents(i, seed)
        x = T.images(i, seed)
        out.append({"x": x, "Ge": Ge, "Gd": Gd, "r64": T.linear_functional(filled, x, Ge, Gd, torch.float64),
                    "r32": T.linear_functional(filled, x, Ge, Gd, torch.float32)})
    return out


@pytest.mark.parametrize("i", range(len(T.SHAPES)))
def test_heads_linear_functional(i, g17, filled, cpu_runs, arith):
    """forward against recording (a); parameter gradients against fp64 with the GPU's masks imposed; the masks against the fp64
    restatement's own (they may differ only where |pre| < 1e-4 rms, at no more than 1e-3 of the elements); no gradient reaches the
    trunk or a tap"""
    c = cpu_runs[i]
    tr = _trainer(filled)
    keep = {}
    with tr.scope():
        taps = tr.taps(c["x"])
        edge_out, dp_out = tr.heads(taps, keep)
        ((c["Ge"].cuda() * edge_out).sum() + (c["Gd"].cuda() * dp_out).sum()).backward()
    worst = 0.0
    for name, got in (("edge_out", edge_out), ("dp_out", dp_out)):
        worst = max(worst, _within(f"[{arith}] shape {i} {name}", got, g17[f"a{i}_{name}"], c["r64"][name]))
    masks = T.masks_from_buffers(keep)
    frac, rel = T.mask_disagreement(masks, c["r64"]["pre"])
    print(f"[{arith}] shape {i}: masks differ at {frac:.2e} of the elements, largest |pre| / rms among them {rel:.2e}")
    assert frac <= 1e-3 and rel < 1e-4
    m64 = T.linear_functional(filled, c["x"], c["Ge"], c["Gd"], torch.float64, masks, c["r64"]["taps"])
    m32 = T.linear_functional(filled, c["x"], c["Ge"], c["Gd"], torch.float32, masks, c["r32"]["taps"])
    named = dict(tr.net.named_parameters())
    for k in m64["grads"]:
        assert named[k].grad is not None and tuple(named[k].grad.shape) == tuple(named[k].shape), k
        worst = max(worst, _within(f"[{arith}] shape {i} grad {k}", named[k].grad, m32["grads"][k], m64["grads"][k]))
    print(f"[{arith}] shape {i}: worst ratio {worst:.2f}")
    # gradients that must not exist
    assert all(p.grad is None for k, p in named.items() if k.startswith("resnet50."))
    assert all(t.grad is None and not t.requires_grad for t in taps)


# ---------------------------------------------------------------------------------------------------------------- PolySGD
def test_poly_sgd_three_steps():
    """three steps on seeded parameters and gradients, two groups with different learning rates, against an fp64 SGD (torch's fp32
    SGD, constructed the reference's way, is the fp32 side); the first step does not read the momentum buffer"""
    from tris_amd.optim import PolySGD
    gen = torch.Generator().manual_seed(11)
    shapes = [(32, 64, 1, 1), (32,), (1, 160, 1, 1), (1,), (256, 448, 1, 1), (2, 256, 1, 1), (7,)]
    init = [torch.randn(s, generator=gen) for s in shapes]
    grads = [[torch.randn(s, generator=gen) for s in shapes] for _ in range(3)]
    split = 4
    mk = lambda ps: [{"params": ps[:split], "lr": 1 * T.LR, "weight_decay": T.WEIGHT_DECAY},
                     {"params": ps[split:], "lr": 10 * T.LR, "weight_decay": T.WEIGHT_DECAY}]
    dev = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    opt = PolySGD(mk(dev), lr=T.LR, weight_decay=T.WEIGHT_DECAY, max_step=T.MAX_STEP)
    for a in opt.arenas:
        a.m.fill_(float("nan"))          # torch creates the buffer from the first gradient: whatever is there is not read
    cpu = [torch.nn.Parameter(t.clone()) for t in init]
    ref = torch.optim.SGD(mk(cpu), T.LR, T.WEIGHT_DECAY)
    p64 = [t.double().clone() for t in init]
    bufs = [None] * len(p64)
    for step in range(3):
        lrs = T.poly_lr([T.LR, 10 * T.LR], step, T.MAX_STEP)
        for p, c, g in zip(dev, cpu, grads[step]):
            p.grad.copy_(g.cuda())
            c.grad = g.clone()
        for grp, lr in zip(ref.param_groups, lrs):
            grp["lr"] = lr
        ref.step()
        opt.step()
        assert [g["lr"] for g in opt.param_groups] == lrs
        for j, (p, g) in enumerate(zip(p64, grads[step])):
            b = [bufs[j]]
            T.sgd_step([p], [g.double()], b, lrs[0 if j < split else 1], T.WEIGHT_DECAY, T.WEIGHT_DECAY)
            bufs[j] = b[0]
    assert opt.global_step == 3
    for j, s in enumerate(shapes):
        _within(f"PolySGD update {s}", dev[j].detach().cpu() - init[j], cpu[j].detach() - init[j], p64[j] - init[j].double())
    sd = opt.state_dict()
    assert sd["global_step"] == 3 and len(sd["state"]) == len(shapes)
    _within("PolySGD momentum buffer", sd["state"][4]["momentum_buffer"], ref.state[cpu[4]]["momentum_buffer"], bufs[4])


# ------------------------------------------------------------------------------------------------------------- train_step
@pytest.fixture(scope="module")
def cpu_steps(g17, filled):
    """the three-step run of the restatement in fp64 and fp32, once"""
    torch.set_num_threads(16)
    seed = int(g17["seed"])
    B, H, W, radius = T.SHAPES[T.STEP_SHAPE]
    x, lab = T.images(T.STEP_SHAPE, seed), T.labels(T.STEP_SHAPE, seed)
    return {"x": x, "label": lab, "radius": radius, "r64": T.train_steps(filled, x, lab, radius, torch.float64),
            "r32": T.train_steps(filled, x, lab, radius, torch.float32)}


def _three_steps(filled, c):
    tr = _trainer(filled, radius=c["radius"])
    outs = [tr.train_step(c["x"], c["label"].cuda()) for _ in range(T.N_STEPS)]
    return tr, outs


def test_train_step_is_repeatable(filled, cpu_steps, arith):
    """two runs of three steps from the same state: bitwise-equal parameters and losses"""
    a, la = _three_steps(filled, cpu_steps)
    b, lb = _three_steps(filled, cpu_steps)
    sa, sb = _head_state(a), _head_state(b)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    for x, y in zip(la, lb):
        assert torch.equal(x["losses"], y["losses"]) and torch.equal(x["total"], y["total"]) and torch.equal(x["counts"], y["counts"])
    assert a.optimizer.global_step == 3 and all(not o["losses"].requires_grad and o["losses"].is_cuda for o in la)
    assert bool(torch.isfinite(torch.stack([o["total"] for o in la])).all())


def test_train_step_is_the_composition_of_its_parts(filled, cpu_steps, arith):
    """one train_step equals, bit for bit, forward + irn_aff_losses + head backward with the loss op's gradients + PolySGD by hand"""
    from tris_amd import irn, irn_loss, ops
    c = cpu_steps
    a = _trainer(filled, radius=c["radius"])
    out = a.train_step(c["x"], c["label"].cuda())
    b = _trainer(filled, radius=c["radius"])
    with b.scope(explicit=True):
        edge_out, dp_out = b.heads(b.taps(c["x"]))
        losses, counts = ops.irn_aff_losses(edge_out, dp_out, c["label"].cuda(), *irn.device_tables(edge_out.device, c["radius"]),
                                            radius=c["radius"])
        irn_loss.total_loss(losses).backward()
        b.optimizer.step()
    assert torch.equal(out["losses"], losses.detach()) and torch.equal(out["counts"], counts)
    sa, sb, s0 = _head_state(a), _head_state(b), filled
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert all(not torch.equal(sa[k].cpu(), s0[k]) for k in sa if k.endswith("weight"))      # and the step moved them


def test_step0_losses_against_the_recording(g17, filled, cpu_steps, arith):
    c = cpu_steps
    tr = _trainer(filled, radius=c["radius"])
    out = tr.train_step(c["x"], c["label"].cuda())
    _within(f"[{arith}] step-0 losses", out["losses"], g17["b_losses"], c["r64"][0])
    assert int(out["counts"].min()) > 0


def test_three_step_update_against_fp64(g17, filled, cpu_steps, arith):
    """p3 - p0 per tensor.  The recording's seed was chosen so that the fp32-to-fp64 distance of this update is below 1e-3
    (near-tied path maxima reroute gradients: a condition on the input)."""
    assert int(g17["update_ok"]) == 1
    c = cpu_steps
    tr, _ = _three_steps(filled, c)
    got = _head_state(tr)
    (_, a64, b64), (_, a32, b32) = c["r64"], c["r32"]
    worst = 0.0
    for k in a64:
        worst = max(worst, _within(f"[{arith}] update {k}", got[k].cpu() - filled[k], a32[k] - b32[k], a64[k] - b64[k]))
    print(f"[{arith}] three-step update: worst ratio {worst:.2f}")


def test_full_size_label_and_errors(filled, cpu_steps, arith):
    """a full-size label goes through irn_loss.reduce_label; one that does not reduce to the maps' size raises ValueError"""
    B, H, W, radius = T.SHAPES[2]
    tr = _trainer(filled, radius=radius)
    x = T.images(2, 0)
    lab = torch.zeros(B, H, W, dtype=torch.uint8)
    lab[:, : H // 2, : W // 2] = 1
    lab[:, H // 2:, 10:20] = 255
    out = tr.train_step(x, lab.cuda())
    assert tuple(out["losses"].shape) == (4,) and bool(torch.isfinite(out["total"]))
    with pytest.raises(ValueError, match="reduces to"):
        tr.train_step(x, torch.zeros(B, H + 8, W, dtype=torch.uint8).cuda())


# -------------------------------------------------------------------------------------------- mean shift, state, inference
def test_fit_mean_shift(g17, filled, arith):
    """train_irn.py:93-106 over two batches against recording (c)"""
    seed = int(g17["seed"])
    tr = _trainer(filled)
    batches = [T.images(i, seed) for i in (0, 2)]
    assert np.array_equal(filled["mean_shift.running_mean"].numpy(), g17["c_start"])
    means = []
    for x in batches:
        taps = T.frozen_taps(filled, x, torch.float64)
        sd64 = {k: v.double() for k, v in filled.items() if k.startswith("fc_")}
        _, dp, _ = T.heads(sd64, taps)
        means.append((dp - filled["mean_shift.running_mean"].double().view(1, 2, 1, 1)).mean(dim=(0, 2, 3)))
    ref64 = torch.stack(means).mean(0)
    got = tr.fit_mean_shift(batches)
    _within(f"[{arith}] running_mean", got, g17["c_running_mean"], ref64)
    assert torch.equal(tr.net.mean_shift.running_mean, got) and torch.equal(tr.state_dict()["mean_shift.running_mean"], got.cpu())


def test_state_dict_round_trip(filled, cpu_steps, arith):
    """the trainer's state dict loads into a fresh network whose uint8 forward equals the trained network's, bit for bit"""
    from tris_amd.irn_net import EdgeDisplacement
    c = cpu_steps
    tr = _trainer(filled, radius=c["radius"])
    tr.train_step(c["x"], c["label"].cuda())
    tr.fit_mean_shift([c["x"]])
    sd = tr.state_dict()
    assert all(not v.is_cuda for v in sd.values()) and set(sd) == set(filled)
    fresh = EdgeDisplacement()
    fresh.load_state_dict(sd)
    fresh.cuda()
    img = O.images()[0]
    e0, d0 = tr.net(img)
    e1, d1 = fresh(img)
    assert torch.equal(e0, e1) and torch.equal(d0, d1)
    assert not torch.equal(sd["fc_dp7.3.weight"], filled["fc_dp7.3.weight"])


def test_inference_is_unchanged_by_a_trainer(filled, arith):
    """forward_raw on a recorded image is bitwise equal before and after an IrnTrainer was constructed and discarded"""
    import gc
    from tris_amd.irn_train import IrnTrainer
    net = _net(filled)
    img = O.images()[0]
    before = net.forward_raw(img)
    tr = IrnTrainer(net, lr=T.LR, weight_decay=T.WEIGHT_DECAY, max_step=T.MAX_STEP)
    del tr
    gc.collect()
    net.load_state_dict(filled)
    after = net.forward_raw(img)
    for k in ("edge_out", "dp_out", "edge", "dp"):
        assert torch.equal(before[k], after[k]), k


def test_training_and_inference_run_the_same_heads(filled, arith):
    """the taps of one uint8 forward (37 x 53: the x2 / x4 branches overhang the crop), passed through IrnTrainer.heads, give
    the inference's own edge_out and dp_out bit for bit: with mean_shift.running_mean at zero the two modes are one computation
    (irn_net.run_heads).  Measured before the two forwards were merged (commit db53847): equal in both arithmetics."""
    from tris_amd.utils.synth import irn_image
    net = _net(filled)
    net.mean_shift.running_mean.zero_()
    raw = net.forward_raw(irn_image(37, 53, seed=3), taps=True)
    tr = _trainer(filled)
    with tr.scope(), torch.no_grad():
        edge_out, dp_out = tr.heads(raw["taps"])
    pairs = (("edge_out", edge_out[:, 0], raw["edge_out"]), ("dp_out", dp_out.permute(0, 2, 3, 1), raw["dp_out"]))
    for name, got, want in pairs:
        assert got.shape == want.shape
        print(f"[{arith}] {name}: largest |training - inference| {float((got - want).abs().max()):.3e}")
    for name, got, want in pairs:
        assert torch.equal(got, want), name
