"""The kernels that turn activations into a loss gradient and a gradient into new weights, on the MI355X, against the fp64 restatement
of tests/oracle_update.py: AdamW through both entry points (tris_adamw_f32, tris_adamw_dev_f32) and through FusedAdamW, SGD with
momentum, the Stage-1 loss and the four-head BCE, forward and backward.  Every output finite and inside the element-wise bound
derived there on every named case; for the optimisers what is compared is the UPDATE p' - p, never p' against |p|; the decay by
itself, the graph path against the host path, one launch against three sub-range launches and the sigmoid at saturated logits are
bit for bit.  The ratios err / bound measured on the MI355X are in profiles/update_parity_floor.txt
(`python tests/test_gpu_update.py` prints that table).
"""
import pytest
import torch

import oracle_update as OU

pytestmark = pytest.mark.gpu

NAN = float("nan")
_id = lambda c: "-".join("x".join(map(str, p)) if isinstance(p, tuple) else str(p) for p in c)

REC = {}            # (kernel, output, case) -> largest err / bound
ASSERT = True       # (the profile mode records without asserting)


def _inside(got, ref, bound, key):
    """on the device of `ref` (the grid-cap references live on the GPU)"""
    got = got.detach().to(ref.device).double().reshape(ref.shape)
    e = (got - ref).abs()
    over = ~(e <= bound)                                                                # (a NaN is outside)
    ratio = float(torch.nan_to_num(e / bound, nan=0.0, posinf=float("inf")).max())     # (0 / 0: an exact output of an exact bound)
    REC[key] = max(REC.get(key, 0.0), ratio)
    print(f"{key}: err / bound up to {ratio:.3f}")
    if ASSERT:
        assert bool(torch.isfinite(got).all()), f"{key}: {int((~torch.isfinite(got)).sum())} elements not finite"
        assert not bool(over.any()), f"{key}: {int(over.sum())} elements outside the bound, err / bound up to {ratio:.3f}"


def _lib():
    from tris_amd import _lib as L
    from tris_amd import ops
    return ops, L


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# =================================================================================================================== AdamW
def _adamw(p, g, m, v, h, dev=False, lo=0, hi=None):
    """one launch on copies of p, m, v (elements [lo, hi) by pointer offset) -> p', m', v'"""
    ops, L = _lib()
    p, m, v = p.clone(), m.clone(), v.clone()
    hi = p.numel() if hi is None else hi
    o, st = 4 * lo, ops._stream()
    if dev:
        row = OU.hyper_row(h).cuda()
        L.call("tris_adamw_dev_f32", p.data_ptr() + o, g.data_ptr() + o, m.data_ptr() + o, v.data_ptr() + o, hi - lo, row.data_ptr(),
               h.b1, h.b2, h.eps, h.wd, st)
        torch.cuda.synchronize()
    else:
        L.call("tris_adamw_f32", p.data_ptr() + o, g.data_ptr() + o, m.data_ptr() + o, v.data_ptr() + o, hi - lo, h.lr, h.b1, h.b2,
               h.eps, h.wd, h.t, st)
    return p, m, v


def _adamw_check(p, g, m, v, h, out, name):
    """out = (p', m', v') of the device, against the float64 step of (p, g, m, v): the moments, the update given the stored moments
    and the update of the pure float64 step"""
    P, M, V = out
    (mr, vr, dp), (b_m, b_v, b_dp) = OU.adamw_ref(p, g, m, v, h)
    (_, _, dp_g), (_, _, b_dp_g) = OU.adamw_ref(p, g, m, v, h, M.to(p.device), V.to(p.device))
    upd = P.to(p.device).double() - p.double()
    _inside(M, mr, b_m, ("adamw", "m", name))
    _inside(V, vr, b_v, ("adamw", "v", name))
    _inside(upd, dp_g, b_dp_g, ("adamw", "dp | moments", name))
    _inside(upd, dp, b_dp, ("adamw", "dp", name))


@pytest.mark.parametrize("c", OU.ADAMW_CASES, ids=lambda c: c.id)
def test_adamw_case(c):
    """both entry points on every named case: the host path inside the bounds and repeatable, the graph path bit for bit the same"""
    host = OU.adamw_inputs(c.stat, c.n, c.fresh)
    p, g, m, v = (t.cuda() for t in host)
    out = _adamw(p, g, m, v, c.h)
    for a, b in zip(out, _adamw(p, g, m, v, c.h)):
        assert _bits_equal(a, b), "two launches on the same input differ"
    _adamw_check(*host, c.h, out, c.id)
    for name, a, b in zip(("p", "m", "v"), out, _adamw(p, g, m, v, c.h, dev=True)):
        assert _bits_equal(a, b), f"tris_adamw_dev_f32 differs from tris_adamw_f32 in {name}'"


@pytest.mark.parametrize("grp", OU.GROUPS)
def test_adamw_carried_steps(grp):
    """t = 1 .. 5, a fresh gradient each step, the device's own state carried over; every step against float64 from that state"""
    p, _, m, v = (t.cuda() for t in OU.adamw_inputs("randn", OU.N_STAT, True))
    for t in OU.STEPS_T:
        g = OU.adamw_inputs("randn", OU.N_STAT, True, seed=t)[1]
        h = OU.hyper(grp, t)
        out = _adamw(p, g.cuda(), m, v, h)
        _adamw_check(p.cpu(), g, m.cpu(), v.cpu(), h, out, f"steps-{grp}-t{t}")
        p, m, v = out


@pytest.mark.parametrize("lr,wd", OU.DECAY_ONLY, ids=str)
@pytest.mark.parametrize("dev", [False, True], ids=["host", "graph"])
def test_adamw_decay_by_itself(lr, wd, dev):
    """g = m = v = 0: p' = fl(p fl(1 - fl(lr wd))) bit for bit and the moments stay zero.  (At lr wd = 5e-8 the factor rounds to
    1 - 2^-24: 19 % more decay than asked for, as torch's float32 mul_ has it: the reason the update bound carries a U |p| term.)"""
    p = OU.adamw_inputs("randn", OU.N_STAT)[0]
    z = torch.zeros(OU.N_STAT, device="cuda")
    P, M, V = _adamw(p.cuda(), z, z, z, OU.hyper("heads", 3, lr=lr, wd=wd), dev=dev)
    assert _bits_equal(P.cpu(), OU.decay_only_ref(p, lr, wd)), "p' is not fl(p fl(1 - fl(lr wd)))"
    assert not bool(M.any()) and not bool(V.any()), "a moment left zero"


@pytest.mark.parametrize("grp", OU.GROUPS)
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_adamw_graph_path_scalars_and_values(grp, t):
    """the row FusedAdamW.push_hyper writes is the row tests/oracle_update.py restates, and with it tris_adamw_dev_f32 is
    tris_adamw_f32 bit for bit"""
    from tris_amd.optim import FusedAdamW
    h = OU.hyper(grp, t)
    w = torch.nn.Parameter(torch.zeros(8, device="cuda"))
    opt = FusedAdamW([w], lr=h.lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    opt.enable_device_hyper()
    opt.push_hyper(t)
    torch.cuda.synchronize()
    assert _bits_equal(opt._hyper[0].cpu(), OU.hyper_row(h)), f"push_hyper wrote {opt._hyper[0].tolist()}, expected {OU.hyper_row(h).tolist()}"
    p, g, m, v = (x.cuda() for x in OU.adamw_inputs("randn", OU.N_STAT, t == 1))
    for name, a, b in zip(("p", "m", "v"), _adamw(p, g, m, v, h), _adamw(p, g, m, v, h, dev=True)):
        assert _bits_equal(a, b), f"tris_adamw_dev_f32 differs from tris_adamw_f32 in {name}' at t = {t}"


@pytest.mark.parametrize("dev", [False, True], ids=["host", "graph"])
def test_adamw_sub_ranges_are_one_launch(dev):
    """one arena of 64 x 37 floats in a single launch, and as three launches by pointer offset (FusedAdamW.step(ranges=..)): bitwise"""
    h = OU.hyper("backbone", 4)
    p, g, m, v = (t.cuda() for t in OU.adamw_inputs("randn", OU.ARENA))
    whole = _adamw(p, g, m, v, h, dev=dev)
    _adamw_check(*OU.adamw_inputs("randn", OU.ARENA), h, whole, "arena")
    cur = (p, m, v)
    for lo, hi in OU.RANGES:
        cur = _adamw(cur[0], g, cur[1], cur[2], h, dev=dev, lo=lo, hi=hi)
    for name, a, b in zip(("p", "m", "v"), whole, cur):
        assert _bits_equal(a, b), f"three sub-range launches differ from one launch in {name}'"


def _cuda_randn(n, seed):
    return torch.randn(n, device="cuda", generator=torch.Generator("cuda").manual_seed(seed))


def test_adamw_past_the_grid_cap():
    """n just past 8192 blocks x 256 threads x 4: the grid-stride loop's second trip and the scalar tail; N(0, 1), the float64
    reference vectorised on the device"""
    n, h = OU.N_GRID_CAP, OU.hyper("heads", 3)
    p, g, m = _cuda_randn(n, 1), _cuda_randn(n, 2), 0.1 * _cuda_randn(n, 3)
    v = 0.01 * _cuda_randn(n, 4) ** 2
    _adamw_check(p, g, m, v, h, _adamw(p, g, m, v, h), "grid-cap")


def test_fused_adamw_five_steps():
    """three parameters whose sizes leave padding (231, 5, and 64 x 16 x 3 x 3 channels-last) through FusedAdamW: five steps, each
    against a float64 AdamW step of the arenas as they stood; the padding of all four arenas still exactly zero; the state_dict()
    moments inside the moment bounds"""
    from tris_amd.optim import Arena, FusedAdamW
    gen = torch.Generator().manual_seed(77)
    init = [torch.randn(*s, generator=gen) for s in OU.FUSED_SHAPES]
    init[2] = init[2].contiguous(memory_format=torch.channels_last)
    ps = [torch.nn.Parameter(t.cuda()) for t in init]
    opt = FusedAdamW([{"params": [ps[0], ps[2]], "lr": 5e-6}, {"params": [ps[1]]}], lr=5e-5, weight_decay=0.01)
    pad = []
    for a in opt.arenas:
        live = torch.zeros(a.numel, dtype=torch.bool)
        for q, o in zip(a.params, a.offsets):
            live[o:o + q.numel()] = True
        assert not bool(live.all()), "this arena has no padding"
        pad.append(~live)
    last = None
    for t in OU.STEPS_T:
        for q in ps:
            q.grad.copy_(torch.randn(q.shape, generator=gen).cuda())
        before = [(a.p.cpu(), a.g.cpu(), a.m.cpu(), a.v.cpu()) for a in opt.arenas]
        opt.step()
        last = []
        for gi, (grp, a, b) in enumerate(zip(opt.param_groups, opt.arenas, before)):
            h = OU.hyper(("backbone", "heads")[gi], t, lr=grp["lr"], wd=grp["weight_decay"])
            assert (h.b1, h.b2, h.eps) == tuple(OU.f32_scalar(x) for x in (*grp["betas"], grp["eps"]))
            _adamw_check(*b, h, (a.p, a.m, a.v), f"fused-group{gi}-t{t}")
            for name, arena in zip("pgmv", (a.p, a.g, a.m, a.v)):
                assert not bool(arena.cpu()[pad[gi]].any()), f"step {t}: the padding of arena {name} of group {gi} is not zero"
            last.append((OU.adamw_ref(*b, h), a))
    sd = opt.state_dict()["state"]
    order = [(0, ps[0]), (0, ps[2]), (1, ps[1])]           # state indices run over the groups' parameters in order
    for idx, (gi, q) in enumerate(order):
        ((mr, vr, _), (b_m, b_v, _)), a = last[gi]
        o = a.offsets[[id(x) for x in a.params].index(id(q))]
        assert float(sd[idx]["step"]) == len(OU.STEPS_T)
        for name, got, ref, bound in (("exp_avg", sd[idx]["exp_avg"], mr, b_m), ("exp_avg_sq", sd[idx]["exp_avg_sq"], vr, b_v)):
            _inside(got, Arena._view(ref, q, o).contiguous(), Arena._view(bound, q, o).contiguous(), ("adamw", f"state_dict {name}", f"param{idx}"))


# ---------------------------------------------------------------------------------------------------------------- SGD
def _sgd(p, g, buf, hy, first):
    ops, L = _lib()
    p, buf = p.clone(), buf.clone()
    L.call("tris_sgd_momentum_f32", p.data_ptr(), g.data_ptr(), buf.data_ptr(), p.numel(), *hy, first, ops._stream())
    return p, buf


def _sgd_check(p, g, buf, hy, first, out, name):
    (br, dp), (b_buf, b_dp) = OU.sgd_ref(p, g, buf, *hy, first)
    _inside(out[1], br, b_buf, ("sgd", "buf", name))
    _inside(out[0].to(p.device).double() - p.double(), dp, b_dp, ("sgd", "dp", name))


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("n", OU.SIZES)
def test_sgd_sizes(n, first):
    """with `first` the buffer is written, not read: it goes in as NaN"""
    p, g, buf, _ = OU.adamw_inputs("randn", n)
    for hy in OU.SGD_HYPER:
        dbuf = torch.full((n,), NAN, device="cuda") if first else buf.cuda()
        _sgd_check(p, g, buf, hy, first, _sgd(p.cuda(), g.cuda(), dbuf, hy, first), f"n{n}-first{first}")


@pytest.mark.parametrize("first", [0, 1])
def test_sgd_past_the_grid_cap(first):
    n, hy = OU.N_GRID_CAP, OU.SGD_HYPER[0]
    p, g, buf = _cuda_randn(n, 5), _cuda_randn(n, 6), _cuda_randn(n, 7)
    _sgd_check(p, g, buf, hy, first, _sgd(p, g, buf, hy, first), f"grid-cap-first{first}")


# =================================================================================================================== Stage-1 loss
def _s1(d, up, with_neg=True):
    """ops.stage1_loss forward and backward under the upstream gradient `up` -> losses, dcls, dfi"""
    ops, _ = _lib()
    cls, fi = d["cls"].cuda().requires_grad_(True), d["fi"].cuda().requires_grad_(True)
    fneg = d["fneg"].cuda() if with_neg and d["fneg"] is not None else None
    out = ops.stage1_loss(cls, fi, d["ft"].cuda(), fneg, *OU.S1_W)
    (out * torch.tensor(up, device="cuda")).sum().backward()
    return out.detach(), cls.grad, fi.grad


@pytest.mark.parametrize("case", OU.S1_CASES, ids=_id)
def test_stage1_loss(case):
    stat, shape = case
    d = OU.s1_inputs(stat, shape)
    for up in OU.S1_UPS:
        losses, dcls, dfi = _s1(d, up)
        if not any(up):
            assert not bool(dcls.any()) and not bool(dfi.any()), "a zero upstream gradient must give exact zeros"
        ref, bnd = OU.s1_ref(d, up)
        for k, got in (("losses", losses), ("dcls", dcls), ("dfi", dfi)):
            _inside(got, ref[k], bnd[k], ("stage1_loss", k, f"{stat}-{_id([shape])}"))


@pytest.mark.parametrize("shape", [s for s in OU.S1_SHAPES if s[0] >= 2], ids=str)
def test_stage1_loss_clamp_window(shape):
    """rows whose cosine is outside [1e-4, 0.9999] have an exactly zero fg contribution to dfi: with dL/dl1 = g0 w1 + g1 = 0 in place
    of 1 they do not change by a bit, the rows inside do; without negatives the rows outside are exactly zero"""
    d = OU.s1_inputs("clamp", shape)
    outside = [b % 6 in (0, 1, 5) for b in range(shape[0])]
    _, _, with_fg = _s1(d, (1.0, 0.0, 0.0, 0.0))
    _, _, without = _s1(d, (1.0, -1.0, 0.0, 0.0))
    _, _, alone = _s1(d, (1.0, 0.0, 0.0, 0.0), with_neg=False)
    for b, out in enumerate(outside):
        assert torch.equal(with_fg[b], without[b]) == out, f"row {b} (cos {OU.CLAMP_COS[b % 6]}): fg contribution {'not ' if out else ''}zero"
        assert (not bool(alone[b].any())) == out, f"row {b} (cos {OU.CLAMP_COS[b % 6]}) without negatives"


# =================================================================================================================== bce4
def _bce4(xs, t, up, heads, grads_for=None):
    """the two ABI calls; absent heads go in as NULL with a NaN-filled gradient buffer -> losses, [d1 .. d4]"""
    ops, L = _lib()
    n, st = t.numel(), ops._stream()
    X = [xs[k].cuda() if k in heads else None for k in range(4)]
    T = t.cuda()
    kind = int(T.dtype == torch.float32)
    losses = torch.full((5,), NAN, device="cuda")
    ws = torch.empty(L.query("tris_bce4_workspace_bytes", n) // 8, dtype=torch.float64, device="cuda")
    L.call("tris_bce4_fwd_f32", *[ops.P(x) for x in X], ops.P(T), kind, n, ops.P(losses), ops.P(ws), st)
    D = [torch.full((n,), NAN, device="cuda") for _ in range(4)]
    G = torch.tensor(up, device="cuda")
    L.call("tris_bce4_bwd_f32", *[ops.P(x) for x in X], ops.P(T), kind, ops.P(G), *[ops.P(x) for x in D], n, st)
    torch.cuda.synchronize()
    return losses, D


@pytest.mark.parametrize("case", OU.BCE_CASES, ids=_id)
def test_bce4(case):
    n, heads, tt, kind = case
    xs, t = OU.bce_inputs(n, tt, kind)
    name = f"{kind}-{tt}-n{n}-heads{len(heads)}"
    for up in OU.BCE_UPS:
        losses, D = _bce4(xs, t, up, heads)
        (L, G), (bL, bG) = OU.bce4_ref(xs, t, up, heads)
        _inside(losses, L, bL, ("bce4", "losses", name))
        for k in range(4):
            if k in heads:
                _inside(D[k], G[k], bG[k], ("bce4", "dx", name))
            else:
                assert float(losses[1 + k]) == 0.0, f"absent head {k + 1} has a loss"
                assert bool(torch.isnan(D[k]).all()), f"the gradient buffer of absent head {k + 1} was written"
        if kind != "randn3":          # sigmoid exactly 1 at x >= 40 and exactly 0 at x = -200: dX = fl((1 - t) gk), fl((0 - t) gk)
            tf, g = t.float(), [OU.f32t(OU.f32_scalar(u)) for u in up]
            for k in heads:
                gk = (g[0] + g[1 + k]) / OU.f32t(float(n))
                got, x = D[k].cpu(), xs[k]
                assert _bits_equal(got[x > 0], ((1.0 - tf) * gk)[x > 0]), "sigmoid is not exactly 1 at a saturated positive logit"
                if kind == "pm200":
                    assert _bits_equal(got[x < 0], ((0.0 - tf) * gk)[x < 0]), "sigmoid is not exactly 0 at x = -200"


def test_bce4_wrapper_is_the_abi_calls():
    ops, _ = _lib()
    n, heads, tt, kind = 257, (0, 1), "i64", "randn3"
    xs, t = OU.bce_inputs(n, tt, kind)
    up = OU.BCE_UPS[1]
    losses, D = _bce4(xs, t, up, heads)
    X = [xs[k].cuda().requires_grad_(True) if k in heads else None for k in range(4)]
    out = ops.bce4(X, t.cuda())
    (out * torch.tensor(up, device="cuda")).sum().backward()
    assert _bits_equal(out.detach(), losses)
    for k in heads:
        assert _bits_equal(X[k].grad, D[k])


if __name__ == "__main__":
    # `python tests/test_gpu_update.py` on the MI355X prints the table of profiles/update_parity_floor.txt
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ASSERT = False
    out, sys.stdout = sys.stdout, open(os.devnull, "w")
    for c in OU.ADAMW_CASES:
        test_adamw_case(c)
    for grp in OU.GROUPS:
        test_adamw_carried_steps(grp)
    test_adamw_past_the_grid_cap()
    test_fused_adamw_five_steps()
    for first in (0, 1):
        for n in OU.SIZES:
            test_sgd_sizes(n, first)
        test_sgd_past_the_grid_cap(first)
    for c in OU.S1_CASES:
        test_stage1_loss(c)
    for c in OU.BCE_CASES:
        test_bce4(c)
    sys.stdout = out
    print("# Losses and optimiser updates against fp64 (csrc/optim.hip AdamW, SGD; csrc/heads.hip Stage-1 loss; csrc/seg.hip bce4): the")
    print("# largest err / bound per kernel, output and case of tests/oracle_update.py, MI355X.  The bounds are the element-wise ones")
    print("# derived there; tests/test_gpu_update.py asserts ratio <= 1.")
    print("# kernel | output | err / bound (largest over the cases) | at case")
    worst = {}
    for (kernel, output, case), ratio in REC.items():
        if (kernel, output) not in worst or ratio > worst[(kernel, output)][0]:
            worst[(kernel, output)] = (ratio, case)
    for (kernel, output), (ratio, case) in worst.items():
        print(f"{kernel:12s} | {output:22s} | {ratio:.3f}{'  EXCEEDS' if ratio > 1 else ''} | {case}")
    print("# every case:")
    for (kernel, output, case), ratio in REC.items():
        print(f"#   {kernel:12s} {output:22s} {case:40s} {ratio:.3f}")
