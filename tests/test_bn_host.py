"""The BatchNorm kernel tests without a GPU: the fp64 restatement of tests/oracle_bn.py agrees with float64 F.batch_norm and
autograd; three float32 evaluations of every expression on the CPU stay inside the derived bounds on every input kind and shape
of tests/test_gpu_bn.py; and the inputs satisfy what the mask checks of that module rely on (hardly any element closer to the
ReLU kink than the forward bound, except where that is the point)."""
import pytest
import torch
import torch.nn.functional as F

import oracle_bn as OB

U = OB.U
CASES = [(k, M, C) for k in OB.KINDS for (M, C) in OB.SHAPES]
_id = lambda c: f"{c[0]}-{c[1]}x{c[2]}"


def _inside(got, ref, bound, what):
    e = (got.double() - ref).abs()
    ratio = float((e / bound.clamp_min(1e-300)).max()) if e.numel() else 0.0
    assert bool((e <= bound).all()), f"{what}: err / bound up to {ratio:.3f}"
    return ratio


def _mask(d, M, C):
    """a mask as the device forward would leave it: the sign of the float64 value, arbitrary where that is within the bound"""
    mean, invstd = OB.stored_stats(*d["key"])
    z, _, _ = OB.apply(d["x"], mean, invstd, d["gamma"], d["beta"])
    return z > 0


def _case(kind, M, C):
    d = dict(OB.inputs(kind, M, C))
    d["key"] = (kind, M, C)
    return d


@pytest.mark.parametrize("case", [c for c in CASES if c[1] > 1], ids=_id)
def test_oracle_agrees_with_float64_batch_norm_and_autograd(case):
    kind, M, C = case
    d = _case(kind, M, C)
    x = d["x"].double().requires_grad_(True)
    gamma, beta = d["gamma"].double().requires_grad_(True), d["beta"].double().requires_grad_(True)
    r, dy = d["resid"].double(), d["dy"].double()
    rm, rv = d["rmean"].double().clone(), d["rvar"].double().clone()
    mom = OB.MOMENTA[0]
    y = F.batch_norm(x.t()[None], rm, rv, gamma, beta, True, mom, OB.EPS)[0].t()
    mean, var, invstd = OB.stats(d["x"])
    (rm_ref, rv_ref), _ = OB.running(d["x"], d["rmean"], d["rvar"], mom)
    mask = _mask(d, M, C)
    out = (y + r) * mask
    (out * dy).sum().backward()

    def rel(a, b, scale=None):
        scale = b.abs().amax(0, keepdim=True) if scale is None else scale
        return float(((a - b).abs() / scale.clamp_min(1e-300)).max())
    # (the scale of an output is its largest term, as in the bounds: the results themselves cancel)
    xs = (d["x"].double() - mean).abs().amax(0) * invstd
    z, _, by = OB.apply(d["x"], mean, invstd, d["gamma"], d["beta"], d["resid"])
    assert rel(y.detach() + r, z, by.amax(0, keepdim=True) / (OB.C_Y * U)) < 1e-12
    assert rel(rm, rm_ref, rm_ref.abs() + d["x"].double().abs().mean(0)) < 1e-12
    assert rel(rv, rv_ref, rv_ref.abs() + mean ** 2) < 1e-12
    (s0, s1), (_, b1), _ = OB.bwd_reduce(d["dy"], d["x"], mean, invstd, mask)
    gsum = (dy * mask).abs().sum(0)
    assert rel(beta.grad, s0, gsum) < 1e-12
    assert rel(gamma.grad, s1, b1 / (OB.C_S * U)) < 1e-12
    dx, bdx, _ = OB.bwd_apply(d["dy"], d["x"], mean, invstd, d["gamma"], s0, s1, 1.0 / M, mask)
    assert rel(x.grad, dx, (bdx / (OB.C_DX * U)).amax(0, keepdim=True) * (1.0 + xs)) < 1e-12


def _three_apply(x, mu, is_, g, b, r):
    d = x - mu
    yield (d * is_) * g + b + r                                              # left to right
    sc = is_ * g
    yield d * sc + b + r                                                     # scale folded first (the kernels' order)
    yield (d.double() * sc.double() + b.double()).float() + r               # ... with the multiply-add fused


def _three_dx(g, x, mu, is_, ga, a, b, ic):
    d = x - mu
    yield ga * is_ * (g - a * ic - d * is_ * b * ic)
    k1, k2, k3 = ga * is_, a * ic, is_ * b * ic
    yield k1 * (g - k2 - d * k3)
    yield k1 * ((g - k2).double() - d.double() * k3.double()).float()


def _three_dzx(g, x, mu, is_):
    d = x - mu
    yield (g * (d * is_)).double().sum(0).float()
    yield ((g * d) * is_).double().sum(0).float()
    yield (g.double() * (d * is_).double()).float().double().flip(0).sum(0).float()


def _three_sums(t):
    """one-pass float64 sums in three orders: pairwise, serial, 256-row partials"""
    t = t.double()
    yield t.sum(0)
    yield t.cumsum(0)[-1]
    yield torch.stack([c.sum(0) for c in t.split(256)]).flip(0).cumsum(0)[-1]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_float32_evaluations_stay_inside_the_bounds(case):
    kind, M, C = case
    d = _case(kind, M, C)
    x, dy, r, g, b = d["x"], d["dy"], d["resid"], d["gamma"], d["beta"]
    # statistics: the kernels' one-pass float64 form
    (mean, var, invstd), (b_mean, b_var, b_inv, _, _) = OB.stats_reference(kind, M, C)
    for s, ss in zip(_three_sums(x), _three_sums(x.double() ** 2)):
        m1 = s / M
        v1 = (ss / M - m1 * m1).clamp_min(0.0)
        _inside(m1.float(), mean, b_mean, "mean")
        _inside(v1.float(), var, b_var, "var")
        _inside((1.0 / torch.sqrt(v1 + OB.EPS)).float(), invstd, b_inv, "invstd")
        for mom in OB.MOMENTA:
            (rm_ref, rv_ref), (b_rm, b_rv) = OB.running(x, d["rmean"], d["rvar"], mom)
            m32 = torch.tensor(mom, dtype=torch.float32)
            unb = v1 * (M / (M - 1.0)) if M > 1 else v1
            _inside((1 - m32) * d["rmean"] + m32 * m1.float(), rm_ref, b_rm, "running_mean")
            _inside((1 - m32) * d["rvar"] + m32 * unb.float(), rv_ref, b_rv, "running_var")
    mu, is_ = OB.stored_stats(kind, M, C)
    z0 = torch.zeros(())
    for resid in (None, r):
        _, y_ref, by = OB.apply(x, mu, is_, g, b, resid, True)
        for y in _three_apply(x, mu, is_, g, b, z0 if resid is None else resid):
            _inside(torch.relu(y), y_ref, by, "y")
    mask = _mask(d, M, C)
    (s0, s1), (b0, b1), dz = OB.bwd_reduce(dy, x, mu, is_, mask)
    gm = dy * mask
    for v in _three_sums(gm):
        _inside(v.float(), s0, b0, "sum_dz")
    for v in _three_dzx(gm, x, mu, is_):
        _inside(v, s1, b1, "sum_dzx")
    a32, b32, ic = s0.float(), s1.float(), OB.f32_scalar(1.0 / M)
    dx_ref, bdx, _ = OB.bwd_apply(dy, x, mu, is_, g, a32, b32, ic, mask)
    for dx in _three_dx(gm, x, mu, is_, g, a32, b32, torch.tensor(ic, dtype=torch.float32)):
        _inside(dx, dx_ref, bdx, "dx")


@pytest.mark.parametrize("shape", OB.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", OB.KINDS)
def test_pooled_forms_stay_inside_the_bounds(kind, shape):
    B, H, W, C = shape
    d = OB.pool_inputs(kind, shape)
    x = d["x"].view(B, H, W, C)
    mu, is_ = OB.stored_stats(kind, B * H * W, C)
    yp_ref, byp = OB.apply_pool(x, mu, is_, d["gamma"], d["beta"])
    for y in _three_apply(x, mu, is_, d["gamma"], d["beta"], torch.zeros(())):
        a, b, c, e = OB.pool4(torch.relu(y))
        _inside(0.25 * (a + b + c + e), yp_ref, byp, "pooled y")
    g = OB.unpool(d["dyp"].view(B, H // 2, W // 2, C))
    assert torch.equal(g.double(), OB.unpool(d["dyp"].view(B, H // 2, W // 2, C).double()))   # the quarter is exact


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_hardly_any_element_sits_at_the_relu_kink(case):
    """the mask checks of tests/test_gpu_bn.py compare the device's sign with float64's wherever |z| exceeds the forward bound:
    that must be (nearly) everywhere"""
    kind, M, C = case
    d = _case(kind, M, C)
    mu, is_ = OB.stored_stats(kind, M, C)
    for resid in (None, d["resid"]):
        z, _, by = OB.apply(d["x"], mu, is_, d["gamma"], d["beta"], resid)
        share = float(((z.abs() <= by) & (by > 0)).double().mean())          # (a bound of zero: the device value is exact)
        assert share < 1e-4, share


def test_crossing_inputs_straddle_the_kink():
    for C in OB.CROSSING_WIDTHS:
        x, mean, invstd, gamma, beta = OB.crossing_inputs(C)
        assert x.shape == (OB.CROSSING_M, C) and bool((gamma != 0).all()) and bool((beta != 0).all())
        assert bool((gamma > 0).any()) and bool((gamma < 0).any())
        z, _, by = OB.apply(x, mean, invstd, gamma, beta)
        assert bool(((z > 0).any(0) & (z < 0).any(0)).all()), "a channel does not change sign over its 17 steps"
        assert float((z.abs() <= by).double().mean()) > 0.25, "the rows are not within the rounding error of the kink"
        xp = OB.crossing_pool_inputs(C)[0]
        zp, _, _ = OB.apply(xp, mean, invstd, gamma, beta)
        others = torch.stack(OB.pool4(zp)[1:])
        assert bool((others <= -4.9).all()) and torch.equal(OB.pool4(xp)[0].reshape(-1, C), x)


def test_shapes_reach_the_paths_they_are_named_for():
    """the launch plans of csrc/norm.hip (col_plan, bn_grid), restated: which loops of the kernels each shape runs"""
    def plan(M, C, target=512):
        cv = C // 4
        cvb = min(cv, 256)
        rs = 256 // cvb
        rpb = max(-(-M // target), rs * 8)
        rpb = -(-rpb // rs) * rs
        return cv, cvb, rs, rpb, -(-M // rpb)
    seen = set()
    for M, C in OB.SHAPES:
        cv, cvb, rs, rpb, nb = plan(M, C)
        if cvb * rs < 256:
            seen.add("idle lanes")
        if cv > 256 and cv % 256:
            seen.add("partial second trip")
        if cv > 256:
            seen.add("second trip")
        if nb > 1 and M % rpb:
            seen.add("ragged last block")
        if nb > 256:
            seen.add("hundreds of blocks")
        if rpb >= 4 * rs and (rpb // rs) % 4:
            seen.add("4-row loop with a tail")
        if -(-(M * cv) // 256) > 4096:
            seen.add("grid cap")
        if (M * cv) > 2 * 4096 * 256 and (M * cv) % (2 * 4096 * 256):
            seen.add("two vectors per trip with a tail")
    assert seen == {"idle lanes", "partial second trip", "second trip", "ragged last block", "hundreds of blocks", "4-row loop with a tail",
                    "grid cap", "two vectors per trip with a tail"}, seen
    for rows in OB.FIN_ROWS:
        part, M = OB.partial_rows(rows, 4)
        assert part.shape == (rows, 2, 4) and M == rows * 128
    assert max(OB.FIN_ROWS) > 2048 > 513                      # both block sizes of the finalizers


# ================================================================================================== hand-offs (tris_amd.ops, no launch)
def test_carry_hands_over_the_riders_and_nothing_else():
    from tris_amd import ops
    assert set(ops.RIDERS) == {"_bn_link", "_bn_lazy", "_pl", "_h2"}
    src, dst = torch.zeros(3), torch.zeros(3)
    for k, name in enumerate(ops.RIDERS):
        setattr(src, name, ("rider", k))
    src._bn_part, src._act_link, src._other = ("part", 1), object(), 5
    assert ops.carry(src, dst) is dst
    assert {k: v for k, v in vars(dst).items()} == {name: ("rider", k) for k, name in enumerate(ops.RIDERS)}
    bare = torch.zeros(3)
    assert vars(ops.carry(torch.zeros(3), bare)) == {}          # a rider the source does not have is not set (to None) either


def test_carry_refuses_the_stand_in_of_a_paired_shortcut():
    from tris_amd import ops
    src, dst = torch.zeros(1).expand(2, 3), torch.zeros(2, 3)
    src._pl = ("tag",)
    src._bn_pair = ops._BnPair(*(torch.zeros(3) for _ in range(5)), 1234, ops._BnPairState(True, (True, True, True)))
    with pytest.raises(RuntimeError, match="bn3"):
        ops.carry(src, dst)
    assert vars(dst) == {}


def test_bwd_link_is_taken_once_and_only_by_the_tensor_that_filled_it():
    from tris_amd import ops
    stat = [torch.zeros(4) for _ in range(5)]
    dz, part, part2 = torch.ones(2, 4), torch.zeros(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64)
    link = ops._BnBwdLink(*stat, False)
    assert link.take(dz) is None                                # never filled
    link.fill(dz, part, 1, 77, part2)
    got = link.take(dz)
    assert isinstance(got, ops._BnTaken) and got._fields == ("part", "rows", "dzw", "part2")
    assert got.part is part and got.rows == 1 and got.dzw == 77 and got.part2 is part2 and tuple(got) == (part, 1, 77, part2)
    assert link.take(dz) is None                                # one use
    link.fill(dz, part, 1)
    got = link.take(dz)
    assert got.dzw is None and got.part2 is None
    link.fill(dz, part, 1)
    dz.add_(1.0)                                                # autograd accumulated a second consumer's gradient into it
    assert link.take(dz) is None
    link.fill(dz, part, 1)
    assert link.take(dz.clone()) is None                        # another tensor arrives
    assert link.take(dz) is None                                # ... and that use emptied the link
    link.fill(dz, part, 1)
    assert link.take(dz.view(4, 2)) is None                     # the same storage under another shape
