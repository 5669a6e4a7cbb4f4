"""The row-normalisation kernel tests without a GPU: three float32 evaluations of every expression of tests/oracle_rownorm.py on the
CPU (left to right, pairwise, the kernel's own lanes / trips / butterfly) stay inside every bound on every input kind and shape of
tests/test_gpu_rownorm.py, no element exempt; every wrong restatement (oracle_rownorm.MUTATIONS) leaves a bound on at least one of
those cases; the float64 references agree with torch's float64 ops and autograd; and the block arithmetic of the LayerNorm backward
is restated exactly for both settings of LN_BWD_BLOCKS (compared with the ABI on the GPU)."""
import pytest
import torch
import torch.nn.functional as F

import oracle_rownorm as OR

ORDERS = ("ltr", "pairwise", "kernel")
_id = lambda c: "-".join("x".join(map(str, p)) if isinstance(p, tuple) else str(p) for p in c)
LN_CASES = [(k, s) for k in OR.LN_KINDS for s in OR.LN_SHAPES]
IN_CASES = [(k, s) for k in OR.IN_KINDS for s in OR.IN_SHAPES]
L2_CASES = [(k, s) for k in OR.L2_KINDS for s in OR.L2_SHAPES]
SM_CASES = [(k, s) for k in OR.SM_KINDS for s in OR.SM_SHAPES]


def _bad(got, ref, bound):
    """number of elements outside the bound (a NaN or an infinity is outside), and the largest err / bound"""
    e = (got.double().reshape(ref.shape) - ref).abs()
    out = ~(e <= bound)
    ratio = float(torch.nan_to_num(e / bound, nan=0.0, posinf=float("inf")).max()) if e.numel() else 0.0
    return int(out.sum()), ratio


def _inside(got, ref, bound, what):
    assert got.dtype == torch.float32 and got.numel() == ref.numel()
    n, ratio = _bad(got, ref, bound)
    assert n == 0, f"{what}: {n} elements outside the bound, err / bound up to {ratio:.3f}"


# ================================================================================================================ evaluations
def _ln_checks(kind, shape, order, mut=None, blocks=None, with_extra=True):
    """every (output, reference, bound) of one LayerNorm case under one float32 evaluation"""
    d = OR.inputs("ln", kind, shape)
    x, g, b, dy = d["x"], d["gamma"], d["beta"], d["dy"]
    y, mean, rstd = OR.ln_fwd_f32(x, g, b, OR.EPS, order, mut)
    (m_ref, r_ref), (b_m, b_r) = OR.ln_stats(x)
    out = [("mean", mean, m_ref, b_m), ("rstd", rstd, r_ref, b_r)]
    if torch.isfinite(mean).all() and torch.isfinite(rstd).all():
        out.append(("y | stats", y, *OR.ln_apply(x, mean, rstd, g, b)))
    out.append(("y composed", y, *OR.ln_composed(x, g, b)))
    sm, sr = m_ref.float(), r_ref.float()                                  # the saved statistics of the backward: the oracle's, rounded
    extra = d["extra"] if with_extra else None
    dx, dg, db = OR.ln_bwd_f32(dy, x, g, sm, sr, extra, order, blocks, mut)
    (dx_ref, dg_ref, db_ref), (b_dx, b_dg, b_db) = OR.ln_bwd(dy, x, g, sm, sr, extra, blocks)
    return out + [("dx", dx, dx_ref, b_dx), ("dgamma", dg, dg_ref, b_dg), ("dbeta", db, db_ref, b_db)]


def _in_checks(kind, shape, order, relu, mut=None):
    d = OR.inputs("in", kind, shape)
    x, g, b, dy = d["x"], d["gamma"], d["beta"], d["dy"]
    y, mean, is_ = OR.in_fwd_f32(x, g, b, OR.EPS, relu, order, mut)
    (m_ref, r_ref), (b_m, b_r) = OR.in_stats(x)
    out = [("mean", mean, m_ref, b_m), ("invstd", is_, r_ref, b_r)]
    if torch.isfinite(mean).all() and torch.isfinite(is_).all():
        out.append(("y | stats", y, *OR.in_apply(x, mean, is_, g, b, relu)))
    out.append(("y composed", y, *OR.in_composed(x, g, b, relu)))
    sm, sr = m_ref.float(), r_ref.float()
    mask = None
    if relu:                                                               # the saved Y of an unmutated forward with the saved statistics
        mask = OR.in_apply(x, sm, sr, g, b, True)[0] > 0
    dx, s1, s0 = OR.in_bwd_f32(dy, x, g, sm, sr, mask, order, mut)
    (dx_ref, s1_ref, s0_ref), (b_dx, b_s1, b_s0) = OR.in_bwd(dy, x, g, sm, sr, mask)
    return out + [("dx", dx, dx_ref, b_dx), ("dgamma_part", s1, s1_ref, b_s1), ("dbeta_part", s0, s0_ref, b_s0)]


def _l2_checks(kind, shape, order, mut=None):
    d = OR.inputs("l2", kind, shape)
    x, dy = d["x"], d["dy"]
    y, iv = OR.l2_fwd_f32(x, order, mut)
    out = [("inv_norm", iv, *OR.l2_stats(x)), ("y | inv_norm", y, *OR.l2_apply(x, iv))]
    iv_ref, _ = OR.l2_stats(x)
    ys, ivs = OR.l2_apply(x, iv_ref.float())[0].float(), iv_ref.float()      # the saved Y and inv_norm of the backward
    return out + [("dx", OR.l2_bwd_f32(dy, ys, ivs, order, mut), *OR.l2_bwd(dy, ys, ivs))]


def _sm_checks(kind, shape, scale, order, mut=None):
    x, dy = OR.sm_x(kind, shape, scale), OR.inputs("sm", kind, shape)["dy"]
    y_ref, b_y = OR.sm_fwd(x, scale)
    ys = y_ref.float()                                                     # the saved Y of the backward
    return [("y", OR.sm_fwd_f32(x, scale, order, mut), y_ref, b_y), ("dx", OR.sm_bwd_f32(dy, ys, scale, order, mut), *OR.sm_bwd(dy, ys, scale))]


def _all_inside(checks, tag):
    names = [c[0] for c in checks]
    assert "y | stats" in names or "y | inv_norm" in names or names == ["y", "dx"], "an output was left out"
    for name, got, ref, bound in checks:
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()) and bool((bound >= 0).all()), (tag, name)
        _inside(got, ref, bound, f"{tag} {name}")


@pytest.mark.parametrize("case", LN_CASES, ids=_id)
def test_layernorm_float32_evaluations_stay_inside_the_bounds(case):
    kind, shape = case
    for order in ORDERS:
        for blocks in OR.LN_BLOCKS:
            for with_extra in (False, True):
                _all_inside(_ln_checks(kind, shape, order, None, blocks, with_extra), f"[{order}, blocks {blocks}, extra {with_extra}]")


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", IN_CASES, ids=_id)
def test_instancenorm_float32_evaluations_stay_inside_the_bounds(case, relu):
    kind, shape = case
    for order in ORDERS:
        _all_inside(_in_checks(kind, shape, order, relu), f"[{order}]")


@pytest.mark.parametrize("case", L2_CASES, ids=_id)
def test_l2norm_float32_evaluations_stay_inside_the_bounds(case):
    kind, shape = case
    norm = OR.inputs("l2", kind, shape)["x"].double().norm(dim=1)
    assert bool((norm >= 2.0 ** -40 * (1 - 1e-6)).all()) and bool((norm <= 2.0 ** 40 * (1 + 1e-6)).all()), "outside the kernel's domain"
    for order in ORDERS:
        _all_inside(_l2_checks(kind, shape, order), f"[{order}]")


@pytest.mark.parametrize("case", SM_CASES, ids=_id)
def test_softmax_float32_evaluations_stay_inside_the_bounds(case):
    kind, shape = case
    for scale in OR.SM_SCALES:
        for order in ORDERS:
            _all_inside(_sm_checks(kind, shape, scale, order), f"[{order}, scale {scale}]")


# ================================================================================================================ mutations
# mutation -> the cases on which it has to leave a bound (at least one of them does; the test names which)
LN_CATCH = {
    "onepass_var": [("offset", (37, 512), {}), ("offset", (5, 100), {})],
    "unbiased_var": [("randn", (5, 1024), {}), ("randn", (5, 4), {})],
    "no_eps": [("const", (5, 100), {}), ("tiny", (5, 256), {})],
    "mean_over_padded_lanes": [("offset", (5, 100), {}), ("randn", (5, 260), {})],
    "bwd_no_c2": [("randn", (5, 256), {}), ("randn", (37, 512), {})],
    "bwd_c1_from_dy": [("dyoff", (5, 256), {}), ("randn", (37, 512), {})],
    "bwd_extra_dropped": [("randn", (5, 8), {"with_extra": True})],
    "dgamma_no_ragged_block": [("randn", (2049, 64), {}), ("randn", (5003, 8), {"blocks": 128})],
    "dgamma_wave0_only": [("randn", (37, 512), {}), ("randn", (5003, 8), {})],
}
IN_CATCH = {
    "unbiased_var": [("randn", (3, 100, 128), 0), ("randn", (2, 2, 1), 0)],
    "group3_dropped": [("randn", (2, 5, 65), 0)],
    "mask_from_x": [("randn", (3, 100, 128), 1), ("randn", (2, 5, 65), 1)],
    "bwd_no_s0": [("dyoff", (3, 100, 128), 0), ("randn", (2, 4, 64), 1)],
}
L2_CATCH = {"eps_under_root": [("scaled", (50, 512)), ("scaled", (5, 64))], "bwd_no_projection": [("randn", (5, 64)), ("randn", (50, 512))]}
SM_CATCH = {
    "scale_after_max": [("wide", (5, 100), OR.SM_SCALES[3]), ("late_max", (5, 130), OR.SM_SCALES[3])],
    "max_first_trip": [("late_max", (5, 65), OR.SM_SCALES[2]), ("late_max", (5, 1600), OR.SM_SCALES[0])],
    "bwd_no_scale": [("randn", (5, 20), OR.SM_SCALES[0]), ("randn", (21, 48), OR.SM_SCALES[3])],
    "bwd_s_first_trip": [("dyoff", (5, 130), OR.SM_SCALES[2]), ("randn", (5, 100), OR.SM_SCALES[2])],
}


def _caught(checks):
    return [name for name, got, ref, bound in checks if _bad(got, ref, bound)[0] > 0]


def test_the_mutation_tables_name_every_mutation_and_only_listed_cases():
    for tag, table in (("ln", LN_CATCH), ("in", IN_CATCH), ("l2", L2_CATCH), ("sm", SM_CATCH)):
        assert list(table) == OR.MUTATIONS[tag]
    assert all((k, s) in LN_CASES and opt.get("blocks") in OR.LN_BLOCKS for v in LN_CATCH.values() for k, s, opt in v)
    assert all((k, s) in IN_CASES for v in IN_CATCH.values() for k, s, _ in v)
    assert all((k, s) in L2_CASES for v in L2_CATCH.values() for k, s in v)
    assert all((k, s) in SM_CASES and sc in OR.SM_SCALES for v in SM_CATCH.values() for k, s, sc in v)


@pytest.mark.parametrize("mut", OR.MUTATIONS["ln"])
def test_layernorm_mutation_is_rejected(mut):
    for kind, shape, opt in LN_CATCH[mut]:
        assert _caught(_ln_checks(kind, shape, "kernel", None, **opt)) == [], "the unmutated kernel order leaves a bound"
        hit = _caught(_ln_checks(kind, shape, "kernel", mut, **opt))
        print(f"{mut} on {kind} {shape}: outside the bound of {hit}")
        assert hit, f"{mut} passes every bound on {kind} {shape}"


@pytest.mark.parametrize("mut", OR.MUTATIONS["in"])
def test_instancenorm_mutation_is_rejected(mut):
    for kind, shape, relu in IN_CATCH[mut]:
        assert _caught(_in_checks(kind, shape, "kernel", relu)) == []
        hit = _caught(_in_checks(kind, shape, "kernel", relu, mut))
        print(f"{mut} on {kind} {shape} relu {relu}: outside the bound of {hit}")
        assert hit, f"{mut} passes every bound on {kind} {shape}"
    gammas = [OR.inputs("in", k, s)["gamma"] for k, s in IN_CASES]
    assert all(bool((g < 0).any()) for g, (k, s) in zip(gammas, IN_CASES) if not (k == "gamma" and s[2] == 1))   # (there gamma[0] = 0)


@pytest.mark.parametrize("mut", OR.MUTATIONS["l2"])
def test_l2norm_mutation_is_rejected(mut):
    for kind, shape in L2_CATCH[mut]:
        assert _caught(_l2_checks(kind, shape, "kernel")) == []
        hit = _caught(_l2_checks(kind, shape, "kernel", mut))
        print(f"{mut} on {kind} {shape}: outside the bound of {hit}")
        assert hit, f"{mut} passes every bound on {kind} {shape}"


@pytest.mark.parametrize("mut", OR.MUTATIONS["sm"])
def test_softmax_mutation_is_rejected(mut):
    for kind, shape, scale in SM_CATCH[mut]:
        assert _caught(_sm_checks(kind, shape, scale, "kernel")) == []
        hit = _caught(_sm_checks(kind, shape, scale, "kernel", mut))
        print(f"{mut} on {kind} {shape} scale {scale}: outside the bound of {hit}")
        assert hit, f"{mut} passes every bound on {kind} {shape}"


# ================================================================================================================ references
def _close(a, b, scale):
    return float(((a - b).abs() / scale.clamp_min(1e-300)).max()) < 1e-11


def test_references_agree_with_float64_torch_and_autograd():
    for kind, shape in (("randn", (37, 512)), ("offset", (5, 100)), ("gamma", (5, 260))):
        d = OR.inputs("ln", kind, shape)
        x, g, b = (d[k].double().requires_grad_(True) for k in ("x", "gamma", "beta"))
        y = F.layer_norm(x, (shape[1],), g, b, OR.EPS)
        (y * d["dy"].double()).sum().backward()
        (mean, rstd), _ = OR.ln_stats(d["x"])
        y_ref, by = OR.ln_apply(d["x"], mean, rstd, d["gamma"], d["beta"])
        (dx, dg, db), (b_dx, b_dg, b_db) = OR.ln_bwd(d["dy"], d["x"], d["gamma"], mean, rstd)
        assert _close(y.detach(), y_ref, by / OR.U) and _close(x.grad, dx, b_dx / OR.U)
        assert _close(g.grad, dg, b_dg / OR.U) and _close(b.grad, db, b_db / OR.U)
        assert _close(OR.ln_composed(d["x"], d["gamma"], d["beta"])[0], y_ref, by / OR.U)
    for kind, shape, relu in (("randn", (3, 100, 128), 0), ("offset", (2, 5, 65), 1), ("gamma", (2, 4, 64), 1)):
        d = OR.inputs("in", kind, shape)
        x, g, b = (d[k].double().requires_grad_(True) for k in ("x", "gamma", "beta"))
        y = F.instance_norm(x.transpose(1, 2), None, None, g, b, True, 0.1, OR.EPS).transpose(1, 2)
        y = torch.relu(y) if relu else y
        (y * d["dy"].double()).sum().backward()
        (mean, is_), _ = OR.in_stats(d["x"])
        y_ref, by = OR.in_apply(d["x"], mean, is_, d["gamma"], d["beta"], relu)
        (dx, s1, s0), (b_dx, b_s1, b_s0) = OR.in_bwd(d["dy"], d["x"], d["gamma"], mean, is_, (y_ref > 0) if relu else None)
        assert _close(y.detach(), y_ref, by / OR.U) and _close(x.grad, dx, b_dx / OR.U)
        assert _close(g.grad, s1.sum(0), b_s1.sum(0) / OR.U) and _close(b.grad, s0.sum(0), b_s0.sum(0) / OR.U)
    d = OR.inputs("l2", "randn", (50, 512))
    x = d["x"].double().requires_grad_(True)
    y = x / x.norm(dim=-1, keepdim=True)
    (y * d["dy"].double()).sum().backward()
    inv, _ = OR.l2_stats(d["x"])
    y_ref, by = OR.l2_apply(d["x"], inv)
    dx, b_dx = OR.l2_bwd(d["dy"], y_ref, inv)
    assert _close(y.detach(), y_ref, by / OR.U) and _close(x.grad, dx, b_dx / OR.U)
    for scale in OR.SM_SCALES:
        xs = OR.sm_x("randn", (21, 48), scale)
        x = xs.double().requires_grad_(True)
        y = torch.softmax(x * scale, -1)
        dy = OR.inputs("sm", "randn", (21, 48))["dy"]
        (y * dy.double()).sum().backward()
        y_ref, by = OR.sm_fwd(xs, scale)
        dx, b_dx = OR.sm_bwd(dy, y_ref, scale)
        assert _close(y.detach(), y_ref, by / OR.U) and _close(x.grad, dx, b_dx / OR.U)


# ================================================================================================================ launch plans
def test_layernorm_backward_block_arithmetic_is_restated():
    """ln_bwd_rpb / the block count / the workspace of csrc/norm.hip for both settings of LN_BWD_BLOCKS, and which loops of the
    backward kernel each shape runs (tests/test_gpu_rownorm.py compares the same formulas with the ABI)"""
    want = {(37, None): (4, 10), (2049, None): (5, 410), (5003, None): (10, 501), (1, None): (4, 1), (2048, None): (4, 512),
            (37, 128): (8, 5), (2049, 128): (17, 121), (5003, 128): (40, 126), (1, 128): (8, 1), (1024, 128): (8, 128), (1025, 128): (9, 114)}
    for (rows, blocks), plan in want.items():
        assert OR.ln_bwd_plan(rows, blocks) == plan, (rows, blocks)
        assert OR.ln_bwd_workspace_bytes(rows, 64, blocks) == max(plan[1], 512) * 2 * 64 * 4
    seen = set()
    for rows, W in OR.LN_SHAPES:
        for blocks in OR.LN_BLOCKS:
            rpb, nb = OR.ln_bwd_plan(rows, blocks)
            last = rows - (nb - 1) * rpb
            if nb > 1 and last < rpb:
                seen.add("ragged last block")
            if last < 4:
                seen.add("a wave without a row")
            if rpb % 4 and rpb > 4:
                seen.add("waves with different row counts")
            if OR.cdiv(rpb, 4) >= 3:
                seen.add("three rows per wave")
            if nb > 256:
                seen.add("hundreds of blocks")
        seen.add(f"{OR.cdiv(W, 256)} trips")
        if (W // 4) % 64:
            seen.add("partial trip")
    assert seen == {"ragged last block", "a wave without a row", "waves with different row counts", "three rows per wave",
                    "hundreds of blocks", "1 trips", "2 trips", "3 trips", "4 trips", "partial trip"}, seen
