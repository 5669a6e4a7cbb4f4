"""tests/oracle_update.py checked on the CPU: the constructions of its cases (cosines on their intended side, the zero count, the
cancellation, the update below half an ulp), the scalars of the two AdamW entry points, float32 restatements of every kernel in
several evaluation orders inside the bounds on every named case, and every mutation outside them (or not finite) on at least one.
The grid-cap size of the optimiser kernels is a launch geometry, not an arithmetic path: it has no restatement here."""
import math

import pytest
import torch

import oracle_update as OU
from oracle_rownorm import U

FORMS = ("plain", "fma")
_id = lambda c: "-".join("x".join(map(str, p)) if isinstance(p, tuple) else str(p) for p in c)


def _out(got, ref, bound):
    """-> the number of elements outside the bound (a NaN or an infinity is outside)"""
    e = (got.double().reshape(ref.shape) - ref).abs()
    return int((~(e <= bound)).sum())


# =================================================================================================================== AdamW
def _adamw_outside(c, p, g, m, v, form, mut=None):
    P, M, V = OU.adamw_f32(p, g, m, v, c.h, form, mut)
    (mr, vr, dp), (b_m, b_v, b_dp) = OU.adamw_ref(p, g, m, v, c.h)
    (_, _, dp_g), (_, _, b_dp_g) = OU.adamw_ref(p, g, m, v, c.h, M, V)
    upd = P.double() - p.double()
    return {"m": _out(M, mr, b_m), "v": _out(V, vr, b_v), "dp": _out(upd, dp, b_dp), "dp | moments": _out(upd, dp_g, b_dp_g)}


@pytest.mark.parametrize("c", OU.ADAMW_CASES, ids=lambda c: c.id)
def test_adamw_restatements_inside(c):
    p, g, m, v = OU.adamw_inputs(c.stat, c.n, c.fresh)
    for form in FORMS:
        bad = _adamw_outside(c, p, g, m, v, form)
        assert not any(bad.values()), f"{c.id} {form}: outside {bad}"


@pytest.mark.parametrize("grp", OU.GROUPS)
def test_adamw_carried_steps_inside(grp):
    for form in FORMS:
        p, _, m, v = OU.adamw_inputs("randn", OU.N_STAT, True)
        for t in OU.STEPS_T:
            g = OU.adamw_inputs("randn", OU.N_STAT, True, seed=t)[1]
            c = OU.ACase(f"steps-{grp}-t{t}", "randn", OU.N_STAT, OU.hyper(grp, t), t == 1)
            bad = _adamw_outside(c, p, g, m, v, form)
            assert not any(bad.values()), f"{c.id} {form}: outside {bad}"
            p, m, v = OU.adamw_f32(p, g, m, v, c.h, form)


@pytest.mark.parametrize("mut", OU.MUTATIONS["adamw"])
def test_adamw_mutations_rejected(mut):
    hit = []
    for c in OU.ADAMW_CASES:
        p, g, m, v = OU.adamw_inputs(c.stat, c.n, c.fresh)
        bad = _adamw_outside(c, p, g, m, v, "plain", mut)
        if any(bad.values()):
            hit.append(c.id)
    print(f"{mut}: rejected on {hit}")
    assert hit, f"{mut} stays inside every bound on every case"


def test_adamw_no_decay_is_seen_by_the_decay_test_at_every_product():
    """one step's decay of the backbone group is below the roundings of |p|: the bitwise decay test is what sees it"""
    p = OU.adamw_inputs("randn", OU.N_STAT)[0]
    for lr, wd in OU.DECAY_ONLY:
        assert not torch.equal(OU.decay_only_ref(p, lr, wd), p)


def test_adamw_scalars_and_decay_factor():
    for grp in OU.GROUPS:
        for t in (1, 2, 1000):
            h = OU.hyper(grp, t)
            row = OU.hyper_row(h)
            bc1, bc2s = OU.adamw_scalars(h)
            assert (float(row[0]), float(row[1]), float(row[2])) == (h.lr, bc1, bc2s)
    one = OU.f32t(1.0)
    for lr, wd in OU.DECAY_ONLY:
        lr32, wd32 = OU.f32t(OU.f32_scalar(lr)), OU.f32t(OU.f32_scalar(wd))
        assert torch.equal(one - lr32 * wd32, OU.fma32(-lr32, wd32, one)), "the contracted decay factor is another float"
    lr32, wd32 = OU.f32t(OU.f32_scalar(5e-6)), OU.f32t(OU.f32_scalar(0.01))
    assert float(one - lr32 * wd32) == 1.0 - 2.0 ** -24
    assert math.isclose(2.0 ** -24 / (5e-6 * 0.01), 1.19, abs_tol=0.005)          # 19 % more decay than asked for


def test_adamw_constructions():
    n, h = OU.N_STAT, OU.hyper("backbone", OU.STAT_T)
    p, g, m, v = OU.adamw_inputs("zero_mix", n)
    assert int((g == 0).sum()) == len(range(OU.ZERO_AT, n, OU.ZERO_EVERY)) and int((v == 0).sum()) > 0
    p, g, m, v = OU.adamw_inputs("cancel", n)
    (mr, _, _), _ = OU.adamw_ref(p, g, m, v, h)
    assert bool((mr.abs() <= 4 * U * (h.b1 * m.double()).abs()).all()) and bool((mr != 0).any())
    p, g, m, v = OU.adamw_inputs("p_big", n)
    (_, _, dp), _ = OU.adamw_ref(p, g, m, v, h)
    assert bool((p.abs() == 1e3).all()) and bool(((dp + h.lr * h.wd * p.double()).abs() < 2.0 ** -15).all())
    p, g, m, v = OU.adamw_inputs("tiny", n)
    (_, vr, _), _ = OU.adamw_ref(p, g, m, v, h)
    assert float(torch.sqrt(vr).median()) < h.eps
    assert OU.N_GRID_CAP // 4 > 8192 * 256 and OU.N_GRID_CAP % 4 == 3


# ---------------------------------------------------------------------------------------------------------------- SGD
def _sgd_outside(n, hy, first, form, mut=None):
    p, g, buf, _ = OU.adamw_inputs("randn", n)
    P, M = OU.sgd_f32(p, g, buf, *hy, first, form, mut)
    (br, dp), (b_buf, b_dp) = OU.sgd_ref(p, g, buf, *hy, first)
    return _out(M, br, b_buf) + _out(P.double() - p.double(), dp, b_dp)


def test_sgd_restatements_inside_and_mutations_rejected():
    cases = [(n, hy, first) for n in OU.SIZES for hy in OU.SGD_HYPER for first in (0, 1)]
    for n, hy, first in cases:
        for form in FORMS:
            assert _sgd_outside(n, hy, first, form) == 0, (n, hy, first, form)
    for mut in OU.MUTATIONS["sgd"]:
        assert any(_sgd_outside(n, hy, first, "plain", mut) for n, hy, first in cases), f"{mut} stays inside every bound"


# =================================================================================================================== Stage-1 loss
def test_stage1_constructions():
    for stat, shape in OU.S1_CASES:
        OU.s1_check_construction(stat, OU.s1_inputs(stat, shape))      # (s1_inputs asserts it too, before anything uses the inputs)
    cp, _ = OU.s1_cosines(OU.s1_inputs("clamp", (6, 512, 3)))
    assert [not (OU.WIN_LO < c < OU.WIN_HI) for c in cp.tolist()] == [True, True, False, False, False, True]
    out = [b % 6 in (0, 1, 5) for b in range(6)]
    assert [not (OU.WIN_LO < c < OU.WIN_HI) for c in OU.CLAMP_COS] == out
    d = OU.s1_inputs("saturated", (6, 512, 3))["cls"]
    assert set(d.diagonal().tolist()) == set(OU.SAT_VALUES) and set(d.flatten().tolist()) == set(OU.SAT_VALUES)


@pytest.mark.parametrize("case", OU.S1_CASES, ids=_id)
def test_stage1_restatements_inside(case):
    stat, shape = case
    d = OU.s1_inputs(stat, shape)
    for up in OU.S1_UPS:
        ref, bnd = OU.s1_ref(d, up)
        for order, form in (("ltr", "plain"), ("kernel", "plain"), ("kernel", "fma")):
            got = OU.s1_f32(d, up, order=order, form=form)
            for k in ("losses", "dcls", "dfi"):
                assert _out(got[k], ref[k], bnd[k]) == 0, f"{stat} {shape} {up} {order} {form}: {k} outside"
            if not any(up):
                assert not bool(got["dcls"].any()) and not bool(got["dfi"].any()), "a zero upstream gradient must give exact zeros"


def test_stage1_clamp_rows_and_scale():
    """outside the window the fg contribution to dfi is exactly zero (K = 0: the whole row), inside it is not; the scale cases have
    the losses of `plain` and its dfi times the inverse scale"""
    d = OU.s1_inputs("clamp", (6, 512, 3))
    ref, _ = OU.s1_ref(d, OU.S1_UPS[1])
    zero = (ref["fg_mag"] == 0).all(1).tolist()
    assert zero == [True, True, False, False, False, True]
    got = OU.s1_f32(dict(d, fneg=None), OU.S1_UPS[1])["dfi"]
    assert [not bool(r.any()) for r in got] == zero
    for shape in OU.S1_SHAPES:
        base, _ = OU.s1_ref(OU.s1_inputs("plain", shape), OU.S1_UPS[1])
        for stat, sc in (("scale_lo", 1e-3), ("scale_hi", 1e3)):
            r, b = OU.s1_ref(OU.s1_inputs(stat, shape), OU.S1_UPS[1])
            assert _out(r["losses"], base["losses"], b["losses"]) == 0
            assert _out(r["dfi"] * sc, base["dfi"], b["dfi"] * sc) == 0


@pytest.mark.parametrize("mut", OU.MUTATIONS["s1"])
def test_stage1_mutations_rejected(mut):
    hit = []
    for stat, shape in OU.S1_CASES:
        if shape[0] > 6:
            continue
        d = OU.s1_inputs(stat, shape)
        ref, bnd = OU.s1_ref(d, OU.S1_UPS[1])
        got = OU.s1_f32(d, OU.S1_UPS[1], mut=mut)
        if any(_out(got[k], ref[k], bnd[k]) for k in ("losses", "dcls", "dfi")):
            hit.append((stat, shape))
    print(f"{mut}: rejected on {hit}")
    assert hit, f"{mut} stays inside every bound on every case"


# =================================================================================================================== bce4
def _bce_outside(case, up, form, mut=None):
    n, heads, tt, kind = case
    xs, t = OU.bce_inputs(n, tt, kind)
    (L, G), (bL, bG) = OU.bce4_ref(xs, t, up, heads)
    gotL, gotG = OU.bce4_f32(xs, t, up, heads, form, mut)
    return _out(gotL, L, bL) + sum(_out(gotG[k], G[k], bG[k]) for k in heads)


@pytest.mark.parametrize("case", OU.BCE_CASES, ids=_id)
def test_bce4_restatements_inside(case):
    for up in OU.BCE_UPS:
        for form in FORMS:
            assert _bce_outside(case, up, form) == 0, (case, up, form)


@pytest.mark.parametrize("mut", OU.MUTATIONS["bce4"])
def test_bce4_mutations_rejected(mut):
    hit = [c for c in OU.BCE_CASES if c[0] <= 2048 and _bce_outside(c, OU.BCE_UPS[1], "plain", mut)]
    print(f"{mut}: rejected on {len(hit)} cases, first {hit[:1]}")
    assert hit, f"{mut} stays inside every bound on every case"
