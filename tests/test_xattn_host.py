"""CPU checks of tests/oracle_xattn.py over exactly the case list of tests/test_gpu_xattn.py: the bounds hold for the restatements
of the kernels' arithmetic (a bound a restatement breaks is a wrong bound), the inputs are what their kinds say, every mutation
breaks the bound it is held against somewhere (a bound no defect can break checks nothing), and the bounds see what the old
whole-tensor yardstick cannot."""
import math

import pytest
import torch

import oracle_xattn as O

H2_PX = ("h2", "px", "h2")
X3_PX = ("x3", "px", "x3")
H2_CHAIN = ("x3", "chain", "h2")
COMBOS = O.FP32_CLASS + (H2_PX, H2_CHAIN)


def worst_of(kind, cases, restate, combo, mul=1.0, **kw):
    worst = {}
    for case in cases:
        x, ref = O.case_of(kind, case)
        got = restate(x, case, **kw)
        assert all(bool(torch.isfinite(t).all()) for t in got.values()), (kind, case)
        for name, r in O.ratios(got, ref, O.bound_of(kind, case, *combo, mul)).items():
            assert r <= 1.0, (kind, case, combo, name, r)
            worst[name] = max(worst.get(name, 0.0), r)
    return worst


@pytest.mark.parametrize("kind", O.KINDS)
def test_restatements_stay_within_the_bounds(kind):
    """torch's fp32 evaluation within the f32 bound, the six-of-nine piece products within the x3 bounds (both backward forms), the
    split4h operands within the h2 bounds -- pixel rows, chain, and amax words 64 times too large under the bound for that amax:
    every output, every element, every case"""
    w = {"fp32": worst_of(kind, O.CASES, O.restate_fp32, O.FP32_CLASS[0]),
         "x3 chain": worst_of(kind, O.CASES, O.restate_x3, O.FP32_CLASS[1]),
         "x3 px": worst_of(kind, O.PERSISTENT, O.restate_x3, X3_PX),
         "h2 px": worst_of(kind, O.PERSISTENT, O.restate_h2, H2_PX),
         "h2 px amax x 64": worst_of(kind, O.PERSISTENT, O.restate_h2, H2_PX, 64.0, amax_mul=64.0),
         "h2 chain": worst_of(kind, O.CASES, O.restate_h2, H2_CHAIN, chain=True)}
    for name, v in w.items():
        top = max(v, key=v.get)
        print(f"{kind}: {name} restatement worst err / bound {v[top]:.3f} ({top})")


def test_bounds_are_finite_and_positive_where_the_reference_is_not_zero():
    for kind in O.KINDS:
        for case in O.CASES:
            _, ref = O.case_of(kind, case)
            for combo in COMBOS:
                if combo[1] == "px" and case not in O.PERSISTENT:
                    continue
                bnd = O.bound_of(kind, case, *combo)
                for name in O.OUTPUTS:
                    b = bnd[name]
                    assert b.shape == ref[name].shape and b.dtype == torch.float64, (kind, case, combo, name)
                    assert bool(torch.isfinite(b).all()) and bool((b >= 0).all()), (kind, case, combo, name)
                    assert bool((b[ref[name] != 0] > 0).all()), (kind, case, combo, name)


def test_the_inputs_are_what_their_kinds_say():
    """late_max / early_max: the dominant logit exceeds 95 and leads every other by at least 30, in both soft-maxes; zero_rows: exact
    zeros in the reference with a zero bound in the f32 and x3 forms; tiny_sentences / tiny_image: the 2^-20 and 2^-12 ratios"""
    for case in O.CASES:
        B, P, N, C, _ = case
        sc = 1.0 / math.sqrt(C)
        for kind in ("late_max", "early_max"):
            x = {k: v.double() for k, v in O.inputs(kind, case).items()}
            assert all(0.7 < float(x[n].min()) and float(x[n].max()) < 1.3 for n in ("Qt", "Qv")), (kind, case)
            for logits, axis, n in (((x["Kv"] @ x["Qt"].t()) * sc, 1, P), ((x["Qv"] @ x["Kt"].t()) * sc, 2, N)):
                top = logits.topk(min(2, n), axis)
                assert bool((top.indices.select(axis, 0) == (n - 1 if kind == "late_max" else 0)).all()), (kind, case, axis)
                assert float(top.values.select(axis, 0).min()) > 95.0, (kind, case, axis, float(top.values.select(axis, 0).min()))
                if n > 1:
                    margin = top.values.select(axis, 0) - top.values.select(axis, 1)
                    assert float(margin.min()) >= 30.0, (kind, case, axis, float(margin.min()))
        x, ref = O.case_of("zero_rows", case)
        rows = O.zero_pixels(case)
        rng = O.cut(case)
        assert set(range(2, min(6, P))) <= set(rows) and (len(rng) < 2 or set(range(*rng[1])) <= set(rows))
        assert bool((x["d_vis"][:, rows] == 0).all()) and bool((x["d_lan"][:, 0] == 0).all())
        assert bool((x["d_vis"][:, [p for p in range(P) if p not in rows]] != 0).any())
        for combo in O.FP32_CLASS:
            if combo[1] == "px" and case not in O.PERSISTENT:
                continue
            bnd = O.bound_of("zero_rows", case, *combo)
            for name in ("dQv", "dS1"):
                assert bool((ref[name][:, rows] == 0).all()) and bool((bnd[name][:, rows] == 0).all()), (case, combo, name)
            assert bool((ref["dS2"][:, :, 0] == 0).all()) and bool((bnd["dS2"][:, :, 0] == 0).all()), (case, combo)
        x = O.inputs("tiny_sentences", case)
        for n in ("Qt", "Kt", "Vt"):
            small, rest = x[n][::3].abs().max(), x[n].abs().max()
            assert N < 2 or 2.0 ** -22 < float(small / rest) < 2.0 ** -18, (case, n)
        x = O.inputs("tiny_image", case)
        for n in ("Qv", "Kv", "Vv", "d_vis", "d_lan"):
            assert 2.0 ** -13.5 < float(x[n][1].abs().max() / x[n][0].abs().max()) < 2.0 ** -10.5, (case, n)
        if N == 1:
            _, ref = O.case_of("randn", case)
            assert bool((ref["Av"] == 1).all()) and bool((ref["dS1"] == 0).all())


@pytest.mark.parametrize("name", O.MUTATIONS)
def test_every_mutation_breaks_the_bound(name):
    """one defect in the fp64 path: some output exceeds its bound in some (kind, case).  The piece-dropping mutations are held
    against the bound of the arithmetic they belong to (h2 / x3 pixel rows), the others against the widest fp32-class bound"""
    found, tried = None, 0
    for kind in O.KINDS:
        for case in O.CASES:
            x, ref = O.case_of(kind, case)
            if name in O.H2_MUTATIONS + O.X3_MUTATIONS and case not in O.PERSISTENT:
                continue
            got = O.mutate(name, x, case)
            if got is None:
                continue
            tried += 1
            bnd = O.bound_of(kind, case, *H2_PX) if name in O.H2_MUTATIONS else O.bound_of(kind, case, *X3_PX) \
                if name in O.X3_MUTATIONS else O.widest_fp32(kind, case)
            r = O.ratios(got, ref, bnd)
            worst = max(r, key=r.get)
            if r[worst] > 1.0 and (found is None or r[worst] > found[1]):
                found = ((kind, case, worst), r[worst])
        if found is not None and name not in O.H2_MUTATIONS + O.X3_MUTATIONS:
            break
    assert found is not None, (name, tried)
    held = "h2" if name in O.H2_MUTATIONS else "x3" if name in O.X3_MUTATIONS else "widest fp32-class"
    print(f"{name}: exceeds the {held} bound at kind, case, output = {found[0]} by {found[1]:.3g}x")


def test_the_bound_sees_a_lost_image_that_the_old_yardstick_cannot():
    """tiny_image: dKv of image 1 replaced by zeros passes max |err| <= 5e-4 max(1, max |ref|) and fails every bound"""
    for case in O.CASES:
        _, ref = O.case_of("tiny_image", case)
        dKv = ref["dKv"].clone()
        dKv[1] = 0.0
        assert float(ref["dKv"][1].abs().max()) > 0
        assert O.old_yardstick_passes(dKv, ref["dKv"]), case
        for combo in COMBOS:
            if combo[1] == "px" and case not in O.PERSISTENT:
                continue
            r = O.ratios(dict(dKv=dKv), ref, O.bound_of("tiny_image", case, *combo))["dKv"]
            assert r > 1.0, (case, combo, r)


def test_the_bound_sees_a_dropped_low_piece_of_ds_that_the_old_yardstick_cannot():
    """randn: the h2 restatement without the low piece of dS (2^-11 of the operand) passes the old yardstick in all six gradients of
    every case and leaves the h2 bound (the mutation test finds it 238 times over on `peaked`)"""
    top = 0.0
    for case in O.PERSISTENT:
        x, ref = O.case_of("randn", case)
        got = O.restate_h2(x, case, drop="dS")
        for n in O.GRADS:
            assert O.old_yardstick_passes(got[n], ref[n]), (case, n)
        r = O.ratios({n: got[n] for n in O.GRADS}, ref, O.bound_of("randn", case, *H2_PX))
        print(f"{case}: low piece of dS dropped: err / bound " + " ".join(f"{n} {v:.3g}" for n, v in r.items()))
        top = max(top, max(r.values()))
    assert top > 1.0, top
