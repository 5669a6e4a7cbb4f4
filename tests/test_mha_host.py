"""CPU checks of tests/oracle_mha.py over exactly the case list of tests/test_gpu_mha.py: the bounds hold for three restatements of
the kernels' arithmetic (a bound the plain reference breaks is a wrong bound), every mutation breaks them somewhere (a bound no
defect can break checks nothing), and the bounds see what the old whole-tensor yardstick cannot."""
import pytest
import torch

import oracle_mha as O


def worst_of(kind, restate, form, **kw):
    worst = {}
    for L, heads, causal in O.CASES:
        qkv, dout, ref, bnd = O.case(kind, L, heads, causal)
        got = restate(qkv, dout, heads, causal, **kw)
        for name, r in O.ratios(got, ref, bnd[form]).items():
            assert r <= 1.0, (kind, L, heads, causal, name, r)
            worst[name] = max(worst.get(name, 0.0), r)
        assert all(bool(torch.isfinite(t).all()) for t in got.values()), (kind, L, heads, causal)
    return worst


@pytest.mark.parametrize("kind", O.KINDS)
def test_fp32_restatements_stay_within_the_bounds(kind):
    """torch's plain fp32 evaluation within the tightest form ("valu": no rescale term) and the flash walk in fp32 within "f32":
    every output, every element, every case"""
    plain = worst_of(kind, O.restate_fp32, "valu")
    flash = worst_of(kind, O.restate_flash_fp32, "f32")
    print(f"{kind}: plain fp32 worst err / bound {max(plain.values()):.3f} {plain}; flash fp32 {max(flash.values()):.3f} {flash}")


@pytest.mark.parametrize("kind", O.KINDS)
def test_h2_restatement_stays_within_bounds_h2(kind):
    """operands rounded as split4h rounds them, scales as the kernels take them, within bounds_h2 -- also with amax words 2^6 too
    large (any upper bound is a valid word) under the bound evaluated with that amax"""
    h2 = worst_of(kind, O.restate_h2, "h2")
    worst = {}
    for L, heads, causal in O.CASES:
        qkv, dout, ref, _ = O.case(kind, L, heads, causal)
        r = O.ratios(O.restate_h2(qkv, dout, heads, causal, amax_mul=64.0), ref, O.bounds_h2(qkv, dout, heads, causal, amax_mul=64.0))
        assert max(r.values()) <= 1.0, (kind, L, heads, causal, r)
        worst = {n: max(worst.get(n, 0.0), v) for n, v in r.items()}
    print(f"{kind}: h2 restatement worst err / bound {max(h2.values()):.3f} {h2}; with amax x 64: {max(worst.values()):.3f} {worst}")


def test_bounds_are_finite_and_positive_where_the_reference_is_not_zero():
    for kind in O.KINDS:
        for L, heads, causal in O.CASES:
            _, _, ref, bnd = O.case(kind, L, heads, causal)
            for form in O.FORMS:
                for name in O.OUTPUTS:
                    b = bnd[form][name]
                    assert b.shape == ref[name].shape and b.dtype == torch.float64
                    assert bool(torch.isfinite(b).all()) and bool((b >= 0).all()), (kind, L, heads, causal, form, name)
                    assert bool((b[ref[name] != 0] > 0).all()), (kind, L, heads, causal, form, name)


def test_the_inputs_are_what_their_kinds_say():
    """late_max / early_max: the dominant key leads every other visible one by at least 30; zero_rows: the dq rows of the zeroed
    queries are exactly zero in the reference with a zero bound (so the kernels must give exact zeros); head_gains: the gains"""
    for L, heads, causal in O.CASES:
        for kind in ("late_max", "early_max"):
            qkv, dout = O.inputs(kind, L, heads, causal)
            q, k, _ = (t.double() for t in O.split_heads(qkv, heads))
            assert bool((q > 0).all())
            s = ((q @ k.transpose(2, 3)) / 8).masked_fill(~O.visible(L, causal), float("-inf"))
            top = s.topk(min(2, L), -1)
            want = torch.zeros(L, dtype=torch.long) if kind == "early_max" else (torch.arange(L) if causal else torch.full((L,), L - 1))
            assert bool((top.indices[..., 0] == want).all()), (kind, L, causal)
            if L > 1:
                margin = top.values[..., 0] - top.values[..., 1]
                rows = slice(1, None) if causal else slice(None)          # (causal row 0 sees one key)
                assert float(margin[:, :, rows].min()) >= 30.0, (kind, L, causal, float(margin[:, :, rows].min()))
        qkv, dout, ref, bnd = O.case("zero_rows", L, heads, causal)
        rows = O.zero_row_set(L)
        assert bool((dout[:, rows] == 0).all()) and (L <= 32 or set(range(32, min(48, L))) <= set(rows))
        for form in ("valu", "f32"):      # (h2: the bound keeps the fixed-point floor of the operands; the GPU test asserts the zeros)
            assert bool((ref["dq"][:, rows] == 0).all()) and bool((bnd[form]["dq"][:, rows] == 0).all())
        qkv, dout = O.inputs("head_gains", L, heads, causal)
        if heads == 3:
            amax = qkv.view(O.NB, L, 3, heads, O.HD).abs().amax((0, 1, 2, 4))
            assert 2.0 ** -11 < float(amax[1] / amax[0]) < 2.0 ** -9 and 2.0 ** -21 < float(amax[2] / amax[0]) < 2.0 ** -19


@pytest.mark.parametrize("name", O.MUTATIONS)
def test_every_mutation_breaks_the_bound(name):
    """one defect in the fp64 path: some output exceeds its bound in some case of the list.  The piece-dropping mutations must
    exceed bounds_h2 (the widest); the others are held against the f32 form, the wider of the two fp32 ones."""
    form = "h2" if name in O.H2_MUTATIONS else "f32"
    found, tried = None, 0
    for kind in O.KINDS:
        for L, heads, causal in O.CASES:
            qkv, dout, ref, bnd = O.case(kind, L, heads, causal)
            got = O.mutate(name, qkv, dout, heads, causal)
            if got is None:
                continue
            tried += 1
            r = O.ratios(got, ref, bnd[form])
            worst = max(r, key=r.get)
            if r[worst] > 1.0 and (found is None or r[worst] > found[1]):
                found = ((kind, L, heads, causal, worst), r[worst])
        if found is not None and name not in O.H2_MUTATIONS:
            break
    assert found is not None, (name, tried)
    print(f"{name}: exceeds the {form} bound at kind, L, heads, causal, output = {found[0]} by {found[1]:.3g}x")


def test_dropping_the_low_piece_of_k_shows_on_every_input_kind():
    """the 11-bit operand: out, lse and dv leave bounds_h2 on every kind with random keys at L = 65 and 129; dq does on head_gains.
    (late_max / early_max: the dominant key is 5.0 in every channel, exact in fp16, and holds all the weight.)"""
    for kind in ("randn", "peaked", "head_gains", "zero_rows"):
        for L in (65, 129):
            qkv, dout, ref, bnd = O.case(kind, L, 3, 0)
            r = O.ratios(O.mutate("k_low_dropped", qkv, dout, 3, 0), ref, bnd["h2"])
            assert min(r["out"], r["lse"], r["dv"]) > 1.0, (kind, L, r)
            if kind == "head_gains":
                assert r["dq"] > 1.0, (kind, L, r)


def test_the_bound_sees_a_lost_head_that_the_old_yardstick_cannot():
    """head_gains: the smallest head's dq replaced by zeros passes max |err| <= 2e-4 max(1, max |ref|) and fails every bound"""
    for L, heads, causal in O.CASES:
        if heads != 3 or L == 1:        # (one key: dS = p (dP - delta) = 0, there is no dq to lose)
            continue
        qkv, dout, ref, bnd = O.case("head_gains", L, heads, causal)
        dq = ref["dq"].clone()
        dq[:, :, 2 * O.HD:] = 0.0
        assert float(ref["dq"][:, :, 2 * O.HD:].abs().max()) > 0
        assert O.old_yardstick_passes(dq, ref["dq"]), (L, causal)
        for form in O.FORMS:
            r = O.ratios(dict(dq=dq), ref, bnd[form])["dq"]
            assert r > 1.0, (L, causal, form, r)
        size = float(bnd["h2"]["dq"][:, :, 2 * O.HD:].max()) / (2e-4 * max(1.0, float(ref["dq"].abs().max())))
        assert size < 1e-6, (L, causal, size)       # the bound on that head against the old tolerance
