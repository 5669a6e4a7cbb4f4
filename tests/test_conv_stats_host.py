"""The yardstick of tests/test_gpu_conv_stats.py, checked without a GPU (tests/oracle_conv_stats.py): at every shape and operand kind the
GPU test runs,
  * an fp32 CPU convolution sits inside the a-priori elementwise bound -- the bound is satisfiable by a plain fp32 product;
  * no group has a zero reference norm, and the generators are deterministic;
  * the h2 operand rounding (scale from the exact amax, or from the BatchNorm bound word for the folded forms), followed by an fp64
    product, stays BELOW the fp32 CPU convolution's group errors: the inputs are inside h2's documented range before a kernel is asked;
  * the same emulation with the residual piece stored WITHOUT its 2^11 pre-scale fails the GPU test's 2x group criterion on the
    kinds with small groups -- while passing the close(..., 2e-4) of the existing convolution tests: the criterion has teeth where
    the old yardstick has none."""
import math

import pytest
import torch

import oracle_conv_stats as O

PLAIN = sorted({(s, 1) for s in O.IMPLICIT + tuple(O.DIRECT_FWD.values()) + tuple(O.DIRECT_FWD_H2.values()) + tuple(O.DIRECT_DGRAD.values()) +
                tuple(O.DIRECT_WGRAD.values())} | {(s, 2) for s in O.IMPLICIT_S2})
CASES = [(shape, stride, kind) for shape, stride in PLAIN for kind in O.KINDS] + [(s, 2, k) for s in O.STEM for k in O.STEM_KINDS]
BNIN_CASES = [(shape, kind) for shape in O.BNIN for kind in O.BNIN_KINDS]
CAUGHT = ("image_2^-20", "image_2^-24", "filters_2^-20", "gradient_like")     # kinds on which the unscaled residual must be rejected


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _rows(shape):
    return (shape[0] * shape[1] * shape[2], O.WORKLOAD_ROWS)


def test_h2_round_is_the_rounding_the_plane_tests_pin():
    """(tests/test_gpu_planes.py compares `_h2_round` bit for bit with what the device writes)"""
    from test_gpu_planes import _h2_round
    x = torch.randn(1 << 14, generator=torch.Generator().manual_seed(0)) * torch.logspace(-8, 2, 1 << 14)
    for amax in (O.amax(x), 700.0 * O.amax(x)):
        assert torch.equal(O.h2_round(x, amax), _h2_round(x, amax))
    lost = O.h2_round(x, O.amax(x), prescale=False)
    tiny = x.abs() < O.amax(x) * 2.0 ** -20
    assert float(((lost - x).abs() / x.abs())[tiny].max()) > 2.0 ** -12      # the mutation: elements 2^-20 down keep < 12 bits


@pytest.mark.parametrize("shape,stride,kind", CASES, ids=_id)
def test_fp32_convolution_is_inside_the_bound_and_groups_are_not_empty(shape, stride, kind):
    c, r = O.operands(kind, shape, stride), O.reference(kind, shape, stride)
    again = O.operands.__wrapped__(kind, shape, stride)
    assert torch.equal(again.x, c.x) and torch.equal(again.w, c.w) and (c.dy is None or torch.equal(again.dy, c.dy))
    assert set(r.ref) == ({"y"} if stride == 2 else {"y", "dx", "dw"})
    f32 = O.products(c.x, c.w, c.dy, stride, torch.float32)
    for k, ref in r.ref.items():
        assert ref.flatten(1).norm(dim=1).min() > 0 and ref.flatten(0, -2).norm(dim=0).min() > 0, k
        for axis, name, m in O.selections(c.small[k], ref.shape[0], ref.shape[-1]):
            assert int(m.sum()) > 0 and m.numel() == ref.shape[0 if axis == 0 else -1], (k, axis, name)
        ratio = O.bound_ratio(f32[k], ref, r.bound[k])
        assert ratio <= 1.0, (k, ratio)          # (measured: <= 0.1)
        assert torch.isfinite(r.bound[k]).all() and float(r.bound[k].min()) > 0


@pytest.mark.parametrize("shape,stride,kind", CASES, ids=_id)
def test_emulated_h2_is_inside_the_criterion_and_the_unscaled_residual_is_not(shape, stride, kind):
    c, r = O.operands(kind, shape, stride), O.reference(kind, shape, stride)
    f32 = O.products(c.x, c.w, c.dy, stride, torch.float32)
    h2, lost = O.emulated(c), O.emulated(c, prescale=False)
    rejected = []
    for k, ref in r.ref.items():
        bad, worst = O.criterion(h2[k], f32[k], ref, c.small[k], 1.0)
        assert not bad, (k, worst, bad)          # (measured: worst 0.80 -- the stem's 27-term sums --, 0.71 elsewhere)
        assert O.close(lost[k], ref, 2e-4), k    # the old yardstick accepts the mutated arithmetic everywhere ...
        rejected += [(k,) + b for b in O.criterion(lost[k], f32[k], ref, c.small[k], 2.0)[0]]
    if kind in CAUGHT and (c.dy is not None or kind != "gradient_like"):     # (a forward alone does not read the gradient-like dy)
        assert rejected, (shape, kind)           # ... the group criterion does not (measured: 3.6x .. 720x)


@pytest.mark.parametrize("shape,kind", BNIN_CASES, ids=_id)
def test_folded_batchnorm_cases(shape, kind):
    c, r = O.bnin_operands(kind, shape), O.bnin_reference(kind, shape)
    again = O.bnin_operands.__wrapped__(kind, shape)
    assert all(torch.equal(getattr(again, n), getattr(c, n)) for n in ("x", "mean", "invstd", "gamma", "beta", "w", "dy"))
    act32 = O.bn_relu(c, torch.float32)
    f32 = O.products(act32, c.w, c.dy, 1, torch.float32)
    for k, ref in r.ref.items():
        assert ref.flatten(1).norm(dim=1).min() > 0 and ref.flatten(0, -2).norm(dim=0).min() > 0, k
        assert O.bound_ratio(f32[k], ref, r.bound[k]) <= 1.0, k
    for rows in _rows(shape):
        bound = O.bn_bound(c, rows)
        assert float(act32.max()) <= bound
        h2, lost = O.bnin_emulated(c, bound), O.bnin_emulated(c, bound, prescale=False)
        rejected = []
        for k, ref in r.ref.items():
            bad, worst = O.criterion(h2[k], f32[k], ref, c.small[k], 1.0)
            assert not bad, (rows, k, worst, bad)            # (measured: <= 0.54 with either bound word)
            assert O.close(lost[k], ref, 2e-4), k
            rejected += O.criterion(lost[k], f32[k], ref, c.small[k], 2.0)[0]
        if kind.startswith("affine") and rows == O.WORKLOAD_ROWS:
            assert rejected, (shape, kind)       # channels 2^-12 down under a bound 2^7 above the maximum (measured: 18x .. 66x)
    assert math.sqrt(O.WORKLOAD_ROWS - 1) > 10 * math.sqrt(_rows(shape)[0] - 1)  # the second bound word really is the looser one
