"""IRNet's affinity / displacement training losses on the MI355X (csrc/irnloss.hip, tris_amd/irn_loss.py) against the fp64 torch
restatement of the contract (tests/oracle_irn_loss.py), which tests/test_irn_loss_host.py holds against the reference's own code.

Bound of every comparison with fp64: 8 x the distance of the fp32 CPU restatement from fp64 on the same input, computed here
(the project's convention for gradient probes); for a scalar the bound is floored at 4 fp32 ulps of the value, 4 * 2^-23 = 4.8e-7
relative, since one fp32 number cannot be asked closer.  Distances measured on the MI355X are in DESIGN.md, "IRNet training
losses"."""
import functools

import numpy as np
import pytest
import torch

import oracle_irn_loss as O

pytestmark = pytest.mark.gpu

ULP4 = 4 * 2.0 ** -23
SHAPES = [(1, 10, 19, 10),      # exactly one source row; no fg pair: l2 = 0
          (2, 21, 23, 10),      # a source region smaller than any tile
          (2, 40, 52, 10),
          (3, 70, 45, 10),      # crosses tile boundaries in both directions, odd sizes
          (2, 12, 14, 5)]
UPSTREAM = (0.3, -1.1, 2.0, 0.7)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def case(shape, weights=None):
    """-> (inputs, fp64 restatement, fp32 restatement), each restatement (losses, counts, d_edge, d_dp); computed once"""
    B, h, w, radius = shape
    x = O.inputs(B, h, w)
    return x, O.restated(*x, radius, torch.float64, weights), O.restated(*x, radius, torch.float32, weights)


def run(edge, dp, label, radius, weights=None):
    """the op on the GPU -> (losses, counts, d_edge, d_dp) as numpy"""
    from tris_amd import irn_loss
    e, d = dev(edge).requires_grad_(True), dev(dp).requires_grad_(True)
    losses, counts = irn_loss.affinity_displacement_losses(e, d, dev(label), radius)
    assert losses.dtype == torch.float32 and losses.shape == (4,) and counts.dtype == torch.int64 and counts.shape == (3,)
    obj = irn_loss.total_loss(losses) if weights is None else losses @ torch.tensor(weights, device="cuda")
    obj.backward()
    return losses.detach().cpu().numpy(), counts.cpu().numpy(), e.grad.cpu().numpy(), d.grad.cpu().numpy()


def check_against_fp64(got, r64, r32, tag):
    l, n, ge, gd = got
    assert np.array_equal(n, r64[1]), (tag, n, r64[1])
    for k in range(4):
        want = float(r64[0][k])
        bound = max(8 * abs(float(r32[0][k]) - want), ULP4 * abs(want))
        err = abs(float(l[k]) - want)
        print(f"{tag}: l{k} = {l[k]:.8g}, |gpu - fp64| = {err:.3e} (relative {err / abs(want) if want else 0.0:.3e}), bound {bound:.3e}")
        assert err <= bound, (tag, k, err, bound)
    for name, g, g64, g32 in (("d_edge", ge, r64[2], r32[2]), ("d_dp", gd, r64[3], r32[3])):
        err, cpu = O.rel_l2(g, g64), O.rel_l2(g32, g64)
        print(f"{tag}: {name} relative L2 gpu {err:.3e}, fp32 cpu {cpu:.3e}, bound {8 * cpu:.3e}")
        assert np.isfinite(g).all()
        assert err <= 8 * cpu, (tag, name, err, 8 * cpu)
        assert not g[g64 == 0].any(), (tag, name, "an entry that is exactly 0 in fp64 is not 0")


# -------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_fp64(shape):
    x, r64, r32 = case(shape)
    if shape == SHAPES[0]:
        assert r64[1][1] == 0 and r64[0][2] == 0                    # the empty fg class
    check_against_fp64(run(*x, shape[3]), r64, r32, str(shape))


# --------------------------------------------------------------------------------------------------- 2. upstream gradient
def test_upstream_gradient():
    shape = (2, 21, 23, 10)
    x, r64, r32 = case(shape, UPSTREAM)
    check_against_fp64(run(*x, shape[3], UPSTREAM), r64, r32, f"{shape} g = {UPSTREAM}")


# -------------------------------------------------------------------------------------------------------------- 3. ties
def test_plateau_gradient_goes_where_the_reference_sends_it(golden):
    g16 = golden("g16_irn_loss.npz")
    edge, dp, label = O.plateau_inputs()
    l, n, ge, _ = run(edge, dp, label, O.PLATEAU_SHAPE[3], (0.5, 0.5, 0.0, 0.0))
    assert np.array_equal(n, g16["plateau_counts"])
    err = O.rel_l2(ge, g16["plateau_d_edge"])
    print(f"plateau: d_edge relative L2 against the reference {err:.3e}")
    assert err <= 1e-6, err
    assert np.array_equal(ge == 0, g16["plateau_d_edge"] == 0)       # the same cells take the gradient


def test_saturated_logits():
    B, h, w, radius = 2, 21, 23, 10
    _, dp, label = O.inputs(B, h, w)
    l, n, ge, gd = run(np.full((B, 1, h, w), 40.0, np.float32), dp, label, radius)
    assert n[0] > 0 and n[1] > 0
    assert abs(l[0] - (-np.log(1e-5))) <= 1e-6 * -np.log(1e-5), l
    assert not ge.any()
    assert np.isfinite(l).all() and np.isfinite(ge).all() and np.isfinite(gd).all()


# -------------------------------------------------------------------------------------------------- 4. degenerate labels
def test_degenerate_labels():
    B, h, w, radius = 2, 21, 23, 10
    edge, dp, _ = O.inputs(B, h, w)
    l, n, ge, gd = run(edge, dp, np.zeros((B, h, w), np.uint8), radius)
    assert l[1] == 0 and l[2] == 0 and l[0] > 0 and l[3] > 0
    assert n[0] == B * 152 * (h - 9) * (w - 18) and n[1] == 0 and n[2] == 0
    assert np.isfinite(ge).all() and np.isfinite(gd).all() and ge.any() and gd.any()
    l, n, ge, gd = run(edge, dp, np.full((B, h, w), 255, np.uint8), radius)
    assert not l.any() and not n.any() and not ge.any() and not gd.any()
    assert not np.isnan(l).any() and not np.isnan(ge).any() and not np.isnan(gd).any()


# ------------------------------------------------------------------------------------------------------ 5. repeatability
def test_bitwise_repeatable():
    shape = (3, 70, 45, 10)
    x, _, _ = case(shape)
    a, b = run(*x, shape[3]), run(*x, shape[3])
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


# ---------------------------------------------------------------------------------------------------------- 6. end to end
def test_composes_with_autograd():
    """edge_out = a x + b from two leaf scalars and elementwise torch ops: total_loss(...).backward() fills a.grad and b.grad as
    the fp64 restatement does"""
    from tris_amd import irn_loss
    shape = (2, 21, 23, 10)
    (x, y, label), _, _ = case(shape)
    leaves = (1.25, -0.5)

    def cpu(dtype):
        a, b = (torch.tensor(v, dtype=dtype, requires_grad=True) for v in leaves)
        l, _ = O.losses(a * torch.from_numpy(x).to(dtype) + b, torch.from_numpy(y).to(dtype), torch.from_numpy(label), shape[3])
        O.total(l).backward()
        return [float(t.grad) for t in (a, b)]

    a, b = (torch.tensor(v, device="cuda", requires_grad=True) for v in leaves)
    d = dev(y).requires_grad_(True)
    losses, _ = irn_loss.affinity_displacement_losses(a * dev(x) + b, d, dev(label), shape[3])
    irn_loss.total_loss(losses).backward()
    assert d.grad is not None and d.grad.shape == d.shape
    w64, w32 = cpu(torch.float64), cpu(torch.float32)
    for name, t, want, f32 in zip("ab", (a, b), w64, w32):
        assert t.grad is not None
        err, bound = abs(float(t.grad) - want), max(8 * abs(f32 - want), ULP4 * abs(want))
        print(f"{name}.grad = {float(t.grad):.8g}, fp64 {want:.8g}, |gpu - fp64| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (name, err, bound)


def test_forward_alone_and_one_sided_gradients():
    """no gradient wanted: the same losses; one of the two maps a leaf: its gradient equals the one of the two-sided run"""
    from tris_amd import irn_loss
    shape = (2, 21, 23, 10)
    (x, y, label), _, _ = case(shape)
    l, n, ge, gd = run(x, y, label, shape[3])
    l0, n0 = irn_loss.affinity_displacement_losses(dev(x), dev(y), dev(label), shape[3])
    assert not l0.requires_grad and np.array_equal(l0.cpu().numpy(), l) and np.array_equal(n0.cpu().numpy(), n)
    e = dev(x).requires_grad_(True)
    irn_loss.total_loss(irn_loss.affinity_displacement_losses(e, dev(y), dev(label), shape[3])[0]).backward()
    assert np.array_equal(e.grad.cpu().numpy(), ge)
    d = dev(y).requires_grad_(True)
    irn_loss.total_loss(irn_loss.affinity_displacement_losses(dev(x), d, dev(label), shape[3])[0]).backward()
    assert np.array_equal(d.grad.cpu().numpy(), gd)


# --------------------------------------------------------------------------------------------------------- 7. reduce_label
@pytest.mark.parametrize("shape", [(2, 50, 61), (512, 512)], ids=lambda s: "x".join(map(str, s)))
def test_reduce_label_equals_pillow_nearest(shape):
    from PIL import Image
    from tris_amd import irn_loss
    rng = np.random.default_rng(3)
    lab = rng.integers(0, 256, size=shape).astype(np.uint8)
    H, W = shape[-2:]
    size = (int(np.round(H * 0.25)), int(np.round(W * 0.25)))
    want = np.stack([np.asarray(Image.fromarray(m).resize(size[::-1], Image.NEAREST)) for m in lab.reshape(-1, H, W)])
    got = irn_loss.reduce_label(dev(lab))
    assert got.dtype == torch.uint8 and got.is_contiguous()
    assert tuple(got.shape) == tuple(shape[:-2]) + size == ((2, 12, 15) if len(shape) == 3 else (128, 128))
    assert np.array_equal(got.cpu().numpy().reshape(want.shape), want)
