"""The Stage-1 head tests without a GPU: the bilinear error bounds of tests/oracle_heads.py hold for PyTorch's own float32 CPU
kernels over the whole sweep of tests/test_gpu_heads.py, the sweep covers what it claims, and the inputs of the kernel tests
satisfy the conditions those tests rely on (exact ties, no pre-activation at the relu kink, LDS sizes on the intended sides of
the entry points' limits).  Also the Python-side argument contracts of ops.score_heads / ops.fg_patches, which raise before any
device call."""
import pytest
import torch
import torch.nn.functional as F

import oracle_heads as OH


def _f32_resize(x, g, size, align):
    xs = x.clone().requires_grad_(True)
    y = F.interpolate(xs[None], size=size, mode="bilinear", align_corners=align)[0]
    y.backward(g)
    return y.detach(), xs.grad


def _check_reference_inside_bounds(case, planes=2):
    Hi, Wi, Ho, Wo, align = case
    x, g = OH.resize_inputs(case, planes)
    y32, dx32 = _f32_resize(x, g, (Ho, Wo), align)
    ef = (y32.double() - OH.resize(x, (Ho, Wo), align)).abs()
    eb = (dx32.double() - OH.resize_adjoint(g, (Hi, Wi), align)).abs()
    bf, bb = OH.resize_fwd_bound(x), OH.resize_bwd_bound(g, (Hi, Wi), align)
    assert bool((ef <= bf).all()), (case, float(ef.max()), float(bf.max()))
    assert bool((eb <= bb).all()), (case, float((eb - bb).max()))
    return float(ef.max()), float(bf.max())


def test_sweep_covers_every_ratio_on_both_axes():
    cases = OH.resize_cases()
    assert 360 <= len(cases) <= 400 and len(set(cases)) == len(cases)
    rows = {(hi, ho, a) for hi, _, ho, _, a in cases}
    cols = {(wi, wo, a) for _, wi, _, wo, a in cases}
    want = {(i, o, a) for i in range(1, 10) for o in range(1, 21) for a in (False, True)}
    want |= {(i, o, a) for i, o in OH.RESIZE_EXTRA for a in (False, True)}
    assert want <= rows and want <= cols
    nh = OH.nhwc_cases()
    want = {(i, o) for i in range(1, 10) for o in range(i, 21)} | {(10, 320)}
    assert want <= {(hi, ho) for hi, _, ho, _ in nh} and want <= {(wi, wo) for _, wi, _, wo in nh}
    assert all(ho >= hi and wo >= wi for hi, wi, ho, wo in nh)
    planes, Hi, Wi, Ho, Wo, _ = OH.GRID_CAP_CASE
    assert planes * Ho * Wo > 8192 * 256            # grid_for's cap in heads.hip: the forward takes its grid-stride loop
    B, C, R, _ = OH.FG_CASES[-1]
    assert B * C * R * R > 8192 * 256


def test_bounds_hold_for_pytorch_float32_over_the_sweep():
    for case in OH.resize_cases():
        _check_reference_inside_bounds(case)
    for Hi, Wi, Ho, Wo in OH.nhwc_cases():
        _check_reference_inside_bounds((Hi, Wi, Ho, Wo, False))
    planes = OH.GRID_CAP_CASE[0]
    _check_reference_inside_bounds(OH.GRID_CAP_CASE[1:], planes)


def test_bound_magnitudes():
    """320 -> 224 with align_corners=True: the float32/float64 gap is of order 1e-4 and the bound about 1.2e-3; at in <= 20 the
    bound is of order 1e-5"""
    err, bound = _check_reference_inside_bounds((320, 320, 224, 224, True))
    assert err < bound and 5e-4 < bound < 3e-3
    for case in [(7, 9, 20, 13, False), (20, 20, 3, 40, True)]:
        x, _ = OH.resize_inputs(case)
        assert float(OH.resize_fwd_bound(x).max()) < 1e-4


def test_bound_is_tight_enough_to_see_a_dropped_window_term():
    """an adjoint that loses the last output of each input's window is outside the backward bound somewhere in the sweep's
    up-scales (what a window() one short would do)"""
    Hi, Ho = 5, 13
    g = OH.resize_inputs((Hi, Hi, Ho, Ho, False))[1]
    full = OH.resize_adjoint(g, (Hi, Hi), False)
    basis = torch.eye(Ho, dtype=torch.float64)[:, None, :].expand(Ho, Ho, Ho)       # row oy of output image oy is ones
    last = OH.resize_adjoint(basis, (Hi, Hi), False).sum(-1)                         # [Ho, Hi]: weight of output row oy on input row y
    drop = torch.zeros(Ho, dtype=torch.bool)
    for y in range(Hi):
        drop[int(torch.nonzero(last[:, y]).max())] = True
    lossy = OH.resize_adjoint(g * (~drop)[None, :, None], (Hi, Hi), False)
    assert bool(((lossy - full).abs() > OH.resize_bwd_bound(g, (Hi, Hi), False)).any())


def test_class_head_inputs():
    for shape in OH.CLS_SHAPES:
        B, P, N = shape
        score, g = OH.cls_inputs(shape, "ties")
        assert score.dtype == torch.float32 and g.shape == (B, N)
        slots = OH.tie_slots(B, P, N)
        assert len(slots) == len([t for t in OH.TIE_GROUPS if max(t) < P]) and len({(b, j) for b, j, _ in slots}) == len(slots)
        _, _, _, dmax = OH.cls_head(score, g, 3.0, 0.01)
        for b, j, pix in slots:
            col = score[b, :, j]
            assert all(col[p].item() == col.max().item() for p in pix)                 # tied bit for bit, and maximal
            assert int((col == col.max()).sum()) == len(pix)
            first = min(pix)
            assert dmax[b, first, j].item() == g[b, j].double().item()                 # the oracle: first maximal pixel only
            assert int((dmax[b, :, j] != 0).sum()) == 1
        ones, g1 = OH.cls_inputs(shape, "ones")
        assert bool((ones == 1.0).all())
        dm = OH.cls_head(ones, g1, 3.0, 0.01)[3]
        assert bool((dm[:, 0, :] == g1.double()).all()) and bool((dm[:, 1:, :] == 0).all())
    assert len(OH.tie_slots(2, 130, 70)) == 4 and len(OH.tie_slots(2, 400, 40)) == 4      # every group planted somewhere
    # the confirmed CPU behaviour: ties at (3, 67), (70, 9), (5, 6, 129) send the gradient to 3, 9 and 5
    for pix, first in (((3, 67), 3), ((70, 9), 9), ((5, 6, 129), 5)):
        for dt in (torch.float32, torch.float64):
            v = torch.zeros(1, 130, dtype=dt)
            v[0, list(pix)] = 2.0
            v.requires_grad_(True)
            torch.max(v, dim=-1).values.sum().backward()
            assert int(v.grad[0].argmax()) == first and float(v.grad.sum()) == 1.0


def test_class_head_lds_sizes():
    B, P, N = OH.CLS_LARGE
    assert OH.cls_lds_bytes(P, N, False) > 60000 and OH.cls_lds_bytes(P, N, True) > 60000
    assert OH.cls_lds_bytes(P, N, True) <= 150 * 1024
    assert abs(OH.cls_lds_bytes(P, N, False) - 68.8e3) < 100
    for shape in OH.CLS_SHAPES:
        if shape != OH.CLS_LARGE:
            assert OH.cls_lds_bytes(shape[1], shape[2], True) <= 60000
    B, P, N = OH.CLS_REFUSED
    assert OH.cls_lds_bytes(P, N, False) > 150 * 1024 and OH.cls_lds_bytes(P, N, True) > 150 * 1024
    assert 170e3 < OH.cls_lds_bytes(P, N, False) < 180e3


def test_class_head_float32_yardstick_is_finite():
    for shape in OH.CLS_SHAPES:
        for kind in OH.CLS_KINDS:
            for focal in OH.FOCAL:
                ref, err32 = OH.cls_reference(shape, kind, focal)
                assert all(bool(torch.isfinite(r).all()) for r in ref[:3]), (shape, kind, focal)
                assert all(e == e and e < 1e-2 * max(1.0, float(r.abs().max())) for e, r in zip(err32, ref[:3])), (shape, kind, focal, err32)


def test_response_map_inputs_clear_the_relu_kink():
    for case in OH.MAPS_CASES:
        h, w, S = case
        assert h * w <= 1024
        score = OH.maps_inputs(case)[0]
        v = OH.maps(score, h, w, S)[0]
        assert float(v.abs().min()) >= OH.MAPS_KINK, (case, float(v.abs().min()))
    assert any(h != w for h, w, _ in OH.MAPS_CASES) and any(h * w == 1024 for h, w, _ in OH.MAPS_CASES)
    assert any((S * S) % 256 for _, _, S in OH.MAPS_CASES) and any(S < h for h, _, S in OH.MAPS_CASES)


def test_fg_layout_round_trip():
    for B, C, R, ps in OH.FG_CASES[:3]:
        x = torch.arange(B * C * R * R, dtype=torch.float32).reshape(B, C, R, R)
        assert torch.equal(OH.fg_unlayout(OH.fg_layout(x, ps), C, R, ps), x)


def test_wrapper_argument_contracts():
    """score_heads refuses h * w != P, fg_patches a non-square image, a cam that is not [B,1,R,R] or a patch size that does not
    divide R: ValueError, raised ahead of every device call (so CPU tensors show it, before the no-GPU error)"""
    from tris_amd import ops
    for h, w in ((2, 2), (3, 3), (6, 0)):
        with pytest.raises(ValueError):
            ops.score_heads(torch.zeros(1, 6, 1), h, w, 4, True)
    with pytest.raises(ValueError):
        ops.score_heads(torch.zeros(6, 1), 2, 3, 4, False)
    img = torch.zeros(2, 3, 8, 8)
    for cam, im, ps in ((torch.zeros(2, 1, 8, 8), torch.zeros(2, 3, 8, 6), 2), (torch.zeros(2, 1, 6, 8), torch.zeros(2, 3, 6, 8), 2),
                        (torch.zeros(2, 1, 8, 6), img, 2), (torch.zeros(2, 3, 8, 8), img, 2), (torch.zeros(1, 1, 8, 8), img, 2),
                        (torch.zeros(2, 8, 8), img, 2), (torch.zeros(2, 1, 8, 8), img, 3), (torch.zeros(2, 1, 8, 8), img, 0)):
        with pytest.raises(ValueError):
            ops.fg_patches(cam, im, ps)
    # well-formed arguments pass the contract and reach the device check
    with pytest.raises(ops.NoGpuError):
        ops.score_heads(torch.zeros(1, 6, 1), 2, 3, 4, True)
    with pytest.raises(ops.NoGpuError):
        ops.fg_patches(torch.zeros(2, 1, 8, 8), img, 2)
