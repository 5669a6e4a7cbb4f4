"""The Stage-1 head kernels (csrc/heads.hip, csrc/bilinear.h) on the MI355X against the fp64 restatement of
tests/oracle_heads.py: the class head with its focal term at every (focal_p, focal_c) of the command line, exact ties included;
the diagonal response maps; the bilinear family (NCHW resize, channels-last upsample) over a sweep of ratios with the oracle's
derived bounds; the foreground patches and the ViT token assembly; launch-to-launch repeatability of every backward; and the
argument contracts of the entry points.

Class-head tolerance (no closed bound: expf and a butterfly summation order): each output's error against fp64 is at most
max(4 * err_cpu32, 32 * 2^-24 * max|ref|), err_cpu32 being the error of the same PyTorch expression in float32 on the CPU.  The
factor 4 allows for the different summation order and a device expf that is one or two ulp off.  The ratios measured on the
MI355X are recorded in profiles/heads_parity_floor.txt.
"""
import functools

import pytest
import torch

import oracle_heads as OH

pytestmark = pytest.mark.gpu

U = OH.U


@pytest.fixture(autouse=True, params=["x3", "h2"])
def arith(request):
    """both arithmetics of the dense products, as tests/test_gpu_stage2.py (these kernels do not depend on it)"""
    from tris_amd import ops
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(request.param)
    yield request.param
    ops.set_gemm_mode(prev)


def _err(a, ref):
    return (a.detach().double().cpu() - ref).abs()


def _inside(a, ref, bound, what):
    e = _err(a, ref)
    worst = float((e - bound).max())
    print(f"{what}: max err {float(e.max()):.3e}, bound up to {float(torch.as_tensor(bound).max()):.3e}")
    assert worst <= 0.0, f"{what}: error exceeds the bound by {worst:.3e} (max err {float(e.max()):.3e})"


# ================================================================================================================ class head
def _cls_abi(ops, score, g, focal, with_fg=True):
    B, P, N = score.shape
    st = ops._stream()
    cls_out = torch.empty(B, N, device="cuda")
    cls_fg = torch.zeros(B, device="cuda") if with_fg else None
    dscore = torch.empty_like(score)
    ops.call("tris_cls_head_fwd_f32", ops.P(score), ops.P(cls_out), ops.P(cls_fg), B, P, N, focal[0], focal[1], st)
    ops.call("tris_cls_head_bwd_f32", ops.P(score), ops.P(g), ops.P(dscore), B, P, N, focal[0], focal[1], st)
    return cls_out, cls_fg, dscore


def _cls_wrapper(ops, score, g, focal):
    """through ops.score_heads on a 1 x P grid with a 1 x 1 map; only cls_out carries a gradient"""
    B, P, N = score.shape
    s = score.clone().requires_grad_(True)
    cls_out, cls_fg, _, _ = ops.score_heads(s, 1, P, 1, True, focal[0], focal[1])
    cls_out.backward(g)
    return cls_out.detach(), cls_fg, s.grad


def cls_measure(ops, shape, kind, focal):
    """-> {output: (err_hip, err_cpu32, tolerance)}, the device gradient, the reference"""
    score, g = OH.cls_inputs(shape, kind)
    ref, err32 = OH.cls_reference(shape, kind, focal)
    sd, gd = score.cuda(), g.cuda()
    run = _cls_abi if shape == (2, 25, 5) else _cls_wrapper
    out = run(ops, sd, gd, focal)
    again = run(ops, sd, gd, focal)
    assert all(torch.equal(a, b) for a, b in zip(out, again)), "two launches on the same inputs differ"
    fig = {}
    for name, a, r, e32 in zip(("cls_out", "cls_fg", "dscore"), out, ref[:3], err32):
        fig[name] = (float(_err(a, r).max()), e32, OH.cls_tolerance(e32, r))
    return fig, out, ref


@pytest.mark.parametrize("kind", OH.CLS_KINDS)
@pytest.mark.parametrize("focal", OH.FOCAL, ids=lambda f: f"p{f[0]:g}c{f[1]:g}")
@pytest.mark.parametrize("shape", OH.CLS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_class_head(shape, focal, kind):
    from tris_amd import ops
    fig, out, ref = cls_measure(ops, shape, kind, focal)
    for name, (eh, e32, tol) in fig.items():
        print(f"{name}: err_hip {eh:.3e} err_cpu32 {e32:.3e} ratio {eh / e32 if e32 > 0 else float('inf'):.2f} tolerance {tol:.3e}")
    for name, (eh, e32, tol) in fig.items():
        assert eh <= tol, f"{name}: err_hip {eh:.3e} > max(4 * {e32:.3e}, floor) = {tol:.3e}"
    if kind in ("ties", "ones"):
        # the max part of the gradient sits on the first maximal pixel of every column and nowhere else
        score, g = OH.cls_inputs(shape, kind)
        dscore, dmax = ref[2], ref[3]
        resid = out[2].double().cpu() - (dscore - dmax)                     # what the device added beyond the smooth part
        gg = g.double().abs()[:, None, :]
        ismax = score == score.amax(1, keepdim=True)
        first = ismax & (ismax.cumsum(1) == 1)
        judged = (gg > 100 * fig["dscore"][2]).expand_as(first)              # (a column whose gradient is at the noise floor says nothing)
        wrong = ((resid.abs() > gg / 2) != first) & judged
        assert not bool(wrong.any()), f"max gradient misplaced at (image, pixel, sentence) {wrong.nonzero().tolist()[:8]}"
        assert bool(judged.any()) or shape == (1, 1, 1)


def test_class_head_cls_fg_is_optional():
    from tris_amd import ops
    score, g = OH.cls_inputs((2, 25, 5), "randn3")
    with_fg = _cls_abi(ops, score.cuda(), g.cuda(), OH.FOCAL[0], True)
    without = _cls_abi(ops, score.cuda(), g.cuda(), OH.FOCAL[0], False)
    assert torch.equal(with_fg[0], without[0]) and torch.equal(with_fg[2], without[2]) and without[1] is None


# ================================================================================================================ response maps
@functools.lru_cache(maxsize=None)
def _maps_ref(case, mode):
    h, w, S = case
    score, _, d_relu, d_sig = OH.maps_inputs(case)
    dr = d_relu if mode in ("relu", "both") else None
    ds = d_sig if mode in ("sig", "both") else None
    return OH.maps(score, h, w, S, dr, ds), OH.maps_bounds(score, h, w, S, dr, ds)


def _diag(d, h, w):
    return OH.maps_diag(d, h, w)


@pytest.mark.parametrize("case", OH.MAPS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_response_maps(case):
    from tris_amd import ops
    h, w, S = case
    B = OH.MAPS_B
    score, g_cls, d_relu, d_sig = OH.maps_inputs(case)
    (v, relu_ref, sig_ref, _), (b_relu, b_sig, _) = _maps_ref(case, "both")
    sd = score.cuda()
    _, _, relu, sig = ops.score_heads(sd, h, w, S, True)
    _inside(relu, relu_ref, b_relu, "relu map")
    _inside(sig, sig_ref, b_sig, "sigmoid map")
    with torch.no_grad():
        assert torch.equal(ops.score_heads(sd, h, w, S, False), relu), "eval path (sig_map == NULL) differs from the training map"
    # bilinear.h's claim: the map is the NCHW resize of the diagonal, bit for bit (on an all-positive diagonal the relu is the identity)
    assert torch.equal(relu, torch.relu(ops.resize_bilinear(_diag(sd, h, w).contiguous(), (S, S), False)))
    pos = sd.abs() + 0.5
    assert torch.equal(ops.score_heads(pos, h, w, S, False), ops.resize_bilinear(_diag(pos, h, w).contiguous(), (S, S), False))
    # backward: adds onto what cls_head_bwd wrote
    st = ops._stream()
    gd, drd, dsd = g_cls.cuda(), d_relu.cuda(), d_sig.cuda()
    base = torch.empty_like(sd)
    ops.call("tris_cls_head_bwd_f32", ops.P(sd), ops.P(gd), ops.P(base), B, h * w, B, 3.0, 0.01, st)
    offdiag = torch.ones(B, h * w, B, dtype=torch.bool)
    for i in range(B):
        offdiag[i, :, i] = False
    totals = {}
    for mode in ("relu", "sig", "both"):
        (_, _, _, d_ref), (_, _, b_bwd) = _maps_ref(case, mode)
        runs = []
        for _ in range(2):
            tot = base.clone()
            ops.call("tris_maps_bwd_f32", ops.P(sd), ops.P(drd) if mode != "sig" else None, ops.P(dsd) if mode != "relu" else None,
                     ops.P(tot), B, h, w, B, S, st)
            runs.append(tot)
        assert torch.equal(runs[0], runs[1]), f"{mode}: two launches differ"
        tot = totals[mode] = runs[0]
        assert torch.equal(tot.cpu()[offdiag], base.cpu()[offdiag]), f"{mode}: an entry off the diagonal changed"
        want = base.double().cpu() + d_ref                                  # the fp64 sum
        bound = b_bwd + U * _diag(want, h, w).abs()                         # (+ the rounding of the float32 accumulation)
        _inside(_diag(tot, h, w), _diag(want, h, w), bound, f"dscore diagonal [{mode}]")
    # the wrapper's backward is the same two launches
    s = sd.clone().requires_grad_(True)
    cls_out, _, r, sg = ops.score_heads(s, h, w, S, True)
    torch.autograd.backward([cls_out, r, sg], [gd, drd, dsd])
    assert torch.equal(s.grad, totals["both"])


# ================================================================================================================ bilinear family
@functools.lru_cache(maxsize=None)
def _resize_ref(case, planes):
    Hi, Wi, Ho, Wo, align = case
    x, g = OH.resize_inputs(case, planes)
    return (OH.resize(x, (Ho, Wo), align), OH.resize_adjoint(g, (Hi, Wi), align), OH.resize_fwd_bound(x),
            OH.resize_bwd_bound(g, (Hi, Wi), align))


def _resize_case(case, planes=2):
    from tris_amd import ops
    Hi, Wi, Ho, Wo, align = case
    x, g = OH.resize_inputs(case, planes)
    y_ref, dx_ref, bf, bb = _resize_ref(case, planes)
    xd, gd = x[None].cuda().requires_grad_(True), g[None].cuda()
    y = ops.resize_bilinear(xd, (Ho, Wo), align)
    assert y.shape == (1, planes, Ho, Wo)
    y.backward(gd)
    _inside(y[0], y_ref, bf, "forward")
    _inside(xd.grad[0], dx_ref, bb, "backward")
    dx2 = torch.empty_like(xd.grad)
    ops.call("tris_resize_bilinear_bwd_f32", ops.P(gd), ops.P(dx2), planes, Hi, Wi, Ho, Wo, int(align), ops._stream())
    assert torch.equal(dx2, xd.grad), "two launches of the backward differ"


def _rid(c):
    return f"{c[0]}x{c[1]}-{c[2]}x{c[3]}" + ("-ac" if len(c) > 4 and c[4] else "")


@pytest.mark.parametrize("case", OH.resize_cases(), ids=_rid)
def test_resize_sweep(case):
    _resize_case(case)


def test_resize_past_the_grid_cap():
    _resize_case(OH.GRID_CAP_CASE[1:], OH.GRID_CAP_CASE[0])


@pytest.mark.parametrize("case", OH.nhwc_cases(), ids=_rid)
def test_upsample_nhwc_sweep(case):
    from tris_amd import ops
    Hi, Wi, Ho, Wo = case
    x, skip, d_up, d_sum = OH.nhwc_inputs(case)
    B, C = x.shape[0], x.shape[3]
    xn = x.permute(0, 3, 1, 2)                                               # [B,C,Hi,Wi]
    up_ref = OH.resize(xn, (Ho, Wo), False).permute(0, 2, 3, 1)
    bf = OH.resize_fwd_bound(xn).permute(0, 2, 3, 1)                         # [B,1,1,C]
    xd, sk = x.cuda().requires_grad_(True), skip.cuda()
    up, s = ops.upsample_nhwc(xd, (Ho, Wo), skip=sk)
    _inside(up, up_ref, bf, "up")
    s_ref = up_ref + skip.double()
    _inside(s, s_ref, bf + U * s_ref.abs(), "up + skip")
    with torch.no_grad():
        assert torch.equal(ops.upsample_nhwc(xd.detach(), (Ho, Wo)), up.detach())
        nchw = ops.resize_bilinear(xn.contiguous().cuda(), (Ho, Wo), False)
    assert torch.equal(nchw.permute(0, 2, 3, 1), up.detach()), "channels-last and NCHW resize differ"
    st = ops._stream()
    du, dsm = d_up.cuda(), d_sum.cuda()
    got = {}
    for mode, gu, gs in (("up", du, None), ("sum", None, dsm), ("both", du, dsm)):
        g64 = (d_up.double() if gu is not None else 0) + (d_sum.double() if gs is not None else 0)
        gn = g64.permute(0, 3, 1, 2)
        ref = OH.resize_adjoint(gn, (Hi, Wi), False).permute(0, 2, 3, 1)
        bound = OH.resize_bwd_bound(gn, (Hi, Wi), False)
        if mode == "both":                                                   # d_up + d_sum is formed in float32 first
            bound = bound + U * OH.resize_adjoint(gn.abs(), (Hi, Wi), False)
        runs = []
        for _ in range(2):
            dx = torch.empty(B, Hi, Wi, C, device="cuda")
            ops.call("tris_upsample_nhwc_bwd_f32", ops.P(gu), ops.P(gs), ops.P(dx), B, Hi, Wi, Ho, Wo, C, st)
            runs.append(dx)
        assert torch.equal(runs[0], runs[1]), f"{mode}: two launches differ"
        _inside(runs[0], ref, bound.permute(0, 2, 3, 1), f"dx [{mode}]")
        got[mode] = runs[0]
    torch.autograd.backward([up, s], [du, dsm])
    assert torch.equal(xd.grad, got["both"])


# ================================================================================================================ patches, tokens
@pytest.mark.parametrize("case", OH.FG_CASES, ids=lambda c: "x".join(map(str, c)))
def test_fg_patches(case):
    from tris_amd import ops
    B, C, R, ps = case
    gen = torch.Generator().manual_seed(B * 1000 + R)
    cam, img = torch.randn(B, 1, R, R, generator=gen), torch.randn(B, C, R, R, generator=gen)
    dp = torch.randn(B, (R // ps) ** 2, C * ps * ps, generator=gen)
    cd = cam.cuda().requires_grad_(True)
    out = ops.fg_patches(cd, img.cuda(), ps)
    assert torch.equal(out.detach().cpu(), OH.fg_layout(cam * img, ps)), "forward is not the float32 product, laid out"
    dpd, imd = dp.cuda(), img.cuda()
    out.backward(dpd)
    terms = OH.fg_unlayout(dp.double(), C, R, ps) * img.double()             # [B,C,R,R]
    _inside(cd.grad, terms.sum(1, keepdim=True), C * U * terms.abs().sum(1, keepdim=True), "dcam")
    d2 = torch.empty_like(cd.grad)
    ops.call("tris_fg_patch_bwd_f32", ops.P(dpd), ops.P(imd), ops.P(d2), B, C, R, ps, ops._stream())
    assert torch.equal(d2, cd.grad), "two launches of the backward differ"


@pytest.mark.parametrize("case", OH.VIT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_vit_assemble(case):
    from tris_amd import ops
    B, T, W = case
    gen = torch.Generator().manual_seed(T * 100 + W)
    emb, cls, pos = torch.randn(B, T - 1, W, generator=gen), torch.randn(W, generator=gen), torch.randn(T, W, generator=gen)
    dx = torch.randn(B, T, W, generator=gen)
    grads = []
    for _ in range(2):
        e, c, p = (t.cuda().requires_grad_(True) for t in (emb, cls, pos))
        x = ops.vit_assemble(e, c, p)
        x.backward(dx.cuda())
        grads.append((e.grad, c.grad, p.grad))
    assert torch.equal(x.detach().cpu(), torch.cat([cls.expand(B, 1, W), emb], 1) + pos), "forward is not the float32 sum"
    de, dc, dpos = grads[0]
    assert torch.equal(de.cpu(), dx[:, 1:]), "demb is not the slice of dx"
    ref, mag = dx.double().sum(0), dx.double().abs().sum(0)                  # any summation order: (B - 1) U sum|terms|
    _inside(dpos, ref, B * U * mag, "dpos")
    _inside(dc, ref[0], B * U * mag[0], "dcls")
    assert all(torch.equal(a, b) for a, b in zip(grads[0], grads[1])), "two launches of the backward differ"


# ================================================================================================================ contracts
SLOT = 1 << 18


class _Arena:
    """one zeroed buffer; every pointer of a refused call points well inside it, further from both ends and from the other
    pointers than any access the kernels could make at the small sizes used here, guard or no guard"""

    def __init__(self):
        self.buf = torch.zeros(1 << 22, device="cuda")

    def p(self, k):
        assert 0 <= k < 8
        return self.buf.data_ptr() + 4 * ((1 << 20) + k * SLOT)

    def untouched(self):
        torch.cuda.synchronize()
        return not bool(self.buf.any())


def _refused(ops, name, *args):
    from tris_amd._lib import TrisHipError
    with pytest.raises(TrisHipError, match=r"hipError_t 1$"):                # hipErrorInvalidValue
        ops.call(name, *args, ops._stream())


def _each_bad(good, positions, bad=(0, -1)):
    """`good` with one of its size arguments replaced by a non-positive value, every position in turn"""
    for k in positions:
        for v in bad:
            yield good[:k] + (v,) + good[k + 1:]


def test_entry_points_refuse_bad_sizes():
    from tris_amd import ops
    A = _Arena()
    a, b, c, d = (A.p(k) for k in range(4))
    for args in _each_bad((a, b, c, 2, 4, 3, 3.0, 0.01), (3, 4, 5)):
        _refused(ops, "tris_cls_head_fwd_f32", *args)
        _refused(ops, "tris_cls_head_bwd_f32", *args)
    for args in _each_bad((a, b, c, 2, 2, 2, 2, 4), (3, 4, 5, 6, 7)):         # B, h, w, N, S
        _refused(ops, "tris_maps_fwd_f32", *args)
    for args in _each_bad((a, b, c, d, 2, 2, 2, 2, 4), (4, 5, 6, 7, 8)):
        _refused(ops, "tris_maps_bwd_f32", *args)
    for args in _each_bad((a, b, 2, 3, 3, 4, 4, 0), (2, 3, 4, 5, 6)):         # planes, Hi, Wi, Ho, Wo
        _refused(ops, "tris_resize_bilinear_fwd_f32", *args)
        _refused(ops, "tris_resize_bilinear_bwd_f32", *args)
    for args in _each_bad((a, b, c, 2, 3, 8, 2), (3, 4, 5, 6)):               # B, C, R, ps
        _refused(ops, "tris_fg_patch_fwd_f32", *args)
        _refused(ops, "tris_fg_patch_bwd_f32", *args)
    for args in _each_bad((2, 3, 4), (0, 1, 2)):                               # B, T, W
        _refused(ops, "tris_vit_assemble_fwd_f32", a, b, c, d, *args)
        _refused(ops, "tris_vit_assemble_bwd_f32", a, b, *args)
    assert A.untouched()


def test_entry_points_refuse_what_the_kernels_cannot_index():
    from tris_amd import ops
    A = _Arena()
    a, b, c, d = (A.p(k) for k in range(4))
    # fewer sentences than images: the diagonal score[i][.][i] and cls_fg[i] do not exist
    _refused(ops, "tris_maps_fwd_f32", a, b, c, 3, 2, 2, 2, 4)
    _refused(ops, "tris_maps_fwd_f32", a, b, None, 3, 2, 2, 2, 4)
    _refused(ops, "tris_maps_bwd_f32", a, b, c, d, 3, 2, 2, 2, 4)
    _refused(ops, "tris_cls_head_fwd_f32", a, b, c, 3, 4, 2, 3.0, 0.01)
    # patches that do not tile the image; a token sequence without a patch
    for R, ps in ((5, 2), (8, 3), (4, 8)):
        _refused(ops, "tris_fg_patch_fwd_f32", a, b, c, 1, 1, R, ps)
        _refused(ops, "tris_fg_patch_bwd_f32", a, b, c, 1, 1, R, ps)
    _refused(ops, "tris_vit_assemble_fwd_f32", a, b, c, d, 2, 1, 4)
    _refused(ops, "tris_vit_assemble_bwd_f32", a, b, 2, 1, 4)
    # the limits the entry points already had: 1024 pixels of LDS for the maps, 150 KB for the class head
    _refused(ops, "tris_maps_fwd_f32", a, b, c, 1, 33, 32, 1, 4)
    _refused(ops, "tris_maps_bwd_f32", a, b, c, d, 1, 32, 33, 1, 4)
    B, P, N = OH.CLS_REFUSED
    _refused(ops, "tris_cls_head_fwd_f32", a, b, c, B, P, N, 3.0, 0.01)
    _refused(ops, "tris_cls_head_bwd_f32", a, b, c, B, P, N, 3.0, 0.01)
    assert A.untouched()
    # without cls_fg the class head takes fewer sentences than images
    score, g = torch.randn(3, 4, 2).cuda(), torch.randn(3, 2).cuda()
    out = torch.empty(3, 2, device="cuda")
    ops.call("tris_cls_head_fwd_f32", ops.P(score), ops.P(out), None, 3, 4, 2, 3.0, 0.01, ops._stream())
    ref = OH.cls_head(score.cpu(), g.cpu(), 3.0, 0.01)[0]
    assert float(_err(out, ref).max()) < 1e-4


def test_wrappers_refuse_bad_shapes():
    from tris_amd import ops
    score = torch.zeros(2, 12, 2, device="cuda")
    for h, w in ((3, 3), (4, 4), (12, 2)):
        with pytest.raises(ValueError):
            ops.score_heads(score, h, w, 8, True)
        with pytest.raises(ValueError):
            ops.score_heads(score, h, w, 8, False)
    img = torch.zeros(2, 3, 8, 8, device="cuda")
    z = lambda *s: torch.zeros(*s, device="cuda")
    for cam, im, ps in ((z(2, 1, 8, 6), z(2, 3, 8, 6), 2), (z(2, 1, 6, 8), z(2, 3, 6, 8), 2), (z(2, 1, 8, 6), img, 2),
                        (z(2, 3, 8, 8), img, 2), (z(1, 1, 8, 8), img, 2), (z(2, 1, 8, 8), img, 3)):
        with pytest.raises(ValueError):
            ops.fg_patches(cam, im, ps)


if __name__ == "__main__":
    # `python tests/test_gpu_heads.py > profiles/heads_parity_floor.txt` on the MI355X: the class-head figures per case
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tris_amd import ops as _ops
    print("# class head (csrc/heads.hip) against fp64: err_hip / err_cpu32 per output, MI355X.  Asserted by tests/test_gpu_heads.py:")
    print("# err_hip <= max(4 * err_cpu32, 32 * 2^-24 * max|ref|).  `floor` marks an output whose err_cpu32 is under the absolute term.")
    print("# A ratio above 4 on a `floor` line: err_cpu32 is far below one ulp of max|ref| (the CPU happened to round most entries")
    print("# exactly) while err_hip is one or two ulp.  `of tol` is err_hip / tolerance.")
    print("# B P N | focal_p focal_c | values | output | err_hip err_cpu32 ratio | of tol")
    worst, worst_tol = 0.0, 0.0
    for shape in OH.CLS_SHAPES:
        for focal in OH.FOCAL:
            for kind in OH.CLS_KINDS:
                fig, _, _ = cls_measure(_ops, shape, kind, focal)
                for name, (eh, e32, tol) in fig.items():
                    at_floor = 4.0 * e32 < tol
                    ratio = eh / e32 if e32 > 0 else float("nan")
                    if not at_floor:
                        worst = max(worst, ratio)
                    worst_tol = max(worst_tol, eh / tol)
                    print(f"{shape[0]:3d} {shape[1]:4d} {shape[2]:3d} | {focal[0]:g} {focal[1]:g} | {kind:8s} | {name:8s} | "
                          f"{eh:.3e} {e32:.3e} {ratio:6.2f}{' floor' if at_floor else ''} | {eh / tol:.3f}{'  EXCEEDS' if eh > tol else ''}")
    print(f"# largest ratio among outputs above the floor: {worst:.2f}; largest err_hip / tolerance: {worst_tol:.3f}")
