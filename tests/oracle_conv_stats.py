"""Yardstick of tests/test_gpu_conv_stats.py (host only: torch CPU, fp64): the 3x3 convolution family -- forward, data gradient,
weight gradient, and the forms that fold relu(bn(x)) into their staging -- at operand statistics other than iid unit-variance noise.

  * operand generators by KIND, seeded from the kind's name (as `_adversarial` of tests/test_gpu_h2.py);
  * fp64 references from torch.nn.functional.conv2d and autograd, and the same products of the operands' ABSOLUTE values;
  * the error of a result per GROUP (its first and its last dimension: image / output channel for y, image / input channel for dx,
    output channel / input channel for dw), ||err||_2 / ||ref||_2 over the group, with each kind's SMALL groups -- those that sit far
    below their tensor's maximum -- judged apart from the rest;
  * the a-priori elementwise bound of an fp32-accumulating product, |err| <= gamma_n (|a| (*) |b|), gamma_n = n u / (1 - n u), with
    u = 2^-23: the unit roundoff of a CHOPPING fp32 accumulate, so it holds whatever the rounding and the summation order of the
    arithmetic under test are.  n = the number of terms of one output element: 9 Cin (y), 9 Cout (dx), B Ho Wo (dw);
  * emulations of the h2 operand rounding (hi + lo' 2^-11, `_h2_round` of tests/test_gpu_planes.py) and of the mistake a staging
    path could make -- the residual piece stored WITHOUT its 2^11 pre-scale -- for tests/test_conv_stats_host.py.

Layouts are the kernels': x [B,H,W,Cin], w [Cout,3,3,Cin], dy [B,Ho,Wo,Cout]; padding 1."""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

U = 2.0 ** -23

KINDS = ("image_2^-20", "image_2^-24", "filters_2^-20", "cin_2^-20", "outlier_1e4", "gains_anti", "student_t", "gradient_like")
STEM_KINDS = ("image_2^-20", "image_2^-24", "outlier_1e4")
BNIN_KINDS = ("affine_2^-12", "affine_gains_anti", "x_student_t")

# B, H, W, Cin, Cout: the smallest shapes each form accepts with B >= 2
IMPLICIT = ((2, 16, 16, 32, 64), (2, 9, 7, 128, 16))        # (the second: no direct kernel takes it)
IMPLICIT_S2 = ((2, 17, 25, 64, 64),)                        # stride-2 forward
STEM = ((2, 32, 32, 3, 32),)                                # stride 2, forward only
DIRECT_FWD = {1: (2, 32, 32, 32, 128), 2: (2, 32, 16, 48, 64), 3: (3, 16, 16, 32, 32), 4: (3, 10, 10, 64, 128), 5: (5, 10, 10, 64, 128),
              6: (2, 8, 32, 32, 128)}                       # configuration of the direct forward / data-gradient kernel -> shape
# Cin = 48 above is no multiple of 32: the fast kernels do not serve that forward in h2 (gemm_params.h gemm_fast_ok), an arming is
# dropped and configuration 2 runs it in x3.  The same map with 64 input channels puts the forward of configuration 2 through h2.
DIRECT_FWD_H2 = {2: (2, 32, 16, 64, 64)}
# a data gradient has Cin output columns, and configurations 1, 4, 5, 6 want more than 64: at the shapes above the data gradient runs
# through configuration 2 or 3 or the implicit GEMM.  The same shapes with Cin and Cout exchanged put it through these four as well.
DIRECT_DGRAD = {cfg: DIRECT_FWD[cfg][:3] + (DIRECT_FWD[cfg][4], DIRECT_FWD[cfg][3]) for cfg in (1, 4, 5, 6)}
DIRECT_WGRAD = {1: (2, 8, 32, 32, 32), 2: (2, 16, 16, 32, 64), 3: (2, 6, 32, 64, 64), 4: (2, 8, 32, 64, 64), 5: (2, 8, 40, 32, 64)}
BNIN = ((2, 16, 32, 32, 32), (3, 16, 16, 64, 64))
WORKLOAD_ROWS = 48 * 80 * 80                                # rows of the widest BatchNorm of the training workload at batch 48


def gamma_n(n):
    return n * U / (1.0 - n * U)


def _gen(kind):
    return torch.Generator().manual_seed(sum(map(ord, kind)))


def _student_t2(shape, g):
    """Student's t with 2 degrees of freedom from the generator: z / sqrt(chi2_2 / 2), chi2_2 / 2 = -ln u"""
    z = torch.randn(shape, generator=g)
    e = -torch.log(torch.rand(shape, generator=g).clamp_min(2.0 ** -24))
    return z / e.sqrt()


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


@functools.lru_cache(maxsize=None)
def operands(kind, shape, stride=1):
    """-> x, w, dy (fp32, CPU; dy None for a strided forward) and `small`: per result the masks (first dimension, last dimension) of the
    groups that sit far below their tensor's maximum (None: no such group along that dimension)."""
    B, H, W, Cin, Cout = shape
    Ho, Wo = out_hw(H, W, stride)
    g = _gen(kind)
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, 3, 3, Cin, generator=g) * 0.1
    dy = torch.randn(B, Ho, Wo, Cout, generator=g)
    odd_img = torch.arange(B) % 2 == 1
    small = {"y": (None, None), "dx": (None, None), "dw": (None, None)}
    if kind == "image_2^-20":
        x[1::2] *= 2.0 ** -20
        dy[1::2] *= 2.0 ** -20
        small = {"y": (odd_img, None), "dx": (odd_img, None), "dw": (None, None)}
    elif kind == "image_2^-24":
        x[1::2] *= 2.0 ** -24
        small = {"y": (odd_img, None), "dx": (None, None), "dw": (None, None)}
    elif kind == "filters_2^-20":
        w[1::3] *= 2.0 ** -20
        dy[..., 1::3] *= 2.0 ** -20
        f = torch.arange(Cout) % 3 == 1
        small = {"y": (None, f), "dx": (None, None), "dw": (f, None)}
    elif kind == "cin_2^-20":
        # (the weight gradient does not read w: there the even input channels are merely judged as a group of their own)
        w[..., ::2] *= 2.0 ** -20
        c = torch.arange(Cin) % 2 == 0
        small = {"y": (None, None), "dx": (None, c), "dw": (None, c)}
    elif kind == "outlier_1e4":
        x[1, 5, 3, 2] = 1e4
        w[3, 1, 2, 1] = -1e4
        dy[0, 2, 4, 7] = 1e4
    elif kind == "gains_anti":
        ga = torch.exp2(torch.rand(Cin, generator=g) * 16 - 8)
        x *= ga
        w /= ga
    elif kind == "student_t":
        x = _student_t2(x.shape, g)
        w = _student_t2(w.shape, g) * 0.02
        dy = _student_t2(dy.shape, g)
    elif kind == "gradient_like":
        dy = torch.randn(dy.shape, generator=g) * 1e-9
        idx = torch.randint(0, dy.numel(), (20,), generator=g)
        dy.view(-1)[idx] = 1e-3
    else:
        raise KeyError(kind)
    return SimpleNamespace(kind=kind, shape=shape, stride=stride, x=x.contiguous(), w=w.contiguous(),
                           dy=dy.contiguous() if stride == 1 else None, small=small)


def products(x, w, dy, stride=1, dtype=torch.float64):
    """y, dx, dw of the 3x3 convolution in `dtype` on the CPU (dy None: y only), channels-last like the operands"""
    xn = x.to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(dy is not None)
    wn = w.to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(dy is not None)
    y = F.conv2d(xn, wn, stride=stride, padding=1)
    out = {"y": y.detach().permute(0, 2, 3, 1).contiguous()}
    if dy is not None:
        gx, gw = torch.autograd.grad(y, (xn, wn), dy.to(dtype).permute(0, 3, 1, 2).contiguous())
        out["dx"] = gx.permute(0, 2, 3, 1).contiguous()
        out["dw"] = gw.permute(0, 2, 3, 1).contiguous()
    return out


def terms(shape, stride=1):
    B, H, W, Cin, Cout = shape
    Ho, Wo = out_hw(H, W, stride)
    return {"y": 9 * Cin, "dx": 9 * Cout, "dw": B * Ho * Wo}


@functools.lru_cache(maxsize=None)
def reference(kind, shape, stride=1):
    """fp64 references of the case and the elementwise a-priori bound gamma_n (|a| (*) |b|) of each result"""
    c = operands(kind, shape, stride)
    ref = products(c.x, c.w, c.dy, stride)
    mag = products(c.x.abs(), c.w.abs(), None if c.dy is None else c.dy.abs(), stride)
    n = terms(shape, stride)
    return SimpleNamespace(ref=ref, bound={k: gamma_n(n[k]) * mag[k] for k in ref})


def bound_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound: <= 1 says the result is an fp32-accumulated product of THESE operands"""
    err = (got.double() - ref).abs()
    return float((err / bound.clamp_min(1e-300)).max())


def group_errors(got, ref):
    """relative L2 error per group along the first and along the last dimension"""
    d = got.double() - ref
    first = d.flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)
    last = d.flatten(0, -2).norm(dim=0) / ref.flatten(0, -2).norm(dim=0)
    return first, last


def selections(small, n_first, n_last):
    """[(axis, name, mask)]: along each dimension the small groups and the rest, or all groups where the kind names none"""
    out = []
    for axis, (m, n) in enumerate(zip(small, (n_first, n_last))):
        if m is None:
            out.append((axis, "all", torch.ones(n, dtype=torch.bool)))
        else:
            out += [(axis, "small", m), (axis, "rest", ~m)]
    return out


def criterion(got, yard, ref, small, factor):
    """The group criterion: maximum and median of the group errors of `got` <= factor x those of `yard` on the same groups, small groups
    and the rest apart.  -> (violations [(axis, selection, statistic, got, yardstick)], worst ratio over everything that was compared)"""
    eg, ey = group_errors(got, ref), group_errors(yard, ref)
    bad, worst = [], 0.0
    for axis, name, m in selections(small, eg[0].numel(), eg[1].numel()):
        for stat, fn in (("max", torch.max), ("median", torch.median)):
            a, b = float(fn(eg[axis][m])), float(fn(ey[axis][m]))
            worst = max(worst, a / b if b > 0 else (0.0 if a == 0 else math.inf))
            if not a <= factor * b:
                bad.append((axis, name, stat, a, b))
    return bad, worst


# ---- the h2 operand rounding and its mutation ------------------------------------------------------------------------------------
def h2_round(x, amax, prescale=True):
    """the value an h2 operand holds at the scale of `amax` (its tensor's largest magnitude or an upper bound of it): hi + lo' 2^-11,
    hi = fp16(x s), lo' = fp16((x s - hi) 2^11), s = 2^(13 - floor(log2 amax)).  prescale=False: the residual piece stored unscaled,
    lo = fp16(x s - hi) -- fp16's subnormal spacing 2^-24 then cuts every element below 2^-13 of the tensor's scale short."""
    s = 2.0 ** (13 - math.floor(math.log2(amax)))
    xs = (x.double() * s).float()
    hi = xs.half()
    k = 2048.0 if prescale else 1.0
    lo = ((xs - hi.float()) * k).half()
    return ((hi.double() + lo.double() / k) / s).float()


def amax(t):
    return float(t.abs().max())


def emulated(case, prescale=True, x_amax=None):
    """the three products in fp64 of h2-rounded operands (x at the scale of x_amax where given: a bound word)"""
    x = h2_round(case.x, amax(case.x) if x_amax is None else x_amax, prescale)
    w = h2_round(case.w, amax(case.w), prescale)
    dy = None if case.dy is None else h2_round(case.dy, amax(case.dy), prescale)
    return products(x, w, dy, case.stride)


def close(a, b, tol):
    """the yardstick of the existing convolution tests (tests/test_gpu_ops.py): max |err| <= tol max(1, max |ref|)"""
    return float((a.double() - b.double()).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ---- conv3x3(relu(bn(x))) with the BatchNorm folded into the staging -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bnin_operands(kind, shape):
    """x (the BatchNorm's raw input), its train-mode mean / invstd as floats, gamma, beta, w, dy.  A per-channel scale on x does not
    survive the normalisation, so the statistics sit in the affine parameters."""
    B, H, W, Cin, Cout = shape
    g = _gen(kind)
    x = torch.randn(B, H, W, Cin, generator=g) * 2 + 0.3
    gamma, beta = 1 + 0.3 * torch.randn(Cin, generator=g), 0.2 * torch.randn(Cin, generator=g)
    w = torch.randn(Cout, 3, 3, Cin, generator=g) * 0.1
    dy = torch.randn(B, H, W, Cout, generator=g)
    small = {"y": (None, None), "dw": (None, None)}
    if kind == "affine_2^-12":
        gamma[::2] *= 2.0 ** -12
        beta[::2] *= 2.0 ** -12
        w[..., ::2] *= 2.0 ** 12
        small["dw"] = (None, torch.arange(Cin) % 2 == 0)
    elif kind == "affine_gains_anti":
        ga = torch.exp2(torch.rand(Cin, generator=g) * 16 - 8)
        gamma *= ga
        beta *= ga
        w /= ga
    elif kind == "x_student_t":
        x = _student_t2(x.shape, g)
    else:
        raise KeyError(kind)
    x2 = x.reshape(-1, Cin)
    mean = x2.mean(0).contiguous()
    invstd = torch.rsqrt(x2.var(0, unbiased=False) + 1e-5).contiguous()
    return SimpleNamespace(kind=kind, shape=shape, stride=1, x=x.contiguous(), mean=mean, invstd=invstd, gamma=gamma.contiguous(),
                           beta=beta.contiguous(), w=w.contiguous(), dy=dy.contiguous(), small=small)


def bn_relu(c, dtype):
    """relu((x - mean) (invstd gamma) + beta) in `dtype` from the float parameters (tris_bn_apply_f32's expression)"""
    t = lambda v: v.to(dtype)
    return torch.relu((t(c.x) - t(c.mean)) * (t(c.invstd) * t(c.gamma)) + t(c.beta))


def bn_bound(c, rows):
    """the value of tris_bn_out_bound_f32's word: max_c |gamma_c| sqrt(rows - 1) + |beta_c| (Samuelson)"""
    return float((c.gamma.abs().double() * math.sqrt(rows - 1) + c.beta.abs().double()).max())


@functools.lru_cache(maxsize=None)
def bnin_reference(kind, shape):
    """fp64 references y = conv(act, w), dw = dy (x) act with act = relu(bn(x)) in fp64, and the a-priori bound of a product whose
    activation operand was FORMED in fp32 by y = (x - mu) * sc + b with sc = invstd * gamma (csrc/norm.hip bn_apply_kernel, `one`; the
    same expression in wgrad3x3_direct_kernel's store_unit and gemm_fast.h's A_HALO staging -- NOT x * scale + shift, whose shift
    would carry mean * scale and cancel): the expression has at most four roundings, each relative to a partial result no larger
    than |x - mean| |invstd gamma| + |beta| (ReLU does not increase a difference), so |act32 - act| <= E = gamma_4 (|x - mean|
    |invstd gamma| + |beta|) and   |err| <= gamma_n (|act| (*) |b|) + (1 + gamma_n) (E (*) |b|)."""
    c = bnin_operands(kind, shape)
    act = bn_relu(c, torch.float64)
    d = lambda v: v.double()
    e_act = gamma_n(4) * ((d(c.x) - d(c.mean)).abs() * (d(c.invstd) * d(c.gamma)).abs() + d(c.beta).abs())
    ref = products(act, c.w, c.dy)
    mag = products(act, c.w.abs(), c.dy.abs())
    mag_e = products(e_act, c.w.abs(), c.dy.abs())
    n = terms(shape)
    return SimpleNamespace(act=act, ref={k: ref[k] for k in ("y", "dw")},
                           bound={k: gamma_n(n[k]) * mag[k] + (1 + gamma_n(n[k])) * mag_e[k] for k in ("y", "dw")})


def bnin_emulated(c, bound, prescale=True):
    """y and dw in fp64 of h2-rounded operands: the fp32 activation at the scale of the BOUND word, w and dy at their amax"""
    act = h2_round(bn_relu(c, torch.float32), bound, prescale)
    p = products(act, h2_round(c.w, amax(c.w), prescale), h2_round(c.dy, amax(c.dy), prescale))
    return {k: p[k] for k in ("y", "dw")}
