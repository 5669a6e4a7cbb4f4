"""fp64 restatement of the four row-wise normalisations -- LayerNorm and InstanceNorm (csrc/norm.hip: tris_layernorm_{fwd,bwd}_f32,
tris_instnorm_{fwd,bwd}_f32), l2norm and softmax (csrc/heads.hip: tris_l2norm_{fwd,bwd}_f32, tris_softmax_{fwd,bwd}_f32) -- the
inputs the kernel tests feed them, the error bounds those tests assert, and float32 restatements of the kernels with the wrong
variants (MUTATIONS) the bounds must reject.  Shared by tests/test_rownorm_host.py (CPU) and tests/test_gpu_rownorm.py.

References.  One float64 function per entry point, taking that entry point's float32 inputs as exact numbers.  The forward kernels
produce statistics (mean / rstd, mean / invstd, inv_norm) and use them: the statistics are held to the two-pass float64 statistics
of the input, the output to the float64 expression evaluated WITH THE STATISTICS THE DEVICE RETURNED (the kernel stores the very
floats it used), and -- LayerNorm, InstanceNorm -- the output once more to the pure float64 normalisation under the composed bound
    b_apply + (1 + 5 U) (|dy/dmean| b_mean + |dy/drstd| b_rstd + |gamma| b_mean b_rstd),   dy/dmean = -rstd gamma, dy/drstd = (x - mean) gamma
so a wrong but self-consistent statistic cannot pass.  The backward kernels take the saved statistics (and the saved Y) as inputs;
the ReLU mask is Y > 0 of the saved output, given to the reference, never recomputed.

Bounds.  Element-wise, one per output element, U = 2^-24 (unit roundoff of float32), TINY = 2^-126.  A float32 sum of terms t_j in any
order of depth at most d is within d U sum |t_j| of the exact sum (first order).  Each constant is the number of float32 roundings on
the path of that output plus one (second-order terms and the float64 work).  kw = ceil(W / 256), k = ceil(C / 64) (ceil(n / 64)),
n4 = ceil(P / 4), r4 = ceil(rpb / 4).

Device functions.  The build (csrc/build.sh) is -O3 without fast-math and hipcc rounds float32 `/` and sqrtf correctly by default:
one rounding each (the probe below confirms sqrtf at 1.000 U, the half ulp at the foot of a binade).  expf: tests/oracle_mha.py
charges the VALU kernels' expf (1 ulp: at most 2 U) inside (C_EXP + 1) U; C_EXPF is that sum, by import.  rsqrtf: the compiler's HIP
math header makes it a device-library call and neither it nor any document available to the build states its accuracy, so it was
measured on the MI355X (tools/rsqrtf_probe.hip, recorded in profiles/rownorm_parity_floor.txt: against float64 at 2^24 arguments
log-uniform over [2^-30, 2^30] the largest relative error, the rounding of the result included, is 1.574 U) and C_RSQ = 3.2 is twice
that, rounded up to one decimal: a property of one instruction sequence, not of a shape.  No other constant comes from a device run.

LayerNorm forward (one wave per row; a lane sums its float4s (3 additions), adds the quads of its kw trips, 6 butterfly steps):
  D = 3 + kw + 6
  mean  = fl(sum) / W: D roundings and the division            |mean - ref| <= (D + 2) U mean_j |x_j|      (not relative to |mean|)
  var^  = sum_j fl(fl(x_j - mean^)^2) / W: exactly, sum_j (x_j - mean^)^2 / W = var + (mean^ - mean)^2, so the mean's error enters
          at second order (+ b_mean^2); roundings: the subtraction (twice, it is squared), the square, D, / W, + eps = D + 5:
          t^ in [(var + eps)(1 - C_V U), (var + b_mean^2 + eps)(1 + C_V U)],  C_V = D + 6
  rstd  = rsqrtf(t^): 1 / sqrt is decreasing and convex, as oracle_bn.py uses for invstd:
          |rstd - ref| <= max(1 / sqrt(t_lo) - ref, ref - 1 / sqrt(t_hi)) + C_RSQ U / sqrt(t_lo)
  y     = ((x - mean) * rstd) * g + b given the stored mean, rstd: four roundings (three where the multiply-add is contracted)
          |y - ref| <= C_Y U (|p| + |b|),  p = (x - mean) rstd g,  C_Y = 5
LayerNorm backward (mean, rstd inputs): xh = fl(fl(x - mean) rstd) (2), dh = fl(dy g) (1),
  c1 = fl(sum dh) / W: dh, D, / W = D + 2                      e_c1 = (D + 3) U mean_j |dh_j|
  c2 = fl(sum dh xh) / W: dh, xh (2), the product, D, / W = D + 5     e_c2 = (D + 6) U mean_j |dh_j xh_j|
  dX = rstd (dh - c1 - xh c2) [+ extra]: the xh c2 path has 3 roundings, then two subtractions, the product with rstd, the add of extra = 7
          |dX - ref| <= |rstd| (e_c1 + |xh| e_c2) + C_DX U (|rstd| (|dh| + |c1| + |xh c2|) + |extra|),  C_DX = 8
  dgamma_w = sum_rows dy xh: three roundings per term; float32 over the r4 rows a wave walks, three float32 additions across the
          waves, float64 over the blocks (part_finalize_kernel<float>), one rounding = 3 + r4 + 3 + 1
          |dgamma - ref| <= (r4 + 8) U sum_rows |dy xh|
  dbeta_w  = sum_rows dy: the same without the per-term roundings     |dbeta - ref| <= (r4 + 5) U sum_rows |dy|
  rpb is ln_bwd_rpb restated (ln_bwd_plan); the workspace is max(blocks, 512) rows of 2 W floats (ln_bwd_workspace_bytes).

InstanceNorm (block = (b, 64 channels) x 4 pixel groups; a thread sums its n4 pixels one after the other, three additions across the
groups): DI = n4 + 3
  mean: DI, / P                                                |mean - ref| <= (DI + 2) U mean_p |x_p|
  var^: as above with C_V = DI + 6; invstd = rsqrtf(var^ + eps): the same convexity bound
  o = (x - mean) * is * g + be: four roundings (three contracted); max(., 0) cannot grow the error     C_Y = 5
  backward (mean, invstd, Y inputs; g = dy under the given mask):
  s0 = sum_p g (dbeta_part): DI                                |s0 - ref| <= (DI + 1) U sum_p |g|
  s1 = sum_p (g (x - mean)) is (dgamma_part): 3 per term, DI   |s1 - ref| <= (DI + 4) U sum_p |g xh|
  d  = ga * is * (g - s0 ip - xh s1 ip), ip = fl(1 / P): s0 ip carries e_s0 / P and 2 roundings; xh s1 ip carries |xh| e_s1 / P and
       2 (xh) + 1 + 1 (ip) + 1 = 5; two subtractions; ga * is; the last product = 9
          |d - ref| <= |ga is| ((e_s0 + |xh| e_s1) / P + C_IDX U (|g| + |s0 / P| + |xh s1 / P|)),  C_IDX = 10

l2norm (a lane sums its k squares one after the other, 6 butterfly steps; no eps: the domain is row norms in [2^-40, 2^40]):
  s = sum v^2: the square, k + 6; sqrtf halves the relative error and rounds once; the reciprocal rounds once
          |inv - ref| <= ((k + 7) / 2 + 3) U ref
  y = x * iv given iv: one rounding                            |y - ref| <= 2 U |ref| + TINY
  backward (Y, inv_norm inputs): s = sum y dy: the product, k + 6      e_s = (k + 8) U sum |y dy|
  dX = (dy - y s) * iv: the product, the subtraction, the product     |dX - ref| <= |iv| (|y| e_s + 4 U (|dy| + |y s|)) + TINY

softmax (z = x scale, exact in float64; m = max_j fl(z_j), a shift that exact arithmetic does not see; a lane adds its k weights, 6
butterfly steps):
  the argument of the exponential is fl(fl(x scale) - m), or fl(x scale - m) where the compiler contracts: at most U |z_j| + U |z_j - m|
  in either form.  As tests/oracle_mha.py sets out, an absolute error e of the exponent is a relative error e of the weight:
          ew_j = U (|z_j| + |z_j - m|) + C_EXPF U                  (the charge grows with |x scale| and with |x scale - m|)
  S = sum_j w_j (>= 1: the maximum's weight is 1): A = sum_j p_j ew_j, k + 6 roundings; the division rounds once; a weight below
  2^-126 may be flushed, and so may the quotient:
          |y_j - ref| <= p_j (ew_j + A + (k + 8) U) + 2 TINY
  backward (Y input): s = sum y dy: e_s = (k + 8) U sum |y dy|;  dX = scale * y * (dy - s): the subtraction and two products
          |dX - ref| <= |scale y| (e_s + 4 U (|dy| + |s|)) + TINY

Nothing else here was fitted to device output; tests/test_rownorm_host.py checks that three float32 evaluations of every expression
on the CPU (left to right, pairwise, and the kernel's own grouping) stay inside the bounds, and that every mutation leaves them.
"Left to right" there means the expressions as written and every sum in the longest left-to-right runs that the depth of its bound
admits, the runs joined by halves (run_sum): a plain left-to-right sum of n terms has depth n - 1, which none of these kernels has
and no bound above is derived for (on the `outlier` rows it is measurably outside them).
"""
import functools

import torch

import oracle_mha

U = 2.0 ** -24
TINY = 2.0 ** -126
C_RSQ = 3.2                          # rsqrtf in U: twice the 1.574 U measured (profiles/rownorm_parity_floor.txt)
C_EXPF = oracle_mha.C_EXP + 1.0      # expf of the VALU kernels (1 ulp: at most 2 U), as tests/oracle_mha.py charges it
C_Y, C_DX, C_IDX = 5, 8, 10


def f32_scalar(v):
    """the float32 nearest to v, as a Python float: what a `float` argument of the C ABI receives"""
    return float(torch.tensor(v, dtype=torch.float64).float())


EPS = f32_scalar(1e-5)

LN_KINDS = ["randn", "offset", "const", "tiny", "outlier", "gamma", "dyoff"]
IN_KINDS = LN_KINDS
L2_KINDS = ["randn", "outlier", "scaled", "sparse"]
SM_KINDS = ["randn", "peaked", "flat", "wide", "late_max", "early_max", "dyoff"]
SM_SCALES = tuple(f32_scalar(s) for s in (1.0 / 32.0, 512.0 ** -0.5, 1.0, -1.0 / 32.0))     # (one negative: the maximum is of x scale)
# (rows, W): one live lane; two; a partial trip; 63 / 64 / 65 live vector lanes; three trips; the fourth trip, partial and full;
# one wave of a block, three, all four, ten blocks; rpb 5 with 410 blocks, a ragged last block, waves with two rows and with one;
# rpb 10, three rows per wave
LN_SHAPES = [(5, W) for W in (4, 8, 100, 252, 256, 260, 768, 1020, 1024)] + [(r, 512) for r in (1, 3, 4, 37)] + [(2049, 64), (5003, 8)]
LN_BLOCKS = (None, 128)              # the LN_BWD_BLOCKS option: unset (512) and 128
IN_SHAPES = [(1, 1, 4), (2, 2, 1), (2, 3, 63), (2, 4, 64), (2, 5, 65), (3, 100, 128), (2, 100, 1024), (1, 1600, 64)]
L2_SHAPES = [(5, C) for C in (1, 63, 64, 65, 1000, 1024)] + [(r, 512) for r in (1, 4, 50)]
SM_SHAPES = [(5, n) for n in (1, 2, 20, 63, 64, 65, 100, 130, 1600)] + [(r, 48) for r in (1, 4, 21)]

MUTATIONS = {
    "ln": ["onepass_var", "unbiased_var", "no_eps", "mean_over_padded_lanes", "bwd_no_c2", "bwd_c1_from_dy", "bwd_extra_dropped",
           "dgamma_no_ragged_block", "dgamma_wave0_only"],
    "in": ["unbiased_var", "group3_dropped", "mask_from_x", "bwd_no_s0"],
    "l2": ["eps_under_root", "bwd_no_projection"],
    "sm": ["scale_after_max", "max_first_trip", "bwd_no_scale", "bwd_s_first_trip"],
}


def f64(t):
    return None if t is None else t.detach().double().cpu()


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------- launch plans
def ln_bwd_plan(rows, blocks=None):
    """ln_bwd_rpb of csrc/norm.hip restated -> (rows per block, blocks); `blocks` is the LN_BWD_BLOCKS option (None: 512)"""
    target = 512 if blocks is None else min(512, max(1, blocks))
    rpb = max(cdiv(rows, target), 4 if target > 128 else 8)
    return rpb, cdiv(rows, rpb)


def ln_bwd_workspace_bytes(rows, W, blocks=None):
    return max(ln_bwd_plan(rows, blocks)[1], 512) * 2 * W * 4


def ln_depth(W):
    return 3 + cdiv(W, 256) + 6


# ------------------------------------------------------------------------------------------------------------------- inputs
def _gen(tag, kind, kinds, shape):
    seed = 40000 + 7919 * ("ln", "in", "l2", "sm").index(tag) + 131 * kinds.index(kind)
    for k, s in enumerate(shape):
        seed += (k + 1) * 17 * (s % 9973)
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def inputs(kernel, kind, shape):
    """-> dict of float32 tensors (shared between the tests: never written to).
    ln: x, dy, extra [rows, W]; gamma, beta [W]          in: x, dy [B, P, C]; gamma, beta [C] (a negative gamma in every kind)
    l2: x, dy [rows, C]                                   sm: x, dy [rows, n]"""
    kinds = {"ln": LN_KINDS, "in": IN_KINDS, "l2": L2_KINDS, "sm": SM_KINDS}[kernel]
    gen = _gen(kernel, kind, kinds, shape)
    rn = lambda *s: torch.randn(*s, generator=gen)
    if kernel in ("ln", "in"):
        if kernel == "ln":
            rows, W = shape
            red, n, idx = 1, W, torch.arange(rows)[:, None]                # statistics per row, over dim 1
        else:
            B, P, W = shape
            red, n, idx = 1, P, torch.arange(W)[None, None, :]             # statistics per (b, channel), over dim 1
        x, dy = rn(*shape), rn(*shape)
        c = torch.arange(W)
        gamma, beta = 1.0 + 0.5 * rn(W), rn(W)
        if kind == "offset":
            x = (x + torch.tensor([0.0, 10.0, 1e3, -1e3])[idx % 4]) * torch.tensor([1e-2, 1.0, 1e2])[idx % 3]
        elif kind == "const":
            x = torch.tensor([0.0, 1.0, 100.25])[idx % 3].expand(*shape).contiguous()
        elif kind == "tiny":
            x = x * 1e-6
        elif kind == "outlier":
            at = torch.randint(0, n, x.sum(red, keepdim=True).shape, generator=gen)
            x = x.scatter(red, at, 1e4 * torch.where(x.gather(red, at) < 0, -1.0, 1.0))
        elif kind == "gamma":
            gamma = torch.tensor([1e-3, 1.0, 1e3])[c % 3] * rn(W)
            gamma[0] = 0.0
            if W > 1:
                beta[1] = 0.0
        elif kind == "dyoff":
            dy = dy + 100.0
        dy[dy == 0] = 1.0
        gamma[(gamma == 0) & ((c != 0) | (kind != "gamma"))] = 1.0
        if kernel == "in":       # the ReLU mask follows the sign of gamma: negative gains at the odd channels (at the only one if C = 1)
            neg = (c % 2 == 1) if W > 1 else torch.ones(1, dtype=torch.bool)
            gamma = torch.where(neg, -gamma.abs(), gamma)
            return dict(x=x.contiguous(), dy=dy, gamma=gamma, beta=beta)
        return dict(x=x.contiguous(), dy=dy, extra=rn(*shape), gamma=gamma, beta=beta)
    rows, n = shape
    x, dy = rn(rows, n), rn(rows, n)
    r = torch.arange(rows)
    if kernel == "l2":
        x[x == 0] = 1.0
        if kind == "outlier":
            at = torch.randint(0, n, (rows, 1), generator=gen)
            x = x.scatter(1, at, 1e4 * torch.where(x.gather(1, at) < 0, -1.0, 1.0))
        elif kind == "scaled":       # row norms 2^-40 .. 2^40 across the rows
            e = torch.linspace(-40.0, 40.0, rows).round() if rows > 1 else torch.tensor([-40.0])
            x = (x.double() / x.double().norm(dim=1, keepdim=True) * (2.0 ** e.double())[:, None]).float()
        elif kind == "sparse":
            at = torch.randint(0, n, (rows, 1), generator=gen)
            x = torch.zeros(rows, n).scatter(1, at, x.gather(1, at))
        return dict(x=x.contiguous(), dy=dy)
    k = cdiv(n, 64)
    x = 3.0 * x
    if kind == "peaked":         # one logit 80 / scale above the rest: x holds the SCALED logits' shape, sm_x() divides by the scale
        x = x.scatter(1, torch.randint(0, n, (rows, 1), generator=gen), x.max(1, keepdim=True).values + 80.0)
    elif kind == "flat":
        x = torch.full((rows, n), 1.5)
    elif kind == "wide":         # scaled logits uniform over [-90, 0] below the maximum
        x = -90.0 * torch.rand(rows, n, generator=gen)
        x = x.scatter(1, torch.randint(0, n, (rows, 1), generator=gen), 0.0)
    elif kind == "late_max":     # the maximum in the last lane-trip, further above the rest than expf's range (a maximum taken
        x = x.scatter(1, (64 * (k - 1) + r % (n - 64 * (k - 1)))[:, None], 100.0)      # over fewer columns overflows)
    elif kind == "early_max":    # ... in the first
        x = x.scatter(1, (r % min(n, 64))[:, None], 100.0)
    elif kind == "dyoff":
        dy = dy + 100.0
    return dict(x=x.contiguous(), dy=dy)


def sm_x(kind, shape, scale):
    """the float32 logits of a softmax case: the stored shape of the SCALED logits divided by the scale (randn x 3 and dyoff: as stored)"""
    x = inputs("sm", kind, shape)["x"]
    return x if kind in ("randn", "dyoff") else (x.double() / scale).float()


# ------------------------------------------------------------------------------------------------------------------- statistics
def _norm_stats(x, dim, depth, eps):
    """two-pass float64 mean / variance / 1 / sqrt(var + eps) over `dim` and the bounds of the float32 mean and rsqrt"""
    x = f64(x)
    n = x.shape[dim]
    mean = x.mean(dim)
    var = ((x - mean.unsqueeze(dim)) ** 2).mean(dim)
    r = 1.0 / torch.sqrt(var + eps)
    b_mean = (depth + 2) * U * x.abs().mean(dim)
    cv = (depth + 6) * U
    r_lo = 1.0 / torch.sqrt((var + b_mean ** 2 + eps) * (1.0 + cv))
    r_hi = 1.0 / torch.sqrt((var + eps) * (1.0 - cv))
    b_r = torch.maximum(r_hi - r, r - r_lo) + C_RSQ * U * r_hi
    return mean, var, r, b_mean, b_r


def _apply(x, mean, r, gamma, beta, dim, relu=False):
    x = f64(x)
    sh = [1] * x.dim()
    sh[-1] = -1
    g, b = f64(gamma).view(sh), f64(beta).view(sh)
    p = (x - f64(mean).unsqueeze(dim)) * f64(r).unsqueeze(dim) * g
    z = p + b
    return (z.clamp_min(0.0) if relu else z), C_Y * U * (p.abs() + b.abs())


def _composed(x, gamma, beta, dim, depth, eps, relu=False):
    mean, var, r, b_mean, b_r = _norm_stats(x, dim, depth, eps)
    y, by = _apply(x, mean, r, gamma, beta, dim, relu)
    sh = [1] * f64(x).dim()
    sh[-1] = -1
    g = f64(gamma).view(sh).abs()
    bm, br = b_mean.unsqueeze(dim), b_r.unsqueeze(dim)
    d = (f64(x) - mean.unsqueeze(dim)).abs()
    return y, by + (1.0 + 5 * U) * (r.unsqueeze(dim) * g * bm + d * g * br + g * bm * br)


# ------------------------------------------------------------------------------------------------------------------- LayerNorm
def ln_stats(x, eps=EPS):
    """x [rows, W] -> (mean, rstd), (b_mean, b_rstd), float64 [rows]"""
    mean, _, r, b_mean, b_r = _norm_stats(x, 1, ln_depth(x.shape[1]), eps)
    return (mean, r), (b_mean, b_r)


def ln_apply(x, mean, rstd, gamma, beta):
    """-> y, bound with the GIVEN statistics"""
    return _apply(x, mean, rstd, gamma, beta, 1)


def ln_composed(x, gamma, beta, eps=EPS):
    """-> y of the pure float64 LayerNorm and the composed bound"""
    return _composed(x, gamma, beta, 1, ln_depth(x.shape[1]), eps)


def ln_bwd(dy, x, gamma, mean, rstd, extra=None, blocks=None):
    """-> (dx, dgamma, dbeta), (b_dx, b_dgamma, b_dbeta)"""
    dy, x, g, mean, rstd = f64(dy), f64(x), f64(gamma)[None], f64(mean)[:, None], f64(rstd)[:, None]
    rows, W = x.shape
    D = ln_depth(W)
    xh, dh = (x - mean) * rstd, dy * g
    c1, c2 = dh.mean(1, keepdim=True), (dh * xh).mean(1, keepdim=True)
    e_c1 = (D + 3) * U * dh.abs().mean(1, keepdim=True)
    e_c2 = (D + 6) * U * (dh * xh).abs().mean(1, keepdim=True)
    dx = rstd * (dh - c1 - xh * c2)
    mag = rstd.abs() * (dh.abs() + c1.abs() + (xh * c2).abs())
    if extra is not None:
        dx = dx + f64(extra)
        mag = mag + f64(extra).abs()
    b_dx = rstd.abs() * (e_c1 + xh.abs() * e_c2) + C_DX * U * mag
    r4 = cdiv(ln_bwd_plan(rows, blocks)[0], 4)
    t = dy * xh
    return (dx, t.sum(0), dy.sum(0)), (b_dx, (r4 + 8) * U * t.abs().sum(0), (r4 + 5) * U * dy.abs().sum(0))


# ------------------------------------------------------------------------------------------------------------------- InstanceNorm
def in_depth(P):
    return cdiv(P, 4) + 3


def in_stats(x, eps=EPS):
    """x [B, P, C] -> (mean, invstd), (b_mean, b_invstd), float64 [B, C]"""
    mean, _, r, b_mean, b_r = _norm_stats(x, 1, in_depth(x.shape[1]), eps)
    return (mean, r), (b_mean, b_r)


def in_apply(x, mean, invstd, gamma, beta, relu):
    return _apply(x, mean, invstd, gamma, beta, 1, relu)


def in_composed(x, gamma, beta, relu, eps=EPS):
    return _composed(x, gamma, beta, 1, in_depth(x.shape[1]), eps, relu)


def in_bwd(dy, x, gamma, mean, invstd, mask=None):
    """-> (dx, dgamma_part, dbeta_part), bounds -- under the GIVEN boolean mask (None: no ReLU)"""
    g = f64(dy) if mask is None else f64(dy) * mask.cpu().double()
    x, ga, mean, is_ = f64(x), f64(gamma)[None, None], f64(mean)[:, None], f64(invstd)[:, None]
    P = x.shape[1]
    DI = in_depth(P)
    xh = (x - mean) * is_
    s0, s1 = g.sum(1, keepdim=True), (g * xh).sum(1, keepdim=True)
    e_s0, e_s1 = (DI + 1) * U * g.abs().sum(1, keepdim=True), (DI + 4) * U * (g * xh).abs().sum(1, keepdim=True)
    a, b = s0 / P, xh * s1 / P
    dx = ga * is_ * (g - a - b)
    b_dx = (ga * is_).abs() * ((e_s0 + xh.abs() * e_s1) / P + C_IDX * U * (g.abs() + a.abs() + b.abs()))
    return (dx, s1[:, 0], s0[:, 0]), (b_dx, e_s1[:, 0], e_s0[:, 0])


# ------------------------------------------------------------------------------------------------------------------- l2norm
def l2_stats(x):
    """-> inv_norm, bound [rows]"""
    x = f64(x)
    inv = 1.0 / x.norm(dim=1)
    return inv, ((cdiv(x.shape[1], 64) + 7) / 2.0 + 3.0) * U * inv


def l2_apply(x, inv):
    y = f64(x) * f64(inv)[:, None]
    return y, 2 * U * y.abs() + TINY


def l2_bwd(dy, y, inv):
    dy, y, inv = f64(dy), f64(y), f64(inv)[:, None]
    s = (y * dy).sum(1, keepdim=True)
    e_s = (cdiv(y.shape[1], 64) + 8) * U * (y * dy).abs().sum(1, keepdim=True)
    return (dy - y * s) * inv, inv.abs() * (y.abs() * e_s + 4 * U * (dy.abs() + (y * s).abs())) + TINY


# ------------------------------------------------------------------------------------------------------------------- softmax
def sm_fwd(x, scale):
    """-> softmax(scale x) over dim 1 and its bound; scale is the float32 value the kernel receives"""
    z = f64(x) * scale
    m = z.max(1, keepdim=True).values.float().double()            # the device's maximum: the rounded product (rounding is monotone)
    a = z - m
    p = torch.softmax(z, 1)
    ew = U * (z.abs() + a.abs()) + C_EXPF * U
    A = (p * ew).sum(1, keepdim=True)
    return p, p * (ew + A + (cdiv(z.shape[1], 64) + 8) * U) + 2 * TINY


def sm_bwd(dy, y, scale):
    dy, y = f64(dy), f64(y)
    s = (y * dy).sum(1, keepdim=True)
    e_s = (cdiv(y.shape[1], 64) + 8) * U * (y * dy).abs().sum(1, keepdim=True)
    return scale * y * (dy - s), (scale * y).abs() * (e_s + 4 * U * (dy.abs() + s.abs())) + TINY


# =================================================================================================== float32 restatements
# Every tensor below is float32 and every operation rounds to float32.  `order` is how a reduction is grouped: "ltr" (one term after
# the other, in the longest runs the depth of the bound admits: run_sum), "pairwise" (halves), "kernel" (the kernel's own lanes, trips
# and butterfly).  `mut` names one of MUTATIONS.
def seq_sum(t, dim):
    """float32 sum along `dim`, one term after the other"""
    parts = t.unbind(dim)
    s = parts[0].clone()
    for p in parts[1:]:
        s = s + p
    return s


def tree_sum(t, dim):
    """float32 sum along `dim` by halves (zero-padded to a power of two; adding zero is exact): the wave butterfly when the length is 64"""
    t = t.movedim(dim, -1)
    n = 1 << max(t.shape[-1] - 1, 0).bit_length()
    t = torch.nn.functional.pad(t, (0, n - t.shape[-1]))
    while t.shape[-1] > 1:
        h = t.shape[-1] // 2
        t = t[..., :h] + t[..., h:]
    return t[..., 0]


def _pad_to(t, dim, mult):
    dim = dim % t.dim()
    n = t.shape[dim]
    pad = cdiv(n, mult) * mult - n
    if pad == 0:
        return t
    z = torch.zeros(*t.shape[:dim], pad, *t.shape[dim + 1:], dtype=t.dtype)
    return torch.cat([t, z], dim)


def run_sum(t, dim, depth):
    """float32 sum along `dim`, left to right in the longest contiguous runs that a depth of `depth` admits, the runs joined by halves
    (a plain left-to-right sum of n terms has depth n - 1: beyond what the kernels do and what the bounds are derived for)"""
    t = t.movedim(dim, -1)
    n, h = t.shape[-1], 0
    while cdiv(n, 1 << h) - 1 + h > depth:
        h += 1
    L = cdiv(n, 1 << h)
    q = torch.nn.functional.pad(t, (0, L * (1 << h) - n)).reshape(*t.shape[:-1], 1 << h, L)
    return tree_sum(seq_sum(q, -1), -1)


def row_sum(t, order, layout):
    """sum over the last dim of [rows, n].  layout "ln": lane l holds the float4s l, l + 64, ..; "lane": lane l holds l, l + 64, .."""
    n = t.shape[-1]
    if order == "ltr":
        return run_sum(t, -1, ln_depth(n) if layout == "ln" else cdiv(n, 64) + 6)
    if order == "pairwise":
        return tree_sum(t, -1)
    if layout == "ln":
        q = _pad_to(t, -1, 256).view(*t.shape[:-1], -1, 64, 4)                  # [.., trip, lane, 4]
        quad = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
        return tree_sum(seq_sum(quad, -2), -1)
    q = _pad_to(t, -1, 64).view(*t.shape[:-1], -1, 64)                          # [.., trip, lane]
    return tree_sum(seq_sum(q, -2), -1)


def pix_sum(t, order, drop_group3=False):
    """sum over dim 1 of [B, P, C].  kernel: pixel group pg = p % 4 adds its pixels one after the other, then ((g0 + g1) + g2) + g3"""
    if order == "ltr" and not drop_group3:
        return run_sum(t, 1, in_depth(t.shape[1]))
    if order == "pairwise" and not drop_group3:
        return tree_sum(t, 1)
    q = _pad_to(t, 1, 4).view(t.shape[0], -1, 4, t.shape[2])
    g = seq_sum(q, 1)
    if drop_group3:
        return (g[:, 0] + g[:, 1]) + g[:, 2]
    return ((g[:, 0] + g[:, 1]) + g[:, 2]) + g[:, 3]


def rsqrt32(v):
    """a correctly rounded 1 / sqrt of the float32 v"""
    return (1.0 / torch.sqrt(v.double())).float()


def ln_fwd_f32(x, gamma, beta, eps, order, mut=None):
    """-> y, mean, rstd"""
    W = x.shape[1]
    eps = torch.tensor(eps, dtype=torch.float32)
    div = float(cdiv(W, 256) * 256) if mut == "mean_over_padded_lanes" else float(W)
    mean = row_sum(x, order, "ln") / div
    if mut == "onepass_var":
        var = (row_sum(x * x, order, "ln") / float(W) - mean * mean).clamp_min(0.0)
    else:
        d = x - mean[:, None]
        var = row_sum(d * d, order, "ln") / (float(W - 1) if mut == "unbiased_var" else float(W))
    rstd = rsqrt32(var if mut == "no_eps" else var + eps)
    y = (x - mean[:, None]) * rstd[:, None] * gamma[None] + beta[None]
    return y, mean, rstd


def block_sum(t, rpb, order, mut=None):
    """column sums of [rows, W] as layernorm_bwd_kernel and part_finalize_kernel<float> form them: float32 inside a block of rpb rows
    (kernel: wave w walks the rows w, w + 4, .. of the block, then ((w0 + w1) + w2) + w3), float64 over the blocks, one rounding"""
    rows, W = t.shape
    nb = cdiv(rows, rpb)
    tp = _pad_to(t, 0, rpb).view(nb, rpb, W)
    if mut == "dgamma_no_ragged_block" and rows % rpb:
        tp = tp[:-1]
    if order == "ltr" and mut is None:
        part = run_sum(tp, 1, cdiv(rpb, 4) + 3)
    elif order == "pairwise" and mut is None:
        part = tree_sum(tp, 1)
    else:
        q = _pad_to(tp, 1, 4).view(tp.shape[0], -1, 4, W)
        w = seq_sum(q, 1)
        part = w[:, 0] if mut == "dgamma_wave0_only" else ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    return part.double().sum(0).float()


def ln_bwd_f32(dy, x, gamma, mean, rstd, extra, order, blocks=None, mut=None):
    """-> dx, dgamma, dbeta"""
    W = x.shape[1]
    xh = (x - mean[:, None]) * rstd[:, None]
    dh = dy * gamma[None]
    c1 = row_sum(dy if mut == "bwd_c1_from_dy" else dh, order, "ln") / float(W)
    c2 = row_sum(dh * xh, order, "ln") / float(W)
    t = dh - c1[:, None]
    if mut != "bwd_no_c2":
        t = t - xh * c2[:, None]
    dx = rstd[:, None] * t
    if extra is not None and mut != "bwd_extra_dropped":
        dx = dx + extra
    rpb = ln_bwd_plan(x.shape[0], blocks)[0]
    pm = mut if mut in ("dgamma_no_ragged_block", "dgamma_wave0_only") else None
    return dx, block_sum(dy * xh, rpb, order, pm), block_sum(dy, rpb, order, pm)


def in_fwd_f32(x, gamma, beta, eps, relu, order, mut=None):
    """-> y, mean, invstd"""
    P = x.shape[1]
    eps = torch.tensor(eps, dtype=torch.float32)
    drop = mut == "group3_dropped" and P % 4 != 0
    mean = pix_sum(x, order, drop) / float(P)
    d = x - mean[:, None]
    var = pix_sum(d * d, order, drop) / (float(P - 1) if mut == "unbiased_var" else float(P))
    is_ = rsqrt32(var + eps)
    y = (x - mean[:, None]) * is_[:, None] * gamma[None, None] + beta[None, None]
    return (torch.relu(y) if relu else y), mean, is_


def in_bwd_f32(dy, x, gamma, mean, invstd, mask, order, mut=None):
    """-> dx, dgamma_part, dbeta_part; mask None: no ReLU"""
    P = x.shape[1]
    if mask is not None and mut == "mask_from_x":
        mask = (x - mean[:, None]) > 0
    g = dy if mask is None else torch.where(mask, dy, torch.zeros(()))
    d = x - mean[:, None]
    s0 = pix_sum(g, order)
    s1 = pix_sum(g * d * invstd[:, None], order)
    ip = torch.tensor(1.0, dtype=torch.float32) / float(P)
    xh = d * invstd[:, None]
    t = g - (0.0 if mut == "bwd_no_s0" else s0[:, None] * ip) - xh * s1[:, None] * ip
    return gamma[None, None] * invstd[:, None] * t, s1, s0


def l2_fwd_f32(x, order, mut=None):
    """-> y, inv_norm"""
    s = row_sum(x * x, order, "lane")
    if mut == "eps_under_root":
        s = s + torch.tensor(1e-12, dtype=torch.float32)
    iv = 1.0 / torch.sqrt(s)
    return x * iv[:, None], iv


def l2_bwd_f32(dy, y, inv, order, mut=None):
    s = row_sum(y * dy, order, "lane")
    return (dy if mut == "bwd_no_projection" else dy - y * s[:, None]) * inv[:, None]


def sm_fwd_f32(x, scale, order, mut=None):
    sc = torch.tensor(scale, dtype=torch.float32)
    z = x * sc
    if mut == "scale_after_max":
        m = x.max(1, keepdim=True).values * sc
    elif mut == "max_first_trip":
        m = z[:, :64].max(1, keepdim=True).values
    else:
        m = z.max(1, keepdim=True).values
    w = torch.exp(z - m)
    return w / row_sum(w, order, "lane")[:, None]


def sm_bwd_f32(dy, y, scale, order, mut=None):
    sc = torch.tensor(1.0 if mut == "bwd_no_scale" else scale, dtype=torch.float32)
    t = y * dy
    s = row_sum(t[:, :64] if mut == "bwd_s_first_trip" else t, order, "lane")
    return sc * y * (dy - s[:, None])
