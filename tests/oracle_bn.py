"""fp64 restatement of the BatchNorm kernels of csrc/norm.hip (tris_bn_stats_f32, tris_bn_finalize_f32, tris_bn_apply_f32,
tris_bn_apply_pool_f32, tris_bn_bwd_reduce_f32, tris_bn_bwd_apply_f32 and the pool forms of the backward), the inputs the kernel
tests feed them, and the error bounds those tests assert.  Shared by tests/test_bn_host.py (CPU) and tests/test_gpu_bn.py.

References.  One float64 function per entry point, taking that entry point's float32 inputs as exact numbers: for the apply and
backward kernels mean, invstd, sum_dz, sum_dzx and inv_count are INPUTS, so the rounding of the stored statistics stays out of the
apply tests.  The ReLU mask of the backward is given to the reference, never recomputed by it.

Bounds.  Element-wise, one per output, from the roundings of the expressions in include/tris_hip.h as the kernels write them.
U = 2^-24 is the unit roundoff of float32 (round to nearest), U53 = 2^-53 that of float64.  Each constant is the number of float32
roundings on the path of an output plus one; the one covers the second-order terms (a product of k factors (1 + e_i), |e_i| <= U,
is within (k + 1) U of 1 for k < 2^20) and the float64 work.

  y = (x - mean) * (invstd * gamma) + beta + resid      [then max(., 0): a contraction, the error cannot grow]
      roundings: x - mean; invstd * gamma; the product; + beta; + resid = 5 (4 where the multiply-add is fused, 3 without resid)
      with p = (x - mean) invstd gamma in float64:
          |y - ref| <= C_Y U (|p| + |beta| + |resid|),   C_Y = 6

  dx = k1 (g - k2 - (x - mean) k3),  k1 = gamma * invstd,  k2 = sum_dz * inv_count,  k3 = invstd * sum_dzx * inv_count
      roundings: k1; k2; k3 (two); x - mean; (x - mean) * k3; the two subtractions; the last product = 9
      with a = sum_dz inv_count and b = xhat sum_dzx inv_count in float64:
          |dx - ref| <= C_DX U |gamma invstd| (|g| + |a| + |b|),   C_DX = 10
      g is the masked gradient dz; in the pool forms it is a quarter of the pooled pixel's gradient, an exact product.

  sum_dzx = sum_m g * ((x - mean) * invstd): three float32 roundings per term; the terms are widened to float64 and summed there
      (M U53 relative to sum |terms|, M < 2^18).  Here the "plus one" is spent on the single rounding of the sum to float32,
      U |ref| <= U sum |terms|; what is left over -- 3 U^2 and M U53, under 2^-11 U relative to sum |terms| -- is not counted,
      which makes the constant a hair tighter than a worst-case proof and no looser than one:
          |sum_dzx - ref| <= C_S U sum_m |g xhat|,   C_S = 4
  sum_dz = sum_m g in float64, rounded once:
          |sum_dz - ref| <= 2 U |ref| + 2^-40 sum_m |g|

  pooled y = 0.25 * (((y0 + y1) + y2) + y3): every partial sum is at most the sum of the four (non-negative) values, three
      roundings, the quarter is exact:
          |yp - ref| <= 0.25 (by0 + by1 + by2 + by3 + 3 U (y0 + y1 + y2 + y3))

  statistics: col_partial_kernel<0> sums x and x * x in float64 (every square of a float32 is exact in float64) in one pass,
  without a shift; bn_finalize_kernel forms mean = s / M and var = ss / M - mean * mean in float64 and rounds each to float32:
          |mean - ref| <= 2 U |ref| + M U53 mean_m |x|
          |var  - ref| <= 2 U ref + (M + 4) U53 (ref + mean^2)          (ref is the two-pass variance)
      the second term is the cancellation of the one-pass form: it reaches one float32 ulp of the variance when
      mean^2 / var ~ 2^29 / M.  invstd = 1 / sqrt(var + eps) is formed from the float64 variance and rounded once; 1 / sqrt is
      decreasing and convex, so with bv = (M + 4) U53 (ref + mean^2) and lo = max(ref - bv, 0)
          |invstd - ref| <= (1 / sqrt(lo + eps) - 1 / sqrt(ref + eps)) + 2 U / sqrt(ref + eps)
      running = (1 - m) * old + m * float(new) in float32: per term the factor 1 - m (or the rounding of `new` to float32), its
      product and the sum = 3 roundings; `new` is the mean, or the variance times M / (M - 1) (M > 1; M = 1: the variance itself):
          |running - ref| <= 4 U (|(1 - m) old| + |m new|) + m * (float64 error of `new`)

Nothing here was fitted to device output; tests/test_bn_host.py checks that three float32 evaluations of every expression on the
CPU (left to right, scale folded first, multiply-add fused) stay inside the bounds.
"""
import functools

import torch

U = 2.0 ** -24
U53 = 2.0 ** -53
C_Y, C_DX, C_S = 6, 10, 4
EPS = float(torch.tensor(1e-5, dtype=torch.float32))      # the float the kernels receive
MOMENTA = (float(torch.tensor(0.1, dtype=torch.float32)), 1.0)

KINDS = ["randn", "offset", "relu", "const", "gamma", "dyoff"]
# (M, C): C/4 = 1 and M = 1 or 2; 255 live lanes of 256; 16 lanes x 16 rows; 252 live lanes; a second trip over the channel vectors
# with one live lane; two full trips; 482 partial blocks with a ragged last one and the grid cap of the apply kernels
SHAPES = [(1, 4), (2, 4), (7, 12), (200, 64), (1000, 48), (4099, 1028), (513, 2048), (131075, 64)]
POOL_SHAPES = [(1, 2, 2, 4), (2, 6, 10, 12), (3, 8, 4, 64)]
CROSSING_WIDTHS = [4, 12, 64]
CROSSING_M = 34
FIN_ROWS = [1, 63, 512, 513, 2049, 10000]
FIN_WIDTHS = [4, 12, 1028]


def f64(t):
    return None if t is None else t.detach().double().cpu()


def f32_scalar(v):
    """the float32 nearest to v, as a Python float: what a `float` argument of the C ABI receives"""
    return float(torch.tensor(v, dtype=torch.float64).float())


# ------------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=4)
def inputs(kind, M, C):
    """-> dict of float32 tensors: x, dy, resid [M, C]; gamma, beta, rmean, rvar [C] (rmean / rvar: arbitrary running statistics)"""
    gen = torch.Generator().manual_seed(20000 + 131 * KINDS.index(kind) + 7 * (M % 9973) + C)
    rn = lambda *s: torch.randn(*s, generator=gen)
    c = torch.arange(C)
    x = rn(M, C)
    gamma, beta = 1.0 + 0.5 * rn(C), rn(C)
    dy, resid = rn(M, C), rn(M, C)
    rmean, rvar = rn(C), torch.rand(C, generator=gen) + 0.25
    if kind == "offset":
        ratio = torch.tensor([0.0, 10.0, 1e3, -1e3])[c % 4]
        scale = torch.tensor([1e-2, 1.0, 1e2])[c % 3]
        x = (x + ratio) * scale
    elif kind == "relu":
        x = torch.relu(3.0 * x + 1.0)
    elif kind == "const":
        x = torch.tensor([0.0, 1.0, 100.25])[c % 3].expand(M, C).contiguous()
    elif kind == "gamma":
        gamma = torch.tensor([1e-3, 1.0, 1e3])[c % 3] * rn(C)
        gamma[0] = 0.0
        beta[1] = 0.0
    elif kind == "dyoff":
        dy = dy + 100.0
    dy[dy == 0] = 1.0
    gamma[(gamma == 0) & (c != 0)] = 1.0
    return dict(x=x, dy=dy, resid=resid, gamma=gamma, beta=beta, rmean=rmean, rvar=rvar)


def pool_inputs(kind, shape):
    """the same tensors on a [B, H, W, C] map, plus the pooled gradient dyp [B, H/2, W/2, C]"""
    B, H, W, C = shape
    d = dict(inputs(kind, B * H * W, C))
    d["dyp"] = d["dy"][:B * (H // 2) * (W // 2)].contiguous()
    return d


def crossing_inputs(C):
    """-> (x [34, C], mean, invstd, gamma, beta): every element of x lies within 8 ulps of the x at which (x - mean) invstd gamma +
    beta changes sign -- rows k = -8 .. 8 of nextafter steps around it, the block of 17 repeated"""
    gen = torch.Generator().manual_seed(777 + C)
    mean = torch.randn(C, generator=gen) * 3.0
    invstd = torch.rand(C, generator=gen) * 2.0 + 0.25
    gamma = (torch.rand(C, generator=gen) + 0.5) * torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    beta = (torch.rand(C, generator=gen) + 0.25) * torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0)
    x0 = (mean.double() - beta.double() / (invstd.double() * gamma.double())).float()
    return crossing_rows(x0, CROSSING_M), mean, invstd, gamma, beta


def crossing_pool_inputs(C):
    """-> (x [1, 4, 34, C], mean, invstd, gamma, beta): every 2x2 window holds one row of crossing_inputs (top left) and three
    pixels at which bn(x) <= -5, so the pooled value is a quarter of relu(bn(.)) of the crossing pixel and has its sign"""
    xc, mean, invstd, gamma, beta = crossing_inputs(C)
    neg = (mean.double() - (beta.double().abs() + 5.0 + beta.double()) / (invstd.double() * gamma.double())).float()
    x = neg.expand(1, 4, CROSSING_M, C).clone()
    x[0, 0::2, 0::2] = xc.view(2, 17, C)
    return x.contiguous(), mean, invstd, gamma, beta


def crossing_rows(x0, M):
    """[M, C]: row m is x0 moved by ((m % 17) - 8) float32 steps"""
    bits = x0.view(torch.int32)
    assert bool((x0 != 0).all()) and bool((x0.abs() > 1e-30).all())
    k = (torch.arange(M, dtype=torch.int32) % 17 - 8)[:, None]
    step = torch.where(x0 > 0, 1, -1).to(torch.int32)[None, :] * k      # towards +inf for k > 0, whatever the sign of x0
    return (bits[None, :] + step).view(torch.float32).contiguous()


# ------------------------------------------------------------------------------------------------------------------- statistics
def stats(x, eps=EPS):
    """-> mean, biased variance (two passes), invstd, all float64 [C]"""
    x = f64(x)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def stats_bounds(x, eps=EPS):
    """-> bounds of (mean, var, invstd) and the float64 parts (e_mean, e_var) carried into the running statistics"""
    x = f64(x)
    M = x.shape[0]
    mean, var, invstd = stats(x, eps)
    e_mean = M * U53 * x.abs().mean(0)
    e_var = (M + 4) * U53 * (var + mean ** 2)
    lo = (var - e_var).clamp_min(0.0)
    b_inv = (1.0 / torch.sqrt(lo + eps) - invstd) + 2 * U * invstd
    return 2 * U * mean.abs() + e_mean, 2 * U * var + e_var, b_inv, e_mean, e_var


def running(x, rmean, rvar, momentum, eps=EPS):
    """-> (running_mean, running_var) after one update and their bounds; momentum is the float32 value the kernel receives"""
    x = f64(x)
    M = x.shape[0]
    mean, var, _ = stats(x, eps)
    _, _, _, e_mean, e_var = stats_bounds(x, eps)
    fac = M / (M - 1.0) if M > 1 else 1.0
    out, bounds = [], []
    for old, new, e in ((f64(rmean), mean, e_mean), (f64(rvar), var * fac, e_var * fac)):
        a, b = (1.0 - momentum) * old, momentum * new
        out.append(a + b)
        bounds.append(4 * U * (a.abs() + b.abs()) + momentum * e)
    return out, bounds


@functools.lru_cache(maxsize=4)
def stats_reference(kind, M, C):
    x = inputs(kind, M, C)["x"]
    return stats(x), stats_bounds(x)


def stored_stats(kind, M, C):
    """the oracle's mean and invstd rounded to float32: the inputs of the apply and backward tests"""
    (mean, _, invstd), _ = stats_reference(kind, M, C)
    return mean.float(), invstd.float()


# ------------------------------------------------------------------------------------------------------------------- forward
def apply(x, mean, invstd, gamma, beta, resid=None, relu=False):
    """-> z (the value before the ReLU), y, bound -- float64, shaped like x"""
    p = (f64(x) - f64(mean)) * f64(invstd) * f64(gamma)
    z = p + f64(beta)
    mag = p.abs() + f64(beta).abs()
    if resid is not None:
        z = z + f64(resid)
        mag = mag + f64(resid).abs()
    return z, (z.clamp_min(0.0) if relu else z), C_Y * U * mag


def pool4(t):
    """[B, H, W, C] -> the four members of every 2x2 window, each [B, H/2, W/2, C]"""
    return t[:, 0::2, 0::2], t[:, 0::2, 1::2], t[:, 1::2, 0::2], t[:, 1::2, 1::2]


def apply_pool(x, mean, invstd, gamma, beta):
    """x [B, H, W, C] -> avgpool2(relu(bn(x))) and its bound"""
    _, y, by = apply(x, mean, invstd, gamma, beta, None, True)
    s, sb = sum(pool4(y)), sum(pool4(by))
    return 0.25 * s, 0.25 * (sb + 3 * U * s)


def unpool(dyp):
    """the gradient avgpool2 hands to each of its four inputs: a quarter of the pooled pixel's (exact in float32)"""
    return 0.25 * dyp.repeat_interleave(2, 1).repeat_interleave(2, 2)


# ------------------------------------------------------------------------------------------------------------------- backward
def bwd_reduce(dy, x, mean, invstd, mask=None):
    """-> (sum_dz, sum_dzx), (bound_dz, bound_dzx), dz -- under the GIVEN boolean mask (None: no ReLU)"""
    g = f64(dy) if mask is None else f64(dy) * mask.cpu().double()
    t = g * ((f64(x) - f64(mean)) * f64(invstd))
    s0, s1 = g.sum(0), t.sum(0)
    return (s0, s1), (2 * U * s0.abs() + 2.0 ** -40 * g.abs().sum(0), C_S * U * t.abs().sum(0)), g


def bwd_apply(dy, x, mean, invstd, gamma, sum_dz, sum_dzx, inv_count, mask=None):
    """-> dx, bound, dz; inv_count a Python float (the float32 value the kernel receives, or 1 / count exactly)"""
    g = f64(dy) if mask is None else f64(dy) * mask.cpu().double()
    xhat = (f64(x) - f64(mean)) * f64(invstd)
    a = f64(sum_dz) * inv_count
    b = xhat * (f64(sum_dzx) * inv_count)
    k1 = f64(gamma) * f64(invstd)
    return k1 * (g - a - b), C_DX * U * k1.abs() * (g.abs() + a.abs() + b.abs()), g


# ------------------------------------------------------------------------------------------------------------------- finalizers
@functools.lru_cache(maxsize=2)
def partial_rows(rows, C):
    """hand-made float64 partial rows [rows][2][C] as a conv epilogue leaves them, and the number of activation rows M they stand
    for: sums of M / rows values around a per-channel mean, sums of their squares"""
    gen = torch.Generator().manual_seed(31 * rows + C)
    per = 128
    mu = torch.randn(C, generator=gen, dtype=torch.float64) * 2.0
    s = per * mu + torch.randn(rows, C, generator=gen, dtype=torch.float64) * per ** 0.5
    ss = per * (1.0 + mu ** 2) + torch.randn(rows, C, generator=gen, dtype=torch.float64).abs() * per ** 0.5
    return torch.stack([s, ss], 1).contiguous(), rows * per


def finalize(part, M, eps=EPS):
    """fp64 sums of the rows -> (sum0, sum1), mean, var, invstd and their bounds given the rows as exact numbers: the sums carry
    rows * U53 of sum |rows|, the variance that of both sums plus four float64 roundings of its own expression"""
    rows = part.shape[0]
    s, ss = part[:, 0].sum(0), part[:, 1].sum(0)
    e_s, e_ss = rows * U53 * part[:, 0].abs().sum(0), rows * U53 * part[:, 1].abs().sum(0)
    mean = s / M
    var = (ss / M - mean ** 2).clamp_min(0.0)
    e_var = e_ss / M + 2 * mean.abs() * e_s / M + 4 * U53 * (ss / M + mean ** 2)
    invstd = 1.0 / torch.sqrt(var + eps)
    lo = (var - e_var).clamp_min(0.0)
    b_inv = (1.0 / torch.sqrt(lo + eps) - invstd) + 2 * U * invstd
    return (s, ss), (2 * U * s.abs() + e_s, 2 * U * ss.abs() + e_ss), (mean, var, invstd), \
        (2 * U * mean.abs() + e_s / M, 2 * U * var + e_var, b_inv)
