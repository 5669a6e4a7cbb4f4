"""fp64 restatement of the kernels that turn activations into a loss gradient and a gradient into new weights -- AdamW and SGD with
momentum (csrc/optim.hip: tris_adamw_f32, tris_adamw_dev_f32, tris_sgd_momentum_f32), the Stage-1 loss (csrc/heads.hip:
tris_stage1_loss_{fwd,bwd}_f32) and the Stage-2 four-head BCE (csrc/seg.hip: tris_bce4_{fwd,bwd}_f32) -- the named cases the kernel
tests feed them, the element-wise error bounds those tests assert, and float32 restatements of the kernels with the wrong variants
(MUTATIONS) the bounds must reject.  Shared by tests/test_update_host.py (CPU) and tests/test_gpu_update.py.  The pattern, the unit
U = 2^-24, TINY = 2^-126 and the way roundings are counted (the float32 roundings on the path of an output, plus one for the second
order and the float64 work) are those of tests/oracle_rownorm.py; `/` and sqrtf are one rounding each (stated there), expf is charged
C_EXPF (from there, by import).

Device functions measured.  logf and log1pf are device-library calls of unstated accuracy.  tools/logf_probe.hip measured them on the
MI355X against float64 at 2^24 arguments log-uniform per range (profiles/update_parity_floor.txt): logf 3.158 U over (1e-4, 1] and
2.927 U over (1, 2] (1 - cos of a negative cosine lands there), log1pf 1.042 U over [2^-126, 1].  C_LOGF = 6.4 and C_LOG1PF = 2.1
are twice the largest, rounded up to one decimal: a property of an instruction sequence, not of a shape.  No other constant comes
from a device run and none is fitted to the kernels' output.

References take the float32 inputs and the float32 values of the scalar arguments as exact numbers.

AdamW (adamw_kernel; lr, b1, b2, eps, wd float32; bc1 = fl(1 - b1^t), bc2s = fl(sqrt(1 - b2^t)) as the launcher forms them: pow and
sqrt in double, one cast each, adamw_scalars).  Per element, each multiply-add in either the contracted or the uncontracted form:
  m' = b1 m + (1 - b1) g: fl(1 - b1), the product, the sum = 3 on the longer path
          |m' - ref| <= C_M U (|b1 m| + |(1 - b1) g|) + TINY,  C_M = 4         (not relative to |m'|: the two terms may cancel)
  v' = b2 v + ((1 - b2) g) g: fl(1 - b2), two products, the sum = 4
          |v' - ref| <= C_V U (|b2 v| + |(1 - b2) g^2|) + TINY,  C_V = 5
  p' = fl(p decay) - q,  decay = fl(1 - fl(lr wd)),  q = fl(fl(step m') / D),  step = fl(lr / bc1),  D = fl(fl(sqrtf(v') / bc2s) + eps).
  What is compared is the UPDATE p' - p (formed exactly in float64 from the two float32 numbers) with
          dp = -lr wd p - A,   A = step m' / (sqrt(v') / bc2s + eps)
  - on |p|: decay lies in [1/2, 1), where floats are 2^-24 apart: its rounding moves it by at most U / 2; the product p decay rounds
    once (U |p|) and so does the last subtraction (U |p'|): C_P = 2.5, three half-ulp bounds and nothing of second order to add.
    This term is why no bound here is in |p| alone times a large constant: with lr wd = 5e-8 (the backbone group) the decay factor
    itself rounds to 1 - 2^-24, which is 19 % more decay than asked for.  torch's float32 `mul_(1 - lr wd)` rounds the same way, so
    it is not a defect, but one step's decay (0.84 U |p|) is below the roundings of |p| and only the bitwise decay test
    (adamw_decay_only) and the heads group (lr wd = 5e-7 = 8.4 U) can see it.
  - on |lr wd p|: the product lr wd rounds once (not at all where contracted): C_W = 2
  - on |A| given m', v': step (1), step m' (1), sqrtf (1), / bc2s (1), + eps (1; all of D is positive, so its three roundings are
    relative to D), the division (1) = 6: C_A = 7
  - composed (m', v' those of the float64 reference, not the stored ones): m' enters linearly, step b_m / D; sqrt is concave, so
    v' within b_v moves D by at most (sqrt(v') - sqrt(max(v' - b_v, 0))) / bc2s = b_D, and A by |A| b_D / (D - b_D).
          |(p' - p) - dp| <= C_P U |p| + C_W U |lr wd p| + C_A U |A| [+ step b_m / D + |A| b_D / (D - b_D)] + TINY
  adamw_ref gives both: the update against the float64 expression WITH THE MOMENTS THE DEVICE STORED (the kernel stores the very
  floats it used; no bracket) and against the pure float64 step (with the bracket), so a wrong but self-consistent moment cannot pass.
  Decay by itself: with g = m = v = 0, q = 0 exactly and p' = fl(p fl(1 - fl(lr wd))) bit for bit; for the three products lr wd
  tested the contracted fl(1 - lr wd) is the same float (tests/test_update_host.py checks it).
SGD (sgd_kernel): g~ = g + wd p (2), buf' = g~ or mom buf + g~ (2 more): the longest path is wd p, the two sums = 3
          |buf' - ref| <= 4 U (|g| + |wd p| + |mom buf|) + TINY
  p' = p - fl(lr buf'): the product, the subtraction (U |p'| <= U |p| + U |lr buf'|)
          |(p' - p) + lr buf'| <= 3 U |lr buf'| + U |p| + lr b_buf + TINY

Stage-1 loss (one workgroup of 256 threads per image; kw = ceil(E / 256)).  A thread accumulates its kw products one after the other
(the product rounds, or not where contracted, each addition does), six butterfly steps, three additions across the waves:
  S = kw + 10 roundings on a sum of E products;  a sum of squares is within S U of itself, a dot product within S U sum |x y|.
  cos = sat / (na sqrt(stt)) forward, sat ia it backward (ia = 1 / sqrtf(saa)): the two norms (S / 2 + 2 each, the backward form),
  two more operations:   b_cos = S U sum |a t| / (|a| |t|) + (S + 7) U |cos|          (the first term does not shrink with cos)
  fg_b  = -logf(clamp(cos, 1e-4, 0.9999)): the clamp does not grow an error; 1 / c is the slope
          b_fg = b_cos / (c - b_cos) + C_LOGF U |fg|          c = clamp(cos); no first term where cos is outside by more than b_cos
  cbs_k = -logf(1 - s_k): the subtraction rounds once; THE BOUND GROWS WITH 1 / (1 - s), the slope of the logarithm, and the
          hard_neg cases (s = 0.999) are there to say so:   e = b_s + U |1 - s|,  b_k = e / (1 - s - e) + C_LOGF U |cbs_k|
  cbs_b = sum_k cbs_k / K: K additions, the division:   mean_k b_k + (K + 2) U mean_k |cbs_k|
  msm: log_sigmoid(x) = min(x, 0) - log1pf(expf(-|x|)): the argument of expf is exact, e = expf(..) is within C_EXPF U e, which
          moves log1p by at most C_EXPF U e / (1 + e) <= C_EXPF U log1p(e); log1pf C_LOG1PF; the subtraction rounds once:
          b_ls = (C_EXPF + C_LOG1PF) U log1p(e) + 2 U |ls| + TINY;   rowloss_b = -sum_j ls_j / N: N additions, the division:
          b_row = mean_j b_ls + (N + 2) U mean_j |ls_j|
  l1, l4, l5 = sum_b (.) / B in loss_finalize_kernel, one thread, B additions and a division: mean_b b + (B + 2) U mean_b |.|
  total = w1 l1 + w4 l4 + w5 l5: three products, two additions:   sum w b_l + 4 U sum |w l|
  backward.  g1 = fl(fl(g0 w1) + g[1]) (two explicit roundings; likewise g4, g5): b_g = 2 U (|g0 w| + |g[.]|)
  dcls = g4 (sg - [j == b]) / (B N), sg = 1 / (1 + expf(-x)): expf C_EXPF, the sum, the division: sg within (C_EXPF + 2) U sg; the
          subtraction, the product, the division by fl(B) fl(N) (exact integers) = 3 more.  Element-wise against |g4| / (B N):
          |dcls - ref| <= (b_g4 |sg - d| + |g4| ((C_EXPF + 2) U sg + 4 U |sg - d|)) / (B N) + TINY
          (sg is exactly 0 where expf overflows: 1 / inf; the float64 value there is below TINY)
  dfi:  c1 = -g1 / (B cos) inside the window 1e-4 < cos < 0.9999, else exactly 0 (the edges themselves are a set of measure zero and
          are not tested: the clamp cases keep the float64 cosine at least 100 U |cos| away from either edge, in fact more than
          1e-5, so that the float32 cosine is on the same side); B cos rounds, the division rounds:
          b_c1 = (b_g1 + |g1| (b_cos / (|cos| - b_cos) + 3 U)) / (B |cos|)                (grows with 1 / cos^2: 2e-4 is a case)
          ck = g5 / (B K (1 - s_k)):  b_ck = (b_g5 + |g5| (e / (1 - s - e) + 3 U)) / (B K (1 - s))      (grows with 1 / (1 - s)^2)
          T1 = c1 t^ (t^ = t it: r = (S / 2 + 2) U for it, two products), Tk = ck n^k, sm = T1 + sum_k Tk (K additions):
          b_sm = b_c1 |t^| + sum_k b_ck |n^k| + (r + 3 U + K U) (|T1| + sum_k |Tk|)
          dot = sum_c sm a^ (a^ = a ia: two products per term, then S):   b_dot = sum_c b_sm |a^| + (S + 2 + S / 2 + 2) U sum_c |sm a^|
          dfi = (sm - a^ dot) ia: a^ dot is two products and ia, the subtraction, the product with ia:
          |dfi - ref| <= (b_sm + |a^| b_dot + (2 r + 5 U) (|T1| + sum_k |Tk| + |a^ dot|)) / |fi| + TINY
          Element-wise against the magnitudes of the terms that form it, |c1 t^|, each |ck n^k| and the projection term, times
          1 / |fi|: sm - a^ (a^ . sm) cancels where the vectors are nearly parallel (the 0.9998 row), so a bound in |dfi| would be wrong.

bce4 (per element fmaxf(x, 0) - x t + log1pf(expf(-|x|)), summed in float64 by thread, block and finalize: the bound does not grow
with n; one cast):  max(x, 0): the two sums = 2; x t: the product, the two sums = 3; the logarithm as above and the last sum:
          |l_k - ref| <= mean(4 U (|max(x, 0)| + |x t|) + (C_EXPF + C_LOG1PF + 2) U log1p(e^-|x|)) + 2 U |l_k| + TINY
          total = ((l1 + l2) + l3) + l4: three additions:   sum b_k + 4 U sum |l_k|
  dX_k = (sg - t) gk, gk = fl(fl(g0 + g[1 + k]) / fl(n)): the sum, the division; sg as above; the subtraction and the product.
  With G = (|g0| + |g[1 + k]|) / n >= |gk| as the scale (g0 and g[1 + k] may cancel):
          |dX - ref| <= (C_EXPF + 7) U G (sg + |t|) + TINY
  An absent head has loss 0 and its gradient buffer is not touched.

Cases (fixed seeds, named below).  AdamW: every gradient statistic (N(0, 1); 1e-8 N(0, 1) with the state such gradients leave, sqrt(v)
below eps; 1e4 N(0, 1); exact zeros at a tenth of the positions; (1 - b1) g cancelling b1 m; |p| = 1e3 with the Adam step below half an
ulp of p) with both Stage-1 groups (lr 5e-6 and 5e-5, wd 0.01) at step 3; p_small (|p| ~ 1e-6 at lr wd = 1e-3), where nothing of |p|
hides the step and the order of decay and step shows; single steps at t = 10, 1000, 100000 and t = 1 from the zero state; t = 1 .. 5
carried over; n = 1 .. 7, 255, 1027 and one size past the grid cap; one arena in one launch and in three.  Stage-1: S1_SHAPES x S1_STATS
(s1_inputs asserts that every constructed cosine is where it is meant to be), three upstream gradients.  bce4: BCE_CASES.

tests/test_update_host.py checks that float32 evaluations of every expression on the CPU -- the expression as written, with the
multiply-adds contracted, the loss sums in the longest left-to-right runs that the depth S admits and in the kernel's own grouping
(256 strided partial sums, then the block tree) -- stay inside these bounds on every case, and that every mutation leaves them.
"""
import collections
import functools
import math

import torch

from oracle_rownorm import C_EXPF, TINY, U, cdiv, f32_scalar, run_sum, tree_sum

C_LOGF = 6.4        # logf in U: twice the 3.158 U measured over (1e-4, 1] (2.927 U over (1, 2]); profiles/update_parity_floor.txt
C_LOG1PF = 2.1      # log1pf in U: twice the 1.042 U measured over [2^-126, 1]
C_M, C_V, C_P, C_W, C_A = 4, 5, 2.5, 2, 7

MUTATIONS = {
    "adamw": ["no_decay", "decay_after_step", "l2_decay", "bc2_not_sqrt", "eps_in_sqrt", "no_bc1", "betas_swapped", "tail_skipped",
              "m_stored_early"],
    "sgd": ["tail_skipped", "first_reads_buf", "decay_dropped"],
    "s1": ["cbs_not_over_K", "c1_no_B", "clamp_grad_outside", "no_projection", "w5_twice", "target_all_ones", "msm_no_N"],
    "bce4": ["unstable", "target_nonzero", "gk_ignored", "no_div_n"],
}

f64 = lambda t: None if t is None else t.detach().double()
f32t = lambda v: torch.tensor(v, dtype=torch.float32)


# =================================================================================================================== AdamW
Hyper = collections.namedtuple("Hyper", "lr b1 b2 eps wd t")      # float32 values as Python floats; t the 1-based step
B1, B2, EPS_ADAM, WD = (f32_scalar(v) for v in (0.9, 0.999, 1e-8, 0.01))
LRS = {"backbone": f32_scalar(5e-6), "heads": f32_scalar(5e-5)}     # the two Stage-1 groups
GROUPS = tuple(LRS)


def hyper(group, t, lr=None, wd=WD):
    return Hyper(LRS[group] if lr is None else f32_scalar(lr), B1, B2, EPS_ADAM, f32_scalar(wd), t)


def adamw_scalars(h):
    """(bc1, bc2s) as tris_adamw_f32 forms them: pow (and sqrt) in double, one cast each"""
    return f32_scalar(1.0 - h.b1 ** h.t), f32_scalar(math.sqrt(1.0 - h.b2 ** h.t))


def hyper_row(h):
    """the float32 row {lr, 1 - b1^t, sqrt(1 - b2^t), 0} as FusedAdamW.push_hyper fills it (assignment into a float32 tensor)"""
    row = torch.zeros(4, dtype=torch.float32)
    row[0] = float(h.lr)
    row[1] = 1.0 - h.b1 ** h.t
    row[2] = math.sqrt(1.0 - h.b2 ** h.t)
    return row


ADAMW_STATS = ["randn", "tiny", "huge", "zero_mix", "cancel", "p_big", "p_small"]
SIZES = (1, 2, 3, 4, 5, 7, 255, 1024 + 3)                 # below one float4, the scalar tail of 1 .. 3, one block and more
N_GRID_CAP = 8192 * 256 * 4 + 4 * 256 * 3 + 3             # past the 8192-block cap: the grid-stride loop takes a second trip
N_STAT = 1024 + 3
LATE_STEPS = (10, 1000, 100000)
DECAY_ONLY = ((5e-6, 0.01), (5e-5, 0.01), (0.1, 0.01))    # lr wd = 5e-8, 5e-7, 1e-3
ARENA = 64 * 37
RANGES = ((0, 64 * 5), (64 * 5, 64 * 30), (64 * 30, ARENA))
FUSED_SHAPES = ((231,), (5,), (64, 16, 3, 3))             # sizes that leave padding in arenas aligned to 64 floats
ZERO_EVERY, ZERO_AT = 10, 3


@functools.lru_cache(maxsize=None)
def adamw_inputs(stat, n, fresh=False, seed=0):
    """-> (p, g, m, v) float32, never written to.  fresh: m = v = 0 (the state before step 1)"""
    gen = torch.Generator().manual_seed(51000 + 97 * ADAMW_STATS.index(stat) + 13 * seed + n % 9973)
    rn = lambda: torch.randn(n, generator=gen)
    p, g, m, v = rn(), rn(), 0.1 * rn(), 0.01 * rn() ** 2
    scale = {"tiny": 1e-8, "huge": 1e4}.get(stat, 1.0)
    g, m, v = g * scale, m * scale, v * (scale * scale)     # a state that such gradients leave: with 1e-8, sqrt(v) << eps
    if stat == "zero_mix":                                   # exact zeros at a tenth of the positions, the state's among them
        z = torch.arange(n) % ZERO_EVERY == ZERO_AT
        g[z] = 0.0
        m[z & (torch.arange(n) % 20 == ZERO_AT)] = 0.0
        v[z & (torch.arange(n) % 20 == ZERO_AT)] = 0.0
    elif stat == "cancel":                                   # (1 - b1) g cancels b1 m to within a few ulps
        g = (-(B1 * m.double()) / (1.0 - B1)).float()
    elif stat == "p_big":                                    # the Adam step is below half an ulp of p (|m| / sqrt(v) at most 1 / 2
        p = torch.where(p < 0, -1e3, 1e3) * torch.ones(n)    # going in, so that the step stays near lr)
        v = 4.0 * m * m
    elif stat == "p_small":                                  # nothing of |p| hides the step: (p - A) decay differs from p decay - A
        p = 1e-6 * p
    if fresh:
        m, v = torch.zeros(n), torch.zeros(n)
    return p, g, m, v


ACase = collections.namedtuple("ACase", "id stat n h fresh")
STAT_T = 3
# every gradient statistic with both groups at step 3 from a seeded state; p_small at lr wd = 1e-3; single steps late in training;
# step 1 from the zero state; the sizes (heads group, step 2)
ADAMW_CASES = [ACase(f"{s}-{grp}", s, N_STAT, hyper(grp, STAT_T), False) for s in ADAMW_STATS[:-1] for grp in GROUPS]
ADAMW_CASES += [ACase("p_small-lrwd1e-3", "p_small", N_STAT, hyper("heads", STAT_T, lr=0.1), False)]
ADAMW_CASES += [ACase(f"t{t}-{grp}", "randn", N_STAT, hyper(grp, t), False) for t in LATE_STEPS for grp in GROUPS]
ADAMW_CASES += [ACase(f"t1-{grp}", "randn", N_STAT, hyper(grp, 1), True) for grp in GROUPS]
ADAMW_CASES += [ACase(f"n{n}", "randn", n, hyper("heads", 2), False) for n in SIZES if n != N_STAT]
STEPS_T = (1, 2, 3, 4, 5)                                  # the carried-over steps: a fresh gradient adamw_inputs(.., seed=t) each


def adamw_ref(p, g, m, v, h, m_used=None, v_used=None):
    """one step in float64 (on whatever device the inputs are) -> (m', v', dp), (b_m, b_v, b_dp), dp = p' - p.
    m_used, v_used: the moments the kernel stored; then dp is the float64 expression of those, with the bound given them."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    bc1, bc2s = adamw_scalars(h)
    m1, m2 = h.b1 * m, (1.0 - h.b1) * g
    v1, v2 = h.b2 * v, (1.0 - h.b2) * g * g
    mr, vr = m1 + m2, v1 + v2
    b_m = C_M * U * (m1.abs() + m2.abs()) + TINY
    b_v = C_V * U * (v1 + v2) + TINY
    given = m_used is not None
    mm, vv = (f64(m_used), f64(v_used)) if given else (mr, vr)
    step = h.lr / bc1
    D = torch.sqrt(vv) / bc2s + h.eps
    A = step * mm / D
    w = h.lr * h.wd * p
    b_dp = C_P * U * p.abs() + C_W * U * w.abs() + C_A * U * A.abs() + TINY
    if not given:
        b_D = (torch.sqrt(vr) - torch.sqrt((vr - b_v).clamp_min(0.0))) / bc2s
        b_dp = b_dp + step * b_m / D + A.abs() * b_D / (D - b_D)
    return (mr, vr, -w - A), (b_m, b_v, b_dp)


def decay_only_ref(p, lr, wd):
    """fl(p fl(1 - fl(lr wd))) as float32"""
    lr, wd = f32t(f32_scalar(lr)), f32t(f32_scalar(wd))
    return p * (1.0 - lr * wd)


def fma32(a, b, c):
    """a b + c rounded once to float32 (the product of two float32 is exact in float64; the one double rounding of the sum is
    beyond what any bound here resolves)"""
    return (a.double() * b.double() + c.double()).float()


def adamw_f32(p, g, m, v, h, form="plain", mut=None):
    """adamw_kernel in float32 on the CPU -> p', m', v'.  form "plain": every operation rounds; "fma": every multiply-add contracted"""
    bc1, bc2s = (f32t(x) for x in adamw_scalars(h))
    lr, b1, b2, eps, wd = (f32t(x) for x in (h.lr, h.b1, h.b2, h.eps, h.wd))
    one = f32t(1.0)
    if mut == "betas_swapped":
        b1, b2 = b2, b1
    if mut == "bc2_not_sqrt":
        bc2s = f32t(f32_scalar(1.0 - h.b2 ** h.t))
    fma = form == "fma"
    decay = fma32(-lr, wd, one) if fma else one - lr * wd
    step = lr if mut == "no_bc1" else lr / bc1
    G = g
    if mut == "l2_decay":
        G = fma32(wd, p, g) if fma else g + wd * p
    P = p if mut in ("no_decay", "l2_decay", "decay_after_step") else p * decay
    if fma:
        M = fma32(b1, m, (one - b1) * G)
        V = fma32(b2, v, ((one - b2) * G) * G)
    else:
        M = b1 * m + (one - b1) * G
        V = b2 * v + (one - b2) * G * G
    D = torch.sqrt(V + eps) / bc2s if mut == "eps_in_sqrt" else torch.sqrt(V) / bc2s + eps
    P = P - step * M / D
    if mut == "decay_after_step":
        P = P * decay
    if mut == "m_stored_early":
        M = b1 * m
    if mut == "tail_skipped":
        k = p.numel() // 4 * 4
        P, M, V = (torch.cat([a[:k], b[k:]]) for a, b in ((P, p), (M, m), (V, v)))
    return P, M, V


# ---------------------------------------------------------------------------------------------------------------- SGD
SGD_HYPER = tuple(tuple(f32_scalar(x) for x in c) for c in ((0.1, 0.9, 1e-4), (0.1, 1e-4, 0.0)))     # (lr, momentum, wd)


def sgd_ref(p, g, buf, lr, mom, wd, first):
    """-> (buf', dp), (b_buf, b_dp)"""
    p, g, buf = f64(p), f64(g), f64(buf)
    w = wd * p
    carry = torch.zeros_like(p) if first else mom * buf
    br = g + w + carry
    b_buf = 4 * U * (g.abs() + w.abs() + carry.abs()) + TINY
    return (br, -lr * br), (b_buf, 3 * U * (lr * br).abs() + U * p.abs() + lr * b_buf + TINY)


def sgd_f32(p, g, buf, lr, mom, wd, first, form="plain", mut=None):
    lr, mom, wd = f32t(lr), f32t(mom), f32t(wd)
    fma = form == "fma"
    G = g if mut == "decay_dropped" else (fma32(wd, p, g) if fma else g + wd * p)
    if first and mut != "first_reads_buf":
        M = G
    else:
        M = fma32(mom, buf, G) if fma else mom * buf + G
    P = fma32(-lr, M, p) if fma else p - lr * M
    if mut == "tail_skipped":
        k = p.numel() // 4 * 4
        P, M = torch.cat([P[:k], p[k:]]), torch.cat([M[:k], buf[k:]])
    return P, M


# =================================================================================================================== Stage-1 loss
S1_SHAPES = ((1, 512, 3), (2, 8, 0), (5, 260, 1), (6, 512, 3), (48, 1024, 3), (3, 1024, 0))      # (B, E, K); cls is [B, B]
S1_STATS = ["plain", "clamp", "hard_neg", "scale_lo", "scale_hi", "saturated"]
S1_CASES = [(s, sh) for s in S1_STATS for sh in S1_SHAPES if not (s == "hard_neg" and sh[2] == 0)]
S1_W = tuple(f32_scalar(w) for w in (1.0, 5.0, 2.0))                                              # w1, w4, w5
S1_UPS = ((1.0, 0.0, 0.0, 0.0), (0.7, -1.3, 0.25, 2.0), (0.0, 0.0, 0.0, 0.0))
CLAMP_COS = (-0.3, 5e-5, 2e-4, 0.5, 0.9998, 0.99995)      # row b gets CLAMP_COS[b % 6]; 1, 2, 6 (mod 6: 0, 1, 5) are outside the window
HARD_COS = (0.999, -0.999)                                 # negative k < 2 of every image
WIN_LO, WIN_HI = f32_scalar(0.0001), f32_scalar(0.9999)
SAT_VALUES = (30.0, -30.0, 90.0, -90.0)


def _at_cosine(a, c, gen):
    """float32 rows at cosine c (float64 [..] broadcast against a's rows) to the float32 rows a, of random length"""
    ah = a.double() / a.double().norm(dim=-1, keepdim=True)
    o = torch.randn(a.shape, generator=gen, dtype=torch.float64)
    o = o - ah * (o * ah).sum(-1, keepdim=True)
    o = o / o.norm(dim=-1, keepdim=True)
    c = torch.as_tensor(c, dtype=torch.float64).unsqueeze(-1)
    length = 0.5 + torch.rand(a.shape[:-1], generator=gen, dtype=torch.float64).unsqueeze(-1)
    return (length * (c * ah + torch.sqrt(1.0 - c * c) * o)).float()


@functools.lru_cache(maxsize=None)
def s1_inputs(stat, shape):
    """-> dict cls [B, B], fi, ft [B, E], fneg [B, K, E] | None, float32, never written to"""
    B, E, K = shape
    gen = torch.Generator().manual_seed(62000 + 101 * S1_STATS.index(stat.replace("scale_hi", "plain").replace("scale_lo", "plain"))
                                        + 7 * B + 3 * E + K)
    cls = 2.0 * torch.randn(B, B, generator=gen)
    fi, ft = torch.randn(B, E, generator=gen), torch.randn(B, E, generator=gen)
    ft[:3] += 2.0 * fi[:3]                   # some clearly positive cosines, as tests/test_gpu_ops.py::test_stage1_loss has them
    fneg = torch.randn(B, K, E, generator=gen) if K else None
    if stat == "clamp":
        ft = _at_cosine(fi, [CLAMP_COS[b % 6] for b in range(B)], gen)
    elif stat == "hard_neg":
        for k in range(min(K, 2)):
            fneg[:, k] = _at_cosine(fi, HARD_COS[k], gen)
    elif stat in ("scale_lo", "scale_hi"):
        fi = fi * (1e-3 if stat == "scale_lo" else 1e3)
    elif stat == "saturated":                # +-30 and +-90, every value on and off the diagonal as b runs
        b, j = torch.arange(B)[:, None], torch.arange(B)[None, :]
        cls = torch.tensor(SAT_VALUES)[(b + 2 * j) % 4].contiguous()
    d = dict(cls=cls, fi=fi.contiguous(), ft=ft.contiguous(), fneg=fneg)
    s1_check_construction(stat, d)
    return d


def s1_check_construction(stat, d):
    """the float64 cosines of the float32 inputs are where the case means them to be (asserted before the inputs are used)"""
    cp, cn = s1_cosines(d)
    if stat == "clamp":
        for b, c in enumerate(cp.tolist()):
            want = CLAMP_COS[b % 6]
            assert abs(c - want) < 1e-6, (b, c, want)
            for edge in (WIN_LO, WIN_HI):      # on the intended side, at least 100 U |cos| (in fact 1e-5) away from the edge
                assert abs(c - edge) > max(100 * U * abs(c), 1e-5) and (c < edge) == (want < edge), (b, c, edge)
    if stat == "hard_neg":
        for k in range(min(cn.shape[1], 2)):
            assert bool(((cn[:, k] - HARD_COS[k]).abs() < 1e-6).all()), (k, cn[:, k])


def s1_cosines(d):
    """float64 cosines of the float32 inputs -> cos_pos [B], cos_neg [B, K] | None"""
    a, t = f64(d["fi"]), f64(d["ft"])
    cp = (a * t).sum(-1) / (a.norm(dim=-1) * t.norm(dim=-1))
    if d["fneg"] is None:
        return cp, None
    n = f64(d["fneg"])
    return cp, (a[:, None] * n).sum(-1) / (a.norm(dim=-1)[:, None] * n.norm(dim=-1))


def _cos(a, y, S):
    """a [B, 1.., E], y [B, .., E] -> cos, b_cos"""
    na, ny = a.norm(dim=-1), y.norm(dim=-1)
    cos = (a * y).sum(-1) / (na * ny)
    return cos, S * U * (a * y).abs().sum(-1) / (na * ny) + (S + 7) * U * cos.abs()


def _ls(x):
    """log_sigmoid in float64 and its bound"""
    l1p = torch.log1p(torch.exp(-x.abs()))
    ls = x.clamp_max(0.0) - l1p
    return ls, (C_EXPF + C_LOG1PF) * U * l1p + 2 * U * ls.abs() + TINY


def _sigmoid(x):
    """-> sigmoid(x) float64 and the bound of 1 / (1 + expf(-x))"""
    sg = torch.sigmoid(x)
    return sg, (C_EXPF + 2) * U * sg


def s1_ref(d, up, w=S1_W):
    """-> ref, bound: dicts with losses [4] = (total, l1, l4, l5), dcls [B, B], dfi [B, E]; up = upstream gradient of the losses"""
    cls, a, t = f64(d["cls"]), f64(d["fi"]), f64(d["ft"])
    B, E = a.shape
    N = cls.shape[1]
    K = 0 if d["fneg"] is None else d["fneg"].shape[1]
    w1, w4, w5 = w
    S = cdiv(E, 256) + 10
    r = (S / 2.0 + 2.0) * U
    # ---- forward
    cos, b_cos = _cos(a, t, S)
    c = cos.clamp(WIN_LO, WIN_HI)
    fg = -torch.log(c)
    clamped = (cos + b_cos < WIN_LO) | (cos - b_cos > WIN_HI)          # the float32 cosine is clamped too: the argument is exact
    b_fg = torch.where(clamped, torch.zeros_like(cos), b_cos / (c - b_cos)) + C_LOGF * U * fg.abs()
    if K:
        nk = f64(d["fneg"])
        s, b_s = _cos(a[:, None], nk, S)
        e = b_s + U * (1.0 - s)
        ck_f = -torch.log(1.0 - s)
        b_k = e / (1.0 - s - e) + C_LOGF * U * ck_f.abs()
        cbs = ck_f.mean(1)
        b_cbs = b_k.mean(1) + (K + 2) * U * ck_f.abs().mean(1)
    else:
        cbs, b_cbs = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    eye = torch.eye(B, N, dtype=torch.bool)
    ls, b_ls = _ls(torch.where(eye, cls, -cls))
    row = -ls.mean(1)
    b_row = b_ls.mean(1) + (N + 2) * U * ls.abs().mean(1)
    mean = lambda v, b: (v.mean(), b.mean() + (B + 2) * U * v.abs().mean())
    (l1, b1), (l4, b4), (l5, b5) = mean(fg, b_fg), mean(row, b_row), mean(cbs, b_cbs)
    total = w1 * l1 + w4 * l4 + w5 * l5
    b_total = w1 * b1 + w4 * b4 + w5 * b5 + 4 * U * (abs(w1 * l1) + abs(w4 * l4) + abs(w5 * l5))
    ref = {"losses": torch.stack([total, l1, l4, l5])}
    bnd = {"losses": torch.stack([b_total, b1, b4, b5])}
    # ---- backward
    g = [f32_scalar(x) for x in up]
    g1, bg1 = g[0] * w1 + g[1], 2 * U * (abs(g[0] * w1) + abs(g[1]))
    g4, bg4 = g[0] * w4 + g[2], 2 * U * (abs(g[0] * w4) + abs(g[2]))
    g5, bg5 = g[0] * w5 + g[3], 2 * U * (abs(g[0] * w5) + abs(g[3]))
    sg, b_sg = _sigmoid(cls)
    dl = sg - eye.double()
    ref["dcls"] = g4 * dl / (B * N)
    bnd["dcls"] = (bg4 * dl.abs() + abs(g4) * (b_sg + 4 * U * dl.abs())) / (B * N) + TINY
    na = a.norm(dim=-1, keepdim=True)
    ah, th = a / na, t / t.norm(dim=-1, keepdim=True)
    inwin = (cos > WIN_LO) & (cos < WIN_HI)
    c1 = torch.where(inwin, -g1 / (B * cos), torch.zeros_like(cos))
    b_c1 = torch.where(inwin, (bg1 + abs(g1) * (b_cos / (cos.abs() - b_cos) + 3 * U)) / (B * cos.abs()), torch.zeros_like(cos))
    T1 = c1[:, None] * th
    sm, mag, b_sm = T1, T1.abs(), b_c1[:, None] * th.abs()
    if K:
        nh = nk / nk.norm(dim=-1, keepdim=True)
        ck = g5 / (B * K * (1.0 - s))
        b_ck = (bg5 + abs(g5) * (e / (1.0 - s - e) + 3 * U)) / (B * K * (1.0 - s))
        Tk = ck[..., None] * nh
        sm, mag, b_sm = sm + Tk.sum(1), mag + Tk.abs().sum(1), b_sm + (b_ck[..., None] * nh.abs()).sum(1)
    b_sm = b_sm + (r + (3 + K) * U) * mag
    dot = (sm * ah).sum(-1, keepdim=True)
    b_dot = (b_sm * ah.abs()).sum(-1, keepdim=True) + ((S + 2) * U + r) * (sm * ah).abs().sum(-1, keepdim=True)
    proj = ah * dot
    ref["dfi"] = (sm - proj) / na
    bnd["dfi"] = (b_sm + ah.abs() * b_dot + (2 * r + 5 * U) * (mag + proj.abs())) / na + TINY
    ref["fg_mag"] = T1.abs() / na           # the magnitude of the fg contribution to dfi (zero outside the window)
    return ref, bnd


def _pad_last(x, mult):
    n = x.shape[-1]
    return torch.nn.functional.pad(x, (0, cdiv(n, mult) * mult - n))


def dot32(x, y, order, form):
    """float32 sum over the last dim of x y.  "ltr": the rounded products in the longest left-to-right runs a depth of kw + 9 admits;
    "kernel": thread tid accumulates c = tid, tid + 256, .. (contracted under "fma"), the wave butterfly, ((w0 + w1) + w2) + w3"""
    x, y = torch.broadcast_tensors(x, y)
    E = x.shape[-1]
    kw = cdiv(E, 256)
    if order == "ltr":
        return run_sum(x * y, -1, kw + 9)
    xq, yq = (_pad_last(v, 256).reshape(*v.shape[:-1], kw, 256) for v in (x, y))
    acc = torch.zeros(*x.shape[:-1], 256)
    for i in range(kw):
        acc = fma32(xq[..., i, :], yq[..., i, :], acc) if form == "fma" else acc + xq[..., i, :] * yq[..., i, :]
    wv = tree_sum(acc.reshape(*acc.shape[:-1], 4, 64), -1)
    return ((wv[..., 0] + wv[..., 1]) + wv[..., 2]) + wv[..., 3]


def _seq(terms):
    s = torch.zeros_like(terms[0])
    for v in terms:
        s = s + v
    return s


def _ls32(x):
    return x.clamp_max(0.0) - torch.log1p(torch.exp(-x.abs()))


def s1_f32(d, up, w=S1_W, order="kernel", form="plain", mut=None):
    """the five kernels of the Stage-1 loss in float32 on the CPU -> dict losses, dcls, dfi"""
    cls, a, t, fneg = d["cls"], d["fi"], d["ft"], d["fneg"]
    B, E = a.shape
    N = cls.shape[1]
    K = 0 if fneg is None else fneg.shape[1]
    w1, w4, w5 = (f32t(x) for x in w)
    fB, fN, fK, one = f32t(float(B)), f32t(float(N)), f32t(float(max(K, 1))), f32t(1.0)
    lo, hi = f32t(WIN_LO), f32t(WIN_HI)
    dot = lambda x, y: dot32(x, y, order, form)
    # ---- clip_loss_fwd_kernel
    saa, stt, sat = dot(a, a), dot(t, t), dot(a, t)
    na = torch.sqrt(saa)
    fg = -torch.log((sat / (na * torch.sqrt(stt))).clamp(lo, hi))
    cbs = torch.zeros(B)
    for k in range(K):
        nk = fneg[:, k]
        cbs = cbs + -torch.log(one - dot(a, nk) / (na * torch.sqrt(dot(nk, nk))))
    if K and mut != "cbs_not_over_K":
        cbs = cbs / fK
    # ---- msm_fwd_kernel, loss_finalize_kernel
    eye = torch.eye(B, N, dtype=torch.bool)
    lsv = _ls32(cls) if mut == "target_all_ones" else _ls32(torch.where(eye, cls, -cls))
    row = -_seq(lsv.unbind(1))
    if mut != "msm_no_N":
        row = row / fN
    l1, l4, l5 = (_seq(v.unbind(0)) / fB for v in (fg, row, cbs))
    if form == "fma":
        total = fma32(w5, l5, fma32(w4, l4, w1 * l1))
    else:
        total = w1 * l1 + w4 * l4 + w5 * l5
    out = {"losses": torch.stack([total, l1, l4, l5])}
    # ---- msm_bwd_kernel
    g = [f32t(f32_scalar(x)) for x in up]
    g1, g4 = g[0] * w1 + g[1], g[0] * w4 + g[2]
    g5 = (g[0] * w5 * w5 + g[3]) if mut == "w5_twice" else g[0] * w5 + g[3]
    sg = one / (one + torch.exp(-cls))
    dl = sg - (one if mut == "target_all_ones" else eye.float())
    out["dcls"] = g4 * dl / (fB if mut == "msm_no_N" else fB * fN)
    # ---- clip_loss_bwd_kernel
    ia, it = one / torch.sqrt(saa), one / torch.sqrt(stt)
    cosp = sat * ia * it
    c1 = -g1 / (cosp if mut == "c1_no_B" else fB * cosp)
    if mut != "clamp_grad_outside":
        c1 = torch.where((cosp > lo) & (cosp < hi), c1, torch.zeros(()))
    sm = c1[:, None] * t * it[:, None]
    for k in range(K):
        nk = fneg[:, k]
        in_ = one / torch.sqrt(dot(nk, nk))
        s = dot(a, nk) * ia * in_
        ck = g5 / ((fB if mut == "cbs_not_over_K" else fB * fK) * (one - s))
        sm = fma32(ck[:, None] * nk, in_[:, None], sm) if form == "fma" else sm + ck[:, None] * nk * in_[:, None]
    dt = dot(sm * a, ia[:, None].expand_as(a))
    if mut == "no_projection":
        out["dfi"] = sm * ia[:, None]
    elif form == "fma":
        out["dfi"] = fma32(-(a * ia[:, None]), dt[:, None], sm) * ia[:, None]
    else:
        out["dfi"] = (sm - a * ia[:, None] * dt[:, None]) * ia[:, None]
    return out


# =================================================================================================================== bce4
BCE_SIZES = (1, 255, 257, 2 * 32 * 32, 131072 + 77, 1048576 + 77)      # the last two pass the caps of red_blocks (2048 x 64) and seg_grid
BCE_HEADS = ((0,), (0, 1), (0, 1, 2, 3))                                # heads present (head 1 always is)
BCE_TARGETS = ("i64", "f32")                                            # int64 in {0, 1, 2}; float32 soft targets in [0, 1]
BCE_KINDS = ("randn3", "pm40", "pm90", "pm200")
BCE_UPS = ((1.0, 0.0, 0.0, 0.0, 0.0), (0.5, -1.0, 0.0, 2.0, 0.25))
# every size with every kind (heads and target type rotating), and every combination at n = 257
BCE_CASES = [(n, BCE_HEADS[(i + j) % 3], BCE_TARGETS[(i + j) % 2], kind)
             for i, n in enumerate(BCE_SIZES) for j, kind in enumerate(BCE_KINDS)]
BCE_CASES += [(257, hd, tt, kind) for hd in BCE_HEADS for tt in BCE_TARGETS for kind in BCE_KINDS
              if (257, hd, tt, kind) not in BCE_CASES]


@functools.lru_cache(maxsize=None)
def bce_inputs(n, ttype, kind):
    """-> (xs: four float32 [n], target [n] int64 | float32), never written to"""
    gen = torch.Generator().manual_seed(73000 + 11 * BCE_KINDS.index(kind) + BCE_TARGETS.index(ttype) + n % 9973)
    xs = []
    for _ in range(4):
        x = 3.0 * torch.randn(n, generator=gen)
        if kind != "randn3":
            x = torch.where(x < 0, -1.0, 1.0) * float(kind[2:])
        xs.append(x)
    t = torch.randint(0, 3, (n,), generator=gen) if ttype == "i64" else torch.rand(n, generator=gen)
    return tuple(xs), t


def bce4_ref(xs, t, up, heads):
    """-> (losses [5], grads {k: [n]}), (b_losses, b_grads); absent heads: loss 0, no gradient"""
    t = f64(t)
    n = t.numel()
    g = [f32_scalar(x) for x in up]
    L, bL, grads, b_grads = [], [], {}, {}
    for k in range(4):
        if k not in heads:
            L.append(torch.zeros((), dtype=torch.float64))
            bL.append(torch.zeros((), dtype=torch.float64))
            continue
        x = f64(xs[k])
        l1p = torch.log1p(torch.exp(-x.abs()))
        mx, xt = x.clamp_min(0.0), x * t
        l = (mx - xt + l1p).mean()
        L.append(l)
        bL.append((4 * U * (mx + xt.abs()) + (C_EXPF + C_LOG1PF + 2) * U * l1p).mean() + 2 * U * l.abs() + TINY)
        sg = torch.sigmoid(x)
        grads[k] = (sg - t) * (g[0] + g[1 + k]) / n
        b_grads[k] = (C_EXPF + 7) * U * ((abs(g[0]) + abs(g[1 + k])) / n) * (sg + t.abs()) + TINY
    tot = sum(L)
    b_tot = sum(bL) + 4 * U * sum(l.abs() for l in L)
    return (torch.stack([tot] + L), grads), (torch.stack([b_tot] + bL), b_grads)


def bce4_f32(xs, t, up, heads, form="plain", mut=None):
    """bce4_fwd_kernel, bce4_finalize_kernel and bce4_bwd_kernel on the CPU: float32 per element, the sums in float64 -> losses, grads"""
    tf = t.float()
    if mut == "target_nonzero":
        tf = (t != 0).float()
    n = t.numel()
    one, fn = f32t(1.0), f32t(float(n))
    g = [f32t(f32_scalar(x)) for x in up]
    L, grads = [], {}
    for k in range(4):
        if k not in heads:
            L.append(f32t(0.0))
            continue
        x = xs[k]
        if mut == "unstable":
            el = (x - x * tf) + torch.log1p(torch.exp(-x))
        elif form == "fma":
            el = fma32(-x, tf, x.clamp_min(0.0)) + torch.log1p(torch.exp(-x.abs()))
        else:
            el = x.clamp_min(0.0) - x * tf + torch.log1p(torch.exp(-x.abs()))
        s = el.double().sum()
        L.append((s if mut == "no_div_n" else s / n).float())
        gk = g[0] if mut == "gk_ignored" else g[0] + g[1 + k]
        if mut != "no_div_n":
            gk = gk / fn
        grads[k] = (one / (one + torch.exp(-x)) - tf) * gk
    tot = ((L[0] + L[1]) + L[2]) + L[3]
    return torch.stack([tot] + L), grads
