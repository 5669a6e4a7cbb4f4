"""fp64 reference, inputs, element-wise error bounds, restatements and mutations for the three self-attention forms
(csrc/attn.hip tris_mha_{fwd,bwd}_f32, csrc/attn_mfma.hip tris_mha_mfma_*, csrc/attn_h2.hip tris_mha_h2_*).  Shared by
tests/test_mha_host.py (CPU) and tests/test_gpu_mha.py.

Notation.  Per sequence and head (head dim 64): s_ij = q_i . k_j / 8 over the VISIBLE keys j (all of them, or j <= i when causal),
m_i = max_j s_ij, lse_i = log sum_j exp(s_ij), p_ij = exp(s_ij - lse_i), out_i = sum_j p_ij v_j, g = dout,
dP_ij = g_i . v_j, delta_i = sum_d g_id out_id (= sum_j p_ij dP_ij), dS_ij = p_ij (dP_ij - delta_i) / 8 (the kernels fold the 1/8
of the logits into dS), dQ_i = sum_j dS_ij k_j, dK_j = sum_i dS_ij q_i, dV_j = sum_i p_ij g_i.  Every sum over keys or queries
below runs over visible pairs only (p, dS and every error term are zero elsewhere).

Bounds.  u = 2^-24.  Worst-case, first order in u, element-wise, in fp64; `form` is "valu", "f32" or "h2".

  es_ij  = 66 u sum_d |q_id| |k_jd| / 8                 the logit: a 64-term dot product (64 u), the scale multiply, one spare
                                                        (tests/test_gpu_packed.py::attention uses the row maximum of this)
  x_ij   = |s_ij - lse_i|   (>= |s_ij - m_i|)           the argument of the exponential
  The exponential.  The flash kernels use __expf, which the compiler's HIP math header on the build machine defines as
  exp2(0x1.715476p+0f * x) with the hardware exp2 (v_exp_f32): the constant is within 0.22 u of log2(e) and the product is
  rounded once, so the exponent carries a relative error of 1.22 u, i.e. the result a relative error of 1.22 u |x| -- the error
  GROWS WITH THE ARGUMENT -- on top of the subtraction s - m that forms x (u |x| more).  We charge 2.25 u x_ij for the two.
  What is left is the accuracy of the exp2 instruction itself, C_EXP u.  Neither the headers nor any document available to the
  build states it, so it was measured on the MI355X (tools/expf_probe.hip, recorded in profiles/mha_parity_floor.txt: __expf
  against fp64 at 2^24 arguments over [-87, 0]; the raw error reaches 64.6 u at x = -86.6 and 1.71 u inside (-1, 0]; with the
  product's 1.25 u |x| taken off the largest value left is 0.795 u) and C_EXP = 1.6 is twice that, rounded up -- a per-ulp
  property of one instruction, not of a shape.  The VALU kernel's expf and torch's exp (1 ulp: at most 2 u) fit the (C_EXP + 1) u that T = 0 leaves.
  Results below 2^-126 may be flushed: every probability carries an absolute 2^-126 as well.
  The online rescale (flash forms): the accumulator and the running sum are multiplied once per key step by
  alpha = exp(m_old - m_new) -- T = ceil(L / 16) steps for f32, ceil(L / 32) for h2, 0 for valu.  The alphas of a weight
  telescope to exp(m_tile(j) - m_final), so their arguments add up to at most x_ij (already charged: the 2.25 u x_ij covers
  |s_ij - m_tile| + |m_tile - m_final| <= x_ij) and each step adds the instruction's C_EXP u and one multiply:
  ew_ij  = es_ij + u ((T + 1) (C_EXP + 1) + 2.25 x_ij)  relative error of the un-normalised weight exp(s_ij - m_i)
  A_i    = sum_j p_ij ew_ij                             relative error of the row sum l_i (before its own roundings)
  out    = sum_j w_ij v_jd / sum_j w_ij:  perturbing the weights moves the numerator by sum_j p_ij ew_ij |v_jd| and the
           denominator by A_i; the row sum, the division and the P V sum are at most 2 L + 8 roundings (any order; the flash
           forms add T merges of partial sums, T <= L / 16 + 1):
  b_out_id = sum_j p_ij ew_ij |v_jd| + (A_i + (2 L + 8) u) sum_j p_ij |v_jd|
  lse    = m + log l (m is only a shift: exact arithmetic does not depend on it).  d lse / d s_ij = p_ij, the sum l has L roundings,
           log is a 1-ulp libm call (__logf is __builtin_logf in that header), the final add is rounded once:
  b_lse_i = A_i + (L + 8) u + 3 u (|m_i| + |lse_i - m_i|)
  The backward recomputes p from the STORED lse (flash forms; the valu form normalises by its own sum, which b_lse covers too):
  eP_ij  = p_ij (es_ij + b_lse_i + u (C_EXP + 2 + 2.25 x_ij)) + 2^-126
  edP_ij = 66 u sum_d |g_id| |v_jd|
  delta  flash forms: sum_d g_id out_id from the stored out:   b_delta_i = sum_d |g_id| b_out_id + 66 u sum_d |g_id| |out_id|
         valu form: sum_j p_ij dP_ij:   b_delta_i = sum_j (eP_ij |dP_ij| + p_ij edP_ij) + (L + 2) u sum_j p_ij |dP_ij|
  eDS_ij = (eP_ij |dP_ij - delta_i| + p_ij (edP_ij + b_delta_i) + 3 u p_ij (|dP_ij| + |delta_i|)) / 8
           (the subtraction and two multiplies; the 1/8 is exact)
  b_dq_id = sum_j eDS_ij |k_jd| + (2 L + 8) u sum_j |dS_ij| |k_jd|        b_dk likewise with q and the sum over queries
  b_dv_jd = sum_i eP_ij |g_id| + (2 L + 8) u sum_i p_ij |g_id|

  h2 (bounds_h2).  csrc/x3_split.h: an operand element x of a tensor with scale s (a power of two bringing the tensor's amax word
  to [2^13, 2^14)) is used as (hi + lo' 2^-11) / s with relative error 2^-22 = 4 u down to 2^-27 of the amax and an absolute error
  phi = 2^-36 / s (<= 2^-49 amax) below; the product lo' x lo' is dropped, 4 u more per term.  With E_x = 4 u |x| + phi every product
  sum_d a_d b_d gains  sum_d (|a| E_b + E_a |b| + E_a E_b + 4 u |a| |b|).  The amax is per TENSOR: all of qkv, all of dout (so a
  head 2^-20 below the largest lives on phi).  Probabilities: fixed scale 2^13, E_p = 4 u p + 2^-49 on top of eP.  dS: the scale
  comes from the largest |dS| of the wave's current block (16 queries x 32 keys in the dQ launch, 32 queries x 16 keys in the
  dK / dV launch); both blocks lie in one 32-aligned 32 x 32 block whose largest true |dS| plus its error bounds the block maximum,
  and the scale keeps one power of two of head room: phi_dS = 2^-48 (max over the 32 x 32 block of |dS| + eDS).
  The h2 kernels' extra fp32 roundings fit the same 66: a product of two fp16 pieces is exact in fp32, so a 64-term sum costs
  63 u instead of 64 u, joining the two accumulators costs 2 u and the inverse scale 1 u.
"""
import functools
import math

import torch

U = 2.0 ** -24
C_EXP = 1.6                 # accuracy of the exp2 instruction in u: twice the 0.795 u measured (see above)
EXP_SLOPE = 2.25
TINY = 2.0 ** -126
HD, NB = 64, 2
KINDS = ["randn", "peaked", "late_max", "early_max", "head_gains", "zero_rows"]
LS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97, 129]
OUTPUTS = ["out", "lse", "delta", "dq", "dk", "dv"]
CASES = [(L, 3, c) for L in LS for c in (0, 1)] + [(L, 1, c) for L in (16, 64) for c in (0, 1)]      # (L, heads, causal)
FORMS = ["valu", "f32", "h2"]
MUTATIONS = ["keys_past_L", "causal_plus_one", "causal_minus_one", "no_rescale", "lse_without_log_l", "delta_omitted",
             "dk_without_scale", "k_low_dropped", "p_low_dropped", "ds_low_dropped"]
H2_MUTATIONS = MUTATIONS[-3:]


def split_heads(x, heads):
    """[N, L, parts * heads * 64] -> parts tensors [N, heads, L, 64] (views)"""
    N, L, C = x.shape
    v = x.view(N, L, C // (heads * HD), heads, HD).permute(2, 0, 3, 1, 4)
    return tuple(v[i] for i in range(v.shape[0]))


def merge_heads(x):
    """[N, heads, L, 64] -> [N, L, heads * 64]"""
    N, H, L, _ = x.shape
    return x.transpose(1, 2).reshape(N, L, H * HD)


def visible(L, causal):
    return torch.ones(L, L, dtype=torch.bool).tril() if causal else torch.ones(L, L, dtype=torch.bool)


def zero_row_set(L):
    """queries whose dout is zero in the `zero_rows` kind: 2..5, and the 16-query tile 32..47 where L > 32.  At L = 33 the tile is
    query 32 alone: the whole last 16-query wave of the dQ launch and the whole last 32-query step of the dK / dV launch are then
    zero (rows clamped to L - 1 included) -- an all-zero dS block in both"""
    return [i for i in list(range(2, 6)) + (list(range(32, 48)) if L > 32 else []) if i < L]


# ------------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def inputs(kind, L, heads, causal):
    """-> qkv [2, L, 3 W], dout [2, L, W] float32 (W = 64 heads); seeded, cached: do not write to them"""
    gen = torch.Generator().manual_seed(7000 + 977 * KINDS.index(kind) + 13 * L + 5 * heads + int(causal))
    W = heads * HD
    qkv = torch.randn(NB, L, 3 * W, generator=gen)
    dout = torch.randn(NB, L, W, generator=gen)
    q, k, v = split_heads(qkv, heads)
    (g,) = split_heads(dout, heads)
    if kind in ("randn", "zero_rows"):
        for h in range(heads):
            qkv.view(NB, L, 3, heads, HD)[:, :, :, h] *= (1.0, 3.0)[h % 2]
        if kind == "zero_rows":
            dout[:, zero_row_set(L)] = 0.0
    elif kind == "peaked":
        q *= math.sqrt(12.0)
        k *= math.sqrt(12.0)
    elif kind in ("late_max", "early_max"):
        q.copy_(0.75 + 0.5 * torch.rand(NB, heads, L, HD, generator=gen))       # sum_d q / 8 = 8 +- 0.2
        k *= 0.1
        if kind == "early_max":
            k[:, :, 0] = 5.0
        elif not causal:
            k[:, :, L - 1] = 5.0
        else:
            k.copy_((5.0 * torch.arange(L, dtype=torch.float32))[None, None, :, None].expand(NB, heads, L, HD))
    elif kind == "head_gains":
        for h in range(heads):
            qkv.view(NB, L, 3, heads, HD)[:, :, :, h] *= 2.0 ** (-10 * h)
            g[:, h] *= 2.0 ** (-7 * h)
    else:
        raise KeyError(kind)
    return qkv, dout


# ---------------------------------------------------------------------------------------------------------------- reference
def evaluate(qkv, dout, heads, causal, dtype=torch.float64, *, pad_keys=0, mask_shift=0, lse_log=True, use_delta=True, dk_gain=1.0):
    """the plain evaluation in `dtype`; the keyword arguments are the defects of the mutations (none: the reference).  The backward
    is the kernels': p from the lse of this forward, delta from its out.  -> dict of OUTPUTS; out [N, L, W], lse / delta
    [N, heads, L], dq / dk / dv [N, L, W]"""
    q, k, v = (t.to(dtype) for t in split_heads(qkv, heads))
    (g,) = (t.to(dtype) for t in split_heads(dout, heads))
    L = q.shape[2]
    keep = visible(L, causal)
    if mask_shift:
        i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
        keep = (j <= i + mask_shift) | (j == 0)
    if pad_keys:                               # keys L .. L + pad - 1 are copies of key L - 1, seen by the queries that see key L - 1
        k = torch.cat([k, k[:, :, -1:].expand(-1, -1, pad_keys, -1)], 2)
        v = torch.cat([v, v[:, :, -1:].expand(-1, -1, pad_keys, -1)], 2)
        keep = torch.cat([keep, keep[:, -1:].expand(-1, pad_keys)], 1)
    s = (q @ k.transpose(2, 3)) * 0.125
    s = s.masked_fill(~keep, float("-inf"))
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    out = (e / l) @ v
    lse = (m + torch.log(l)) if lse_log else m
    p = torch.exp(s - lse)
    dp = g @ v.transpose(2, 3)
    delta = (g * out).sum(-1, keepdim=True)
    ds = p * ((dp - delta) if use_delta else dp) * 0.125
    dq, dk, dv = ds @ k, (ds.transpose(2, 3) @ q) * dk_gain, p.transpose(2, 3) @ g
    return dict(out=merge_heads(out), lse=lse[..., 0], delta=delta[..., 0], dq=merge_heads(dq), dk=merge_heads(dk[:, :, :L]),
                dv=merge_heads(dv[:, :, :L]))


def reference(qkv, dout, heads, causal):
    return evaluate(qkv, dout, heads, causal, torch.float64)


def restate_fp32(qkv, dout, heads, causal):
    """torch's own fp32 evaluation of the same formulas"""
    return evaluate(qkv, dout, heads, causal, torch.float32)


def restate_flash(qkv, dout, heads, causal, dtype=torch.float32, rescale=True):
    """the flash walk in `dtype`: keys in blocks of 64 and sub-tiles of 16 with a running maximum and sum, the accumulator rescaled
    by exp(m_old - m_new) at every sub-tile (rescale False: the running sum is, the accumulator is not -- a mutation); the backward
    from the stored lse and out, dQ summed key tile by key tile, dK / dV query tile by query tile"""
    q, k, v = (t.to(dtype) for t in split_heads(qkv, heads))
    (g,) = (t.to(dtype) for t in split_heads(dout, heads))
    N, H, L, _ = q.shape
    keep = visible(L, causal)
    s = ((q * 0.125) @ k.transpose(2, 3)).masked_fill(~keep, float("-inf"))
    m = torch.full((N, H, L, 1), float("-inf"), dtype=dtype)
    l = torch.zeros(N, H, L, 1, dtype=dtype)
    acc = torch.zeros(N, H, L, HD, dtype=dtype)
    for kb in range(0, L, 64):
        for k0 in range(kb, min(kb + 64, L), 16):
            st = s[..., k0:k0 + 16]
            mn = torch.maximum(m, st.max(-1, keepdim=True).values)
            p = torch.exp(st - mn)
            alpha = torch.exp(m - mn)
            l = l * alpha + p.sum(-1, keepdim=True)
            acc = (acc * alpha if rescale else acc) + p @ v[:, :, k0:k0 + 16]
            m = mn
    out = acc * (1.0 / l)
    lse = m + torch.log(l)
    delta = (g * out).sum(-1, keepdim=True)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)
    for t0 in range(0, L, 16):
        t = slice(t0, t0 + 16)
        p = torch.exp(s[..., t] - lse)                                            # all queries x a key tile
        dq += (p * (g @ v[:, :, t].transpose(2, 3) - delta) * 0.125) @ k[:, :, t]
        p = torch.exp(s[:, :, t] - lse[:, :, t])                                  # a query tile x all keys
        ds = p * (g[:, :, t] @ v.transpose(2, 3) - delta[:, :, t]) * 0.125
        dk += ds.transpose(2, 3) @ q[:, :, t]
        dv += p.transpose(2, 3) @ g[:, :, t]
    return dict(out=merge_heads(out), lse=lse[..., 0], delta=delta[..., 0], dq=merge_heads(dq), dk=merge_heads(dk), dv=merge_heads(dv))


def restate_flash_fp32(qkv, dout, heads, causal):
    return restate_flash(qkv, dout, heads, causal, torch.float32)


# ------------------------------------------------------------------------------------------------------------ h2 restatement
def h2_scale(amax):
    """h2_scale_from_bits of csrc/x3_split.h for the float `amax` (>= 0): 2^(13 - floor(log2 amax)), 1 for 0 or below 2^-100"""
    amax = float(amax)
    if amax == 0.0 or math.frexp(amax)[1] - 1 < -100:
        return 1.0
    return 2.0 ** max(-120, min(120, 13 - (math.frexp(amax)[1] - 1)))


def h2_pieces(x, s):
    """split4h: x float32 (any shape), s a power of two (float or broadcastable tensor) -> hi, lo' as float64"""
    xs = (x.float() * s).float()
    hi = xs.half().float()
    lo = ((xs - hi) * 2048.0).half().double()
    return hi.double(), lo


def h2_matmul(a, b, drop_a=False, drop_b=False):
    """a = (hi, lo'), b = (hi, lo') already laid out for `@`: hi hi + 2^-11 (lo' hi + hi lo'), in fp64"""
    r = a[0] @ b[0]
    x = 0.0
    if not drop_a:
        x = x + a[1] @ b[0]
    if not drop_b:
        x = x + a[0] @ b[1]
    return r + x / 2048.0


def block_max(a, bq, bk):
    """[..., L, L] -> the maximum of each bq x bk block, broadcast back to [..., L, L]"""
    L = a.shape[-1]
    Lq, Lk = -(-L // bq) * bq, -(-L // bk) * bk
    pad = torch.zeros(*a.shape[:-2], Lq, Lk, dtype=a.dtype)
    pad[..., :L, :L] = a
    mx = pad.view(*a.shape[:-2], Lq // bq, bq, Lk // bk, bk).amax((-3, -1), keepdim=True)
    return mx.expand(*a.shape[:-2], Lq // bq, bq, Lk // bk, bk).reshape(*a.shape[:-2], Lq, Lk)[..., :L, :L]


def pow2_scale_of(mx):
    """h2_scale_from_bits for a tensor of float32 block maxima"""
    e = torch.floor(torch.log2(mx.double().clamp_min(2.0 ** -140)))
    s = torch.pow(2.0, (13 - e).clamp(-120, 120))
    return torch.where((mx == 0) | (e < -100), torch.ones_like(s), s)


def restate_h2(qkv, dout, heads, causal, amax_mul=1.0, drop=None):
    """fp64 products of operands rounded exactly as split4h rounds them, with the kernels' scales: one per tensor from its amax
    (times amax_mul: any upper bound is a valid word), 2^13 for the probabilities, the block maximum for dS.  Everything else in
    fp64.  drop in {None, "k", "p", "ds"}: that operand's low piece left out of every product it enters (the mutations)."""
    s_qkv, s_g = h2_scale(float(qkv.abs().max()) * amax_mul), h2_scale(float(dout.abs().max()) * amax_mul)
    q, k, v = (h2_pieces(t, s_qkv) for t in split_heads(qkv, heads))
    (g,) = (h2_pieces(t, s_g) for t in split_heads(dout, heads))
    (g_raw,) = split_heads(dout.double(), heads)
    T = lambda a: (a[0].transpose(2, 3), a[1].transpose(2, 3))
    L = q[0].shape[2]
    keep = visible(L, causal)
    dk_ = drop == "k"
    s = (h2_matmul(q, T(k), drop_b=dk_) * (0.125 / (s_qkv * s_qkv))).masked_fill(~keep, float("-inf"))
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    out = h2_matmul(h2_pieces(e, 8192.0), v, drop_a=drop == "p") / (8192.0 * s_qkv) / l
    lse = m + torch.log(l)
    p = torch.exp(s - lse)
    dp = h2_matmul(g, T(v)) / (s_qkv * s_g)
    delta = (g_raw * out).sum(-1, keepdim=True)
    ds = p * (dp - delta) * 0.125
    sd = pow2_scale_of(block_max(ds.float().abs(), 16, 32))
    dq = torch.zeros_like(q[0])              # the scale differs from block to block: sum the 32-key steps one by one
    for k0 in range(0, L, 32):
        t = slice(k0, k0 + 32)
        d = h2_pieces(ds[..., t], sd[..., t][..., :1])
        dq += h2_matmul(d, (k[0][:, :, t], k[1][:, :, t]), drop_a=drop == "ds", drop_b=dk_) / (sd[..., t][..., :1] * s_qkv)
    sd = pow2_scale_of(block_max(ds.float().abs(), 32, 16))
    dk = torch.zeros_like(q[0])
    for q0 in range(0, L, 32):
        t = slice(q0, q0 + 32)
        sc = sd[:, :, t][:, :, :1].transpose(2, 3)                               # [N, H, L keys, 1]
        d = h2_pieces(ds[:, :, t].transpose(2, 3), sc)
        dk += h2_matmul(d, (q[0][:, :, t], q[1][:, :, t]), drop_a=drop == "ds") / (sc * s_qkv)
    dv = h2_matmul(T(h2_pieces(p, 8192.0)), g, drop_a=drop == "p") / (8192.0 * s_g)
    return dict(out=merge_heads(out), lse=lse[..., 0], delta=delta[..., 0], dq=merge_heads(dq), dk=merge_heads(dk), dv=merge_heads(dv))


# ---------------------------------------------------------------------------------------------------------------- mutations
def mutate(name, qkv, dout, heads, causal):
    """the fp64 path with exactly one defect -> dict of OUTPUTS, or None where the defect does not exist (the causal ones without a
    mask, keys past L at a multiple of 16)"""
    L = qkv.shape[1]
    if name == "keys_past_L":
        return evaluate(qkv, dout, heads, causal, pad_keys=-L % 16) if L % 16 else None
    if name in ("causal_plus_one", "causal_minus_one"):
        return evaluate(qkv, dout, heads, causal, mask_shift=1 if name == "causal_plus_one" else -1) if causal and L > 1 else None
    if name == "no_rescale":
        return restate_flash(qkv, dout, heads, causal, torch.float64, rescale=False)
    if name == "lse_without_log_l":
        return evaluate(qkv, dout, heads, causal, lse_log=False)
    if name == "delta_omitted":
        return evaluate(qkv, dout, heads, causal, use_delta=False)
    if name == "dk_without_scale":
        return evaluate(qkv, dout, heads, causal, dk_gain=8.0)
    return restate_h2(qkv, dout, heads, causal, drop={"k_low_dropped": "k", "p_low_dropped": "p", "ds_low_dropped": "ds"}[name])


# ------------------------------------------------------------------------------------------------------------------- bounds
def bounds(qkv, dout, heads, causal, form="f32", amax_mul=1.0):
    """element-wise bounds of OUTPUTS in fp64 (module docstring), shaped like reference()'s"""
    q, k, v = (t.double() for t in split_heads(qkv, heads))
    (g,) = (t.double() for t in split_heads(dout, heads))
    L = q.shape[2]
    keep = visible(L, causal)
    T = {"valu": 0, "f32": -(-L // 16), "h2": -(-L // 32)}[form]
    tr = lambda a: a.transpose(2, 3)
    if form == "h2":
        eta = kap = 4 * U
        phi, phi_g = 2.0 ** -36 / h2_scale(float(qkv.abs().max()) * amax_mul), 2.0 ** -36 / h2_scale(float(dout.abs().max()) * amax_mul)
    else:
        eta = kap = phi = phi_g = 0.0
    qa, ka, va, ga = q.abs(), k.abs(), v.abs(), g.abs()
    Eq, Ek, Ev, Eg = eta * qa + phi, eta * ka + phi, eta * va + phi, eta * ga + phi_g
    perr = lambda A, EA, B, EB: A @ EB + EA @ B + EA @ EB + kap * (A @ B)         # operand representation (zero unless h2)
    nsum = (2 * L + 8) * U

    s = ((q @ tr(k)) * 0.125).masked_fill(~keep, float("-inf"))
    m = s.max(-1, keepdim=True).values
    lse = torch.logsumexp(s, -1, keepdim=True)
    p = torch.exp(s - lse)
    x = (s - lse).abs().masked_fill(~keep, 0.0)
    es = ((66 * U * (qa @ tr(ka)) + perr(qa, Eq, tr(ka), tr(Ek))) * 0.125).masked_fill(~keep, 0.0)
    ew = es + U * ((T + 1) * (C_EXP + 1) + EXP_SLOPE * x)
    A = (p * ew).sum(-1, keepdim=True)
    Ep = eta * p + (2.0 ** -49 if form == "h2" else 0.0) * keep
    out = p @ v
    pva = p @ va
    b_out = (p * ew) @ va + (A + nsum) * pva + perr(p, Ep, va, Ev)
    b_lse = A + (L + 8) * U + 3 * U * (m.abs() + (lse - m).abs())
    eP = (p * (es + b_lse + U * (C_EXP + 2 + EXP_SLOPE * x)) + TINY) * keep
    dp = g @ tr(v)
    edP = 66 * U * (ga @ tr(va)) + perr(ga, Eg, tr(va), tr(Ev))
    delta = (g * out).sum(-1, keepdim=True)
    if form == "valu":
        b_delta = (eP * dp.abs() + p * edP).sum(-1, keepdim=True) + (L + 2) * U * (p * dp.abs()).sum(-1, keepdim=True)
    else:
        b_delta = (ga * b_out).sum(-1, keepdim=True) + 66 * U * (ga * out.abs()).sum(-1, keepdim=True)
    ds = p * (dp - delta) * 0.125
    eDS = (eP * (dp - delta).abs() + p * (edP + b_delta) + 3 * U * p * (dp.abs() + delta.abs())) * 0.125
    dsa = ds.abs()
    if form == "h2":
        EdS = eDS * (1 + eta) + eta * dsa + (2.0 ** -48 * block_max(dsa + eDS, 32, 32)) * keep
        EP = eP * (1 + eta) + Ep
    else:
        EdS, EP = eDS, eP
    b_dq = perr(dsa, EdS, ka, Ek) + nsum * (dsa @ ka) if form == "h2" else EdS @ ka + nsum * (dsa @ ka)
    b_dk = perr(tr(dsa), tr(EdS), qa, Eq) + nsum * (tr(dsa) @ qa) if form == "h2" else tr(EdS) @ qa + nsum * (tr(dsa) @ qa)
    b_dv = perr(tr(p), tr(EP), ga, Eg) + nsum * (tr(p) @ ga) if form == "h2" else tr(EP) @ ga + nsum * (tr(p) @ ga)
    return dict(out=merge_heads(b_out), lse=b_lse[..., 0], delta=b_delta[..., 0], dq=merge_heads(b_dq), dk=merge_heads(b_dk),
                dv=merge_heads(b_dv))


def bounds_h2(qkv, dout, heads, causal, amax_mul=1.0):
    return bounds(qkv, dout, heads, causal, "h2", amax_mul)


@functools.lru_cache(maxsize=None)
def case(kind, L, heads, causal):
    """-> (qkv, dout, reference, {form: bounds}) of one case, computed once and shared: do not write to them"""
    qkv, dout = inputs(kind, L, heads, causal)
    return qkv, dout, reference(qkv, dout, heads, causal), {f: bounds(qkv, dout, heads, causal, f) for f in FORMS}


def ratios(got, ref, bound):
    """-> {output: max over the elements of |got - ref| / bound} for the outputs present in `got` (0 / 0 counts as 0)"""
    r = {}
    for name, val in got.items():
        err = (val.double() - ref[name]).abs()
        r[name] = float(torch.where(err == 0, torch.zeros_like(err), err / bound[name]).max())
    return r


def old_yardstick_passes(got, ref):
    """tests/test_gpu_ops.py::test_mha: max |err| <= 2e-4 max(1, max |ref|) over the whole tensor"""
    return float((got.double() - ref).abs().max()) <= 2e-4 * max(1.0, float(ref.abs().max()))
