"""fp64 reference, inputs, element-wise error bounds, restatements and mutations for bilateral cross attention (ops.xattn):
csrc/xattn.hip (the two- / three-launch pair, tris_softmax_col_bwd_f32), csrc/xattn_fused.hip (channel slices) and csrc/xattn_px.hip
(pixel rows, forward and backward).  Shared by tests/test_xattn_host.py (CPU) and tests/test_gpu_xattn.py.

Notation (include/tris_hip.h).  Pixels Qv, Kv, Vv [B, P, C], sentences Qt, Kt, Vt [N, C] shared by all images, sc = 1 / sqrt(C).
  S1 = sc Qv Kt^T [B, P, N]   Av  = softmax over n (a row)            new_vis = Av Vt           [B, P, C]
  S2 = sc Kv Qt^T [B, P, N]   AtT = softmax over p (a column)         new_lan = AtT^T Vv        [B, N, C]
  dAv = d_vis Vt^T    r_p = sum_n Av dAv     dS1 = sc Av (dAv - r)     dQv = dS1 Kt    dKt = sum_bp dS1^T Qv    dVt = sum_bp Av^T d_vis
  dAt = Vv d_lan^T    c_n = sum_p AtT dAt    dS2 = sc AtT (dAt - c)    dKv = dS2 Qt    dQt = sum_bp dS2^T Kv    dVv = AtT d_lan
The pixel-row launches cut an image into S workgroups, workgroup s owning pixels [s P / S, (s + 1) P / S) (`cut`).

Bounds.  u = 2^-24.  Worst case, first order in u, element-wise, in fp64.  Three arithmetics:
  f32  the f32-input MFMA (the pair in the f32 mode, and at C = 64 | 128 in every mode);
  x3   every operand is EXACTLY hi + mid + lo (three bf16 pieces, csrc/x3_split.h); mfma6 / mfma6_n keep SIX of the nine piece
       products (lo hi, hi lo, mid mid, mid hi, hi mid, hi hi) and drop mid lo, lo mid, lo lo.  With round-to-nearest pieces
       |mid| <= 2^-9 (1 + 2^-9) |x| and |lo| <= 2^-18 (1 + 2^-9) |x|, so the dropped products weigh at most
       (2 2^-27 + 2^-36) (1 + 2^-9)^2 < X3_DROP = 2.05 2^-27 of |a| |b| per term;
  h2   an operand x of a tensor with the power-of-two scale s (its amax word brought to [2^13, 2^14)) is used as (hi + lo' 2^-11) / s:
       relative error 2^-22 = 4 u down to 2^-27 of the amax and the absolute floor phi = 2^-36 / s below (split4h); lo' x lo' is
       dropped, 4 u more per term.  E_x = 4 u |x| + phi, and a product sum_k a_k b_k gains
       sum_k (|a| E_b + E_a |b| + E_a E_b + 4 u |a| |b|)  (`perr`, as bounds_h2 of tests/oracle_mha.py).  The scales are per TENSOR
       over the whole batch for the eight inputs (any upper bound is a valid amax word: `amax_mul`), the fixed 2^13 for the
       probabilities inside the pixel-row launches (phi = 2^-49), and for dS1 / dS2 inside the pixel-row backward the scale
       h2_scale_from_bits takes from the largest COMPUTED magnitude m of the workgroup's own rows (`half_scale`): it brings m to
       [2^13, 2^14) and keeps no further head room, phi = 2^-36 / s <= 2^-49 m <= 2^-49 max over the range of (|dS| + eDS).
       Operands of the dense-product core (Av, AtT, dS1, dS2 in the chain and in the three [N, C] sums) take the per-tensor amax of
       a pre-pass over what the device computed; one power of two is allowed for the difference to the true maximum: 2^-48 max.
  Roundings of a product sum_k a_k b_k (`running`).  Every product of two pieces is exact in fp32 and every addition into an
  accumulator rounds once, by at most u times the partial sum it produces.  The kernels cut the k axis into `chunks` contiguous
  parts (the four waves of a workgroup; the eight channel slices of csrc/xattn_fused.hip; one part for the products over sentences
  or pixels), walk a part in MFMA steps of 32 k-values into one accumulator and add the parts at the end.  Inside a step the order
  is the hardware's, so each of its <= 32 additions is charged the largest partial sum the step can hold, |S_before| + sum_step |a b|
  with S_before the exact sum of the part's earlier steps: the bound follows the partial sums of the data instead of charging
  n u sum |a b|, which at C = 1024 would hide a lost 2^-11 piece behind the logits.  The f32 kernels' finer steps (16x16x4) and
  any order of the steps' own additions lie inside this.  x3: the five lower piece MFMAs of a step add into the SAME accumulator
  before hi x hi, each addition at |S_before| plus at most 2^-7 of the step: 6 x 32 roundings at |S_before|, 1.05 x 32 at the
  step.  h2: hi x hi has an accumulator of its own; the cross terms' accumulator rounds 2^-11 times as much.  On top,
  (chunks + 3) u sum |a b|: the additions of the parts, the join of the two h2 accumulators, the inverse scale, one spare.
      rnd(a, b) = u (sum_parts sum_steps len (c6 |S_before| + 1.05 sum_step |a b|) + (chunks + 3) sum |a b|),  c6 = 6 (x3) | 1
  "core": the dense-product core in the current mode is held to gamma_n sum |a b|, gamma_n = n 2^-23 / (1 - n 2^-23) with the chopping
  unit 2^-23 (tests/oracle_conv_stats.py): whatever the order, the split-K and the rounding of its summation are.
  sc is formed in fp32 (1.0f / sqrtf(C)): 2 u against the fp64 1 / sqrt(C); with the scale multiply 4 u sum |a b| more on a logit.

  es_pn  = sc (rnd(Qv, Kt) + 4 u sum_c |Qv| |Kt| + perr)                       the logit (likewise es2 with Kv, Qt)
  x      = |s - lse| (>= |s - max|)                                            the argument of the exponential
  ew     = es + u (C_EXP + 1 + 2.25 x)             the weight exp(s - max): __expf (x3, h2, slices) and expf (f32) with C_EXP = 1.6
                                                   and the slope 2.25 u of tests/oracle_mha.py (provenance there; not re-measured)
  p_j = w_j / sum_k w_k moves by p_j (d_j - sum_k p_k d_k) when the weights move by the relative d_k, |d_k| <= ew_k:
  b_Av   = Av ((1 - Av) ew + sum_{k != j} Av_k ew_k + (N + 4) u) + 2^-126      (the sum's N roundings, reciprocal, multiply; flush)
  b_AtT  likewise over the P pixels of a column.
  b_new_vis = rnd(Av, Vt) + perr(Av, b_Av [+ E_p], |Vt|, E_Vt)                  b_new_lan = rnd(AtT^T, Vv) + perr(...)
  The backward reads the STORED Av / AtT (error b_Av / b_AtT of the forward that ran).  Its in-launch products run in the
  arithmetic of the pixel-row backward (x3 | h2, four waves) or in the core (the chain):
  e_dAv = rnd(d_vis, Vt^T) [core: gamma_C sum |d_vis| |Vt|] + perr
  r     = sum_n Av dAv.  The stored probabilities of a row sum to 1 within (N + 4) u, so their errors move r by at most
          sum_n b_Av |dAv - r| + (N + 4) u |r|:      e_r = that + sum_n Av e_dAv + (N + 2) u sum_n Av |dAv|
  eDS1  = sc (b_Av |dAv - r| + Av ((1 - 2 Av) e_dAv + e_r) + 5 u Av (|dAv| + |r|))
          (dAv_j enters dAv_j - r with the weight 1 - Av_j and e_r already holds Av_j e_dAv_j; subtraction, two multiplies, sc)
  eDS2 likewise with dAt = Vv d_lan^T and the column sum c over P pixels -- partial sums of the S workgroups, S more roundings.
  b_dQv = rnd(dS1, Kt) + perr(|dS1|, eDS1 [+ E_dS], |Kt|, E_Kt)                b_dKv (dS2 Qt), b_dVv (AtT d_lan) likewise
  b_dVt = gamma_BP (Av^T |d_vis|) + perr(Av^T, b_Av [+ E], |d_vis|, E)         b_dKt (dS1^T Qv), b_dQt (dS2^T Kv) likewise: split-K
          products of the core over the dS the launch wrote.
  A zero row of d_vis makes dAv, r, eDS1 and (f32, x3) b_dQv of that row exactly zero: the kernels must give exact zeros.
  tris_softmax_col_bwd_f32 on given Y, dY (`col_bwd_reference`): |sc Y| ((P + 2) u sum_p |Y dY| + 3 u (|dY| + |c|)) -- a P-term sum
  and three roundings (subtraction, two multiplies); sc is the caller's float, shared with the reference.

Inputs.  late_max / early_max put the constant 3.0 sqrt(1024 / C) into the dominant row -- 3.0 at C = 1024 -- and re-centre every
row of Qt / Qv (uniform in [0.75, 1.25]) to the mean 1, so that the dominant logit is 3 sqrt(1024) = 96 > 95 in every row at every C
of the case list.  (A fixed 3.0 gives 68 at C = 512 and 24 at C = 64, and without the re-centring a row of 64 or 512 channels
falls below 95 by chance: 94.8 at (2, 8, 1, 512).)
"""
import functools
import math
import zlib

import torch

from oracle_mha import C_EXP, EXP_SLOPE, TINY, U, h2_matmul, h2_pieces, h2_scale

X3_DROP = 2.05 * 2.0 ** -27
U_CHOP = 2.0 ** -23
CUS = 256                     # compute units of the MI355X: the plan of the unpinned case
# (B, P, N, C, S): S = the XATTN_PX_SLOTS pin, 0 = unpinned
PERSISTENT = [(2, 8, 1, 512, 0), (2, 33, 17, 512, 2), (2, 57, 33, 1024, 4), (2, 100, 48, 1024, 5), (3, 100, 5, 1024, 7),
              (2, 104, 64, 1024, 8)]
# the persistent forms must decline: C, C, and P = 105 (out_lds_bytes of csrc/xattn.hip accepts P <= 208 at N <= 64; 105 is the
# smallest P above 104 that is no multiple of 16)
PAIR_ONLY = [(2, 25, 17, 64, 0), (2, 37, 64, 128, 0), (2, 105, 33, 512, 0)]
CASES = PERSISTENT + PAIR_ONLY
KINDS = ["randn", "peaked", "late_max", "early_max", "tiny_sentences", "tiny_image", "outlier", "zero_rows"]
FWD_OUT = ["new_vis", "new_lan", "Av", "AtT"]
PX_OUT = ["dQv", "dKv", "dVv", "dS1", "dS2"]
GRADS = ["dQv", "dKv", "dVv", "dQt", "dKt", "dVt"]
OUTPUTS = FWD_OUT + GRADS + ["dS1", "dS2"]
MUTATIONS = ["local_max", "own_range_norm", "padded_sentences", "range_off_by_one", "att_in_dvt", "ds1_without_rowsum",
             "ds2_sum_over_sentences", "ds2_without_scale", "image0_probabilities", "kt_low_dropped", "p_low_dropped",
             "ds_low_dropped", "vv_third_piece_dropped"]
H2_MUTATIONS = MUTATIONS[9:12]
X3_MUTATIONS = MUTATIONS[12:]
# operands of every product, by tag; CORE: the three [N, C] sums, dense-product core in both backward forms
TAGS = dict(s1=("Qv", "Kt"), s2=("Kv", "Qt"), nv=("Av", "Vt"), nl=("AtT", "Vv"), dav=("d_vis", "Vt"), dat=("Vv", "d_lan"),
            dqv=("dS1", "Kt"), dkv=("dS2", "Qt"), dvv=("AtT", "d_lan"), dvt=("Av", "d_vis"), dkt=("dS1", "Qv"), dqt=("dS2", "Kv"))
FWD_TAGS = ("s1", "s2", "nv", "nl")
CORE_TAGS = ("dvt", "dkt", "dqt")


def plan_slots(B, P, C, cus=CUS, pin=0):
    """xp_slots of csrc/xattn_px.hip: workgroups per image of the pixel-row launches, 0 = they decline"""
    if P < 1 or P > 104 or C not in (512, 1024):
        return 0
    units = C // 32
    smin = max((P + 31) // 32, (units + 7) // 8)
    smax = min(cus // B, 8, P)
    if 0 < pin < smax:
        smax = pin
    return smax if smax >= smin else 0


def cut(case):
    """-> [(p0, p1)] of the S workgroups of an image; [] where the pixel-row forms decline"""
    B, P, N, C, pin = case
    S = plan_slots(B, P, C, CUS, pin)
    return [((s * P) // S, ((s + 1) * P) // S) for s in range(S)]


def pair_arith(mode, case):
    """arithmetic tris_xattn_fwd_f32 runs in: its split-bf16 kernels need the x3 / h2 mode, P <= 128 and C = 256 | 512 | 1024"""
    _, P, _, C, _ = case
    return "x3" if mode != "f32" and P <= 128 and C in (256, 512, 1024) else "f32"


def zero_pixels(case):
    """pixels whose d_vis is zero in `zero_rows`: 2..5 and the whole range of workgroup 1 of the cut"""
    P, rng = case[1], cut(case)
    own = list(range(*rng[1])) if len(rng) > 1 else []
    return sorted({p for p in list(range(2, 6)) + own if p < P})


# ------------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def inputs(kind, case):
    """-> dict of float32 tensors Qv, Kv, Vv [B, P, C], Qt, Kt, Vt [N, C], d_vis [B, P, C], d_lan [B, N, C]; seeded from the kind's
    name, cached: do not write to them"""
    B, P, N, C, _ = case
    gen = torch.Generator().manual_seed(zlib.crc32(kind.encode()) + 131 * P + 17 * N + C + B)
    rn = lambda *s: torch.randn(*s, generator=gen)
    x = dict(Qv=rn(B, P, C), Kv=rn(B, P, C), Vv=rn(B, P, C), Qt=rn(N, C), Kt=rn(N, C), Vt=rn(N, C))
    for t in x.values():
        t *= 1.5
    x.update(d_vis=rn(B, P, C), d_lan=rn(B, N, C))
    if kind == "randn":
        pass
    elif kind == "peaked":                       # logit = sc sum_c q k: standard deviation sigma_q sigma_k = 12
        for n in ("Qv", "Kv", "Qt", "Kt"):
            x[n] *= math.sqrt(12.0) / 1.5
    elif kind in ("late_max", "early_max"):
        top = 3.0 * math.sqrt(1024.0 / C)
        for n in ("Qt", "Qv"):                   # uniform in [0.75, 1.25], every row re-centred to the mean 1: its dominant logit is 96
            u = 0.75 + 0.5 * torch.rand(x[n].shape, generator=gen, dtype=torch.float64)
            x[n].copy_(u - u.mean(-1, keepdim=True) + 1.0)
        x["Kv"] *= 0.1 / 1.5
        x["Kt"] *= 0.1 / 1.5
        x["Kv"][:, P - 1 if kind == "late_max" else 0] = top
        x["Kt"][N - 1 if kind == "late_max" else 0] = top
    elif kind == "tiny_sentences":
        for n in ("Qt", "Kt", "Vt"):
            x[n][::3] *= 2.0 ** -20
    elif kind == "tiny_image":
        for n in ("Qv", "Kv", "Vv", "d_vis", "d_lan"):
            x[n][1] *= 2.0 ** -12
    elif kind == "outlier":
        x["Vv"][0, P // 2, 7] = 1e4
        x["Vt"][N // 2, 11] = 1e4
        x["d_vis"][B - 1, P - 1, 3] = 1e4
    elif kind == "zero_rows":
        x["d_vis"][:, zero_pixels(case)] = 0.0
        x["d_lan"][:, 0] = 0.0
    else:
        raise KeyError(kind)
    return x


# ---------------------------------------------------------------------------------------------------------------- reference
def evaluate(x, case, dtype=torch.float64, mm=None, store=None, defect=None):
    """the plain evaluation in `dtype`.  mm(tag, a, b): the product a @ b of TAGS[tag] (restatements round the operands there);
    store(v): the rounding of an intermediate the kernels keep in fp32; defect: the name of one mutation.  -> dict of OUTPUTS"""
    B, P, N, C, _ = case
    sc = 1.0 / math.sqrt(C)
    t = {k: v.to(dtype) for k, v in x.items()}
    mm = mm or (lambda tag, a, b: a @ b)
    store = store or (lambda v: v)
    rng = cut(case)
    Qv, Kv = t["Qv"], t["Kv"]
    if defect == "range_off_by_one":           # the last pixel of workgroup 0 is served from the row before it
        p1 = rng[0][1]
        Qv, Kv = Qv.clone(), Kv.clone()
        Qv[:, p1 - 1], Kv[:, p1 - 1] = Qv[:, p1 - 2], Kv[:, p1 - 2]
    s1 = mm("s1", Qv, t["Kt"].t()) * sc
    if defect == "padded_sentences":           # the padding columns of the last fragment (logit 0) take part in the soft-max
        s1 = torch.cat([s1, torch.zeros(B, P, -N % 16, dtype=s1.dtype)], 2)
    Av = store(torch.softmax(s1, 2)[..., :N])
    s2 = mm("s2", Kv, t["Qt"].t()) * sc
    if defect == "own_range_norm":
        AtT = torch.cat([torch.softmax(s2[:, a:b], 1) for a, b in rng], 1)
    elif defect == "local_max":                # exp(s - the OWN range's maximum) over the sum of everyone's such weights
        e = torch.cat([torch.exp(s2[:, a:b] - s2[:, a:b].amax(1, keepdim=True)) for a, b in rng], 1)
        AtT = e / e.sum(1, keepdim=True)
    else:
        AtT = torch.softmax(s2, 1)
    AtT = store(AtT)
    new_vis = mm("nv", Av, t["Vt"])
    At_used = AtT[:1].expand(B, P, N) if defect == "image0_probabilities" else AtT
    new_lan = mm("nl", At_used.transpose(1, 2), t["Vv"])
    dAv = mm("dav", t["d_vis"], t["Vt"].t())
    r = 0.0 if defect == "ds1_without_rowsum" else (Av * dAv).sum(2, keepdim=True)
    dS1 = store(sc * Av * (dAv - r))
    dAt = mm("dat", t["Vv"], t["d_lan"].transpose(1, 2))
    c = (AtT * dAt).sum(2 if defect == "ds2_sum_over_sentences" else 1, keepdim=True)
    dS2 = store((1.0 if defect == "ds2_without_scale" else sc) * AtT * (dAt - c))
    flat = lambda a: a.reshape(B * P, -1)
    return dict(new_vis=new_vis, new_lan=new_lan, Av=Av, AtT=AtT, dS1=dS1, dS2=dS2,
                dQv=mm("dqv", dS1, t["Kt"]), dKv=mm("dkv", dS2, t["Qt"]), dVv=mm("dvv", AtT, t["d_lan"]),
                dVt=mm("dvt", flat(AtT if defect == "att_in_dvt" else Av).t(), flat(t["d_vis"])),
                dKt=mm("dkt", flat(dS1).t(), flat(Qv)), dQt=mm("dqt", flat(dS2).t(), flat(Kv)))


def reference(x, case):
    return evaluate(x, case, torch.float64)


def restate_fp32(x, case):
    """torch's own fp32 evaluation of the same formulas"""
    return evaluate(x, case, torch.float32)


# ------------------------------------------------------------------------------------------------------------ x3 restatement
def x3_pieces(v):
    """split8: v (rounded to fp32) as the exact sum of three round-to-nearest bf16 pieces -> (hi, mid, lo) in fp64"""
    v = v.float()
    hi = v.bfloat16().float()
    r = v - hi
    mid = r.bfloat16().float()
    lo = (r - mid).bfloat16().float()
    return hi.double(), mid.double(), lo.double()


def x3_matmul(a, b, drop_b_lo=False):
    """the six piece products mfma6 keeps (hi hi, hi mid, mid hi, mid mid, hi lo, lo hi), in fp64; drop_b_lo: b's third piece left out"""
    (ah, am, al), (bh, bm, bl) = x3_pieces(a), x3_pieces(b)
    r = ah @ bh + ah @ bm + am @ bh + am @ bm + al @ bh
    return r if drop_b_lo else r + ah @ bl


def restate_x3(x, case, drop=None):
    """every product on operands that are exact three-piece sums with the dropped piece products removed, probabilities and dS kept
    in fp32, everything else in fp64.  drop = "Vv": the third piece of Vv left out of every product it enters (the mutation)"""
    def mm(tag, a, b):
        if drop is not None and TAGS[tag][0] == drop:             # a b = (b^T a^T)^T: the dropped piece is a's
            return x3_matmul(b.transpose(-1, -2), a.transpose(-1, -2), drop_b_lo=True).transpose(-1, -2)
        return x3_matmul(a, b, drop_b_lo=drop is not None and TAGS[tag][1] == drop)
    return evaluate(x, case, torch.float64, mm=mm, store=lambda v: v.float().double())


# ------------------------------------------------------------------------------------------------------------ h2 restatement
def range_max(a, case):
    """[B, P, N] -> the maximum of each workgroup's own rows, per image, as [B, P, 1]"""
    return torch.cat([a[:, p0:p1].amax((1, 2), keepdim=True).expand(-1, p1 - p0, 1) for p0, p1 in cut(case)], 1)


def pow2_scale(mx):
    """h2_scale_from_bits for a tensor of maxima"""
    e = torch.floor(torch.log2(mx.double().clamp_min(2.0 ** -140)))
    s = torch.pow(2.0, (13 - e).clamp(-120, 120))
    return torch.where((mx == 0) | (e < -100), torch.ones_like(s), s)


def restate_h2(x, case, amax_mul=1.0, drop=None, chain=False):
    """fp64 products of operands rounded exactly as split4h rounds them, with the kernels' scales: one per input tensor from its
    amax (times amax_mul), 2^13 for the probabilities and the own-range maximum for dS inside the pixel-row launches, the tensor's
    own amax in the dense-product core.  chain: the forward is the pair's (x3), every backward product the core's.
    drop in {None, "Kt", "p", "dS"}: that operand's low piece left out of every product it enters (the mutations)"""
    scale_in = {k: h2_scale(float(v.abs().max()) * amax_mul) for k, v in x.items()}
    dropped = {None: (), "Kt": ("Kt",), "p": ("Av", "AtT"), "dS": ("dS1", "dS2")}[drop]

    def scale(name, v, tag, a_side):
        if name in scale_in:
            return scale_in[name]
        if tag in CORE_TAGS or chain:
            return h2_scale(float(v.float().abs().max()))
        if name in ("Av", "AtT"):
            return 8192.0
        assert a_side and tag in ("dqv", "dkv")
        return pow2_scale(range_max(v.float().abs(), case))

    def mm(tag, a, b):
        if chain and tag in FWD_TAGS:
            return x3_matmul(a, b)
        na, nb = TAGS[tag]
        sa, sb = scale(na, a, tag, True), scale(nb, b, tag, False)
        return h2_matmul(h2_pieces(a.float(), sa), h2_pieces(b.float(), sb), drop_a=na in dropped, drop_b=nb in dropped) / (sa * sb)
    return evaluate(x, case, torch.float64, mm=mm, store=lambda v: v.float().double())


# ---------------------------------------------------------------------------------------------------------------- mutations
def mutate(name, x, case):
    """the fp64 path with exactly one defect -> dict of OUTPUTS, or None where the defect does not exist at this case"""
    rng, N = cut(case), case[2]
    if name in ("local_max", "own_range_norm"):
        return evaluate(x, case, defect=name) if len(rng) > 1 else None
    if name == "range_off_by_one":
        return evaluate(x, case, defect=name) if len(rng) > 1 and rng[0][1] >= 2 else None
    if name == "padded_sentences":
        return evaluate(x, case, defect=name) if N % 16 else None
    if name in H2_MUTATIONS:
        return restate_h2(x, case, drop={"kt_low_dropped": "Kt", "p_low_dropped": "p", "ds_low_dropped": "dS"}[name]) if rng else None
    if name == "vv_third_piece_dropped":
        return restate_x3(x, case, drop="Vv")
    return evaluate(x, case, defect={"att_in_dvt": "att_in_dvt", "ds1_without_rowsum": "ds1_without_rowsum",
                                     "ds2_sum_over_sentences": "ds2_sum_over_sentences", "ds2_without_scale": "ds2_without_scale",
                                     "image0_probabilities": "image0_probabilities"}[name])


# ------------------------------------------------------------------------------------------------------------------- bounds
G_STEP = 32        # k-values one MFMA step adds into an accumulator (16x16x32; the f32 kernels' finer steps lie inside such a block)


def running(A, Bm, chunks, x3):
    """the roundings of the product A @ Bm (signed operands, k last / first) in units of u, from the partial sums themselves: the k
    axis is cut into `chunks` contiguous parts (one per wave or slice), each summed step by step (module docstring)"""
    K = A.shape[-1]
    part = -(-K // chunks)
    total = (chunks + 3.0) * (A.abs() @ Bm.abs())          # merges of the parts, join of the two h2 accumulators, inverse scale, spare
    for k_lo in range(0, K, part):
        run = None
        for k0 in range(k_lo, min(k_lo + part, K), G_STEP):
            k1 = min(k0 + G_STEP, k_lo + part, K)
            a_blk, b_blk = A[..., k0:k1], Bm[..., k0:k1, :]
            total = total + (k1 - k0) * 1.05 * (a_blk.abs() @ b_blk.abs())
            if run is not None:
                total = total + (k1 - k0) * (6.0 if x3 else 1.0) * run.abs()
            run = a_blk @ b_blk if run is None else run + a_blk @ b_blk
    return total


def gamma_core(n):
    return n * U_CHOP / (1.0 - n * U_CHOP)


def bounds(x, case, fwd="x3", bwd="px", mode="x3", amax_mul=1.0, chunks=4):
    """element-wise bounds of OUTPUTS in fp64 (module docstring), shaped like reference()'s.  fwd: the arithmetic of the forward that
    wrote the probabilities (f32 | x3 | h2), chunks: the parts its C-term sums are cut into (4 waves; 8 channel slices); bwd: "px"
    (the pixel-row backward in `mode` = x3 | h2) or "chain" (dense-product core in `mode` = f32 | x3 | h2); the three [N, C] sums
    run through the core in `mode` either way.  amax_mul: the amax words of the input tensors are that much too large (h2)"""
    B, P, N, C, _ = case
    sc = 1.0 / math.sqrt(C)
    t = {k: v.double() for k, v in x.items()}
    phi_in = {k: 2.0 ** -36 / h2_scale(float(v.abs().max()) * amax_mul) for k, v in x.items()}
    T = lambda m: m.transpose(-1, -2)
    flat = lambda m: m.reshape(B * P, -1)

    def rep(arith, name, val, err=None, phi=None):
        """error of the operand as the product sees it: what it inherited (err) plus its representation in `arith`"""
        err = torch.zeros_like(val) if err is None else err
        if arith != "h2":
            return err
        return err * (1 + 4 * U) + 4 * U * val.abs() + (phi_in[name] if phi is None else phi)

    def prod(arith, core, A, EA, Bm, EB, W=1):
        """bound of the product of the signed operands A, Bm with operand errors EA, EB: roundings + representation"""
        kap = {"f32": 0.0, "x3": X3_DROP, "h2": 4 * U}[arith]
        Aa, Ba = A.abs(), Bm.abs()
        mag = Aa @ Ba
        r = gamma_core(A.shape[-1]) * mag if core else U * running(A, Bm, W, arith == "x3")
        return r + Aa @ EB + EA @ Ba + EA @ EB + kap * mag

    # ---- forward, arithmetic `fwd` ------------------------------------------------------------------------------------------
    def softmax_side(q, k, axis, n):
        s = (t[q] @ T(t[k])) * sc
        es = sc * (prod(fwd, False, t[q], rep(fwd, q, t[q]), T(t[k]), T(rep(fwd, k, t[k])), chunks) + 4 * U * (t[q].abs() @ T(t[k].abs())))
        lse = torch.logsumexp(s, axis, keepdim=True)
        p = torch.exp(s - lse)
        ew = es + U * (C_EXP + 1 + EXP_SLOPE * (s - lse).abs())
        A = (p * ew).sum(axis, keepdim=True)
        return p, p * ((1 - p) * ew + (A - p * ew) + (n + 4) * U) + TINY

    Av, bAv = softmax_side("Qv", "Kt", 2, N)
    AtT, bAt = softmax_side("Kv", "Qt", 1, P)
    p_fix = 2.0 ** -49                                                          # probabilities at the fixed scale 2^13
    b = dict(Av=bAv, AtT=bAt)
    b["new_vis"] = prod(fwd, False, Av, rep(fwd, None, Av, bAv, p_fix), t["Vt"], rep(fwd, "Vt", t["Vt"]))
    b["new_lan"] = prod(fwd, False, T(AtT), T(rep(fwd, None, AtT, bAt, p_fix)), t["Vv"], rep(fwd, "Vv", t["Vv"]))

    # ---- backward ------------------------------------------------------------------------------------------------------------
    chain = bwd == "chain"
    S = max(1, len(cut(case)))

    def own_phi(val, err, name):
        """phi of a device-made operand (Av, AtT, dS1, dS2) in the in-launch products"""
        if mode != "h2":
            return 0.0
        if chain:
            return 2.0 ** -48 * float((val.abs() + err).max())
        if name in ("Av", "AtT"):
            return p_fix
        return 2.0 ** -49 * range_max(val.abs() + err, case)

    core_phi = lambda val, err: 2.0 ** -48 * float((val.abs() + err).max())

    def softmax_bwd(pr, bpr, g, Vn, axis, n, extra):
        """-> dS, eDS for the probabilities pr (error bpr) and d = g . Vn^T"""
        d = t[g] @ T(t[Vn])
        ed = prod(mode, chain, t[g], rep(mode, g, t[g]), T(t[Vn]), T(rep(mode, Vn, t[Vn])), 4)
        dot = (pr * d).sum(axis, keepdim=True)
        edot = (bpr * (d - dot).abs() + pr * ed).sum(axis, keepdim=True) + (n + 4) * U * dot.abs() \
            + (n + extra + 2) * U * (pr * d.abs()).sum(axis, keepdim=True)
        dS = sc * pr * (d - dot)
        eDS = sc * (bpr * (d - dot).abs() + pr * ((1 - 2 * pr) * ed + edot) + 5 * U * pr * (d.abs() + dot.abs()))
        return dS, eDS

    dS1, e1 = softmax_bwd(Av, bAv, "d_vis", "Vt", 2, N, 0)
    dS2, e2 = softmax_bwd(AtT, bAt, "Vv", "d_lan", 1, P, S)
    b["dS1"], b["dS2"] = e1, e2
    b["dQv"] = prod(mode, chain, dS1, rep(mode, None, dS1, e1, own_phi(dS1, e1, "dS1")), t["Kt"], rep(mode, "Kt", t["Kt"]))
    b["dKv"] = prod(mode, chain, dS2, rep(mode, None, dS2, e2, own_phi(dS2, e2, "dS2")), t["Qt"], rep(mode, "Qt", t["Qt"]))
    b["dVv"] = prod(mode, chain, AtT, rep(mode, None, AtT, bAt, own_phi(AtT, bAt, "AtT")), t["d_lan"], rep(mode, "d_lan", t["d_lan"]))
    b["dVt"] = prod(mode, True, T(flat(Av)), T(flat(rep(mode, None, Av, bAv, core_phi(Av, bAv)))), flat(t["d_vis"]), flat(rep(mode, "d_vis", t["d_vis"])))
    b["dKt"] = prod(mode, True, T(flat(dS1)), T(flat(rep(mode, None, dS1, e1, core_phi(dS1, e1)))), flat(t["Qv"]), flat(rep(mode, "Qv", t["Qv"])))
    b["dQt"] = prod(mode, True, T(flat(dS2)), T(flat(rep(mode, None, dS2, e2, core_phi(dS2, e2)))), flat(t["Kv"]), flat(rep(mode, "Kv", t["Kv"])))
    return b


def col_bwd_reference(Y, dY, scale):
    """tris_softmax_col_bwd_f32 on Y, dY [B, P, N] -> (dX, bound) in fp64; scale: the float the kernel is given"""
    Y, dY = Y.double(), dY.double()
    P = Y.shape[1]
    c = (Y * dY).sum(1, keepdim=True)
    dX = scale * Y * (dY - c)
    bound = abs(scale) * Y.abs() * ((P + 2) * U * (Y * dY).abs().sum(1, keepdim=True) + 3 * U * (dY.abs() + c.abs()))
    return dX, bound


# combinations (forward arithmetic, backward form, mode) the device tests run; FP32_CLASS: those without fp16 pieces
FP32_CLASS = (("f32", "chain", "f32"), ("x3", "chain", "x3"), ("x3", "px", "x3"))


@functools.lru_cache(maxsize=None)
def case_of(kind, case):
    """-> (inputs, reference) of one case, computed once and shared: do not write to them"""
    x = inputs(kind, case)
    return x, reference(x, case)


@functools.lru_cache(maxsize=None)
def bound_of(kind, case, fwd, bwd, mode, amax_mul=1.0, chunks=4):
    return bounds(inputs(kind, case), case, fwd, bwd, mode, amax_mul, chunks)


@functools.lru_cache(maxsize=None)
def widest_fp32(kind, case):
    """the element-wise maximum of the fp32-class bounds"""
    bs = [bound_of(kind, case, *c) for c in FP32_CLASS]
    return {k: torch.stack([b[k] for b in bs]).amax(0) for k in OUTPUTS}


def ratios(got, ref, bound):
    """-> {output: max over the elements of |got - ref| / bound} for the outputs present in `got` (0 / 0 counts as 0)"""
    r = {}
    for name, val in got.items():
        err = (val.double() - ref[name]).abs()
        r[name] = float(torch.where(err == 0, torch.zeros_like(err), err / bound[name]).max())
    return r


def old_yardstick_passes(got, ref, tol=5e-4):
    """tests/test_gpu_ops.py::test_xattn_fused: max |err| <= tol max(1, max |ref|) over the whole tensor"""
    return float((got.double() - ref).abs().max()) <= tol * max(1.0, float(ref.abs().max()))
