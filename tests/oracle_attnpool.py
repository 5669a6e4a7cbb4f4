"""fp64 restatements, input builders and error bounds for CLIP's attention pooling (csrc/attnpool.hip tris_attnpool_{tokens,pool}_f32,
tris_amd.CLIP.clip.model.AttentionPool2d).  Shared by tests/test_attnpool_host.py (CPU), tests/test_gpu_attnpool.py and
tools/record_attnpool_golden.py.  Every function is generic in the dtype of its inputs: float64 gives the reference, float32 the
"reference's own fp32 error" the module tests compare against.

Notation.  x [B,h,w,C] channels-last, pos [S*S+1, C], L = hw + 1, d = C / heads, u = 2^-24.
  tokens   T[b,0] = mean_i x[b,i] + pos[0];  T[b,1+i] = x[b,i] + g[i],  g = F.interpolate(pos[1:] as an S x S grid, (h, w), bilinear)
  full     CLIP/clip/model.py:80-104 through oracle.tris_oracle.attnpool (multi-head attention of all L tokens, c_proj)
  folded   token 0 of `full` with q_h = W_q,h T_0 + b_q,h, U_h = W_k,h^T q_h, P_h = softmax_j(T_j . U_h / sqrt(d)) (the term q_h . b_k,h is
           constant over j and cancels), pooled_h = sum_j P_hj T_j, head output W_v,h pooled_h + b_v,h (sum_j P_hj = 1), c_proj.

Bounds (worst case, first order in u, element-wise).
  mean row     hw - 1 adds, one division, one add:                      (hw + 2) u sum_i |x_i| / hw + u |pos_0|
  pixel row    weights with relative error u each (csrc/bilinear.h lerp_exact_of), products and sums of the blend relative to
               sum_k w_k |p_k|: at most 6 roundings on any path;  the closing add:   8 u sum_k w_k |p_k| + 2 u (|x| + |g|)
  logits       es_j = (C + 2) u scale sum_c |T_jc| |U_c|     a C-term dot product, the scale multiply, one spare (tests/oracle_mha.py es)
  weights      ew_j = es_j + u (C_EXP + 1 + 2.25 x_j),  x_j = |s_j - lse|    (tests/oracle_mha.py ew with T = 0: no online rescale)
  P            A = sum_j p_j ew_j;  eP_j = p_j (ew_j + A + (L + 2) u) + 2^-126     (the sum of L terms, one division)
  pooled       sum_j eP_j |T_jc| + (L + 2) u sum_j p_j |T_jc|                        (an L-term weighted sum of fused multiply-adds)
  row sums     sum_j P_j = 1 within (L + 4) u    (the L-term sum the kernel divides by, the divisions)
"""
import functools
import math

import torch
import torch.nn.functional as F

import oracle_mha as M
from oracle import tris_oracle as O

U = M.U
# name -> (B, C, heads, out, S, h, w): identity resize, non-square enlarging, shrinking; the RN50 training shape (320 px)
CASES = {
    "3x3": (3, 128, 2, 64, 3, 3, 3),
    "5x4": (3, 128, 2, 64, 3, 5, 4),
    "2x2": (3, 128, 2, 64, 3, 2, 2),
    "rn50": (2, 2048, 32, 1024, 7, 10, 10),
}
SMALL = ["3x3", "5x4", "2x2"]
PREFIX = "attnpool"


def module_state(C, heads, out, S, seed):
    """seeded float32 state dict of one AttentionPool2d under PREFIX: CLIP's initialisation scales (CLIP/clip/model.py:61, :510-515),
    biases NON-zero so that the cancelling q . b_k term and the b_v term of the folded form are exercised"""
    g = torch.Generator().manual_seed(seed)
    sd = {PREFIX + ".positional_embedding": torch.randn(S * S + 1, C, generator=g) / C ** 0.5}
    for name, n in (("q_proj", C), ("k_proj", C), ("v_proj", C), ("c_proj", out)):
        sd[f"{PREFIX}.{name}.weight"] = torch.randn(n, C, generator=g) * C ** -0.5
        sd[f"{PREFIX}.{name}.bias"] = 0.1 * torch.randn(n, generator=g)
    return sd


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (sd float32, x [B,h,w,C] float32 channels-last, heads, S); seeded, cached: do not write to them"""
    B, C, heads, out, S, h, w = CASES[name]
    sd = _module(C, heads, out, S)                         # (the three small maps share ONE module, as the golden file records it)
    x = torch.randn(B, h, w, C, generator=torch.Generator().manual_seed(9150 + sorted(CASES).index(name)))
    return sd, x, heads, S


@functools.lru_cache(maxsize=None)
def _module(C, heads, out, S):
    return module_state(C, heads, out, S, 9100 + C)


def to(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------------------- restatements
def pos_grid(pos, S, h, w):
    """pos[1:] as an S x S grid resized to h x w -> [hw, C] (CLIP/clip/model.py:76-77)"""
    C = pos.shape[1]
    sp = F.interpolate(pos[1:].reshape(1, S, S, C).permute(0, 3, 1, 2), size=(h, w), mode="bilinear")
    return sp.reshape(C, h * w).permute(1, 0)


def tokens(pos, x, S):
    """x [B,h,w,C] -> T [B, hw+1, C] (CLIP/clip/model.py:72-80, batch-first)"""
    B, h, w, C = x.shape
    t = x.reshape(B, h * w, C)
    return torch.cat([t.mean(dim=1, keepdim=True) + pos[0], t + pos_grid(pos, S, h, w)], dim=1)


def full(sd, x, heads, S):
    """-> (global_feat [B,out], feature_map [B,out,h,w]) in the dtype of the inputs"""
    return O.attnpool(sd, PREFIX, x.permute(0, 3, 1, 2), heads, S)


def pool(T, Uq, scale):
    """-> P [B,heads,L], pooled [B,heads,C]"""
    Pr = torch.softmax(torch.einsum("bjc,bhc->bhj", T, Uq) * scale, dim=-1)
    return Pr, torch.einsum("bhj,bjc->bhc", Pr, T)


def folded_query(sd, T, heads):
    """U [B,heads,C] of the folded form"""
    B, L, C = T.shape
    d = C // heads
    q0 = T[:, 0] @ sd[PREFIX + ".q_proj.weight"].t() + sd[PREFIX + ".q_proj.bias"]
    return torch.einsum("bhd,hdc->bhc", q0.view(B, heads, d), sd[PREFIX + ".k_proj.weight"].view(heads, d, C))


def folded(sd, x, heads, S):
    """global_feat [B,out] through the folded form, in the dtype of the inputs"""
    T = tokens(sd[PREFIX + ".positional_embedding"], x, S)
    B, L, C = T.shape
    d = C // heads
    _, pooled = pool(T, folded_query(sd, T, heads), 1.0 / math.sqrt(d))
    o = torch.einsum("bhc,hdc->bhd", pooled, sd[PREFIX + ".v_proj.weight"].view(heads, d, C)).reshape(B, C)
    o = o + sd[PREFIX + ".v_proj.bias"]
    return o @ sd[PREFIX + ".c_proj.weight"].t() + sd[PREFIX + ".c_proj.bias"]


def rel_err(got, ref):
    """e = max |got - ref| / max |ref| (ref float64)"""
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=None)
def module_reference(name):
    """-> dict: f64 outputs of both forms and the error e of the float32 evaluation of the same restatements (the reference's own
    fp32 error on these inputs), computed once"""
    sd, x, heads, S = case(name)
    sd64, x64 = to(sd, torch.float64), x.double()
    g64, f64 = full(sd64, x64, heads, S)
    fo64 = folded(sd64, x64, heads, S)
    g32, f32 = full(sd, x, heads, S)
    return dict(glob=g64, fmap=f64, folded=fo64, e_glob=rel_err(g32, g64), e_fmap=rel_err(f32, f64),
                e_folded=rel_err(folded(sd, x, heads, S), fo64))


# ------------------------------------------------------------------------------------------------------------------- bounds
def tokens_bounds(pos, x, S):
    """element-wise bound [B, hw+1, C] (float64) of the tokens kernel against tokens() in float64"""
    pos, x = pos.double(), x.double()
    B, h, w, C = x.shape
    hw = h * w
    t = x.reshape(B, hw, C)
    mean = (hw + 2) * U * t.abs().sum(dim=1, keepdim=True) / hw + U * pos[0].abs()
    wp = pos_grid(pos.abs(), S, h, w)                      # sum_k w_k |p_k|: the weights are non-negative
    pix = 8 * U * wp + 2 * U * (t.abs() + pos_grid(pos, S, h, w).abs())
    return torch.cat([mean, pix], dim=1)


def pool_bounds(T, Uq, scale):
    """-> element-wise bounds (bP [B,heads,L], bpooled [B,heads,C]) of the pool kernel against pool() in float64"""
    T, Uq = T.double(), Uq.double()
    B, L, C = T.shape
    s = torch.einsum("bjc,bhc->bhj", T, Uq) * scale
    lse = torch.logsumexp(s, dim=-1, keepdim=True)
    p = torch.exp(s - lse)
    es = (C + 2) * U * scale * torch.einsum("bjc,bhc->bhj", T.abs(), Uq.abs())
    ew = es + U * (M.C_EXP + 1 + M.EXP_SLOPE * (s - lse).abs())
    A = (p * ew).sum(dim=-1, keepdim=True)
    eP = p * (ew + A + (L + 2) * U) + M.TINY
    bpooled = torch.einsum("bhj,bjc->bhc", eP, T.abs()) + (L + 2) * U * torch.einsum("bhj,bjc->bhc", p, T.abs())
    return eP, bpooled


def worst_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound (0 / 0 counts as 0)"""
    err = (got.double().cpu() - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())
