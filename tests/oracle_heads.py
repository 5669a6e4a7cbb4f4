"""fp64 restatement of the Stage-1 head kernels (csrc/heads.hip, csrc/bilinear.h) on the CPU, the inputs the kernel tests
feed them, and the error bounds those tests assert.  Shared by tests/test_heads_host.py (CPU) and tests/test_gpu_heads.py.

Class head.  model_stage1.py:80-108 with torch autograd; `dtype` selects float64 (the reference) or float32 (the same
expression at the kernels' precision: its error against float64 is the yardstick of the class-head tolerance).  torch.max on
the CPU sends the gradient of a tied maximum to the first maximal pixel, which is what cls_head_bwd_kernel's tie-break restates.

Bilinear family.  F.interpolate(mode="bilinear") on float64.  The kernels, like PyTorch in float32, form the source position
in float32: one rounding of the scale, one of the product, and half an ulp of the position where the product is contracted
into the weight's subtraction (the note in bilinear.h).  Each is at most 2^-24 relative to a position < in, so a weight is off by
at most

    delta(in) = 4 * 2^-24 * max(1, in)                                      per axis.

Bilinear interpolation is continuous in the position, so an index that flips at an integer position costs no more than that.
The blend itself is three float32 lerps.  Hence, with U = 2^-24:

    forward, per plane:        (delta(Hi) + delta(Wi)) * (max x - min x) + 8 U max|x|
    backward, per input pixel: (delta(Hi) + delta(Wi)) * n_y n_x max|g| + 8 U (A^T |g|)

n_a = ceil(2 out_a / in_a) + 2 bounds the outputs that reference one input along an axis and A^T |g| is the float64 backward of
|g|.  Derived, not measured; tests/test_heads_host.py checks that PyTorch's own float32 kernels stay inside them.
"""
import functools
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24

# ------------------------------------------------------------------------------------------------------------ class head
CLS_SHAPES = [(1, 1, 1), (2, 25, 5), (3, 64, 3), (2, 65, 2), (2, 130, 70), (66, 9, 66), (2, 400, 40)]
CLS_LARGE = (2, 400, 40)       # past the 60000-byte switch to the raised dynamic-LDS limit
CLS_REFUSED = (1, 1024, 40)    # past the 150 KB the entry points accept
FOCAL = [(3.0, 0.01), (2.0, 0.05), (1.0, 0.5)]
CLS_KINDS = ["randn3", "randn40", "ones", "ties"]
# planted equal maxima: same lane of the pixel loop, neighbouring lanes, a later pixel in a lower lane, a three-way tie
TIE_GROUPS = [(3, 67), (5, 6), (70, 9), (5, 6, 129)]


def cls_lds_bytes(P, N, backward):
    """dynamic LDS of cls_head_{fwd,bwd}_kernel (the expressions of the entry points in heads.hip)"""
    return 4 * (P * (N + 1) + (3 * P + 3 * N if backward else 2 * P))


def tie_slots(B, P, N):
    """-> [(image, sentence, pixels)]: every group of TIE_GROUPS that fits P, each in a column of its own"""
    slots = [(b, j) for b in range(B) for j in range(N)]
    fit = [g for g in TIE_GROUPS if max(g) < P]
    return [(b, j, g) for (b, j), g in zip(slots, fit)]


@functools.lru_cache(maxsize=None)
def cls_inputs(shape, kind):
    """-> (score [B,P,N], g [B,N]) float32"""
    B, P, N = shape
    gen = torch.Generator().manual_seed(1000 + 7 * B + 3 * P + N + CLS_KINDS.index(kind))
    g = torch.randn(B, N, generator=gen)
    if kind == "ones":
        return torch.ones(B, P, N), g
    score = torch.randn(B, P, N, generator=gen) * (40.0 if kind == "randn40" else 3.0)
    if kind == "ties":
        for b, j, pix in tie_slots(B, P, N):
            score[b, list(pix), j] = score[b, :, j].max() + 1.0
    return score, g


def cls_head(score, g, focal_p, focal_c, dtype=torch.float64):
    """-> cls_out [B,N], cls_fg [min(B,N)], dscore [B,P,N], and the part of dscore that comes through the max alone"""
    s = score.detach().to(dtype).requires_grad_(True)
    B, P, N = s.shape
    st = s.transpose(1, 2)                                       # [B, N, P]: the reference's [B, N, h, w], pixels flattened
    st = torch.cat([torch.ones_like(st[:, :1]), st], 1)
    masks = torch.softmax(st, 1)
    mm = masks.mean(-1)
    cls_11 = torch.max(st, dim=-1).values
    cls_out = (st.mean(-1) + cls_11 + torch.pow(1 - mm, focal_p) * torch.log(focal_c + mm))[:, 1:]
    idx = torch.arange(min(B, N))
    cls_fg = mm[idx, 1 + idx]
    gd = g.to(dtype)
    (dscore,) = torch.autograd.grad((cls_out * gd).sum(), s, retain_graph=True)
    (dmax,) = torch.autograd.grad((cls_11[:, 1:] * gd).sum(), s)
    return cls_out.detach(), cls_fg.detach(), dscore, dmax


@functools.lru_cache(maxsize=None)
def cls_reference(shape, kind, focal):
    """-> (fp64 outputs, err_cpu32 per output): the float32 CPU evaluation of the same expression against float64"""
    score, g = cls_inputs(shape, kind)
    ref = cls_head(score, g, *focal)
    f32 = cls_head(score, g, *focal, dtype=torch.float32)
    err32 = [float((a.double() - b).abs().max()) for a, b in zip(f32[:3], ref[:3])]
    return ref, err32


def cls_tolerance(err32, ref):
    return max(4.0 * err32, 32.0 * U * float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------------------ bilinear family
def delta(n_in):
    return 4.0 * U * max(1, n_in)


def n_refs(n_out, n_in):
    return math.ceil(2.0 * n_out / n_in) + 2


def resize(x, size, align):
    """x [.., Hi, Wi] -> float64 [.., Ho, Wo]"""
    x = x.double()
    lead = x.shape[:-2]
    y = F.interpolate(x.reshape(1, -1, *x.shape[-2:]), size=tuple(size), mode="bilinear", align_corners=bool(align))
    return y.reshape(*lead, *size)


def resize_adjoint(g, in_size, align):
    """the float64 backward of `resize`: g [.., Ho, Wo] -> [.., Hi, Wi]"""
    g = g.double()
    x = torch.zeros(*g.shape[:-2], *in_size, dtype=torch.float64, requires_grad=True)
    (dx,) = torch.autograd.grad(resize(x, g.shape[-2:], align), x, g)
    return dx


def resize_fwd_bound(x):
    """per plane, broadcastable against the output: [.., 1, 1]"""
    x = x.double()
    Hi, Wi = x.shape[-2:]
    hi, lo = x.amax((-2, -1), keepdim=True), x.amin((-2, -1), keepdim=True)
    return (delta(Hi) + delta(Wi)) * (hi - lo) + 8.0 * U * x.abs().amax((-2, -1), keepdim=True)


def resize_bwd_bound(g, in_size, align):
    """per input pixel: [.., Hi, Wi]"""
    g = g.double()
    Hi, Wi = in_size
    Ho, Wo = g.shape[-2:]
    gmax = g.abs().amax((-2, -1), keepdim=True)
    return ((delta(Hi) + delta(Wi)) * n_refs(Ho, Hi) * n_refs(Wo, Wi) * gmax
            + 8.0 * U * resize_adjoint(g.abs(), in_size, align))


def _paired(axis, shift):
    """every (in, out) of `axis` on the row axis of one case and on the column axis of another"""
    return [(hi, axis[(k + shift) % len(axis)][0], ho, axis[(k + shift) % len(axis)][1]) for k, (hi, ho) in enumerate(axis)]


RESIZE_EXTRA = [(320, 224), (10, 320), (40, 11), (7, 3)]


def resize_cases():
    """(Hi, Wi, Ho, Wo, align): in 1..9 x out 1..20 x both conventions, plus the model's own ratios"""
    axis = [(i, o) for i in range(1, 10) for o in range(1, 21)]
    cases = []
    for align in (False, True):
        cases += [c + (align,) for c in _paired(axis, 67)]
        cases += [(i, i, o, o, align) for i, o in RESIZE_EXTRA]
    return cases


def nhwc_cases():
    """(Hi, Wi, Ho, Wo): the same sweep restricted to out >= in (align_corners=False is the only convention of upsample_nhwc)"""
    axis = [(i, o) for i in range(1, 10) for o in range(i, 21)]
    return _paired(axis, 53) + [(i, i, o, o) for i, o in RESIZE_EXTRA if o >= i]


GRID_CAP_CASE = (9, 16, 16, 512, 512, False)                            # planes first: 2.36 M outputs against 8192 * 256


def resize_inputs(case, planes=2):
    """-> (x [planes, Hi, Wi], g [planes, Ho, Wo]) float32"""
    Hi, Wi, Ho, Wo, align = case
    gen = torch.Generator().manual_seed(((Hi * 331 + Wi) * 331 + Ho) * 331 + Wo + int(align))
    return torch.randn(planes, Hi, Wi, generator=gen), torch.randn(planes, Ho, Wo, generator=gen)


def nhwc_inputs(case, B=2, C=4):
    """-> (x [B,Hi,Wi,C], skip, d_up, d_sum [B,Ho,Wo,C]) float32"""
    Hi, Wi, Ho, Wo = case
    gen = torch.Generator().manual_seed(((Hi * 331 + Wi) * 331 + Ho) * 331 + Wo + 5)
    return (torch.randn(B, Hi, Wi, C, generator=gen),) + tuple(torch.randn(B, Ho, Wo, C, generator=gen) for _ in range(3))


# ------------------------------------------------------------------------------------------------------------ response maps
# (h, w, S): non-square grids, an S*S that ends inside a 256-thread block, the 1024-pixel limit, a down-scale.  The seed of each
# is one for which no pre-activation lies within 1e-5 of the relu kink (asserted in tests/test_heads_host.py).
MAPS_CASES = [(1, 1, 3), (5, 8, 20), (8, 5, 33), (10, 10, 17), (32, 32, 40), (6, 4, 5)]
MAPS_SEED = {(1, 1, 3): 0, (5, 8, 20): 0, (8, 5, 33): 0, (10, 10, 17): 0, (32, 32, 40): 1, (6, 4, 5): 0}
MAPS_B = 3
MAPS_KINK = 1e-5


@functools.lru_cache(maxsize=None)
def maps_inputs(case):
    """-> (score [B, h*w, B], g_cls [B,B], d_relu, d_sig [B,1,S,S]) float32"""
    h, w, S = case
    gen = torch.Generator().manual_seed(MAPS_SEED[case] * 7919 + h * 97 + w * 13 + S)
    B = MAPS_B
    return (torch.randn(B, h * w, B, generator=gen) * 3.0, torch.randn(B, B, generator=gen),
            torch.randn(B, 1, S, S, generator=gen), torch.randn(B, 1, S, S, generator=gen))


def maps_diag(score, h, w):
    B = score.shape[0]
    return torch.stack([score[i, :, i].reshape(1, h, w) for i in range(B)], 0)       # model_stage1.py:110-113


def maps(score, h, w, S, d_relu=None, d_sig=None):
    """-> (pre-activation v, relu(v), sigmoid(v) [B,1,S,S], dscore [B,P,N]) in float64"""
    s = score.detach().double().requires_grad_(True)
    v = F.interpolate(maps_diag(s, h, w), size=(S, S), mode="bilinear", align_corners=False)
    r, sg = F.relu(v), torch.sigmoid(v)
    loss = (v * 0.0).sum()
    if d_relu is not None:
        loss = loss + (r * d_relu.double()).sum()
    if d_sig is not None:
        loss = loss + (sg * d_sig.double()).sum()
    (dscore,) = torch.autograd.grad(loss, s)
    return v.detach(), r.detach(), sg.detach(), dscore


def maps_bounds(score, h, w, S, d_relu=None, d_sig=None):
    """-> (relu bound, sigmoid bound [B,1,1,1], bound of the diagonal's gradient [B,1,h,w]).
    relu is 1-Lipschitz and sigmoid 1/4-Lipschitz in the pre-activation, whose bound is the resize's; 1/(1 + expf(-v)) adds a few
    roundings on a value <= 1 (8 U).  Backward: the gradient that enters the resize's adjoint is d_relu [v > 0] + d_sig s (1 - s);
    |d/dv s(1-s)| < 0.1, so it is off by at most |d_sig| (0.1 fb + 8 U) plus its own rounding, and that error goes through A^T."""
    v, _, sg, _ = maps(score, h, w, S)
    fb = resize_fwd_bound(maps_diag(score, h, w))
    ge = torch.zeros_like(v)
    dge = torch.zeros_like(v)
    if d_relu is not None:
        ge = ge + d_relu.double() * (v > 0)
    if d_sig is not None:
        ge = ge + d_sig.double() * sg * (1 - sg)
        dge = dge + d_sig.double().abs() * (0.1 * fb + 8.0 * U)
    dge = dge + 2.0 * U * ge.abs()
    bwd = resize_bwd_bound(ge, (h, w), False) + resize_adjoint(dge, (h, w), False)
    return fb, fb / 4 + 8.0 * U, bwd


# ------------------------------------------------------------------------------------------------------------ patches, tokens
FG_CASES = [(1, 3, 32, 32), (2, 3, 96, 32), (3, 1, 8, 2), (12, 3, 256, 32)]     # the last: past the 8192-block grid cap
VIT_CASES = [(1, 2, 4), (3, 5, 96), (2, 50, 768)]


def fg_layout(fg, ps):
    """[B,C,R,R] -> the patch-GEMM operand [B, (R/ps)^2, C*ps*ps] (the reshape of test_fg_patches_and_vit_assemble)"""
    B, C, R, _ = fg.shape
    G = R // ps
    return fg.reshape(B, C, G, ps, G, ps).permute(0, 2, 4, 1, 3, 5).reshape(B, G * G, C * ps * ps)


def fg_unlayout(dp, C, R, ps):
    """the inverse of fg_layout: [B, G*G, C*ps*ps] -> [B,C,R,R]"""
    B = dp.shape[0]
    G = R // ps
    return dp.reshape(B, G, G, C, ps, ps).permute(0, 3, 1, 4, 2, 5).reshape(B, C, R, R)
