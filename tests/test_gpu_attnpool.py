"""CLIP's attention pooling on the MI355X: the two kernels against fp64 with derived element-wise bounds (tests/oracle_attnpool.py),
both module forms against fp64 relative to the reference's own fp32 error, CLIP.forward end to end, and what must not have moved.

Measured on the MI355X (e = max |got - f64| / max |f64| per output tensor; limit = 8 x the e of the float32 evaluation of the same
restatement, computed in the test; see DESIGN.md section 20 for the table):
  case   arithmetic  global_feat  feature_map  global_only   (fp32 restatement: global_feat / feature_map / global_only)
  3x3    x3          3.11e-07     4.49e-07     2.41e-07      (2.40e-07 / 4.77e-07 / 1.70e-07)
  3x3    h2          2.16e-07     2.32e-07     2.41e-07
  5x4    x3          3.06e-07     3.20e-07     3.71e-07      (3.75e-07 / 4.55e-07 / 2.28e-07)
  5x4    h2          2.10e-07     2.41e-07     3.71e-07
  2x2    x3          2.93e-07     2.84e-07     3.11e-07      (2.40e-07 / 3.54e-07 / 1.78e-07)
  2x2    h2          2.30e-07     1.64e-07     3.11e-07
  rn50   x3          7.80e-07     1.15e-06     6.21e-07      (3.02e-07 / 5.50e-07 / 5.93e-07)
  rn50   h2          2.58e-07     4.20e-07     6.21e-07
Every case is within 2.6 x the fp32 restatement's error, against the limit of 8 x.  (The fp32 restatement's figure depends on the host's
BLAS; the limit is computed where the test runs.)  The kernels alone sit at 0.49 of their derived bound at most (tokens) and 0.005 (pool);
CLIP.forward on the seed-filled RN50 is within 1.1e-06 of the fp64 logits (limit 2e-4).
"""
import functools
import math

import pytest
import torch

import oracle_attnpool as A
from oracle import tris_oracle as O

pytestmark = pytest.mark.gpu

U = A.U


@pytest.fixture(params=["x3", "h2"])
def arith(request):
    """both arithmetics of the dense products (the module and end-to-end tests)"""
    from tris_amd import ops
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(request.param)
    yield request.param
    ops.set_gemm_mode(prev)


@functools.lru_cache(maxsize=None)
def _module_of(C, heads, out, S):
    from tris_amd.CLIP.clip.model import AttentionPool2d
    m = AttentionPool2d(S, C, heads, out)
    m.load_state_dict({k[len(A.PREFIX) + 1:]: v for k, v in A._module(C, heads, out, S).items()})
    return m.cuda().eval()


def module_of(name):
    B, C, heads, out, S, h, w = A.CASES[name]
    return _module_of(C, heads, out, S)


# ------------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("name", list(A.CASES))
def test_tokens_against_fp64(name):
    from tris_amd import ops
    sd, x, heads, S = A.case(name)
    pos = sd[A.PREFIX + ".positional_embedding"]
    got = ops.attnpool_tokens(x.cuda(), pos.cuda(), S)
    again = ops.attnpool_tokens(x.cuda(), pos.cuda(), S)
    B, h, w, C = x.shape
    assert tuple(got.shape) == (B, h * w + 1, C) and torch.equal(got, again)       # a launch is bitwise repeatable
    ref, bound = A.tokens(pos.double(), x.double(), S), A.tokens_bounds(pos, x, S)
    r_mean, r_pix = A.worst_ratio(got[:, :1], ref[:, :1], bound[:, :1]), A.worst_ratio(got[:, 1:], ref[:, 1:], bound[:, 1:])
    print(f"tokens {name}: worst error / bound: mean row {r_mean:.3f}, pixel rows {r_pix:.3f}")
    assert r_mean <= 1.0 and r_pix <= 1.0
    if name == "3x3":            # S x S onto S x S: the resize is the identity and the pixel rows are x + pos, bit for bit
        assert torch.equal(got[:, 1:].cpu(), x.reshape(B, h * w, C) + pos[1:])


@functools.lru_cache(maxsize=None)
def _pool_case(name, spread):
    """-> T [B,L,C], U [B,heads,C] float32 (CPU), scale.  spread: U rescaled so that the logits reach +-spread (0: as they come)"""
    sd, x, heads, S = A.case(name)
    T = A.tokens(sd[A.PREFIX + ".positional_embedding"], x, S)
    Uq = A.folded_query(sd, T, heads).contiguous()
    scale = 1.0 / math.sqrt(T.shape[2] // heads)
    if spread:
        s = torch.einsum("bjc,bhc->bhj", T.double(), Uq.double()) * scale
        Uq = (Uq * (spread / float(s.abs().max()))).contiguous()
    return T, Uq, scale


@pytest.mark.parametrize("name,spread", [(n, 0) for n in A.CASES] + [("5x4", 40), ("rn50", 40)])
def test_pool_against_fp64(name, spread):
    from tris_amd import ops
    T, Uq, scale = _pool_case(name, spread)
    B, L, C = T.shape
    Pg, pooled = ops.attnpool_pool(T.cuda(), Uq.cuda(), scale)
    assert tuple(Pg.shape) == (B, Uq.shape[1], L) and tuple(pooled.shape) == tuple(Uq.shape) and pooled.is_contiguous()
    Pr, pr = A.pool(T.double(), Uq.double(), scale)
    bP, bp = A.pool_bounds(T, Uq, scale)
    if spread:
        s = torch.einsum("bjc,bhc->bhj", T.double(), Uq.double()) * scale
        assert float(s.max()) > 0.9 * spread or float(s.min()) < -0.9 * spread       # exp(s) itself would overflow float32 at 89
        assert float((s.max(-1).values - s.min(-1).values).max()) > spread
    rows = float((Pg.double().sum(-1) - 1.0).abs().max())
    rP, rp = A.worst_ratio(Pg, Pr, bP), A.worst_ratio(pooled, pr, bp)
    print(f"pool {name} spread {spread}: |row sum - 1| {rows / U:.2f} u (limit {L + 4} u); worst error / bound: P {rP:.3f}, pooled {rp:.3f}")
    assert rows <= (L + 4) * U
    assert rP <= 1.0 and rp <= 1.0
    # the head-major layout a per-head batched product writes: taken without a copy, pooled comes back in the same layout, same bytes
    U_hm = Uq.cuda().transpose(0, 1).contiguous().transpose(0, 1)
    P2, pooled2 = ops.attnpool_pool(T.cuda(), U_hm, scale)
    assert pooled2.transpose(0, 1).is_contiguous() and torch.equal(P2, Pg) and torch.equal(pooled2, pooled)


# ------------------------------------------------------------------------------------------------------------------ modules
@pytest.mark.parametrize("name", list(A.CASES))
def test_module_forms_against_fp64(name, arith):
    m = module_of(name)
    sd, x, heads, S = A.case(name)
    B, h, w, C = x.shape
    ref = A.module_reference(name)
    xc = x.cuda()
    with torch.no_grad():
        glob, fmap = m(xc)                               # channels-last, as forward_cl returns it
        glob_n, fmap_n = m(xc.permute(0, 3, 1, 2))       # NCHW-shaped view, as the reference's callers pass it: same buffer, same bytes
        g_only = m(xc, global_only=True)
        glob_c, fmap_c = m(xc.permute(0, 3, 1, 2).contiguous())    # NCHW in memory too: transposed by ops.nchw_to_nhwc first
    assert torch.equal(glob, glob_c) and torch.equal(fmap, fmap_c)
    out = ref["glob"].shape[1]
    assert tuple(glob.shape) == (B, out) and tuple(fmap.shape) == (B, out, h, w) and tuple(g_only.shape) == (B, out)
    assert torch.equal(glob, glob_n) and torch.equal(fmap, fmap_n)
    e = dict(glob=A.rel_err(glob, ref["glob"]), fmap=A.rel_err(fmap, ref["fmap"]), folded=A.rel_err(g_only, ref["folded"]))
    lim = dict(glob=8 * ref["e_glob"], fmap=8 * ref["e_fmap"], folded=8 * ref["e_folded"])
    print(f"module {name} [{arith}]: e = " + ", ".join(f"{k} {e[k]:.3g} (fp32 restatement {lim[k] / 8:.3g}, limit {lim[k]:.3g})" for k in e))
    assert e["glob"] <= lim["glob"] and e["fmap"] <= lim["fmap"] and e["folded"] <= lim["folded"]
    # the folded form agrees with token 0 of the full form within the sum of the two limits
    both = float((g_only.double() - glob.double()).abs().max().cpu() / ref["glob"].abs().max())
    assert both <= lim["glob"] + lim["folded"], both
    # the reference's layout [B, out, h, w]: a value at a position no transposition maps onto itself
    b, c, y, xx = B - 1, 5, h - 1, 0
    assert abs(float(fmap[b, c, y, xx]) - float(ref["fmap"][b, c, y, xx])) <= lim["fmap"] * float(ref["fmap"].abs().max())
    if h * w > 1 and (h - 1, 0) != (0, w - 1):
        assert abs(float(ref["fmap"][b, c, y, xx]) - float(ref["fmap"][b, c, 0, w - 1])) > 1e-3    # (the check can tell them apart)


# --------------------------------------------------------------------------------------------------------------- end to end
def _ids(n, L, seed):
    """n token rows [n, L]: start token, words, the end token (the largest id: encode_text reads that row) at a different place each"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(n, L, dtype=torch.int64)
    for i, ln in enumerate([5, 9, L][:n]):
        ids[i, 0] = 49406
        ids[i, 1:ln - 1] = torch.randint(1, 49000, (ln - 2,), generator=g)
        ids[i, ln - 1] = 49407
    return ids


@functools.lru_cache(maxsize=None)
def _clip(arch):
    import warnings
    from tris_amd.CLIP import clip
    from tris_amd.utils.synth import seed_fill
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m, _ = clip.load(arch, device="cuda", txt_length=20)
    seed_fill(m.state_dict(), 2020)
    return m.eval()


def _compose(m, img, ids):
    from tris_amd import ops
    with torch.no_grad():
        fi = ops.l2norm(m.encode_image_pooled(img))
        ft = ops.l2norm(m.encode_text(ids)[1])
        return ops.matmul(fi, ft, tB=True) * m.logit_scale.exp()


def test_clip_forward_rn50_end_to_end(arith):
    m = _clip("RN50")
    img = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(31))     # c4 is 2 x 2: the 7 x 7 grid shrinks
    ids = _ids(3, 20, 32)
    with torch.no_grad():
        li, lt = m(img.cuda(), ids.cuda())
    assert tuple(li.shape) == (2, 3) and tuple(lt.shape) == (3, 2) and torch.equal(lt, li.t())
    assert torch.equal(li, _compose(m, img.cuda(), ids.cuda()))                      # bit for bit what the pieces give
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    with torch.no_grad():
        fi = O.encode_image_rn(sd, "", img.double(), False, with_attnpool=True)[4][0]
        ft = O.encode_text(sd, "", ids)[1]
        want = sd["logit_scale"].exp() * (fi / fi.norm(dim=1, keepdim=True)) @ (ft / ft.norm(dim=1, keepdim=True)).t()
    err = float((li.double().cpu() - want).abs().max())
    print(f"CLIP.forward RN50 [{arith}]: logits max |err| vs fp64 {err:.3g} (logits up to {float(want.abs().max()):.3g})")
    assert err < 2e-4            # the eval-mode trunk tolerance of tests/test_gpu_parity.py:97


def test_clip_forward_vit_goes_through_the_same_call(arith):
    m = _clip("ViT-B-32")
    img = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(33))
    ids = _ids(3, 20, 34)
    with torch.no_grad():
        li, lt = m(img.cuda(), ids.cuda())
        emb = m.encode_image_pooled(img.cuda())
    assert tuple(li.shape) == (2, 3) and torch.equal(lt, li.t()) and bool(torch.isfinite(li).all())
    assert tuple(emb.shape) == (2, 512) and torch.equal(li, _compose(m, img.cuda(), ids.cuda()))
    assert float(li.abs().max()) <= float(m.logit_scale.detach().exp()) * (1 + 1e-5)          # cosines times the scale


# ------------------------------------------------------------------------------------------------------ nothing else moved
def test_default_forward_still_returns_none_and_pool_is_opt_in():
    m = _clip("RN50")
    img = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(31)).cuda()
    with torch.no_grad():
        outs = m.encode_image(img)
        pooled = m.visual(img, pool=True)
        direct = m.visual.attnpool(pooled[3])
    assert len(outs) == 5 and outs[4] is None
    assert all(getattr(p, "_tris_no_grad_path", False) for p in m.visual.attnpool.parameters())
    assert all(torch.equal(a, b) for a, b in zip(outs[:4], pooled[:4]))
    assert isinstance(pooled[4], list) and len(pooled[4]) == 2
    x_global, x_local = pooled[4]
    assert tuple(x_global.shape) == (2, 1024) and tuple(x_local.shape) == (2, 1024, 2, 2)
    assert torch.equal(x_global, direct[0]) and torch.equal(x_local, direct[1])
    with pytest.raises(NotImplementedError, match="AttentionPool2d"):
        m.visual.attnpool(pooled[3].clone().requires_grad_())
