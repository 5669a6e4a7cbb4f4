"""The four row-wise normalisations on the MI355X, through the C ABI, against the fp64 restatement of tests/oracle_rownorm.py:
LayerNorm and InstanceNorm (csrc/norm.hip), l2norm and softmax (csrc/heads.hip), forward and backward.  Every output finite and inside
the element-wise bound derived there on every input kind and shape (outputs pre-filled with NaN, so an unwritten element fails);
launch-to-launch repeatability; the LayerNorm backward under both settings of LN_BWD_BLOCKS and with each optional pointer; the
LayerNorm forward under a row limit; the h2 amax by-product of the four norm.hip kernels bit for bit; the argument contracts of the
eight entry points; and the ops wrappers bit-identical to the chain of ABI calls.  The ratios err / bound measured on the MI355X are
in profiles/rownorm_parity_floor.txt (`python tests/test_gpu_rownorm.py > profiles/rownorm_parity_floor.txt`).
"""
import math

import pytest
import torch

import oracle_rownorm as OR
from test_gpu_bn import _Arena, _refused

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = 12345.0
_id = lambda c: "-".join("x".join(map(str, p)) if isinstance(p, tuple) else str(p) for p in c)
LN_CASES = [(k, s) for k in OR.LN_KINDS for s in OR.LN_SHAPES]
IN_CASES = [(k, s) for k in OR.IN_KINDS for s in OR.IN_SHAPES]
L2_CASES = [(k, s) for k in OR.L2_KINDS for s in OR.L2_SHAPES]
SM_CASES = [(k, s) for k in OR.SM_KINDS for s in OR.SM_SHAPES]

REC = {}            # (kernel, output, kind, shape) -> largest err / bound
ASSERT = True       # (the profile mode records without asserting)


def _inside(got, ref, bound, key):
    got = got.detach().double().cpu().reshape(ref.shape)
    e = (got - ref).abs()
    over = ~(e <= bound)                                                                # (a NaN is outside)
    ratio = float(torch.nan_to_num(e / bound, nan=0.0, posinf=float("inf")).max())     # (0 / 0: an exact output of an exact bound)
    REC[key] = max(REC.get(key, 0.0), ratio)
    print(f"{key}: err / bound up to {ratio:.3f}")
    if ASSERT:
        assert bool(torch.isfinite(got).all()), f"{key}: {int((~torch.isfinite(got)).sum())} elements not finite"
        assert not bool(over.any()), f"{key}: {int(over.sum())} elements outside the bound, err / bound up to {ratio:.3f}"


def _lib():
    from tris_amd import ops
    from tris_amd._lib import query
    return ops, query


def _dev(d, *names):
    return [d[n].cuda() for n in names]


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _same(a, b):
    """two launches wrote the same bits (the outputs are finite wherever they were written)"""
    return all((x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _bits(t):
    return int(t.abs().max().view(torch.int32)) if t.numel() else 0


# ================================================================================================================ launches
def _ln_fwd(ops, x, g, b, stats=True):
    rows, W = x.shape
    y = _nan(rows, W)
    mean, rstd = (_nan(rows), _nan(rows)) if stats else (None, None)
    ops.call("tris_layernorm_fwd_f32", ops.P(x), ops.P(g), ops.P(b), ops.P(y), ops.P(mean), ops.P(rstd), rows, W, OR.EPS, ops._stream())
    return y, mean, rstd


def _ln_ws(query, rows, W, blocks, guard=256):
    """a workspace of exactly tris_layernorm_bwd_workspace_bytes followed by a guard, all sentinels"""
    n = query("tris_layernorm_bwd_workspace_bytes", rows, W)
    assert n == OR.ln_bwd_workspace_bytes(rows, W, blocks), "ln_bwd_rpb is not what tests/oracle_rownorm.py restates"
    return torch.full((n // 4 + guard,), SENTINEL, device="cuda"), n // 4


def _ln_bwd(ops, query, dy, x, g, mean, rstd, extra, blocks, want_dx=True, want_p=True):
    rows, W = x.shape
    ws, n = _ln_ws(query, rows, W, blocks)
    dx = _nan(rows, W) if want_dx else None
    dg, db = (_nan(W), _nan(W)) if want_p else (None, None)
    ops.call("tris_layernorm_bwd_f32", ops.P(dy), ops.P(x), ops.P(g), ops.P(mean), ops.P(rstd), ops.P(dx), ops.P(dg), ops.P(db), rows, W,
             ops.P(ws), ops.P(extra), ops._stream())
    torch.cuda.synchronize()
    assert bool((ws[n:] == SENTINEL).all()), "the workspace guard was written"
    if not want_p:
        assert bool((ws == SENTINEL).all()), "the workspace was written without a parameter gradient"
    return dx, dg, db


def _in_fwd(ops, x, g, b, relu):
    B, P, C = x.shape
    y, mean, is_ = _nan(B, P, C), _nan(B, C), _nan(B, C)
    ops.call("tris_instnorm_fwd_f32", ops.P(x), ops.P(g), ops.P(b), ops.P(y), ops.P(mean), ops.P(is_), B, P, C, OR.EPS, int(relu), ops._stream())
    return y, mean, is_


def _in_bwd(ops, dy, y, x, g, mean, is_, relu):
    B, P, C = x.shape
    dx, dgp, dbp = _nan(B, P, C), _nan(B, C), _nan(B, C)
    ops.call("tris_instnorm_bwd_f32", ops.P(dy), ops.P(y), ops.P(x), ops.P(g), ops.P(mean), ops.P(is_), ops.P(dx), ops.P(dgp), ops.P(dbp),
             B, P, C, int(relu), ops._stream())
    return dx, dgp, dbp


# ================================================================================================================ LayerNorm
@pytest.mark.parametrize("case", LN_CASES, ids=_id)
def test_layernorm_forward(case):
    ops, _ = _lib()
    kind, (rows, W) = case
    d = OR.inputs("ln", kind, (rows, W))
    x, g, b = _dev(d, "x", "gamma", "beta")
    runs = [_ln_fwd(ops, x, g, b) for _ in range(2)]
    assert _same(*runs), "two launches on the same input differ"
    y, mean, rstd = runs[0]
    y0, _, _ = _ln_fwd(ops, x, g, b, stats=False)
    assert torch.equal(y0, y), "mean = rstd = NULL changes Y"
    (m_ref, r_ref), (b_m, b_r) = OR.ln_stats(d["x"])
    key = lambda o: ("layernorm_fwd", o, kind, (rows, W))
    _inside(mean, m_ref, b_m, key("mean"))
    _inside(rstd, r_ref, b_r, key("rstd"))
    _inside(y, *OR.ln_apply(d["x"], mean, rstd, d["gamma"], d["beta"]), key("y | stats"))
    _inside(y, *OR.ln_composed(d["x"], d["gamma"], d["beta"]), key("y composed"))


@pytest.fixture
def ln_blocks():
    """sets the LN_BWD_BLOCKS option for a test and restores the default whatever happens"""
    ops, _ = _lib()
    try:
        yield lambda v: ops.set_option("LN_BWD_BLOCKS", v)
    finally:
        ops.set_option("LN_BWD_BLOCKS", None)


@pytest.mark.parametrize("case", LN_CASES, ids=_id)
def test_layernorm_backward(case, ln_blocks):
    """tris_layernorm_bwd_f32 from the statistics the device forward stored, under LN_BWD_BLOCKS unset and 128, with dX = NULL, with
    dgamma = dbeta = NULL and with `extra`"""
    ops, query = _lib()
    kind, (rows, W) = case
    d = OR.inputs("ln", kind, (rows, W))
    x, g, b, dy, extra = _dev(d, "x", "gamma", "beta", "dy", "extra")
    _, mean, rstd = _ln_fwd(ops, x, g, b)
    key = lambda o: ("layernorm_bwd", o, kind, (rows, W))
    for blocks in OR.LN_BLOCKS:
        ln_blocks(blocks)
        assert query("tris_layernorm_bwd_workspace_bytes", rows, W) == OR.ln_bwd_workspace_bytes(rows, W, blocks)
        runs = [_ln_bwd(ops, query, dy, x, g, mean, rstd, None, blocks) for _ in range(2)]
        assert _same(*runs), "two launches on the same input differ"
        dx, dg, db = runs[0]
        (dx_ref, dg_ref, db_ref), (b_dx, b_dg, b_db) = OR.ln_bwd(d["dy"], d["x"], d["gamma"], mean, rstd, None, blocks)
        _inside(dx, dx_ref, b_dx, key("dx"))
        _inside(dg, dg_ref, b_dg, key("dgamma"))
        _inside(db, db_ref, b_db, key("dbeta"))
        _, dg1, db1 = _ln_bwd(ops, query, dy, x, g, mean, rstd, None, blocks, want_dx=False)
        assert torch.equal(dg1, dg) and torch.equal(db1, db), "dX = NULL changes dgamma / dbeta"
        dx2, _, _ = _ln_bwd(ops, query, dy, x, g, mean, rstd, None, blocks, want_p=False)
        assert torch.equal(dx2, dx), "dgamma = dbeta = NULL changes dX"
        dx3, dg3, db3 = _ln_bwd(ops, query, dy, x, g, mean, rstd, extra, blocks)
        assert torch.equal(dg3, dg) and torch.equal(db3, db), "`extra` changes dgamma / dbeta"
        (dx3_ref, _, _), (b_dx3, _, _) = OR.ln_bwd(d["dy"], d["x"], d["gamma"], mean, rstd, d["extra"], blocks)
        _inside(dx3, dx3_ref, b_dx3, key("dx + extra"))


def _limit_word(limit):
    return torch.tensor([limit, limit], dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("shape,limit", [((5, 100), 3), ((37, 512), 16), ((37, 512), 1), ((2049, 64), 1024), ((4, 512), 4)], ids=str)
def test_layernorm_forward_under_a_row_limit(shape, limit):
    """rows below the limit inside the bound; rows at or above it keep their NaN pre-fill bit for bit, in Y, mean and rstd; the amax
    by-product is that of the written rows"""
    ops, _ = _lib()
    rows, W = shape
    d = OR.inputs("ln", "offset", shape)
    x, g, b = _dev(d, "x", "gamma", "beta")
    x = x.clone()
    x[limit:] = NAN                                          # nothing lives behind the limit
    fill = torch.tensor(0x7FC01234, dtype=torch.int32, device="cuda").view(torch.float32)   # a NaN with a payload of its own
    y, mean, rstd = (fill.expand(s).contiguous() for s in ((rows, W), (rows,), (rows,)))
    am = torch.zeros(2048, dtype=torch.int32, device="cuda")
    word = _limit_word(limit)
    try:
        with ops.rows_limit(word):
            ops.call("tris_amax_next", ops.P(am))
            ops.call("tris_layernorm_fwd_f32", ops.P(x), ops.P(g), ops.P(b), ops.P(y), ops.P(mean), ops.P(rstd), rows, W, OR.EPS, ops._stream())
    finally:
        ops.call("tris_rows_limit_thread", None)
    torch.cuda.synchronize()
    for t in (y, mean, rstd):
        assert bool((t[limit:].view(torch.int32) == 0x7FC01234).all()), "a row at or above the limit was written"
    (m_ref, r_ref), (b_m, b_r) = OR.ln_stats(d["x"][:limit])
    key = lambda o: ("layernorm_fwd", o, "limit", shape)
    _inside(mean[:limit], m_ref, b_m, key("mean"))
    _inside(rstd[:limit], r_ref, b_r, key("rstd"))
    _inside(y[:limit], *OR.ln_apply(d["x"][:limit], mean[:limit], rstd[:limit], d["gamma"], d["beta"]), key("y | stats"))
    _inside(y[:limit], *OR.ln_composed(d["x"][:limit], d["gamma"], d["beta"]), key("y composed"))
    assert int(am.max()) == _bits(y[:limit]), "the amax by-product is not max|Y| of the written rows"
    del word


# ================================================================================================================ InstanceNorm
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", IN_CASES, ids=_id)
def test_instancenorm(case, relu):
    """forward and backward; the backward takes the device forward's statistics and (ReLU) its saved Y, whose sign is the mask given
    to the reference"""
    ops, _ = _lib()
    kind, shape = case
    d = OR.inputs("in", kind, shape)
    x, g, b, dy = _dev(d, "x", "gamma", "beta", "dy")
    runs = [_in_fwd(ops, x, g, b, relu) for _ in range(2)]
    assert _same(*runs), "two launches on the same input differ"
    y, mean, is_ = runs[0]
    (m_ref, r_ref), (b_m, b_r) = OR.in_stats(d["x"])
    key = lambda e, o: (e, o, f"{kind}{'+relu' if relu else ''}", shape)
    _inside(mean, m_ref, b_m, key("instnorm_fwd", "mean"))
    _inside(is_, r_ref, b_r, key("instnorm_fwd", "invstd"))
    _inside(y, *OR.in_apply(d["x"], mean, is_, d["gamma"], d["beta"], relu), key("instnorm_fwd", "y | stats"))
    _inside(y, *OR.in_composed(d["x"], d["gamma"], d["beta"], relu), key("instnorm_fwd", "y composed"))
    runs = [_in_bwd(ops, dy, y if relu else None, x, g, mean, is_, relu) for _ in range(2)]
    assert _same(*runs), "two launches on the same input differ"
    dx, dgp, dbp = runs[0]
    (dx_ref, s1, s0), (b_dx, b_s1, b_s0) = OR.in_bwd(d["dy"], d["x"], d["gamma"], mean, is_, (y > 0) if relu else None)
    _inside(dx, dx_ref, b_dx, key("instnorm_bwd", "dx"))
    _inside(dgp, s1, b_s1, key("instnorm_bwd", "dgamma_part"))
    _inside(dbp, s0, b_s0, key("instnorm_bwd", "dbeta_part"))
    if not relu:      # Y is not read without the ReLU
        assert _same(_in_bwd(ops, dy, y, x, g, mean, is_, 0), runs[0]), "Y changes the backward without a ReLU"


# ================================================================================================================ l2norm
@pytest.mark.parametrize("case", L2_CASES, ids=_id)
def test_l2norm(case):
    ops, _ = _lib()
    kind, (rows, C) = case
    d = OR.inputs("l2", kind, (rows, C))
    x, dy = _dev(d, "x", "dy")
    st = ops._stream()
    runs = []
    for _ in range(2):
        y, inv, dx = _nan(rows, C), _nan(rows), _nan(rows, C)
        ops.call("tris_l2norm_fwd_f32", ops.P(x), ops.P(y), ops.P(inv), rows, C, st)
        ops.call("tris_l2norm_bwd_f32", ops.P(dy), ops.P(y), ops.P(inv), ops.P(dx), rows, C, st)
        runs.append((y, inv, dx))
    assert _same(*runs), "two launches on the same input differ"
    y, inv, dx = runs[0]
    key = lambda e, o: (e, o, kind, (rows, C))
    _inside(inv, *OR.l2_stats(d["x"]), key("l2norm_fwd", "inv_norm"))
    _inside(y, *OR.l2_apply(d["x"], inv), key("l2norm_fwd", "y | inv_norm"))
    _inside(dx, *OR.l2_bwd(d["dy"], y, inv), key("l2norm_bwd", "dx"))


# ================================================================================================================ softmax
@pytest.mark.parametrize("case", SM_CASES, ids=_id)
def test_softmax(case):
    ops, _ = _lib()
    kind, (rows, n) = case
    dy_h = OR.inputs("sm", kind, (rows, n))["dy"]
    dy = dy_h.cuda()
    st = ops._stream()
    for scale in OR.SM_SCALES:
        x_h = OR.sm_x(kind, (rows, n), scale)
        x = x_h.cuda()
        runs = []
        for _ in range(2):
            y, dx = _nan(rows, n), _nan(rows, n)
            ops.call("tris_softmax_fwd_f32", ops.P(x), ops.P(y), rows, n, scale, st)
            ops.call("tris_softmax_bwd_f32", ops.P(dy), ops.P(y), ops.P(dx), rows, n, scale, st)
            runs.append((y, dx))
        assert _same(*runs), "two launches on the same input differ"
        y, dx = runs[0]
        key = lambda e, o: (e, o, kind, (rows, n))
        _inside(y, *OR.sm_fwd(x_h, scale), key("softmax_fwd", "y"))
        _inside(dx, *OR.sm_bwd(dy_h, y, scale), key("softmax_bwd", "dx"))


# ================================================================================================================ amax by-product
def _armed(ops, launch):
    """-> (what launch() returned, the 2048-word buffer it was armed with)"""
    am = torch.zeros(2048, dtype=torch.int32, device="cuda")
    ops.call("tris_amax_next", ops.P(am))
    out = launch()
    torch.cuda.synchronize()
    return out, am


def _amax_is(am, t, what):
    assert int(am.max()) == _bits(t), f"{what}: the amax by-product is not max |out|, bit for bit"
    assert not bool(am.view(-1, 16)[:, 1:].any()), f"{what}: a word other than every 16th was used"


def _unarmed_leaves(ops, launch, what):
    """the arming is one-shot: the launch after an armed one leaves the buffer, refilled with a sentinel, untouched"""
    _, am = _armed(ops, launch)
    am.fill_(0x5A5A5A5A)
    launch()
    torch.cuda.synchronize()
    assert bool((am == 0x5A5A5A5A).all()), what


@pytest.mark.parametrize("case", [("randn", (37, 512)), ("offset", (5, 100)), ("gamma", (5, 1024)), ("randn", (2049, 64)), ("tiny", (5003, 8))],
                         ids=_id)
def test_layernorm_amax_by_product(case, ln_blocks):
    ops, query = _lib()
    kind, shape = case
    d = OR.inputs("ln", kind, shape)
    x, g, b, dy, extra = _dev(d, "x", "gamma", "beta", "dy", "extra")
    fwd = lambda: _ln_fwd(ops, x, g, b)
    (y, mean, rstd), am = _armed(ops, fwd)
    _amax_is(am, y, "layernorm_fwd")
    assert _same(fwd(), (y, mean, rstd)), "the arming changes the outputs"
    for blocks in OR.LN_BLOCKS:
        ln_blocks(blocks)
        for ex in (None, extra):
            bwd = lambda **kw: _ln_bwd(ops, query, dy, x, g, mean, rstd, ex, blocks, **kw)
            (dx, dg, db), am = _armed(ops, bwd)
            _amax_is(am, dx, "layernorm_bwd")
            assert _same(bwd(), (dx, dg, db)), "the arming changes the outputs"
        _, am = _armed(ops, lambda: bwd(want_dx=False))
        assert not bool(am.any()), "layernorm_bwd with dX = NULL left an amax"
        _unarmed_leaves(ops, bwd, "an unarmed layernorm_bwd wrote an amax")
    _unarmed_leaves(ops, fwd, "an unarmed layernorm_fwd wrote an amax")


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", [("randn", (3, 100, 128)), ("offset", (2, 5, 65)), ("gamma", (2, 3, 63)), ("randn", (1, 1600, 64)),
                                  ("outlier", (2, 100, 1024))], ids=_id)
def test_instancenorm_amax_by_product(case, relu):
    ops, _ = _lib()
    kind, shape = case
    d = OR.inputs("in", kind, shape)
    x, g, b, dy = _dev(d, "x", "gamma", "beta", "dy")
    fwd = lambda: _in_fwd(ops, x, g, b, relu)
    (y, mean, is_), am = _armed(ops, fwd)
    _amax_is(am, y, "instnorm_fwd")
    assert _same(fwd(), (y, mean, is_)), "the arming changes the outputs"
    bwd = lambda: _in_bwd(ops, dy, y, x, g, mean, is_, relu)
    out, am = _armed(ops, bwd)
    _amax_is(am, out[0], "instnorm_bwd")
    assert _same(bwd(), out), "the arming changes the outputs"
    _unarmed_leaves(ops, fwd, "an unarmed instnorm_fwd wrote an amax")
    _unarmed_leaves(ops, bwd, "an unarmed instnorm_bwd wrote an amax")


# ================================================================================================================ contracts
def test_entry_points_refuse_what_the_kernels_cannot_index():
    """every call outside the contracts of include/tris_hip.h returns hipErrorInvalidValue before any launch: a sentinel-filled arena
    that every pointer points into is untouched afterwards"""
    ops, _ = _lib()
    A = _Arena()
    p = [A.p(k) for k in range(10)]
    eps = OR.EPS

    def each_null(name, ptrs, tail, optional=()):
        for k in range(len(ptrs)):
            if k not in optional:
                _refused(ops, name, *ptrs[:k], None, *ptrs[k + 1:], *tail)
    # LayerNorm forward (X, gamma, beta, Y, mean, rstd, rows, W, eps)
    for rows, W in ((0, 8), (-1, 8), (8, 0), (8, 2), (8, -4), (8, 6), (8, 1028)):
        _refused(ops, "tris_layernorm_fwd_f32", *p[:6], rows, W, eps)
        _refused(ops, "tris_layernorm_bwd_f32", *p[:8], rows, W, p[8], p[9])
        _refused(ops, "tris_layernorm_bwd_f32", *p[:8], rows, W, p[8], None)
    each_null("tris_layernorm_fwd_f32", p[:6], (8, 8, eps))                  # (one of mean / rstd NULL among them)
    # LayerNorm backward (dY, X, gamma, mean, rstd, dX, dgamma, dbeta, rows, W, workspace, extra)
    each_null("tris_layernorm_bwd_f32", p[:8], (8, 8, p[8], None), optional=(5,))     # (one of dgamma / dbeta NULL among them)
    _refused(ops, "tris_layernorm_bwd_f32", *p[:8], 8, 8, None, None)        # parameter gradients without a workspace
    _refused(ops, "tris_layernorm_bwd_f32", *p[:5], None, None, None, 8, 8, p[8], None)      # nothing to do
    _refused(ops, "tris_layernorm_bwd_f32", *p[:5], None, None, None, 8, 8, p[8], p[9])
    # InstanceNorm forward (X, gamma, beta, Y, mean, invstd, B, P, C, eps, relu)
    for dims in ((0, 4, 4), (-1, 4, 4), (2, 0, 4), (2, -1, 4), (2, 4, 0), (2, 4, -1)):
        for relu in (0, 1):
            _refused(ops, "tris_instnorm_fwd_f32", *p[:6], *dims, eps, relu)
            _refused(ops, "tris_instnorm_bwd_f32", *p[:9], *dims, relu)
    each_null("tris_instnorm_fwd_f32", p[:6], (2, 4, 4, eps, 0))
    # InstanceNorm backward (dY, Y, X, gamma, mean, invstd, dX, dgamma_part, dbeta_part, B, P, C, relu)
    each_null("tris_instnorm_bwd_f32", p[:9], (2, 4, 4, 0), optional=(1,))
    each_null("tris_instnorm_bwd_f32", p[:9], (2, 4, 4, 1))                  # (with the ReLU, Y among them)
    # l2norm (X, Y, inv_norm, rows, C) / (dY, Y, inv_norm, dX, rows, C); softmax (X, Y, rows, n, scale) / (dY, Y, dX, rows, n, scale)
    for rows, C in ((0, 8), (-1, 8), (4, 0), (4, -1)):
        _refused(ops, "tris_l2norm_fwd_f32", *p[:3], rows, C)
        _refused(ops, "tris_l2norm_bwd_f32", *p[:4], rows, C)
        _refused(ops, "tris_softmax_fwd_f32", *p[:2], rows, C, 1.0)
        _refused(ops, "tris_softmax_bwd_f32", *p[:3], rows, C, 1.0)
    each_null("tris_l2norm_fwd_f32", p[:3], (4, 8))
    each_null("tris_l2norm_bwd_f32", p[:4], (4, 8))
    each_null("tris_softmax_fwd_f32", p[:2], (4, 8, 1.0))
    each_null("tris_softmax_bwd_f32", p[:3], (4, 8, 1.0))
    for scale in (math.inf, -math.inf, math.nan):
        _refused(ops, "tris_softmax_fwd_f32", *p[:2], 4, 8, scale)
        _refused(ops, "tris_softmax_bwd_f32", *p[:3], 4, 8, scale)
    assert A.untouched()


# ================================================================================================================ the wrappers
@pytest.fixture(params=["x3", "h2"])
def mode(request):
    ops, _ = _lib()
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(request.param)
    try:
        ops.h2_begin_step()
        ops.h2_end_step()
        yield request.param
    finally:
        ops.set_gemm_mode(prev)


def _word_of(ops, t):
    """the amax word h2_mark_next armed for `t` (None outside h2)"""
    slot = ops._h2_tag_slot(t)
    if slot is None:
        return None
    pool = ops._H2.pool
    i = (slot - pool.data_ptr()) // 4
    return pool[i:i + ops.H2_SUB]


def _tagged(ops, mode, t, what):
    w = _word_of(ops, t)
    assert (w is not None) == (mode == "h2"), f"{what}: amax word {'missing' if w is None else 'unexpected'} in {mode}"
    if w is not None:
        torch.cuda.synchronize()
        assert int(w.max()) == _bits(t), f"{what}: the word h2_mark_next armed does not hold max |out|"


@pytest.mark.parametrize("boxed", [False, True])
def test_layer_norm_wrapper_is_the_chain_of_abi_calls(mode, boxed):
    ops, query = _lib()
    shape = (37, 512)
    d = OR.inputs("ln", "randn", shape)
    x, g, b, dy, extra = _dev(d, "x", "gamma", "beta", "dy", "extra")
    y, mean, rstd = _ln_fwd(ops, x, g, b)
    dx, dg, db = _ln_bwd(ops, query, dy, x, g, mean, rstd, extra if boxed else None, None)
    xs, gs, bs = (t.clone().requires_grad_(True) for t in (x, g, b))
    box = ops.GradBox() if boxed else None
    out = ops.layer_norm(xs.view(1, *shape), gs, bs, OR.EPS, box)
    _tagged(ops, mode, out, "layer_norm")
    if boxed:
        assert box.deposit(extra.clone())      # the residual gradient a later op of the block leaves for this LayerNorm
    out.backward(dy.view(1, *shape))
    assert torch.equal(out.detach().view(shape), y), "y differs from the chain of ABI calls"
    for name, got, want in (("dx", xs.grad.view(shape), dx), ("dgamma", gs.grad, dg), ("dbeta", bs.grad, db)):
        assert torch.equal(got, want), f"{name} differs from the chain of ABI calls"
    assert not boxed or (box.consumed and box.value is None)


@pytest.mark.parametrize("relu", [False, True])
def test_instance_norm_wrapper_is_the_chain_of_abi_calls(mode, relu):
    ops, _ = _lib()
    shape = (3, 100, 128)
    d = OR.inputs("in", "randn", shape)
    x, g, b, dy = _dev(d, "x", "gamma", "beta", "dy")
    y, mean, is_ = _in_fwd(ops, x, g, b, relu)
    dx, dgp, dbp = _in_bwd(ops, dy, y if relu else None, x, g, mean, is_, relu)
    dg, db = torch.empty_like(g), torch.empty_like(b)
    ops.colsum(dgp, shape[0], shape[2], dg)
    ops.colsum(dbp, shape[0], shape[2], db)
    xs, gs, bs = (t.clone().requires_grad_(True) for t in (x, g, b))
    out = ops.instance_norm(xs, gs, bs, relu, OR.EPS)
    _tagged(ops, mode, out, "instance_norm")
    out.backward(dy)
    for name, got, want in (("y", out.detach(), y), ("dx", xs.grad, dx), ("dgamma", gs.grad, dg), ("dbeta", bs.grad, db)):
        assert torch.equal(got, want), f"{name} differs from the chain of ABI calls"


def test_l2norm_and_softmax_wrappers_are_the_chain_of_abi_calls(mode):
    ops, _ = _lib()
    st = ops._stream()
    rows, C = 50, 512
    d = OR.inputs("l2", "randn", (rows, C))
    x, dy = _dev(d, "x", "dy")
    y, inv, dx = _nan(rows, C), _nan(rows), _nan(rows, C)
    ops.call("tris_l2norm_fwd_f32", ops.P(x), ops.P(y), ops.P(inv), rows, C, st)
    ops.call("tris_l2norm_bwd_f32", ops.P(dy), ops.P(y), ops.P(inv), ops.P(dx), rows, C, st)
    xs = x.clone().requires_grad_(True)
    out = ops.l2norm(xs)
    out.backward(dy)
    assert torch.equal(out.detach(), y) and torch.equal(xs.grad, dx), "l2norm differs from the chain of ABI calls"
    rows, n = 21, 48
    for scale in OR.SM_SCALES[:2]:
        x, dy = OR.sm_x("randn", (rows, n), scale).cuda(), OR.inputs("sm", "randn", (rows, n))["dy"].cuda()
        y, dx = _nan(rows, n), _nan(rows, n)
        ops.call("tris_softmax_fwd_f32", ops.P(x), ops.P(y), rows, n, scale, st)
        ops.call("tris_softmax_bwd_f32", ops.P(dy), ops.P(y), ops.P(dx), rows, n, scale, st)
        xs = x.clone().requires_grad_(True)
        out = ops.softmax(xs, scale)
        out.backward(dy)
        assert torch.equal(out.detach(), y) and torch.equal(xs.grad, dx), "softmax differs from the chain of ABI calls"


if __name__ == "__main__":
    # `python tests/test_gpu_rownorm.py > profiles/rownorm_parity_floor.txt` on the MI355X
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ASSERT = False
    out, sys.stdout = sys.stdout, open(os.devnull, "w")
    _ops, _ = _lib()
    _set = lambda v: _ops.set_option("LN_BWD_BLOCKS", v)
    try:
        for c in LN_CASES:
            test_layernorm_forward(c)
            test_layernorm_backward(c, _set)
    finally:
        _set(None)
    for c in IN_CASES:
        for relu in (0, 1):
            test_instancenorm(c, relu)
    for c in L2_CASES:
        test_l2norm(c)
    for c in SM_CASES:
        test_softmax(c)
    sys.stdout = out
    print("# Row normalisations (csrc/norm.hip LayerNorm, InstanceNorm; csrc/heads.hip l2norm, softmax) against fp64: the largest")
    print("# err / bound per entry point, output and input kind over the shapes of tests/oracle_rownorm.py, MI355X.  The bounds are the")
    print("# element-wise ones derived there; tests/test_gpu_rownorm.py asserts ratio <= 1.")
    print("# entry point | output | kind | err / bound (largest over the shapes) | at shape")
    worst, per_kind = {}, {}
    for (entry, output, kind, shape), ratio in REC.items():
        k = (entry, output, kind)
        if k not in per_kind or ratio > per_kind[k][0]:
            per_kind[k] = (ratio, shape)
        worst[(entry, output)] = max(worst.get((entry, output), 0.0), ratio)
    for (entry, output, kind), (ratio, shape) in per_kind.items():
        print(f"{entry:14s} | {output:12s} | {kind:12s} | {ratio:.3f}{'  EXCEEDS' if ratio > 1 else ''} | {'x'.join(map(str, shape))}")
    print("# largest ratio per entry point and output:")
    for (entry, output), ratio in worst.items():
        print(f"#   {entry:14s} {output:12s} {ratio:.3f}")
