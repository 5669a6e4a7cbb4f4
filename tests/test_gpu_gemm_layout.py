"""tris_gemm_f32 and tris_colsum_f32 on NON-PACKED operands (include/tris_hip.h: lda / ldb / ldc / ldr, batch strides, misaligned
bases), through the C ABI directly -- the layouts that decide between the fast and the generic kernel, the 16-byte and the scalar
loaders and epilogues, and the three split-K reduce kernels (csrc/gemm_conv.hip vecA / vecB / fastA / fastB, csrc/gemm_core.h vecC /
vecCfin / wide).  tests/oracle_gemm_layout.py builds every operand inside a poisoned buffer (NaN around A, B, bias and resid and in
the workspace, one finite bit pattern everywhere in C) and restates the header's formula by flat indexing in fp64 and fp32; the
class each case is predicted to reach is pinned in tests/test_gemm_layout_host.py.

Ground rule (as tests/test_gpu_irn_train.py::_within, here in max-abs): the distance of the GPU result to fp64 is at most 8 x the
distance of the fp32 CPU evaluation to fp64, floored at one fp32 ulp of the largest reference magnitude.  Every call also has to
return 0, leave a finite window, leave everything outside the window bitwise the sentinel and leave its inputs bitwise unchanged.

The three arithmetics are selected process-wide (tris_set_gemm_mode 0 / 1 / 3); h2 then runs with unit operand scales, which is
why the operands are N(0, 1) against N(0, 0.1).  ops.gemm is NOT used: its h2 pre-pass takes the amax of whole tensors and would
read the NaN padding."""
import functools

import numpy as np
import pytest
import torch

import oracle_gemm_layout as G

pytestmark = pytest.mark.gpu

MODES = {"f32": 0, "x3": 1, "h2": 3}
CASES = G.cases()
BY_NAME = {c.name: c for c in CASES}
SPLIT = [c for c in CASES if c.slabs]


@pytest.fixture(scope="module")
def ops():
    from tris_amd import ops as o
    return o


def _set_mode(o, m):
    prev = o.query("tris_get_gemm_mode")
    o.call("tris_set_gemm_mode", m)
    return prev


@pytest.fixture(scope="module", params=list(MODES))
def mode(request, ops):
    """the arithmetic of the dense products, process-wide; the previous one is put back (as tests/test_gpu_ops.py does)"""
    prev = _set_mode(ops, MODES[request.param])
    yield request.param
    ops.call("tris_set_gemm_mode", prev)


@pytest.fixture()
def x3(ops):
    prev = _set_mode(ops, MODES["x3"])
    yield "x3"
    ops.call("tris_set_gemm_mode", prev)


@functools.lru_cache(maxsize=None)
def _problem(name, pre=False):
    """buffers and references of a case: computed once, shared by the three arithmetics, never written to"""
    case = BY_NAME[name] if name in BY_NAME else EXTRA[name]
    bufs = G.lay_out(case, seed=sum(map(ord, name)))
    ref64 = G.reference(case, bufs, torch.float64, pre_activation=pre).numpy()
    ref32 = G.reference(case, bufs, torch.float32, pre_activation=pre).numpy()
    for v in bufs.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case, bufs, ref64, ref32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _within(what, got, ref32, ref64):
    """the ground rule; prints the figures before it asserts; returns the ratio"""
    e_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
    e_gpu = float(np.abs(got.astype(np.float64) - ref64).max())
    floor = float(np.spacing(np.float32(np.abs(ref64).max())))
    ratio = e_gpu / max(e_ref, floor / 8)
    print(f"RATIO {what}: e_ref {e_ref:.3e} gpu {e_gpu:.3e} floor {floor:.3e} ratio {ratio:.2f}")
    assert e_gpu <= max(8 * e_ref, floor), (what, e_gpu, e_ref, floor)
    return ratio


def _launch(ops, case, bufs, pre_buf=None, tickets=None, declinable=False):
    """one tris_gemm_f32 call on device copies of the buffers -> (ran, C buffer, pre_out buffer) as numpy; checks what every call
    has to leave alone: the inputs and the guard behind the workspace, bit for bit"""
    dev = {k: torch.from_numpy(np.array(v)).cuda() for k, v in bufs.items() if isinstance(v, np.ndarray)}
    off = bufs["off"]
    ptr = lambda k: ops.P(dev[k], off.get(k, 0)) if k in dev else None
    pre = None
    if pre_buf is not None:
        pre = torch.from_numpy(np.array(pre_buf)).cuda()
        ops.call("tris_gemm_epilogue_next", ops.P(pre, off["C"]), None)
    if tickets is not None:
        ops.call("tris_splitk_tickets_next", tickets.data_ptr(), tickets.numel())
    args = ("tris_gemm_f32", ptr("A"), ptr("B"), ptr("C"), case.M, case.N, case.K, case.lda, case.ldb, case.ldc, case.tA, case.tB,
            case.batch, case.sA, case.sB, case.sC, ptr("bias"), case.bias_mode, ptr("resid"), case.ldr, case.sR, case.act,
            float(case.alpha), ptr("ws"), case.ws_bytes(), ops._stream())
    if declinable:
        ran = ops._declinable(*args)
    else:
        ops.call(*args)          # (raises on a non-zero return code)
        ran = True
    torch.cuda.synchronize()
    for k in ("A", "B", "bias", "resid"):
        if k in dev:
            assert np.array_equal(_bits(dev[k].cpu().numpy()), _bits(bufs[k])), f"{case.name}: input {k} was written to"
    if "ws" in dev:
        assert (_bits(dev["ws"].cpu().numpy())[-G.GUARD:] == G.NAN_BITS).all(), f"{case.name}: wrote behind the workspace"
    return ran, dev["C"].cpu().numpy(), None if pre is None else pre.cpu().numpy()


def _check_output(what, case, cbuf, ref32, ref64):
    assert (_bits(G.outside(case, cbuf)) == G.SENTINEL_BITS).all(), f"{what}: wrote outside the M x N x batch window"
    win = G.window(case, cbuf)
    assert np.isfinite(win).all(), f"{what}: {np.count_nonzero(~np.isfinite(win))} non-finite values in the window"
    return _within(what, win, ref32, ref64)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_gemm_on_layout(ops, mode, name):
    case, bufs, ref64, ref32 = _problem(name)
    _, cbuf, _ = _launch(ops, case, bufs)
    _check_output(f"{mode} {G.predict(case)} {name}", case, cbuf, ref32, ref64)


def test_fast_kernel_prediction_is_what_the_library_decides(ops, x3):
    """The armed epilogue exists in the fast kernel only: an armed call is declined exactly where the header-level predicates of
    oracle_gemm_layout.predict say 'generic' -- the observable that ties the pinned classes to the library's own dispatch
    (row-major A, one batch: what the arming is defined for).  A case that cannot reach its class fails here; nothing skips."""
    seen = set()
    for case in CASES:
        if case.tA or case.batch != 1:
            continue
        _, bufs, _, _ = _problem(case.name)
        ran, cbuf, pre = _launch(ops, case, bufs, pre_buf=bufs["C"], declinable=True)
        want = G.predict(case, armed=True).startswith("fast")
        assert ran == want, (case.name, ran, G.predict(case, armed=True))
        seen.add(want)
        if not ran:
            assert (_bits(cbuf) == G.SENTINEL_BITS).all() and (_bits(pre) == G.SENTINEL_BITS).all(), case.name
    assert seen == {True, False}


# ---- the armed epilogue (tris_gemm_epilogue_next): pre_out carries C's layout ------------------------------------------------------
EXTRA = {}
for _l in ("L1", "L2", "L4"):
    for _M, _N, _K, _tB in ((130, 68, 96, 1), (200, 136, 64, 0)):
        _c = G.Case(f"armed-{_l}-{_M}x{_N}x{_K}-N{'T' if _tB else 'N'}", _M, _N, _K, 0, _tB, _l, bias_mode=1, act=2, resid=True, alpha=0.5)
        EXTRA[_c.name] = _c


@pytest.mark.parametrize("name", [n for n in EXTRA if "-L2-" not in n])
def test_armed_epilogue_on_layout(ops, mode, name):
    case, bufs, ref64, ref32 = _problem(name)
    _, _, pre64, pre32 = _problem(name, True)
    ran, cbuf, pre = _launch(ops, case, bufs, pre_buf=bufs["C"], declinable=True)
    assert ran, "the fast kernel serves this layout: the armed product must not be declined"
    _check_output(f"{mode} armed-C {name}", case, cbuf, ref32, ref64)
    _check_output(f"{mode} armed-pre {name}", case, pre, pre32, pre64)


@pytest.mark.parametrize("name", [n for n in EXTRA if "-L2-" in n])
def test_armed_epilogue_declines_odd_leading_dimensions(ops, mode, name):
    case, bufs, _, _ = _problem(name)
    ran, cbuf, pre = _launch(ops, case, bufs, pre_buf=bufs["C"], declinable=True)
    assert not ran                                                   # TRIS_DECLINED
    assert (_bits(cbuf) == G.SENTINEL_BITS).all() and (_bits(pre) == G.SENTINEL_BITS).all()    # nothing launched


# ---- the fused split-K finish (tris_splitk_tickets_next) ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in SPLIT])
def test_fused_finish_is_the_reduce_launch_bit_for_bit(ops, mode, name):
    """With zeroed tickets the last block of every tile sums the slabs inside the product's launch; the header promises the separate
    reduce launch's result bit for bit.  Where the fused form does not apply (generic kernel; the wide reduce's order without the
    vector finish) the armed call runs the two launches -- the counter tells which happened."""
    case, bufs, ref64, ref32 = _problem(name)
    _, separate, _ = _launch(ops, case, bufs)
    tickets = torch.zeros(64, dtype=torch.int32, device="cuda")
    before = ops.query("tris_splitk_fused_launches")
    _, fused, _ = _launch(ops, case, bufs, tickets=tickets)
    took = ops.query("tris_splitk_fused_launches") - before
    assert took == (1 if G.fused_finish_applies(case) else 0), (name, took, G.predict(case))
    assert int(tickets.abs().max()) == 0                             # every launch leaves the tickets zero
    _check_output(f"{mode} fused {G.predict(case)} {name}", case, fused, ref32, ref64)
    assert np.array_equal(_bits(fused), _bits(separate))


def test_fused_finish_reaches_both_forms():
    """(table check: the 4-slab product takes the fused finish under the padded and under the odd-output layout)"""
    assert G.fused_finish_applies(BY_NAME["L1-200x136x4096-NT-ws4"]) and G.fused_finish_applies(BY_NAME["L4-200x136x4096-NT-ws4"])
    assert not G.fused_finish_applies(BY_NAME["L2-200x136x4096-NT-ws4"])


# ---- tiles and loop forms under x3 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", [0, 1])
@pytest.mark.parametrize("tile", ["128x128", "128x64", "64x64"])      # (128x32 needs N <= 32, 256x128 needs M >= 256: neither product)
@pytest.mark.parametrize("name", ["L1-200x136x64-NN", "L4-130x68x96-NT"])
def test_forced_tiles_on_layout(ops, x3, name, tile, pipe):
    case, bufs, ref64, ref32 = _problem(name)
    ops.set_option("FORCE_TILE", tile)
    ops.set_option("FORCE_PIPE", pipe)         # (both are reset after every GPU test by conftest.py)
    _, cbuf, _ = _launch(ops, case, bufs)
    _check_output(f"x3 {G.predict(case)} tile {tile} pipe {pipe} {name}", case, cbuf, ref32, ref64)


# ---- column sums (bias gradients) ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _colsum_problem(M, N, form):
    buf, off, ld = G.colsum_lay_out(M, N, form, seed=1000 * N + M)
    r64 = G.colsum_reference(buf, off, M, N, ld, torch.float64).numpy()
    r32 = G.colsum_reference(buf, off, M, N, ld, torch.float32).numpy()
    buf.setflags(write=False)
    return buf, off, ld, r64, r32


@pytest.mark.parametrize("form", G.COLSUM_FORMS)
@pytest.mark.parametrize("N", G.COLSUM_N_VEC + G.COLSUM_N_SCALAR)
@pytest.mark.parametrize("M", G.COLSUM_M)
def test_colsum_on_layout(ops, M, N, form):
    """out[n] = sum_m X[m*ld+n]: the vector kernel (fp64 partials) and the one-thread-per-column kernel (N % 4, ld % 4 or a
    misaligned X), NaN between the rows and around X, a sentinel around out, against the fp64 column sum"""
    buf, off, ld, r64, r32 = _colsum_problem(M, N, form)
    kind = G.colsum_predict(N, form)
    ws_bytes = ops.query("tris_col_workspace_bytes", M, N)
    assert ws_bytes > 0
    if kind == "vector" and M >= 2500:
        assert ws_bytes // (16 * N) > 1                               # more than one partial row
    X = torch.from_numpy(np.array(buf)).cuda()
    out = torch.from_numpy(np.full(N + 2 * G.GUARD, G.SENTINEL_BITS, np.uint32).view(np.float32)).cuda()
    ws = torch.from_numpy(np.full(ws_bytes // 4 + G.GUARD, G.NAN_BITS, np.uint32).view(np.float32)).cuda()
    ops.call("tris_colsum_f32", ops.P(X, off), M, N, ld, ops.P(out, G.GUARD), ops.P(ws), ops._stream())
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.array_equal(_bits(X.cpu().numpy()), _bits(buf))
    assert (_bits(ws.cpu().numpy())[-G.GUARD:] == G.NAN_BITS).all()
    assert (_bits(o[:G.GUARD]) == G.SENTINEL_BITS).all() and (_bits(o[G.GUARD + N:]) == G.SENTINEL_BITS).all()
    got = o[G.GUARD:G.GUARD + N]
    assert np.isfinite(got).all()
    _within(f"colsum {kind} M{M} N{N} {form}", got, r32, r64)
