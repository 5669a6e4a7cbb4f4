"""The 3x3 convolution family against fp64 at ADVERSARIAL operand statistics (tests/oracle_conv_stats.py): dark images next to bright
ones, filters and channels 2^-20 below their tensor's maximum, outliers, anti-correlated per-channel gains, heavy tails,
gradient-like tensors -- what tests/test_gpu_h2.py asks of ops.gemm, asked of every convolution entry point with staging and
splitting code of its own: the implicit GEMM's gathers, the direct forward / data-gradient kernels (configurations 1-6), the direct
weight-gradient kernel (1-5, nine tap accumulators and a transient cross-product set), the stem's first convolution, the forms that
fold relu(bn(x)) into their staging under a BOUND word, and every one of them on operand planes.

Through the C ABI.  Per form x kind x arithmetic (x3, h2):
  * everything is finite;
  * the YARDSTICK -- mode f32, implicit GEMM, same operands -- satisfies the a-priori elementwise bound gamma_n (|a| (*) |b|): a
    gather or indexing fault shared by all arithmetics cannot hide behind a ratio;
  * the arithmetic's group errors (per image / channel; maximum and median; small groups and the rest apart) are <= 2.0 x the
    yardstick's on the same groups -- the criterion of the dense products (tests/test_gpu_h2.py), taken over as it is;
  * h2 on operand planes is bit-identical to h2 splitting the same fp32 operands in the kernel;
  * the launch counters say the form under test ran, and a result counts as h2 only where the fast kernels serve the product: there
    the armed run must differ from the x3 run in its bits; anywhere else the library drops the arming and the run must BE the x3 run.
tests/test_conv_stats_host.py shows on the CPU that the h2 operand rounding meets this criterion on every input here (<= 0.8x an fp32
convolution) and that a residual piece stored without its 2^11 pre-scale does not.  Every case prints its worst ratios
(pytest -s): DESIGN.md "Accuracy evidence (1b)" records them."""
import math

import pytest
import torch

import oracle_conv_stats as O

pytestmark = pytest.mark.gpu

WORD = 2048
FACTOR = 2.0


@pytest.fixture()
def ops():
    from tris_amd import ops as o
    prev = o.get_gemm_mode()
    with o.autotune_off():     # (the launch counts below are those of the static choice: a tuner would time every candidate on first sight)
        yield o
    o.set_gemm_mode(prev)
    for name in ("CONV_DIRECT", "WGRAD_DIRECT", "STEM_CONV1"):
        o.set_option(name, None)


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _word(ops, t):
    w = torch.zeros(WORD, device="cuda", dtype=torch.int32)
    ops.call("tris_amax_bits_f32", ops.P(t), t.numel(), w.data_ptr(), ops._stream())
    return w


def _planes(ops, t, w):
    o = torch.empty_like(t)
    ops.call("tris_h2_planes_f32", ops.P(t), ops.P(o), t.numel(), w.data_ptr(), ops._stream())
    return o


def _launches():
    from tris_amd import _lib
    return _lib.query("tris_direct_launches", 0), _lib.query("tris_direct_launches", 1)


# which products the fast kernels serve (gemm_params.h gemm_fast_ok): only those run in h2 when armed -- for any other the library drops
# the arming and runs its default arithmetic, x3 -- and only those take planes
def _fast(prod, shape, stride=1):
    B, H, W, Cin, Cout = shape
    Ho, Wo = O.out_hw(H, W, stride)
    if prod == "y":
        return Cin % 32 == 0 and B * Ho * Wo >= 4 and Cout >= 4
    if prod == "dx":
        return Cout % 32 == 0 and Cin % 4 == 0
    return Cout % 4 == 0 and Cin % 4 == 0 and (B * Ho * Wo) % 32 == 0


def _planes_ok(prod, shape, stride=1):
    return stride == 1 and _fast(prod, shape) and shape[3] % 8 == 0 and shape[4] % 8 == 0


# the direct configuration that takes the DATA GRADIENT of each forward shape (0: none, the implicit GEMM).  A data gradient has Cin
# output columns: configurations 1, 4, 5, 6 want more than 64 (conv_direct_cfg.h halo_ok), 3 at most 32 on a map of 16-row patches,
# 2 takes 33 .. 64.  The launch counter holds the table to the library.
DGRAD_CFG = {1: 3, 2: 2, 3: 3, 4: 0, 5: 0, 6: 0}


class _Run:
    """the three products of one case through the C ABI in one arithmetic: 'f32' | 'x3' | 'h2' | 'h2pl' (h2 on operand planes)"""

    def __init__(self, ops, c):
        self.ops, self.c = ops, c
        self.x, self.w = c.x.cuda(), c.w.cuda()
        self.dy = None if c.dy is None else c.dy.cuda()
        self.words = {k: _word(ops, t) for k, t in (("x", self.x), ("w", self.w), ("dy", self.dy)) if t is not None}
        self.pl = {}
        self.ws = ops.workspace(0)

    def _operands(self, arith, a, b):
        """arm the next product for operands named a, b (h2) and return the pointers to hand over"""
        ops = self.ops
        if arith == "h2":
            ops.call("tris_h2_next", self.words[a].data_ptr(), self.words[b].data_ptr(), 0.0, 0.0)
        elif arith == "h2pl":
            for k in (a, b):
                if k not in self.pl:
                    self.pl[k] = _planes(ops, getattr(self, k), self.words[k])
            ops.call("tris_h2_next_planes", self.words[a].data_ptr(), self.words[b].data_ptr(), 0)
            return ops.P(self.pl[a]), ops.P(self.pl[b])
        return ops.P(getattr(self, a)), ops.P(getattr(self, b))

    def product(self, prod, arith):
        ops, (B, H, W, Cin, Cout), stride = self.ops, self.c.shape, self.c.stride
        ops.set_gemm_mode("f32" if arith == "f32" else "x3")
        Ho, Wo = O.out_hw(H, W, stride)
        if prod == "y":
            out = torch.full((B, Ho, Wo, Cout), float("nan"), device="cuda")
            pa, pb = self._operands(arith, "x", "w")
            ops.call("tris_conv3x3_fwd_f32", pa, pb, ops.P(out), B, H, W, Cin, Cout, stride, ops._stream())
        elif prod == "dx":
            out = torch.full((B, H, W, Cin), float("nan"), device="cuda")
            pa, pb = self._operands(arith, "dy", "w")
            ops.call("tris_conv3x3_dgrad_f32", pa, pb, ops.P(out), B, H, W, Cin, Cout, ops._stream())
        else:
            out = torch.full((Cout, 3, 3, Cin), float("nan"), device="cuda")
            pa, pb = self._operands(arith, "dy", "x")          # (weight gradients: A = dY, B = the convolution's input)
            ops.call("tris_conv3x3_wgrad_f32", pb, pa, ops.P(out), B, H, W, Cin, Cout, stride, ops.P(self.ws), self.ws.numel() * 4,
                     ops._stream())
        torch.cuda.synchronize()
        return out.cpu()


def _implicit(ops):
    ops.set_option("CONV_DIRECT", "0")
    ops.set_option("WGRAD_DIRECT", "0")
    ops.set_option("STEM_CONV1", "0")


def _judge(tag, got, yard, ref, small, report):
    assert torch.isfinite(got).all(), tag
    bad, worst = O.criterion(got, yard, ref, small, FACTOR)
    report.append(f"{tag} {worst:.2f}")
    assert not bad, (tag, worst, bad)


def _judge_x3_h2(tag, k, run, x3, armed, yard, r, report):
    """x3 and the ARMED run of product k.  Only a product the fast kernels serve runs in h2: it is judged as h2 and must differ from x3
    in its bits; for any other the library drops the arming, the run must BE the x3 run bit for bit and is not reported as h2."""
    c = run.c
    _judge(f"{tag}/x3", x3, yard[k], r.ref[k], c.small[k], report)
    if _fast(k, c.shape, c.stride):
        assert not torch.equal(armed, x3), (tag, "armed for h2, yet the x3 result bit for bit")
        _judge(f"{tag}/h2", armed, yard[k], r.ref[k], c.small[k], report)
    else:
        assert torch.equal(armed, x3), (tag, "not served by the fast kernels, yet the arming changed the result")
        report.append(f"{tag}/armed =x3")


def _yardstick(ops, run, r, prods):
    """mode f32, implicit GEMM: inside the a-priori bound element by element"""
    _implicit(ops)
    n0 = _launches()
    yard = {k: run.product(k, "f32") for k in prods}
    assert _launches() == n0
    for k in prods:
        assert torch.isfinite(yard[k]).all(), k
        ratio = O.bound_ratio(yard[k], r.ref[k], r.bound[k])
        assert ratio <= 1.0, ("yardstick outside the a-priori bound", k, ratio)
    return yard


@pytest.mark.parametrize("kind", O.KINDS)
@pytest.mark.parametrize("shape,stride", [(s, 1) for s in O.IMPLICIT] + [(s, 2) for s in O.IMPLICIT_S2], ids=_id)
def test_implicit_gemm_convolutions(ops, shape, stride, kind):
    """A_IM2COL / B_KN_DGRAD / B_KN_IM2COL gathers: forward (stride 1 and 2), data gradient, weight gradient"""
    c, r = O.operands(kind, shape, stride), O.reference(kind, shape, stride)
    run = _Run(ops, c)
    prods = tuple(r.ref)
    yard = _yardstick(ops, run, r, prods)
    report = []
    n0 = _launches()
    for k in prods:
        got = {a: run.product(k, a) for a in ("x3", "h2")}
        _judge_x3_h2(k, k, run, got["x3"], got["h2"], yard, r, report)
        if _planes_ok(k, shape, stride):
            assert torch.equal(run.product(k, "h2pl"), got["h2"]), (k, "planes")
            report.append(f"{k}/planes =")
    assert _launches() == n0                    # no direct kernel: CONV_DIRECT = WGRAD_DIRECT = 0
    print(f"\nimplicit {_id(shape)} s{stride} {kind}: " + ", ".join(report))


@pytest.mark.parametrize("kind", O.STEM_KINDS)
@pytest.mark.parametrize("shape", O.STEM, ids=_id)
def test_stem_first_convolution(ops, shape, kind):
    """Cin = 3, stride 2, forward only: the dedicated kernel (exact fp32 products whatever the mode) and, STEM_CONV1=0, the generic one.
    No launch counter covers the dedicated kernel; the statistics entry point tells: it hands back one partial row per BLOCK of the
    dedicated kernel and none from the generic kernel, which does not fuse statistics for a product the fast kernels do not serve."""
    import ctypes
    B, H, W, Cin, Cout = shape
    c, r = O.operands(kind, shape, 2), O.reference(kind, shape, 2)
    assert not _fast("y", shape, 2)
    run = _Run(ops, c)
    yard = _yardstick(ops, run, r, ("y",))
    Ho, Wo = O.out_hw(H, W, 2)
    blocks = -(-(-(-B * Ho * Wo // 32)) // 4)          # run_stem_conv1: a wave per 32 pixels, four waves per block
    report = []
    for stem, rows_want in ((None, blocks), ("0", 0)):
        ops.set_option("STEM_CONV1", stem)
        got = {a: run.product("y", a) for a in ("x3", "h2")}
        assert torch.equal(got["h2"], got["x3"])       # exact fp32 products whatever the mode, armed or not
        _judge(f"y[{'stem' if stem is None else 'generic'}]/x3=h2", got["x3"], yard["y"], r.ref["y"], c.small["y"], report)
        ops.set_gemm_mode("x3")
        y = torch.full((B, Ho, Wo, Cout), float("nan"), device="cuda")
        part = torch.zeros((-(-B * Ho * Wo // 128) + 8) * 2 * Cout, device="cuda", dtype=torch.float64)
        rows = ctypes.c_int(-1)
        ops.call("tris_conv3x3_fwd_bnstat_f32", ops.P(run.x), ops.P(run.w), ops.P(y), B, H, W, Cin, Cout, 2, part.data_ptr(), ctypes.byref(rows),
                 ops._stream())
        torch.cuda.synchronize()
        assert rows.value == rows_want, (stem, rows.value)           # which kernel this option state sends the shape to
        assert torch.equal(y.cpu(), got["x3"])                       # ... and it is the one that produced the judged result
        if rows_want:
            s1 = part[:rows_want * 2 * Cout].view(rows_want, 2, Cout)[:, 0].sum(0).cpu()
            assert torch.allclose(s1, got["x3"].double().sum((0, 1, 2)), rtol=1e-9, atol=1e-12)
    print(f"\nstem {_id(shape)} {kind}: " + ", ".join(report))


@pytest.mark.parametrize("kind", O.KINDS)
@pytest.mark.parametrize("cfg,shape", sorted(O.DIRECT_FWD.items()) + sorted(O.DIRECT_FWD_H2.items()), ids=_id)
def test_direct_forward_and_data_gradient(ops, cfg, shape, kind):
    """A_HALO: one split of the input window per 16-channel chunk, 2-D patches (1-3, 6) and flattened pixel runs (4, 5).  The forward of
    configuration 2 at 48 input channels is no h2 product (x3 whatever the arming, asserted): its h2 form runs at 64 input channels."""
    c, r = O.operands(kind, shape), O.reference(kind, shape)
    run = _Run(ops, c)
    yard = _yardstick(ops, run, r, ("y", "dx"))
    assert _fast("y", shape) or shape == O.DIRECT_FWD[2]
    report = []
    for k, forced in (("y", cfg), ("dx", DGRAD_CFG[cfg])):
        _direct(ops, run, k, forced, yard, r, report)
    print(f"\ndirect {cfg} {_id(shape)} {kind}: " + ", ".join(report))


def _direct(ops, run, k, forced, yard, r, report):
    c = run.c
    ops.set_option("CONV_DIRECT", str(forced))
    got = {}
    for a in ("x3", "h2") + (("h2pl",) if _planes_ok(k, c.shape) else ()):
        n0 = _launches()[0]
        got[a] = run.product(k, a)
        assert _launches()[0] - n0 == (1 if forced else 0), (k, a, forced)     # the direct kernel ran
    _judge_x3_h2(f"{k}[{forced}]", k, run, got["x3"], got["h2"], yard, r, report)
    if "h2pl" in got:
        assert torch.equal(got["h2pl"], got["h2"]), (k, "planes")
        report.append(f"{k}/planes =")


@pytest.mark.parametrize("kind", O.KINDS)
@pytest.mark.parametrize("cfg", sorted(O.DIRECT_DGRAD))
def test_direct_data_gradient_of_the_wide_configurations(ops, cfg, kind):
    """configurations 1, 4, 5, 6 take a data gradient only with more than 64 input channels: the forward's shapes with Cin and Cout
    exchanged (B_KN_DGRAD: the mirrored-tap weight loader next to the A_HALO window)"""
    shape = O.DIRECT_DGRAD[cfg]
    B, H, W, Cin, Cout = shape
    c, r = O.operands(kind, shape), O.reference(kind, shape)
    run = _Run(ops, c)
    yard = _yardstick(ops, run, r, ("dx",))
    assert _fast("dx", shape) and _planes_ok("dx", shape)
    report = []
    _direct(ops, run, "dx", cfg, yard, r, report)
    print(f"\ndirect-dgrad {cfg} {_id(shape)} {kind}: " + ", ".join(report))


@pytest.mark.parametrize("kind", O.KINDS)
@pytest.mark.parametrize("cfg", sorted(O.DIRECT_WGRAD))
def test_direct_weight_gradient(ops, cfg, kind):
    """wgrad3x3_direct_kernel: nine tap accumulators, in h2 one transient cross-product set per tap and window folded in with 2^-11"""
    shape = O.DIRECT_WGRAD[cfg]
    c, r = O.operands(kind, shape), O.reference(kind, shape)
    run = _Run(ops, c)
    yard = _yardstick(ops, run, r, ("dw",))
    ops.set_option("WGRAD_DIRECT", str(cfg))
    got, report = {}, []
    assert _fast("dw", shape) and _planes_ok("dw", shape)       # every shape here is an h2 product, also on planes
    for a in ("x3", "h2", "h2pl"):
        n0 = _launches()[1]
        got[a] = run.product("dw", a)
        assert _launches()[1] - n0 == 1, a
    _judge_x3_h2("dw", "dw", run, got["x3"], got["h2"], yard, r, report)
    assert torch.equal(got["h2pl"], got["h2"])
    print(f"\nwgrad {cfg} {_id(shape)} {kind}: " + ", ".join(report))


@pytest.mark.parametrize("kind", O.BNIN_KINDS)
@pytest.mark.parametrize("loose", [False, True], ids=["own-rows", "workload-rows"])
@pytest.mark.parametrize("shape", O.BNIN, ids=_id)
def test_batchnorm_folded_forward_and_weight_gradient(ops, shape, loose, kind):
    """conv3x3(relu(bn(x))) formed while staging, split under the scale of tris_bn_out_bound_f32's word -- xhat_max = sqrt(rows - 1) of
    the shape itself, and of the training workload's widest BatchNorm (a word 2^7 .. 2^8 above the true maximum)"""
    B, H, W, Cin, Cout = shape
    M = B * H * W
    c, r = O.bnin_operands(kind, shape), O.bnin_reference(kind, shape)
    x, w, dy = c.x.cuda(), c.w.cuda(), c.dy.cuda()
    mean, invstd, gamma, beta = c.mean.cuda(), c.invstd.cuda(), c.gamma.cuda(), c.beta.cuda()
    ws = ops.workspace(0)
    # yardstick: the materialised BatchNorm output through the implicit GEMM in f32
    act = torch.empty_like(x)
    ops.call("tris_bn_apply_f32", ops.P(x), ops.P(mean), ops.P(invstd), ops.P(gamma), ops.P(beta), None, ops.P(act), M, Cin, 1, ops._stream())
    _implicit(ops)
    ops.set_gemm_mode("f32")
    yard = {"y": torch.full((B, H, W, Cout), float("nan"), device="cuda"), "dw": torch.full((Cout, 3, 3, Cin), float("nan"), device="cuda")}
    n0 = _launches()
    ops.call("tris_conv3x3_fwd_f32", ops.P(act), ops.P(w), ops.P(yard["y"]), B, H, W, Cin, Cout, 1, ops._stream())
    ops.call("tris_conv3x3_wgrad_f32", ops.P(act), ops.P(dy), ops.P(yard["dw"]), B, H, W, Cin, Cout, 1, ops.P(ws), ws.numel() * 4, ops._stream())
    torch.cuda.synchronize()
    assert _launches() == n0
    yard = {k: v.cpu() for k, v in yard.items()}
    for k in yard:
        assert torch.isfinite(yard[k]).all(), k
        ratio = O.bound_ratio(yard[k], r.ref[k], r.bound[k])
        assert ratio <= 1.0, ("yardstick outside the a-priori bound", k, ratio)
    for name in ("CONV_DIRECT", "WGRAD_DIRECT"):
        ops.set_option(name, None)
    ops.set_gemm_mode("x3")
    assert ops.conv3x3_bnin_ok(shape[:4], Cout)
    rows = O.WORKLOAD_ROWS if loose else M
    bound = torch.zeros(WORD, device="cuda", dtype=torch.int32)
    ops.call("tris_bn_out_bound_f32", ops.P(gamma), ops.P(beta), Cin, math.sqrt(rows - 1), bound.data_ptr(), ops._stream())
    ww, wd = _word(ops, w), _word(ops, dy)
    torch.cuda.synchronize()
    got_bound = float(bound.max().view(torch.float32))
    assert abs(got_bound - O.bn_bound(c, rows)) <= 1e-6 * got_bound and float(act.max()) <= got_bound
    assert _fast("y", shape) and _fast("dw", shape)            # both are h2 products: the armings below are honoured
    report, seen = [], {}
    for a in ("x3", "h2"):
        y, dw = torch.full((B, H, W, Cout), float("nan"), device="cuda"), torch.full((Cout, 3, 3, Cin), float("nan"), device="cuda")
        n0 = _launches()
        if a == "h2":
            ops.call("tris_h2_next", bound.data_ptr(), ww.data_ptr(), 0.0, 0.0)
        ops.call("tris_conv3x3_fwd_bnin_f32", ops.P(x), ops.P(mean), ops.P(invstd), ops.P(gamma), ops.P(beta), ops.P(w), ops.P(y), B, H, W, Cin,
                 Cout, None, None, ops._stream())
        if a == "h2":
            ops.call("tris_h2_next", wd.data_ptr(), bound.data_ptr(), 0.0, 0.0)
        ops.call("tris_conv3x3_wgrad_bnin_f32", ops.P(x), ops.P(mean), ops.P(invstd), ops.P(gamma), ops.P(beta), ops.P(dy), ops.P(dw), B, H, W,
                 Cin, Cout, ops.P(ws), ws.numel() * 4, ops._stream())
        torch.cuda.synchronize()
        n1 = _launches()
        assert (n1[0] - n0[0], n1[1] - n0[1]) == (1, 1), a      # both folded forms are direct kernels (static choice: the fixture)
        seen[a] = (y.cpu(), dw.cpu())
        _judge(f"y/{a}", y.cpu(), yard["y"], r.ref["y"], c.small["y"], report)
        _judge(f"dw/{a}", dw.cpu(), yard["dw"], r.ref["dw"], c.small["dw"], report)
    assert not torch.equal(seen["h2"][0], seen["x3"][0]) and not torch.equal(seen["h2"][1], seen["x3"][1])   # h2 really ran
    print(f"\nbnin {_id(shape)} {kind} rows {rows} (word / max {got_bound / float(act.max()):.0f}): " + ", ".join(report))
