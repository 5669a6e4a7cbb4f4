"""Down-sampling Bottlenecks with bn3 and the shortcut BatchNorm paired (cfg.bn_pair): the forward pair pass
(tris_bn_apply_pair_pl_f32), the stride-2 shortcut's pooled gradient read in place by conv1's data gradient
(tris_gemm_resid_pool_next) and the backward pair (tris_gemm_bnbwd_x2_next, tris_part_finalize_pair_f32,
tris_bn_bwd_apply_pair_pl_f32).  Every new launch against the chain of launches it replaces, on the same inputs, BIT for bit; the
values against the fp64 restatement of tests/oracle_bn.py inside the bounds tests/test_gpu_bn.py uses; the blocks with the switch on
and off; the argument contracts; the old chain of calls with a SyncBatchNorm group, with the switch off and in x3.

Inputs: every kind of oracle_bn.inputs (the shortcut takes another kind's tensors at the same shape), and inputs within 8 float32
steps of the kink of the SUM bn3(x3) + bn_s(xs).  Shapes [B, H, W, C]: a tail of one 512-element unit, several units with a ragged
end, several blocks -- and the streaming form.  planes.hip pl_big switches to it when the streams of a launch exceed the 256 MB
memory-side cache, so the smallest shapes that reach it are 89 MB (three streams, the forward pair: [349526, 64]) and 54 MB (five
streams, the backward pair: [209716, 64]) per tensor, not a few MB; one row more leaves the last unit ragged.  Those two cases compare
bit for bit on the device and judge a slice of rows against the oracle.

Bounds.  Forward: C_Y U (|p3| + |beta3| + |ps| + |beta_s|) -- the shortcut's value carries four fp32 roundings and the closing add a
fifth, bn3's value four and the add, and the 22-bit + sign plane representation is within U of the value (|lo' error| <= 2^-12
|residual| <= 2^-24 |y|): six = C_Y.  Backward: C_DX likewise (nine roundings + the representation), judged where the plane format is
relative.  Third sum: C_S U sum |dz xhat_s| over the masked gradient the launch itself stored (test_backward's bound).

Where the cases differ from the ones the change was specified with, and why: (1) Bottleneck(16, 8) on [2, 8, 8, 16] has no backward on
this stack with the switch on or off -- tris_conv3x3_dgrad_bnbwd_f32 refuses a 3x3 data gradient over 8 channels -- so it runs forward
only, and Bottleneck(64, 32) on [2, 16, 16, 64], the smallest block whose products all take the fused epilogues, runs forward and
backward; (2) a [120, 64] product is below the 128 rows the fused backward reduction needs: it declines armed or not, which is what
that case checks; (3) a lone block has no consumer that links bn3's backward, so the backward pair is exercised by two linked blocks."""
import math

import pytest
import torch

import oracle_bn as OB

pytestmark = pytest.mark.gpu

WORD = 2048
SENTINEL = 12345.0
GUARD = 1024
BIG_M = 349527
SHAPES = [(1, 4, 4, 8), (2, 6, 10, 64), (2, 6, 10, 256)]
# the shortcut's inputs are those of another kind at the same shape (its own x, gamma, beta and statistics)
SHORTCUT_KIND = {"randn": "offset", "offset": "relu", "relu": "gamma", "const": "randn", "gamma": "dyoff", "dyoff": "const"}
CASES = [(k, s) for k in OB.KINDS for s in SHAPES]
_id = lambda c: f"{c[0]}-" + "x".join(map(str, c[1]))


@pytest.fixture()
def ops():
    from tris_amd import ops as o
    from tris_amd.config import cfg
    prev, prev_pl, prev_pair, prev_parts = o.get_gemm_mode(), cfg.h2_planes, cfg.bn_pair, cfg.bn_pair_parts
    o.set_gemm_mode("h2")
    cfg.h2_planes = True
    cfg.bn_pair_parts = "fwd,pool,bwd"        # (every part on, whatever the default is: each test switches cfg.bn_pair)
    yield o
    cfg.h2_planes, cfg.bn_pair, cfg.bn_pair_parts = prev_pl, prev_pair, prev_parts
    o.set_gemm_mode(prev)


def _inside(got, ref, bound, key):
    e = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    over = e > bound
    ratio = float(torch.nan_to_num(e / bound, nan=0.0, posinf=float("inf")).max())
    print(f"{key}: err / bound up to {ratio:.3f}")
    assert not bool(over.any()), f"{key}: {int(over.sum())} elements outside the bound, err / bound up to {ratio:.3f}"


def _word_state(w):
    """what an amax word holds, whichever of its lines the launch's blocks happened to use (csrc/planes.h pl_floor_commit files the
    below-floor counts by XCD and block index): the bits of the bound, and the number of non-zero outputs under the 2^-27 floor"""
    lines = w.view(-1, 16)
    return int(lines[:, 0].max()), int(lines[:, 1].sum())


def _guarded(n):
    """n floats followed by a guard, all sentinels"""
    return torch.full((n + GUARD,), SENTINEL, device="cuda")


def _bound_words(ops, g3, b3, gs, bs, M, C):
    """the word the model forms: the shortcut's Samuelson bound, chained into bn3's as add_word"""
    ws, w = (torch.zeros(WORD, device="cuda", dtype=torch.int32) for _ in range(2))
    xm = math.sqrt(max(M - 1, 1))
    ops.call("tris_bn_out_bound2_f32", ops.P(gs), ops.P(bs), C, xm, None, ws.data_ptr(), ops._stream())
    ops.call("tris_bn_out_bound2_f32", ops.P(g3), ops.P(b3), C, xm, ws.data_ptr(), w.data_ptr(), ops._stream())
    return w


def _both(ops, x3, st3, xs, sts, M, C):
    """-> (planes, mask bytes, word) of the two-launch chain and of the pair pass, each into guarded buffers of its own"""
    mu3, is3, g3, b3 = st3
    mus, iss, gs, bs = sts
    n = M * C
    out = []
    for pair in (False, True):
        w = _bound_words(ops, g3, b3, gs, bs, M, C)
        y, mask = _guarded(n), torch.full((n // 8 + GUARD,), 0xA5, device="cuda", dtype=torch.uint8)
        if pair:
            ops.call("tris_bn_mask_next", mask.data_ptr())
            ops.call("tris_bn_apply_pair_pl_f32", ops.P(x3), ops.P(mu3), ops.P(is3), ops.P(g3), ops.P(b3), ops.P(xs), ops.P(mus),
                     ops.P(iss), ops.P(gs), ops.P(bs), ops.P(y), w.data_ptr(), M, C, ops._stream())
        else:
            idn = torch.empty(n, device="cuda")
            ops.call("tris_bn_apply_f32", ops.P(xs), ops.P(mus), ops.P(iss), ops.P(gs), ops.P(bs), None, ops.P(idn), M, C, 0,
                     ops._stream())
            ops.call("tris_bn_mask_next", mask.data_ptr())
            ops.call("tris_bn_apply_pl_f32", ops.P(x3), ops.P(mu3), ops.P(is3), ops.P(g3), ops.P(b3), ops.P(idn), 1, None, ops.P(y),
                     w.data_ptr(), M, C, 1, ops._stream())
        out.append((y, mask, w))
    torch.cuda.synchronize()
    return out


def _same_bits(ops, chain, pair, n):
    (ya, ma, wa), (yb, mb, wb) = chain, pair
    assert bool((yb[n:] == SENTINEL).all()) and bool((mb[n // 8:] == 0xA5).all()), "the pair pass wrote behind its outputs"
    assert torch.equal(ya.view(torch.int32), yb.view(torch.int32)), \
        f"{int((ya.view(torch.int32) != yb.view(torch.int32)).sum())} plane words differ from the two-launch chain"
    assert torch.equal(ma, mb), "ReLU-mask bytes differ from the two-launch chain"
    assert _word_state(wa) == _word_state(wb), "the amax word (bound, below-floor count) differs from the two-launch chain"
    got = torch.empty(n, device="cuda")
    ops.call("tris_h2_unplanes_f32", ops.P(yb), ops.P(got), n, wb.data_ptr(), ops._stream())
    bits = (mb[:n // 8, None].int() >> torch.arange(8, device="cuda")) & 1
    assert torch.equal(bits.reshape(-1).bool(), got > 0), "a mask bit is not the sign of the plane element"
    return got


def _stats_dev(kind, M, C):
    d = OB.inputs(kind, M, C)
    mean, invstd = OB.stored_stats(kind, M, C)
    return d, (mean, invstd), tuple(t.cuda() for t in (mean, invstd, d["gamma"], d["beta"]))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_pair_equals_two_launches(ops, case):
    kind, (B, H, W, C) = case
    M = B * H * W
    d3, (mean3, inv3), st3 = _stats_dev(kind, M, C)
    ds, (mean_s, inv_s), sts = _stats_dev(SHORTCUT_KIND[kind], M, C)
    x3, xs = d3["x"].cuda(), ds["x"].cuda()
    chain, pair = _both(ops, x3, st3, xs, sts, M, C)
    got = _same_bits(ops, chain, pair, M * C)
    z3, _, by3 = OB.apply(d3["x"], mean3, inv3, d3["gamma"], d3["beta"])
    zs, _, bys = OB.apply(ds["x"], mean_s, inv_s, ds["gamma"], ds["beta"])
    _inside(got, (z3 + zs).clamp_min(0.0), by3 + bys, ("apply_pair", "y", kind, (B, H, W, C)))


@pytest.mark.parametrize("C", [8, 64])
def test_forward_pair_at_the_kink_of_the_sum(ops, C):
    """x3 within 8 float32 steps of the value at which bn3(x3) + bn_s(xs) changes sign, for every element: the mask bytes and the planes
    are the chain's, and wherever float64 is sure of the sign the mask has it"""
    M = OB.CROSSING_M
    _, mean3, inv3, g3, b3 = OB.crossing_inputs(C)
    ds = OB.inputs("randn", M, C)
    mean_s, inv_s = OB.stored_stats("randn", M, C)
    zs, _, bys = OB.apply(ds["x"], mean_s, inv_s, ds["gamma"], ds["beta"])
    x0 = (mean3.double() - (b3.double() + zs) / (inv3.double() * g3.double())).float()             # [M, C]
    k = (torch.arange(M, dtype=torch.int32) % 17 - 8)[:, None]
    x3c = (x0.view(torch.int32) + torch.where(x0 > 0, 1, -1).to(torch.int32) * k).view(torch.float32).contiguous()
    st3 = tuple(t.cuda() for t in (mean3, inv3, g3, b3))
    sts = tuple(t.cuda() for t in (mean_s, inv_s, ds["gamma"], ds["beta"]))
    chain, pair = _both(ops, x3c.cuda(), st3, ds["x"].cuda(), sts, M, C)
    got = _same_bits(ops, chain, pair, M * C)
    z3, _, by3 = OB.apply(x3c, mean3, inv3, g3, b3)
    z, by = z3 + zs, by3 + bys
    # the inputs do sit at the kink: in float64 the sum changes sign between the steps -8 and +8 of every column, and some elements
    # are closer to zero than the float32 evaluation can resolve
    assert bool((z[0] * z[16] < 0).all()) and bool((z.abs() <= by).any())
    _inside(got, z.clamp_min(0.0), by, ("apply_pair", "y", "crossing", (M, C)))
    judged = z.abs() > by
    assert torch.equal((got.cpu().view(M, C) > 0)[judged], (z > 0)[judged])


def test_forward_pair_streaming_form(ops):
    """the smallest [M, 64] above pl_big's threshold, plus a row (a ragged last unit): bit for bit on the device, rows of both ends
    against the oracle"""
    M, C = BIG_M, 64
    assert M * C // 8 * 32 * 3 > (256 << 20) >= (M - 2) * C // 8 * 32 * 3
    gen = torch.Generator(device="cuda").manual_seed(5)
    x3 = torch.randn(M, C, device="cuda", generator=gen) * 2 + 0.3
    xs = torch.randn(M, C, device="cuda", generator=gen) * 0.5 - 1.0
    par = lambda: (1 + 0.3 * torch.randn(C, device="cuda", generator=gen), 0.2 * torch.randn(C, device="cuda", generator=gen))
    (g3, b3), (gs, bs) = par(), par()
    stat = lambda x: (x.double().mean(0).float(), torch.rsqrt(x.double().var(0, unbiased=False) + OB.EPS).float())
    (mu3, is3), (mus, iss) = stat(x3), stat(xs)
    chain, pair = _both(ops, x3, (mu3, is3, g3, b3), xs, (mus, iss, gs, bs), M, C)
    got = _same_bits(ops, chain, pair, M * C).view(M, C)
    rows = torch.cat([torch.arange(0, 96), torch.arange(M - 96, M)])
    z3, _, by3 = OB.apply(x3[rows.cuda()], mu3, is3, g3, b3)
    zs, _, bys = OB.apply(xs[rows.cuda()], mus, iss, gs, bs)
    _inside(got[rows.cuda()], (z3 + zs).clamp_min(0.0), by3 + bys, ("apply_pair", "y", "streaming", (M, C)))


# ================================================================================================================ the block
def _block(inplanes, planes, stride, seed):
    from tris_amd.CLIP.clip.model import Bottleneck
    torch.manual_seed(seed)
    net = Bottleneck(inplanes, planes, stride).cuda().train()
    with torch.no_grad():
        for n_, p in net.named_parameters():
            if p.dim() == 1:
                p.copy_(1 + 0.2 * torch.randn_like(p) if n_.endswith("weight") else 0.1 * torch.randn_like(p))
    return net


def _run_block(ops, stride, names=None, dims=(64, 32, 16), backward=True):
    """one Bottleneck(inplanes, planes, stride) on [2, hw, hw, inplanes] in an h2 step of its own -> output, input gradient,
    parameter gradients"""
    inplanes, planes, hw = dims
    net = _block(inplanes, planes, stride, 11)
    torch.manual_seed(12)
    x = torch.relu(torch.randn(2, hw, hw, inplanes, device="cuda")).requires_grad_()
    orig = ops.call

    def spy(name, *a):
        names.append(name)
        return orig(name, *a)
    if names is not None:
        ops.call = spy
    try:
        ops.h2_begin_step()
        y = ops.unplanes(net(x))
        if backward:
            (y * torch.linspace(-1, 1, y.shape[-1], device="cuda")).sum().backward()
            ops.wgrad_join()
        ops.h2_end_step()
    finally:
        ops.call = orig
    torch.cuda.synchronize()
    if not backward:
        return y.detach().clone(), None, {}
    return y.detach().clone(), x.grad.clone(), {n_: p.grad.clone() for n_, p in net.named_parameters()}


# Bottleneck(64, 32) on [2, 16, 16, 64] is the smallest block whose every product takes the fused epilogues the model's blocks take
# (every reduction length a multiple of 32, at least 128 rows behind the stride-2 pool for the statistics partials).
# Bottleneck(16, 8) on [2, 8, 8, 16] runs FORWARD only: tris_conv3x3_dgrad_bnbwd_f32 refuses a 3x3 data gradient over 8 channels
# (Cout % 16), with the switch on or off, so that block has no backward on this stack; its statistics come from passes of their own.
BLOCKS = [((64, 32, 16), True), ((16, 8, 8), False)]


@pytest.mark.parametrize("dims,backward", BLOCKS, ids=["64x32", "16x8-forward"])
@pytest.mark.parametrize("stride", [2, 1])
def test_bottleneck_on_vs_off(ops, stride, dims, backward):
    from tris_amd.config import cfg
    res, names = {}, {}
    for on in (True, False):
        cfg.bn_pair = on
        names[on] = []
        res[on] = _run_block(ops, stride, names[on], dims, backward)
    assert names[True].count("tris_bn_apply_pair_pl_f32") == 1 and "tris_bn_apply_f32" not in names[True], "the pair pass did not run"
    assert "tris_bn_apply_pair_pl_f32" not in names[False] and names[False].count("tris_bn_apply_f32") == 1
    assert len(names[True]) < len(names[False]), "the pair path saves the shortcut's apply launch"
    (y1, gx1, g1), (y0, gx0, g0) = res[True], res[False]
    assert torch.equal(y1, y0), "output"
    if not backward:
        return
    # stride 2: the shortcut's pooled gradient reaches conv1's epilogue as it is; the expansion pass is gone
    assert names[True].count("tris_gemm_resid_pool_next") == (1 if stride == 2 else 0) and "tris_avgpool2_bwd_f32" not in names[True]
    assert "tris_gemm_resid_pool_next" not in names[False] and names[False].count("tris_avgpool2_bwd_f32") == (1 if stride == 2 else 0)
    assert torch.equal(gx1, gx0), "input gradient"
    for n_ in g0:
        assert torch.equal(g1[n_], g0[n_]), n_


# ================================================================================================================ fallbacks
def _forward_calls(ops, monkeypatch, group=None):
    net = _block(64, 32, 2, 11)
    if group is not None:
        from tris_amd import comm
        from tris_amd.CLIP.clip.model import BatchNorm2d
        monkeypatch.setattr(comm, "world_size", lambda g: 1)
        monkeypatch.setattr(comm, "syncbn_mailbox", lambda g, n: None)
        monkeypatch.setattr(comm, "syncbn_all_gather_into", lambda out, src, group=None: out.copy_(src))
        for m in net.modules():
            if isinstance(m, BatchNorm2d):
                m.process_group = group
    torch.manual_seed(12)
    x = torch.relu(torch.randn(2, 16, 16, 64, device="cuda")).requires_grad_()
    names, orig = [], ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), orig(name, *a))[1])
    ops.h2_begin_step()
    y = ops.unplanes(net(x))
    ops.h2_end_step()
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "call", orig)
    return names, y.detach()


@pytest.mark.parametrize("how", ["group", "switch", "x3"])
def test_fallback_is_the_old_chain(ops, monkeypatch, how):
    from tris_amd.config import cfg
    cfg.bn_pair = True
    base, y_pair = _forward_calls(ops, monkeypatch)
    assert base.count("tris_bn_apply_pair_pl_f32") == 1
    if how == "switch":
        cfg.bn_pair = False
    elif how == "x3":
        ops.set_gemm_mode("x3")
    names, y = _forward_calls(ops, monkeypatch, group=object() if how == "group" else None)
    assert "tris_bn_apply_pair_pl_f32" not in names
    # the shortcut BatchNorm writes its fp32 output (tris_bn_apply_f32, the one launch of that name in a block on planes; all four
    # BatchNorms of the block in x3), and bn3 reads it back as its residual
    if how == "x3":
        assert names.count("tris_bn_apply_f32") >= 2 and "tris_bn_apply_pl_f32" not in names
    else:
        assert names.count("tris_bn_apply_f32") == 1
        assert names.count("tris_bn_apply_pl_f32") == 2 and names.count("tris_bn_apply_pool_pl_f32") == 1
    if how == "switch":
        assert torch.equal(y, y_pair)


@pytest.mark.parametrize("why", ["no_planes", "no_relu"])
def test_a_batchnorm_that_cannot_pair_writes_the_shortcut_after_all(ops, why):
    """ops.batch_norm(pair=True) hands back an unallocated stand-in; a BatchNorm that takes it as its residual but cannot run the pair
    pass (no plane output, or no ReLU) writes the shortcut's output first and goes on as without the switch: forward and every
    gradient bit for bit the switch-off chain's"""
    from tris_amd.config import cfg
    B, H, W, C = 2, 6, 10, 64
    d3, ds = OB.inputs("randn", B * H * W, C), OB.inputs("offset", B * H * W, C)
    res = {}
    for on in (True, False):
        cfg.bn_pair = on
        leaves = [t.clone().cuda().requires_grad_() for t in (d3["x"].view(B, H, W, C), d3["gamma"], d3["beta"],
                                                            ds["x"].view(B, H, W, C), ds["gamma"], ds["beta"])]
        x3, g3, b3, xs, gs, bs = leaves
        rm, rv, rm_s, rv_s = (t.clone().cuda() for t in (d3["rmean"], d3["rvar"], ds["rmean"], ds["rvar"]))
        ops.h2_begin_step()
        idn = ops.batch_norm(xs, gs, bs, rm_s, rv_s, training=True, pair=True)
        assert hasattr(idn, "_bn_pair") == on
        if on:
            assert idn.untyped_storage().nbytes() == 4 and tuple(idn.shape) == (B, H, W, C)     # nothing of the output's size exists
        y = ops.batch_norm(x3, g3, b3, rm, rv, resid=idn, relu=why != "no_relu", training=True, planes=why != "no_planes")
        y = ops.unplanes(y)
        y.backward(d3["dy"].view(B, H, W, C).cuda())
        ops.h2_end_step()
        torch.cuda.synchronize()
        res[on] = [y.detach().clone(), rm, rv, rm_s, rv_s] + [t.grad.clone() for t in leaves]
    for k, (a, b) in enumerate(zip(res[True], res[False])):
        assert torch.equal(a, b), k


# ================================================================================================================ contracts
def test_entry_point_refuses_what_the_kernel_cannot_index(ops):
    from tris_amd._lib import TrisHipError
    buf = torch.full((1 << 22,), SENTINEL, device="cuda")
    p = [buf.data_ptr() + 4 * ((1 << 19) + k * (1 << 18)) for k in range(12)]
    word = torch.zeros(WORD, device="cuda", dtype=torch.int32)
    wp = word.data_ptr()

    def refused(*args):
        with pytest.raises(TrisHipError, match=r"hipError_t 1$"):                # hipErrorInvalidValue
            ops.call("tris_bn_apply_pair_pl_f32", *args, ops._stream())
    for C in (4, 12, 6, 24, 4096):                                               # not whole groups of 8, or no divisor of 2048
        refused(*p[:11], wp, 8, C)
    refused(*p[:11], None, 8, 8)                                                 # no amax word
    refused(*p[:11], wp, 0, 8)                                                   # no rows
    for k in range(11):                                                          # a null or misaligned pointer, one at a time
        for bad in (None, p[k] + 4):
            a = list(p[:11])
            a[k] = bad
            refused(*a, wp, 8, 8)
    mask = torch.full((64,), 0xA5, device="cuda", dtype=torch.uint8)
    ops.call("tris_bn_mask_next", mask.data_ptr())                               # a refused call consumes the arming
    refused(*p[:11], wp, 8, 12)
    x = torch.randn(8, 8, device="cuda")
    c = [torch.ones(8, device="cuda") for _ in range(8)]
    y = torch.empty(8, 8, device="cuda")
    ops.call("tris_bn_apply_pair_pl_f32", ops.P(x), *(ops.P(t) for t in c[:4]), ops.P(x), *(ops.P(t) for t in c[4:]), ops.P(y), wp, 8, 8,
             ops._stream())
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()) and bool((mask == 0xA5).all())


# ================================================================================================================ pooled residual
def _gemm(ops, A, Wt, C, resid, ldr, pool=None):
    """C [M, N] = A [M, K] . Wt [N, K]^T + resid, one slice (no workspace: the form the pooled residual runs in)"""
    M, K = A.shape
    N = Wt.shape[0]
    if pool is not None:
        ops.call("tris_gemm_resid_pool_next", pool[0], pool[1])
    ops.call("tris_gemm_f32", ops.P(A), ops.P(Wt), ops.P(C), M, N, K, K, K, C.stride(0), 0, 1, 1, 0, 0, 0, None, 0, ops.P(resid), ldr, 0, 0,
             1.0, None, 0, ops._stream())


@pytest.mark.parametrize("N", [64, 62], ids=["vector-epilogue", "scalar-epilogue"])
@pytest.mark.parametrize("shape", [(2, 6, 10), (2, 40, 60), (3, 2, 2)], ids=lambda s: "x".join(map(str, s)))
def test_pooled_residual_epilogue(ops, shape, N):
    """tris_gemm_f32 with the pooled residual == tris_avgpool2_bwd_f32 into a full-size tensor + the same product reading that"""
    B, H, W = shape
    M, K, ld = B * H * W, 32, 64
    gen = torch.Generator(device="cuda").manual_seed(M + N)
    A = torch.randn(M, K, device="cuda", generator=gen)
    Wt = torch.randn(N, K, device="cuda", generator=gen) * 0.1
    g = torch.randn(B, H // 2, W // 2, ld, device="cuda", generator=gen)
    full = torch.empty(B, H, W, ld, device="cuda")
    ops.call("tris_avgpool2_bwd_f32", ops.P(g), ops.P(full), B, H, W, ld, ops._stream())
    assert torch.equal(full, 0.25 * g.repeat_interleave(2, 1).repeat_interleave(2, 2))
    want, got = _guarded(M * N), _guarded(M * N)
    _gemm(ops, A, Wt, want[:M * N].view(M, N), full, ld)
    _gemm(ops, A, Wt, got[:M * N].view(M, N), g, ld, pool=(H, W))
    torch.cuda.synchronize()
    assert torch.equal(want, got)
    ref = A.double() @ Wt.double().t() + full.view(M, ld)[:, :N].double()
    assert float((got[:M * N].view(M, N).double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    # the arming is one-shot: the next product reads its residual row for row again
    again = _guarded(M * N)
    _gemm(ops, A, Wt, again[:M * N].view(M, N), full, ld)
    torch.cuda.synchronize()
    assert torch.equal(again, want)


def test_pooled_residual_in_the_fused_backward_reduction(ops):
    """tris_gemm_bnbwd_f32 (conv1's data gradient of a block behind a linked bn3): masked gradient and partial sums bit for bit"""
    import ctypes
    B, H, W, N, K = 2, 40, 60, 64, 32
    M = B * H * W
    d = OB.inputs("randn", M, N)
    mean, invstd = OB.stored_stats("randn", M, N)
    x, gam, bet, mean_d, inv_d = d["x"].cuda(), d["gamma"].cuda(), d["beta"].cuda(), mean.cuda(), invstd.cuda()
    gen = torch.Generator(device="cuda").manual_seed(3)
    dy = torch.randn(M, K, device="cuda", generator=gen)
    Wkn = torch.randn(K, N, device="cuda", generator=gen) * 0.1
    g = torch.randn(B, H // 2, W // 2, N, device="cuda", generator=gen)
    full = torch.empty(B, H, W, N, device="cuda")
    ops.call("tris_avgpool2_bwd_f32", ops.P(g), ops.P(full), B, H, W, N, ops._stream())
    out = []
    for pool in (None, (H, W)):
        dz = _guarded(M * N)
        part = torch.full((((M + 127) // 128) * 2 * N + 64,), SENTINEL, device="cuda", dtype=torch.float64)
        rows = ctypes.c_int(0)
        if pool is not None:
            ops.call("tris_gemm_resid_pool_next", *pool)
        ops.call("tris_gemm_bnbwd_f32", ops.P(dy), ops.P(Wkn), ops.P(dz), M, N, K, ops.P(g if pool else full), N, ops.P(x), None,
                 ops.P(mean_d), ops.P(inv_d), ops.P(gam), ops.P(bet), part.data_ptr(), ctypes.byref(rows), ops._stream())
        assert rows.value == (M + 127) // 128
        out.append((dz, part))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_pooled_residual_contract(ops):
    from tris_amd._lib import TrisHipError
    M, N, K = 64, 64, 32
    A, Wt, C = torch.randn(M, K, device="cuda"), torch.randn(N, K, device="cuda"), torch.full((M, N), SENTINEL, device="cuda")
    g = torch.randn(M // 4 + 8, N, device="cuda")

    def refused(pool, resid, ldr):
        with pytest.raises(TrisHipError, match=r"hipError_t 1$"):
            _gemm(ops, A, Wt, C, resid, ldr, pool=pool)
    for pool in ((3, 4), (4, 3), (1, 1), (0, 4), (4, -2), (4, 6)):     # odd or empty maps; M = 64 is no multiple of 4 x 6
        refused(pool, g, N)
    refused((4, 4), None, N)                                           # no residual to pool
    refused((4, 4), g.view(-1)[1:], N)                                 # misaligned rows
    refused((4, 4), g, N + 2)
    torch.cuda.synchronize()
    assert bool((C == SENTINEL).all())
    _gemm(ops, A, Wt, C, None, 0)                                      # a refused call consumed its arming
    torch.cuda.synchronize()
    assert torch.allclose(C, A @ Wt.t(), atol=1e-3)


# ================================================================================================================ backward pair
def _bnbwd(ops, dy, Wkn, resid, x, y, mean, invstd, gamma, beta, x2=None):
    """tris_gemm_bnbwd_f32 -> (dz, part, rows[, part2]); x2 = (xs, mean_s, invstd_s): armed with tris_gemm_bnbwd_x2_next"""
    import ctypes
    M, K = dy.shape
    N = Wkn.shape[1]
    nrow = (M + 127) // 128
    dz = _guarded(M * N)
    part, part2 = (torch.full((nrow * 2 * N + 64,), SENTINEL, device="cuda", dtype=torch.float64) for _ in range(2))
    rows = ctypes.c_int(-1)
    if x2 is not None:
        ops.call("tris_gemm_bnbwd_x2_next", ops.P(x2[0]), ops.P(x2[1]), ops.P(x2[2]), part2.data_ptr())
    ops.call("tris_gemm_bnbwd_f32", ops.P(dy), ops.P(Wkn), ops.P(dz), M, N, K, ops.P(resid), N, ops.P(x), ops.P(y), ops.P(mean),
             ops.P(invstd), ops.P(gamma), ops.P(beta), part.data_ptr(), ctypes.byref(rows), ops._stream())
    torch.cuda.synchronize()
    return dz, part, rows.value, part2


@pytest.mark.parametrize("M,N,tile", [(120, 64, None), (4800, 64, None), (4800, 128, "128x128"), (4800, 128, "128x64")],
                         ids=["120x64", "4800x64", "4800x128-tile128x128", "4800x128-tile128x64"])
def test_epilogue_third_sum(ops, M, N, tile):
    """tris_gemm_bnbwd_f32 with a second BatchNorm armed: sum(dz xhat_s) inside test_backward's bound of the fp64 sum over the masked
    gradient the launch stored; dz and the two other sums the bits of the launch without it.  M = 120 is below the 128 rows the fused
    reduction needs: the launch declines (no rows, nothing written) armed or not, and the arming does not outlive it.  N = 128: both
    tile widths of the EPI_PAIR kernels (the fused reduction fixes 128 rows)."""
    K = 32
    ops.set_option("FORCE_TILE", tile)
    d3, ds = OB.inputs("randn", M, N), OB.inputs("offset", M, N)
    (mean3, inv3), (mean_s, inv_s) = OB.stored_stats("randn", M, N), OB.stored_stats("offset", M, N)
    x3, g3, b3, xs = d3["x"].cuda(), d3["gamma"].cuda(), d3["beta"].cuda(), ds["x"].cuda()
    m3, i3, m_s, i_s = mean3.cuda(), inv3.cuda(), mean_s.cuda(), inv_s.cuda()
    gen = torch.Generator(device="cuda").manual_seed(M)
    dy = torch.randn(M, K, device="cuda", generator=gen)
    Wkn = torch.randn(K, N, device="cuda", generator=gen) * 0.2
    plain = _bnbwd(ops, dy, Wkn, None, x3, None, m3, i3, g3, b3)
    armed = _bnbwd(ops, dy, Wkn, None, x3, None, m3, i3, g3, b3, x2=(xs, m_s, i_s))
    again = _bnbwd(ops, dy, Wkn, None, x3, None, m3, i3, g3, b3)
    assert plain[2] == armed[2] == again[2] == (0 if M < 128 else (M + 127) // 128)
    assert torch.equal(plain[0], armed[0]) and torch.equal(plain[1], armed[1]), "the arming changes dz or the other two sums"
    assert torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1]) and bool((again[3] == SENTINEL).all()), "the arming outlived its call"
    if M < 128:
        assert bool((armed[0] == SENTINEL).all()) and bool((armed[1] == SENTINEL).all()) and bool((armed[3] == SENTINEL).all())
        return
    rows = armed[2]
    p2 = armed[3][:rows * 2 * N].view(rows, 2, N)
    assert bool((p2[:, 1] == SENTINEL).all()) and bool((armed[3][rows * 2 * N:] == SENTINEL).all()), "part2: only the first N of a row"
    dz = armed[0][:M * N].view(M, N)
    assert 0.2 < float((dz != 0).double().mean()) < 0.8
    (_, s1), (_, bnd1), _ = OB.bwd_reduce(dz, ds["x"], mean_s, inv_s)
    _inside(p2[:, 0].sum(0).float(), s1, bnd1, ("gemm_bnbwd", "sum_dzx2", "offset", (M, N)))
    (_, s3), (_, bnd3), _ = OB.bwd_reduce(dz, d3["x"], mean3, inv3)       # (the existing second sum, for comparison)
    _inside(armed[1][:rows * 2 * N].view(rows, 2, N)[:, 1].sum(0).float(), s3, bnd3, ("gemm_bnbwd", "sum_dzx", "randn", (M, N)))


@pytest.mark.parametrize("C", [8, 64, 1024])
@pytest.mark.parametrize("rows", [1, 63, 2049])
def test_pair_finalizer_equals_two_bound_finalizers(ops, rows, C):
    pa, M = OB.partial_rows(rows, C)
    pb, _ = OB.partial_rows(rows + 1, C)
    part, part2 = pa.cuda(), pb[:rows].contiguous().cuda()
    both2 = torch.stack([part[:, 0], part2[:, 0]], 1).contiguous()       # what a launch of its own would finalize for the shortcut
    gen = torch.Generator(device="cuda").manual_seed(rows + C)
    g3, i3, gs, i_s = (torch.randn(C, device="cuda", generator=gen) for _ in range(4))
    dzw = torch.zeros(WORD, device="cuda", dtype=torch.int32)
    dzw[16 * 5] = torch.tensor(0.37, dtype=torch.float32).view(torch.int32)
    inv_cnt, xm, st = OB.f32_scalar(1.0 / M), math.sqrt(M - 1), ops._stream()
    want = []
    for p_, g_, i_ in ((part, g3, i3), (both2, gs, i_s)):
        o = torch.full((2 * C,), SENTINEL, device="cuda")
        w = torch.zeros(WORD, device="cuda", dtype=torch.int32)
        ops.call("tris_part_finalize_bound_f32", p_.data_ptr(), rows, C, ops.P(o), ops.P(o, C), ops.P(g_), ops.P(i_), inv_cnt, xm,
                 dzw.data_ptr(), w.data_ptr(), st)
        want.append((o, w))
    o3, os_ = torch.full((2 * C + 8,), SENTINEL, device="cuda"), torch.full((2 * C + 8,), SENTINEL, device="cuda")
    w3, ws = (torch.zeros(WORD, device="cuda", dtype=torch.int32) for _ in range(2))
    ops.call("tris_part_finalize_pair_f32", part.data_ptr(), part2.data_ptr(), rows, C, ops.P(o3), ops.P(o3, C), ops.P(os_), ops.P(os_, C),
             ops.P(g3), ops.P(i3), ops.P(gs), ops.P(i_s), inv_cnt, xm, dzw.data_ptr(), w3.data_ptr(), ws.data_ptr(), st)
    torch.cuda.synchronize()
    assert torch.equal(o3[:2 * C], want[0][0]) and torch.equal(os_[:2 * C], want[1][0])
    assert bool((o3[2 * C:] == SENTINEL).all()) and bool((os_[2 * C:] == SENTINEL).all())
    assert torch.equal(w3, want[0][1]) and torch.equal(ws, want[1][1]) and int(w3.max()) > 0 and int(ws.max()) > 0


def _bwd_pair_case(ops, x3, st3, xs, sts, dz, sums3, sums_s, M, C):
    """-> the (dX planes, word) pairs of two tris_bn_bwd_apply_pl_f32 launches and of the pair pass, fed the same sums"""
    mu3, is3, g3 = st3
    mus, iss, gs = sts
    n, inv_cnt, xm, st = M * C, OB.f32_scalar(1.0 / M), math.sqrt(max(M - 1, 1)), ops._stream()
    assert torch.equal(sums3[:C], sums_s[:C])           # one sum(dz) for both
    dzw = torch.zeros(WORD, device="cuda", dtype=torch.int32)
    ops.call("tris_amax_bits_f32", ops.P(dz), n, dzw.data_ptr(), st)

    def words():
        out = []
        for g_, i_, s_ in ((g3, is3, sums3), (gs, iss, sums_s)):
            w = torch.zeros(WORD, device="cuda", dtype=torch.int32)
            ops.call("tris_bn_bwd_bound_f32", ops.P(g_), ops.P(i_), ops.P(s_), ops.P(s_, C), C, inv_cnt, xm, dzw.data_ptr(), w.data_ptr(), st)
            out.append(w)
        return out
    wa, wb = words(), words()
    a3, a_s, b3, b_s = (_guarded(n) for _ in range(4))
    for x_, (mu, is_, g_), s_, o, w in ((x3, st3, sums3, a3, wa[0]), (xs, sts, sums_s, a_s, wa[1])):
        ops.call("tris_bn_bwd_apply_pl_f32", ops.P(dz), None, ops.P(x_), ops.P(mu), ops.P(is_), ops.P(g_), ops.P(s_), ops.P(s_, C), inv_cnt,
                 ops.P(o), w.data_ptr(), None, M, C, None, st)
    ops.call("tris_bn_bwd_apply_pair_pl_f32", ops.P(dz), ops.P(x3), ops.P(mu3), ops.P(is3), ops.P(g3), ops.P(sums3, C), ops.P(xs), ops.P(mus),
             ops.P(iss), ops.P(gs), ops.P(sums_s, C), ops.P(sums3), inv_cnt, ops.P(b3), wb[0].data_ptr(), ops.P(b_s), wb[1].data_ptr(), M, C, st)
    torch.cuda.synchronize()
    for name, a, b, u, v in (("dX3", a3, b3, wa[0], wb[0]), ("dXs", a_s, b_s, wa[1], wb[1])):
        assert bool((b[n:] == SENTINEL).all()), f"{name}: written behind the output"
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: planes differ from tris_bn_bwd_apply_pl_f32"
        assert _word_state(u) == _word_state(v), f"{name}: the amax word (bound, below-floor count) differs"
    out = []
    for b, w in ((b3, wb[0]), (b_s, wb[1])):
        got = torch.empty(n, device="cuda")
        ops.call("tris_h2_unplanes_f32", ops.P(b), ops.P(got), n, w.data_ptr(), st)
        out.append((got, float(w.max().view(torch.float32))))
    return out


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_backward_pair_equals_two_applies(ops, case):
    kind, (B, H, W, C) = case
    M = B * H * W
    d3, (mean3, inv3), st3 = _stats_dev(kind, M, C)
    ds, (mean_s, inv_s), sts = _stats_dev(SHORTCUT_KIND[kind], M, C)
    mask = torch.rand(M, C, generator=torch.Generator().manual_seed(M + C)) < 0.5
    dz_h = torch.where(mask, d3["dy"], torch.zeros(()))
    (s0, s13), _, _ = OB.bwd_reduce(dz_h, d3["x"], mean3, inv3)
    (_, s1s), _, _ = OB.bwd_reduce(dz_h, ds["x"], mean_s, inv_s)
    sums3, sums_s = torch.cat([s0, s13]).float().cuda(), torch.cat([s0, s1s]).float().cuda()
    (got3, amax3), (got_s, amax_s) = _bwd_pair_case(ops, d3["x"].cuda(), st3[:3], ds["x"].cuda(), sts[:3], dz_h.cuda(), sums3, sums_s, M, C)
    inv_cnt = OB.f32_scalar(1.0 / M)
    for name, got, amax, d, mu, is_, s1 in (("dx3", got3, amax3, d3, mean3, inv3, s13), ("dxs", got_s, amax_s, ds, mean_s, inv_s, s1s)):
        ref, bound, _ = OB.bwd_apply(dz_h, d["x"], mu, is_, d["gamma"], s0.float(), s1.float(), inv_cnt)
        # against float64 where the plane format is relative (csrc/planes.h: an element keeps its 22 bits while its hi piece is a normal
        # fp16 number, |x s| >= 2^-14; one scale serves the tensor, and the `gamma` kind spreads the channels over 2^20): the bound of
        # tris_bn_bwd_apply_f32 -- nine roundings, and the plane representation within U of the value, C_DX = 10 in all
        scale = 2.0 ** (13 - math.floor(math.log2(amax))) if amax > 0 else 1.0
        rel = (ref.abs() * scale >= 2.0 ** -14).reshape(-1)
        _inside(got.cpu()[rel], ref.reshape(-1)[rel], bound.reshape(-1)[rel], ("bwd_apply_pair", name, kind, (B, H, W, C)))


def test_backward_pair_streaming_form(ops):
    """the smallest [M, 64] at which the pair pass (five streams) takes the streaming form, plus a row; the two single passes (three
    streams each) are still in the grid-stride form there: the same bits across the two forms"""
    M, C = 209717, 64
    assert M * C // 8 * 32 * 5 > (256 << 20) >= (M - 2) * C // 8 * 32 * 5
    gen = torch.Generator(device="cuda").manual_seed(9)
    x3 = torch.randn(M, C, device="cuda", generator=gen) * 2 + 0.3
    xs = torch.randn(M, C, device="cuda", generator=gen) * 0.5 - 1.0
    dz = torch.randn(M, C, device="cuda", generator=gen) * (torch.rand(M, C, device="cuda", generator=gen) < 0.5)
    stat = lambda x: (x.double().mean(0).float(), torch.rsqrt(x.double().var(0, unbiased=False) + OB.EPS).float(),
                      1 + 0.3 * torch.randn(C, device="cuda", generator=gen))
    st3, sts = stat(x3), stat(xs)
    s0 = dz.double().sum(0)
    s1 = lambda x, st: (dz.double() * ((x.double() - st[0].double()) * st[1].double())).sum(0)
    sums3, sums_s = torch.cat([s0, s1(x3, st3)]).float(), torch.cat([s0, s1(xs, sts)]).float()
    _bwd_pair_case(ops, x3, st3, xs, sts, dz, sums3, sums_s, M, C)


def test_backward_pair_contracts(ops):
    from tris_amd._lib import TrisHipError
    buf = torch.full((1 << 22,), SENTINEL, device="cuda")
    p = [buf.data_ptr() + 4 * ((1 << 18) + k * (1 << 18)) for k in range(14)]
    w3, ws = (torch.zeros(WORD, device="cuda", dtype=torch.int32) for _ in range(2))

    def args(ptrs, a, b, M=8, C=8):
        return (*ptrs[:12], 0.125, ptrs[12], a, ptrs[13], b, M, C)

    def refused(name, *a):
        with pytest.raises(TrisHipError, match=r"hipError_t 1$"):
            ops.call(name, *a, ops._stream())
    for C in (4, 12, 24, 4096):
        refused("tris_bn_bwd_apply_pair_pl_f32", *args(p, w3.data_ptr(), ws.data_ptr(), C=C))
    refused("tris_bn_bwd_apply_pair_pl_f32", *args(p, w3.data_ptr(), ws.data_ptr(), M=0))
    refused("tris_bn_bwd_apply_pair_pl_f32", *args(p, None, ws.data_ptr()))
    refused("tris_bn_bwd_apply_pair_pl_f32", *args(p, w3.data_ptr(), None))
    refused("tris_bn_bwd_apply_pair_pl_f32", *args(p, w3.data_ptr(), w3.data_ptr()))          # one word for two tensors
    refused("tris_bn_bwd_apply_pair_pl_f32", *args(p[:12] + [p[12], p[12]], w3.data_ptr(), ws.data_ptr()))   # one output for both
    for k in range(14):
        for bad in (None, p[k] + 4):
            q = list(p)
            q[k] = bad
            refused("tris_bn_bwd_apply_pair_pl_f32", *args(q, w3.data_ptr(), ws.data_ptr()))
    # the finalizer: every pointer, at least one row, two different words
    fin = lambda q, rows=4, a=w3.data_ptr(), b=ws.data_ptr(), dzw=w3.data_ptr(): (q[0], q[1], rows, 8, q[2], q[3], q[4], q[5], q[6], q[7],
                                                                                 q[8], q[9], 0.125, 2.0, dzw, a, b)
    refused("tris_part_finalize_pair_f32", *fin(p, rows=0))
    refused("tris_part_finalize_pair_f32", *fin(p, b=w3.data_ptr()))
    refused("tris_part_finalize_pair_f32", *fin(p, a=None))
    refused("tris_part_finalize_pair_f32", *fin(p, dzw=None))
    for k in range(10):
        q = list(p)
        q[k] = None
        refused("tris_part_finalize_pair_f32", *fin(q))
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()) and int(w3.max()) == 0 and int(ws.max()) == 0
    # the arming of the product: a null or misaligned pointer fails the armed call, and the arming is gone with it
    import ctypes
    M, N, K = 256, 64, 32
    x, dy, Wkn = torch.randn(M, N, device="cuda"), torch.randn(M, K, device="cuda"), torch.randn(K, N, device="cuda")
    c = [torch.ones(N, device="cuda") for _ in range(4)]
    part = torch.empty(2 * 2 * N, device="cuda", dtype=torch.float64)
    for bad in ((None, ops.P(c[0]), ops.P(c[1]), part.data_ptr()), (ops.P(x) + 4, ops.P(c[0]), ops.P(c[1]), part.data_ptr()),
                (ops.P(x), ops.P(c[0]), ops.P(c[1]), None)):
        dz, rows = torch.full((M, N), SENTINEL, device="cuda"), ctypes.c_int(-1)
        ops.call("tris_gemm_bnbwd_x2_next", *bad)
        with pytest.raises(TrisHipError, match=r"hipError_t 1$"):
            ops.call("tris_gemm_bnbwd_f32", ops.P(dy), ops.P(Wkn), ops.P(dz), M, N, K, None, N, ops.P(x), None, ops.P(c[0]), ops.P(c[1]),
                     ops.P(c[2]), ops.P(c[3]), part.data_ptr(), ctypes.byref(rows), ops._stream())
        torch.cuda.synchronize()
        assert rows.value == 0 and bool((dz == SENTINEL).all())


def test_linked_pair_of_blocks_on_vs_off(ops):
    """a down-sampling Bottleneck whose output feeds the next block and nothing else (link_out): bn3's sums AND the shortcut
    BatchNorm's third sum come out of that block's conv1 data gradient, one finalizer, one apply pass for both input gradients.
    Against the switch off: the output and every gradient that does not pass through the shortcut BatchNorm's sums are the same bits;
    those sums are formed in another order (fp32 over a lane's 16 rows, then fp64, against fp64 throughout in the pass of their own),
    each within C_S U sum|terms| of the exact sum (test_epilogue_third_sum), so what depends on them -- the shortcut BatchNorm's and
    convolution's parameter gradients, the block's input gradient -- agrees to a few U relative to its own size: 1e-5 in norm is
    two orders above that and five below a wrong term."""
    from tris_amd.config import cfg
    from tris_amd.CLIP.clip.model import Bottleneck
    res, names = {}, {}
    for on in (True, False):
        cfg.bn_pair = on
        b1, b2 = _block(64, 32, 2, 21), _block(128, 32, 1, 22)
        assert isinstance(b1, Bottleneck)
        cap = {}

        def grab(mod, inp, out, cap=cap):
            # the shortcut BatchNorm's node keeps (x, gamma, beta, mean, invstd, y); the gradient it is handed is the masked dz
            st = out.grad_fn.saved_tensors
            cap.update(xs=st[0].detach().clone(), mean=st[3].detach().clone(), invstd=st[4].detach().clone())
            out.register_hook(lambda g: cap.__setitem__("dz", g.detach().clone()))
        hook = b1.downsample[2].register_forward_hook(grab)
        torch.manual_seed(23)
        x = torch.relu(torch.randn(2, 32, 32, 64, device="cuda")).requires_grad_()
        names[on], orig = [], ops.call
        ops.call = lambda name, *a, _n=names[on]: (_n.append(name), orig(name, *a))[1]
        try:
            ops.h2_begin_step()
            y = ops.unplanes(b2(b1(x, link_out=True)))
            (y * torch.linspace(-1, 1, y.shape[-1], device="cuda")).sum().backward()
            ops.wgrad_join()
            ops.h2_end_step()
        finally:
            ops.call = orig
        torch.cuda.synchronize()
        g = {"1." + n_: p.grad.clone() for n_, p in b1.named_parameters()}
        g.update({"2." + n_: p.grad.clone() for n_, p in b2.named_parameters()})
        res[on] = (y.detach().clone(), x.grad.clone(), g)
        hook.remove()
        # the shortcut BatchNorm's dgamma and dbeta of THIS run against float64 sums over the dz, xs and statistics of this run.
        # dgamma: test_backward's bound, C_S U sum|dz xhat_s|.  dbeta: test_backward's bound 2 U |ref| + 2^-40 sum|dz| holds for sums
        # formed in fp64 throughout (switch off: col_partial_kernel<1>); the product's epilogue adds a lane's <= 16 rows in fp32
        # before it widens (gemm_fast.h, as for every linked BatchNorm's dbeta), 15 roundings of partial sums <= the lane's
        # sum|dz| each: + 15 U sum|dz| with the switch on
        C_ = cap["xs"].shape[-1]
        dz2, xs2 = cap["dz"].reshape(-1, C_), cap["xs"].reshape(-1, C_)
        (s0, s1), (bd0, bd1), _ = OB.bwd_reduce(dz2, xs2, cap["mean"], cap["invstd"])
        assert 0.1 < float((dz2 != 0).double().mean()) < 0.9
        if on:
            bd0 = bd0 + 15 * OB.U * dz2.double().abs().sum(0).cpu()
        _inside(g["1.downsample.1.weight"], s1, bd1, ("block", "dgamma_s", "on" if on else "off", tuple(xs2.shape)))
        _inside(g["1.downsample.1.bias"], s0, bd0, ("block", "dbeta_s", "on" if on else "off", tuple(xs2.shape)))
    n1, n0 = names[True], names[False]
    assert n1.count("tris_bn_bwd_apply_pair_pl_f32") == 1 and n1.count("tris_part_finalize_pair_f32") == 1
    assert n1.count("tris_gemm_bnbwd_x2_next") == 1 and n0.count("tris_bn_bwd_bound_f32") - n1.count("tris_bn_bwd_bound_f32") == 1
    assert "tris_bn_bwd_apply_pair_pl_f32" not in n0 and "tris_gemm_bnbwd_x2_next" not in n0
    # gone with the switch on: the shortcut's reduction pass, its bound launch, its apply pass (and the forward's shortcut apply)
    assert n0.count("tris_bn_bwd_reduce_f32") - n1.count("tris_bn_bwd_reduce_f32") == 1
    assert n0.count("tris_bn_bwd_apply_pl_f32") - n1.count("tris_bn_bwd_apply_pl_f32") == 2
    (y1, gx1, g1), (y0, gx0, g0) = res[True], res[False]
    assert torch.equal(y1, y0)
    dependent = {"1.downsample.0.weight", "1.downsample.1.weight", "1.downsample.1.bias"}
    for n_ in g0:
        if n_ in dependent:
            assert float((g1[n_] - g0[n_]).norm()) <= 1e-5 * float(g0[n_].norm()), n_
        else:
            assert torch.equal(g1[n_], g0[n_]), n_
    assert float((gx1 - gx0).norm()) <= 1e-5 * float(gx0.norm())
