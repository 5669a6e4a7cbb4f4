"""Per-kernel parity: every HIP op (through the C ABI, via tris_amd.ops) against a plain PyTorch fp32 CPU
reference of the same op, forward and backward.  Tolerances are fp32-roundoff class (the MFMA path is exact f32)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tris_amd.config import cfg as CFG

pytestmark = pytest.mark.gpu

TOL = 2e-4


def dev(t):
    return t.cuda()


def close(a, b, tol=TOL, name=""):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    err = (a - b).abs().max().item()
    ref = max(1.0, b.abs().max().item())
    assert err <= tol * ref, f"{name}: max err {err:.3e} (ref scale {ref:.3e})"


def leaf(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).requires_grad_(True)


def gpu_leaf(t):
    return t.detach().clone().cuda().requires_grad_(True)


_VARIANT = {"x3-classic": ("FORCE_PIPE", 0), "h2-pipe": ("PIPE", 1)}


@pytest.fixture(scope="module", params=["x3", "x3-classic", "h2", "h2-pipe", "f32"])
def ops(request):
    """Every kernel test runs under all three arithmetics of the dense-product core -- split-bf16 x3 (default), the two-piece fp16
    h2 (operand scales from device-side amax words) and the f32-input MFMA -- and x3 / h2 under both loop structures: the
    pipelined one (two 16-deep LDS stages, one barrier per K tile; x3's static default for wide gathers) and the classic one
    (h2's static default): options FORCE_PIPE=0 / PIPE=1."""
    from tris_amd import ops as o
    prev = o.get_gemm_mode()
    o.set_gemm_mode(request.param.split("-")[0])
    if request.param in _VARIANT:
        o.set_option(*_VARIANT[request.param])
    yield o
    if request.param in _VARIANT:
        o.set_option(_VARIANT[request.param][0], None)
    o.set_gemm_mode(prev)


@pytest.fixture(autouse=True)
def _pin_variant(request):
    """(the per-test option reset of conftest.py would drop the module-scoped fixture's option: put it back)"""
    if "ops" in request.fixturenames:
        v = _VARIANT.get(request.node.callspec.params.get("ops"))
        if v is not None:
            from tris_amd import ops as o
            o.set_option(*v)
    yield


@pytest.mark.parametrize("M,N,K", [(100, 48, 1024), (130, 70, 52), (256, 256, 64), (48, 1024, 2048), (7, 5, 27),
                                   (3000, 64, 64), (1000, 200, 16),
                                   (200, 70, 64), (129, 33, 96)])   # fast kernel, N % 4 != 0: the scalar epilogue
def test_linear_fwd_bwd(ops, M, N, K):
    x, w, b, r = leaf(M, K), leaf(N, K, scale=0.1), leaf(N), leaf(M, N)
    y = x @ w.t() + b + r
    y.backward(torch.ones_like(y) * 0.5 + y.detach() * 0.1)
    gx, gw, gb, gr = gpu_leaf(x), gpu_leaf(w), gpu_leaf(b), gpu_leaf(r)
    gy = ops.linear(gx, gw, gb, gr)
    gy.backward(torch.ones_like(gy) * 0.5 + gy.detach() * 0.1)
    close(gy, y, name="y")
    close(gx.grad, x.grad, name="dx")
    close(gw.grad, w.grad, name="dw")
    close(gb.grad, b.grad, name="db")
    close(gr.grad, r.grad, name="dresid")


def test_gemm_epilogue_variants(ops):
    """bias per row / per column, alpha, batched residual: the vector epilogue (aligned, N % 4 == 0) and the scalar one
    (C / residual offset by one float) must give the same numbers as torch"""
    B, M, N, K = 3, 160, 96, 64
    g = torch.Generator().manual_seed(11)
    A, Bm = torch.randn(B, M, K, generator=g), torch.randn(B, N, K, generator=g)
    R, bias_r, bias_c = torch.randn(B, M, N, generator=g), torch.randn(M, generator=g), torch.randn(N, generator=g)
    dA, dB, dR = A.cuda(), Bm.cuda(), R.cuda()
    for mode, bias in ((1, bias_c), (2, bias_r)):
        ref = 0.5 * (A @ Bm.transpose(1, 2)) + (bias[None, None, :] if mode == 1 else bias[None, :, None]) + R
        for off in (0, 1):                                   # off = 1: C and the residual lose their 16-byte alignment
            buf = torch.full((B * M * N + 4,), float("nan"), device="cuda")
            rbuf = torch.zeros(B * M * N + 4, device="cuda")
            rbuf[off:off + B * M * N] = dR.flatten()
            C, Rv = buf[off:off + B * M * N], rbuf[off:off + B * M * N]
            ops.gemm(dA, dB, C, M, N, K, K, K, N, False, True, batch=B, sA=M * K, sB=N * K, sC=M * N, bias=bias.cuda(),
                     bias_mode=mode, resid=Rv, ldr=N, sR=M * N, alpha=0.5)
            close(C.view(B, M, N), ref, name=f"bias_mode {mode} offset {off}")


@pytest.mark.parametrize("M,N,K,tA,tB,slices", [(2048, 512, 4096, False, True, 8), (2048, 1024, 4096, False, False, 4),
                                                 (4096, 1024, 4096, False, True, 2), (1024, 2048, 4800, True, False, 4),
                                                 (2044, 508, 4096, False, True, 8)])
def test_fused_splitk_finish_equals_the_reduce_launch(ops, M, N, K, tA, tB, slices):
    """Split-K products armed with a ticket array (tris_splitk_tickets_next: ops.gemm does it) finish inside their own launch: the
    last-arriving block of each tile sums the slabs.  The result is the two-launch form's BIT FOR BIT (same slice order), with bias,
    QuickGELU / ReLU, residual and alpha in the finish; the ticket array is zero again afterwards; the launch counter says the fused
    form ran (static cost model: these shapes split into `slices`); FUSE_SPLITK=0 restores the reduce launch."""
    from tris_amd import _lib
    g = torch.Generator().manual_seed(5 + M + N)
    A = torch.randn((K, M) if tA else (M, K), generator=g).cuda()
    B = (torch.randn((N, K) if tB else (K, N), generator=g) * 0.05).cuda()
    bias, R = torch.randn(N, generator=g).cuda(), torch.randn(M, N, generator=g).cuda()
    ref = 0.5 * ((A.t() if tA else A).double().cpu() @ (B.t() if tB else B).double().cpu()) + bias.double().cpu()
    ref = (ref * torch.sigmoid(1.702 * ref) + R.double().cpu()).float()
    out = {}
    for fused in (True, False):
        ops.set_option("FUSE_SPLITK", None if fused else "0")
        n0 = _lib.query("tris_splitk_fused_launches")
        C = torch.full((M, N), float("nan"), device="cuda")
        with CFG.override(fuse_splitk=True):      # (opt-in since the round-6 measurement: ops.gemm arms the ticket array only then)
            ops.gemm(A, B, C, M, N, K, M if tA else K, K if tB else N, N, tA, tB, bias=bias, bias_mode=1, resid=R, ldr=N, act=2, alpha=0.5)
        torch.cuda.synchronize()
        took = _lib.query("tris_splitk_fused_launches") - n0
        assert took == (1 if fused else 0), (fused, took, slices)
        out[fused] = C
    ops.set_option("FUSE_SPLITK", None)
    assert torch.equal(out[True], out[False])
    close(out[True], ref, tol=3e-4)
    assert int(ops.splitk_tickets().abs().sum()) == 0


def test_linear_relu_and_gelu_epilogues(ops):
    x, w, b = leaf(70, 96), leaf(40, 96, scale=0.2), leaf(40)
    y = F.relu(x @ w.t() + b)
    y.sum().backward()
    gx, gw, gb = gpu_leaf(x), gpu_leaf(w), gpu_leaf(b)
    gy = ops.linear(gx, gw, gb, None, 1)
    gy.sum().backward()
    close(gy, y)
    close(gx.grad, x.grad)
    close(gw.grad, w.grad)
    with torch.no_grad():
        h = x @ w.t() + b
        close(ops.linear(gx, gw, gb, None, 2), h * torch.sigmoid(1.702 * h))


@pytest.mark.parametrize("tB", [False, True])
def test_matmul_and_bmm(ops, tB):
    A = leaf(3, 50, 36)
    B2 = leaf(20, 36) if tB else leaf(36, 20)
    C = A @ (B2.t() if tB else B2)
    C.backward(C.detach())
    gA, gB = gpu_leaf(A), gpu_leaf(B2)
    gC = ops.matmul(gA, gB, tB)
    gC.backward(gC.detach())
    close(gC, C)
    close(gA.grad, A.grad)
    close(gB.grad, B2.grad)
    # batched, and shared-A batched
    for shared in (False, True):
        A3 = leaf(12, 40) if shared else leaf(4, 12, 40)
        B3 = leaf(4, 9, 40) if tB else leaf(4, 40, 9)
        ref = torch.matmul(A3, B3.transpose(1, 2) if tB else B3) * 0.5
        ref.backward(ref.detach())
        gA3, gB3 = gpu_leaf(A3), gpu_leaf(B3)
        out = ops.bmm(gA3, gB3, tB, 0.5)
        out.backward(out.detach())
        close(out, ref)
        close(gA3.grad, A3.grad, name="dA")
        close(gB3.grad, B3.grad, name="dB")


@pytest.mark.parametrize("B,H,W,Cin,Cout,stride", [(2, 20, 20, 32, 64, 1), (2, 12, 10, 64, 64, 1), (1, 9, 7, 128, 16, 1),
                                                     (2, 32, 32, 3, 32, 2), (3, 16, 16, 16, 48, 1), (3, 33, 31, 3, 32, 2),
                                                     (1, 9, 7, 3, 16, 1), (4, 320, 320, 3, 32, 2), (2, 24, 24, 32, 32, 1),
                                                     (2, 16, 16, 64, 32, 1), (1, 40, 40, 32, 32, 2)])
def test_conv3x3(ops, B, H, W, Cin, Cout, stride):
    x, w = leaf(B, Cin, H, W), leaf(Cout, Cin, 3, 3, scale=0.1)
    y = F.conv2d(x, w, stride=stride, padding=1)
    y.backward(y.detach() * 0.1 + 1)
    gx = x.detach().permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(stride == 1)
    gw = w.detach().clone().contiguous(memory_format=torch.channels_last).cuda().requires_grad_(True)
    gy = ops.conv3x3(gx, gw, stride)
    gy.backward(gy.detach() * 0.1 + 1)
    close(gy.permute(0, 3, 1, 2), y, name="y")
    close(gw.grad, w.grad, name="dw")
    if stride == 1:
        close(gx.grad.permute(0, 3, 1, 2), x.grad, name="dx")


@pytest.mark.parametrize("cfg,B,H,W,Cin,Cout", [(1, 2, 32, 32, 32, 128), (1, 1, 16, 48, 128, 160), (2, 2, 32, 16, 48, 64),
                                                (3, 2, 16, 32, 64, 32), (3, 3, 16, 16, 32, 32), (4, 3, 10, 10, 64, 128),
                                                (4, 2, 12, 20, 128, 256), (4, 1, 40, 40, 128, 128), (5, 5, 10, 10, 64, 128),
                                                (5, 2, 20, 20, 32, 192), (5, 1, 40, 40, 128, 128), (6, 2, 8, 32, 32, 128),
                                                (6, 1, 24, 16, 64, 192)])
@pytest.mark.parametrize("arith", ["x3", "h2"])
def test_conv3x3_direct_kernels(cfg, B, H, W, Cin, Cout, arith, monkeypatch):
    """Every configuration of the direct 3x3 convolution (one split of the input window per 16-channel chunk, tris_amd/csrc/
    gemm_fast.h A_HALO) -- forward, fused BatchNorm statistics and data gradient -- against the fp32 CPU reference and against
    the implicit GEMM it replaces: 2-D patches (cfg 1-3, 6) and flattened pixel runs in padded coordinates (cfg 4, 5: tiles that
    cross row and image boundaries, a ragged last tile).  In both arithmetics that have direct kernels."""
    from tris_amd import ops as o
    prev = o.get_gemm_mode()
    o.set_gemm_mode(arith)
    try:
        x, w = leaf(B, Cin, H, W), leaf(Cout, Cin, 3, 3, scale=0.1)
        y = F.conv2d(x, w, padding=1)
        gy0 = torch.randn(y.shape, generator=torch.Generator().manual_seed(5))
        y.backward(gy0)
        outs = {}
        for mode in ("0", str(cfg)):
            o.set_option("CONV_DIRECT", mode)
            gx = x.detach().permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)
            gw = w.detach().clone().contiguous(memory_format=torch.channels_last).cuda().requires_grad_(True)
            gy = o.conv3x3(gx, gw, 1, stats=True)
            part = getattr(gy, "_bn_part", None)
            g, b = torch.ones(Cout).cuda(), torch.zeros(Cout).cuda()
            rm, rv = torch.zeros(Cout).cuda(), torch.ones(Cout).cuda()
            with torch.no_grad():
                o.batch_norm(gy, g, b, rm, rv, None, False, True)
            gy.backward(gy0.permute(0, 2, 3, 1).contiguous().cuda())
            outs[mode] = (gy.detach().cpu(), gx.grad.cpu(), rm.cpu(), rv.cpu(), part[1] if part is not None else 0)
            close(gy.permute(0, 3, 1, 2), y, name=f"y[{mode}]")
            close(gx.grad.permute(0, 3, 1, 2), x.grad, name=f"dx[{mode}]")
            close(gw.grad, w.grad, name=f"dw[{mode}]")
        a, d = outs["0"], outs[str(cfg)]
        close(d[0], a[0], 2e-6, name="direct vs implicit: y")
        close(d[1], a[1], 2e-6, name="direct vs implicit: dx")
        close(d[2], a[2], 1e-5, name="running_mean from the fused statistics")
        close(d[3], a[3], 1e-5, name="running_var from the fused statistics")
        if Cin % 32 == 0 and B * H * W >= 128:      # (the statistics epilogue's own preconditions)
            tiles = (B * (H // 16) * (W // 16) if cfg <= 3 else B * (H // 8) * (W // 16) if cfg == 6 else
                     -(-B * H * W // (128 if cfg == 4 else 256)))
            assert d[4] == tiles, (d[4], tiles)     # the direct kernel ran (one partial row per M tile), not a fallback
    finally:
        o.set_gemm_mode(prev)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 16, 32, 32, 32), (2, 32, 16, 32, 64), (3, 16, 16, 64, 64), (1, 16, 48, 128, 128),
                                            (2, 10, 10, 64, 64)])
@pytest.mark.parametrize("arith", ["x3", "h2"])
def test_batchnorm_relu_folded_into_the_direct_convolution(B, H, W, Cin, Cout, arith, monkeypatch):
    """conv3x3(relu(bn(x))) with the BatchNorm output never written (ops.batch_norm lazy=True -> the direct kernels normalise x
    while staging their windows, forward and weight gradient) == the same chain with the BatchNorm output materialised; and
    both against the fp32 CPU reference.  The last shape has no direct kernel: lazy must quietly fall back."""
    from tris_amd import ops as o
    from tris_amd._lib import query
    prev = o.get_gemm_mode()
    o.set_gemm_mode(arith)
    try:
        x, w = leaf(B, Cin, H, W), leaf(Cout, Cin, 3, 3, scale=0.1)
        g0 = torch.rand(Cin, generator=torch.Generator().manual_seed(1)) + 0.5
        b0 = torch.randn(Cin, generator=torch.Generator().manual_seed(2)) * 0.3
        gam, bet = g0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        y = F.conv2d(F.relu(F.batch_norm(x, None, None, gam, bet, True, 0.1, 1e-5)), w, padding=1)
        gy0 = torch.randn(y.shape, generator=torch.Generator().manual_seed(5))
        y.backward(gy0)
        ok = o.conv3x3_bnin_ok((B, H, W, Cin), Cout)
        assert ok == (H % 8 == 0 and W % 16 == 0)
        outs = {}
        for lazy in (False, True):
            gx = x.detach().permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)
            gw = w.detach().clone().contiguous(memory_format=torch.channels_last).cuda().requires_grad_(True)
            gg, gb = g0.clone().cuda().requires_grad_(True), b0.clone().cuda().requires_grad_(True)
            rm, rv = torch.zeros(Cin).cuda(), torch.ones(Cin).cuda()
            n0 = (query("tris_direct_launches", 0), query("tris_direct_launches", 1))
            a = o.batch_norm(gx, gg, gb, rm, rv, None, True, True, lazy=lazy and ok)
            assert hasattr(a, "_bn_lazy") == (lazy and ok)
            if lazy and ok:
                a.detach().fill_(float("nan"))     # the buffer is never read: poison it
            gy = o.conv3x3(a, gw, 1)
            gy.backward(gy0.permute(0, 2, 3, 1).contiguous().cuda())
            o.wgrad_join()
            torch.cuda.synchronize()
            if lazy and ok:
                assert query("tris_direct_launches", 0) - n0[0] >= 1 and query("tris_direct_launches", 1) - n0[1] == 1
            outs[lazy] = [t.detach().cpu() for t in (gy, gx.grad, gw.grad, gg.grad, gb.grad, rm, rv)]
            close(gy.permute(0, 3, 1, 2), y, name=f"y[{lazy}]")
            close(gx.grad.permute(0, 3, 1, 2), x.grad, 5e-4, name=f"dx[{lazy}]")
            close(gw.grad, w.grad, name=f"dw[{lazy}]")
            close(gg.grad, gam.grad, 5e-4, name=f"dgamma[{lazy}]")
            close(gb.grad, bet.grad, 5e-4, name=f"dbeta[{lazy}]")
        for u, v, name in zip(outs[True], outs[False], ("y", "dx", "dw", "dgamma", "dbeta", "running_mean", "running_var")):
            close(u, v, 5e-6, name="folded vs materialised: " + name)
    finally:
        o.set_gemm_mode(prev)


@pytest.mark.parametrize("cfg,B,H,W,Cin,Cout", [(1, 2, 8, 32, 32, 32), (1, 3, 12, 16, 32, 32), (2, 2, 16, 16, 32, 64),
                                                (3, 2, 6, 32, 64, 64), (3, 1, 4, 16, 128, 192), (3, 5, 10, 48, 64, 128),
                                                (2, 2, 8, 32, 64, 128), (4, 2, 8, 32, 64, 64), (4, 3, 12, 16, 128, 64),
                                                (5, 2, 8, 40, 32, 64), (5, 1, 16, 24, 96, 128)])
@pytest.mark.parametrize("arith", ["x3", "h2"])
def test_conv3x3_direct_weight_gradient(cfg, B, H, W, Cin, Cout, arith, monkeypatch):
    """The direct 3x3 weight-gradient kernel (one split of each dY / input window, nine taps read the same LDS image;
    tris_amd/csrc/conv_direct.hip wgrad3x3_direct_kernel) against the fp32 CPU reference and the implicit GEMM."""
    from tris_amd import ops as o
    prev = o.get_gemm_mode()
    o.set_gemm_mode(arith)
    try:
        x, w = leaf(B, Cin, H, W), leaf(Cout, Cin, 3, 3, scale=0.1)
        y = F.conv2d(x, w, padding=1)
        gy0 = torch.randn(y.shape, generator=torch.Generator().manual_seed(5))
        y.backward(gy0)
        got, ran = {}, []
        from tris_amd._lib import query
        for mode in ("0", str(cfg)):
            o.set_option("WGRAD_DIRECT", mode)
            gx = x.detach().permute(0, 2, 3, 1).contiguous().cuda()
            gw = w.detach().clone().contiguous(memory_format=torch.channels_last).cuda().requires_grad_(True)
            n0 = query("tris_direct_launches", 1)
            o.conv3x3(gx, gw, 1).backward(gy0.permute(0, 2, 3, 1).contiguous().cuda())
            torch.cuda.synchronize()
            ran.append(query("tris_direct_launches", 1) - n0)
            got[mode] = gw.grad.detach().cpu()
            close(got[mode], w.grad, name=f"dw[{mode}]")
        close(got[str(cfg)], got["0"], 2e-6, name="direct vs implicit")
        assert ran == [0, 1], ran   # the direct kernel ran exactly when asked to
    finally:
        o.set_gemm_mode(prev)


@pytest.mark.parametrize("res,relu", [(False, True), (True, True), (False, False)])
@pytest.mark.parametrize("shape", [(2, 10, 10, 64), (3, 40, 40, 32), (2, 5, 5, 2048)])
def test_batchnorm_train(ops, shape, res, relu):
    C = shape[-1]
    x, g, b = leaf(*shape), leaf(C), leaf(C)
    x.data = x.data * 2 + 3  # a mean of 1.5 std: the one-pass fp64 sums (no shift) stay within (M + 4) 2^-53 (var + mean^2), tests/oracle_bn.py
    r = leaf(*shape, seed=5) if res else None
    rm, rv = torch.zeros(C), torch.ones(C)
    y = F.batch_norm(x.permute(0, 3, 1, 2), rm, rv, g, b, True, 0.1, 1e-5).permute(0, 2, 3, 1)
    if res:
        y = y + r
    if relu:
        y = F.relu(y)
    (y * y).sum().backward()
    gx, gg, gb = gpu_leaf(x), gpu_leaf(g), gpu_leaf(b)
    gr = gpu_leaf(r) if res else None
    grm, grv = torch.zeros(C).cuda(), torch.ones(C).cuda()
    gy = ops.batch_norm(gx, gg, gb, grm, grv, gr, relu, True)
    (gy * gy).sum().backward()
    close(gy, y, name="y")
    close(grm, rm, name="running_mean")
    close(grv, rv, name="running_var")
    close(gx.grad, x.grad, 5e-4, name="dx")
    close(gg.grad, g.grad, 5e-4, name="dgamma")
    close(gb.grad, b.grad, 5e-4, name="dbeta")
    if res:
        close(gr.grad, r.grad, name="dresid")
    # eval mode
    with torch.no_grad():
        ye = F.batch_norm(x.permute(0, 3, 1, 2), rm, rv, g, b, False, 0.1, 1e-5).permute(0, 2, 3, 1)
        close(ops.batch_norm(gx, gg, gb, grm, grv, None, False, False), ye, name="eval")


@pytest.mark.parametrize("M,C", [(76800, 512), (300001, 128)])
def test_batchnorm_streaming_form_equals_the_default_form(ops, M, C):
    """Launches whose streams exceed the 256 MB memory-side cache take the nontemporal one-piece-per-block form of bn_apply /
    bn_bwd_apply (csrc/norm.hip, STREAM_FORM): same arithmetic per element, so bit-identical to the grid-stride form -- with and
    without the residual / ReLU, the three mask sources of the backward, the optional masked-gradient output, a ragged tail
    (300001 rows: the last block is partial) and the amax by-product."""
    import tris_amd.ops as o
    g = torch.Generator(device="cuda").manual_seed(11)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    x, r, dy = rnd(M, C) * 2 + 1, rnd(M, C), rnd(M, C)
    mean, invstd, gamma, beta = rnd(C), rnd(C).abs() + 0.5, rnd(C), rnd(C)
    sdz, sdzx = rnd(C) * 100, rnd(C) * 100
    assert 3 * x.numel() * 4 > 256 << 20
    P, st = o.P, o._stream()

    def fwd(resid, relu):
        y = torch.empty_like(x)
        am = torch.zeros(2048, dtype=torch.int32, device="cuda")
        o.call("tris_amax_next", P(am))
        o.call("tris_bn_apply_f32", P(x), P(mean), P(invstd), P(gamma), P(beta), P(r) if resid else None, P(y), M, C, int(relu), st)
        return y, int(am.max())

    def bwd(mask, want_dz):
        y = torch.relu((x - mean) * (invstd * gamma) + beta + r) if mask == "y" else None
        dx, dz = torch.empty_like(x), (torch.empty_like(x) if want_dz else None)
        o.call("tris_bn_bwd_apply_f32", P(dy), P(y), P(x), P(mean), P(invstd), P(gamma), P(sdz), P(sdzx), 1.0 / M, P(dx), P(dz), M, C,
               P(beta) if mask == "beta" else None, st)
        return dx, dz

    cases = [lambda: fwd(True, True), lambda: fwd(False, True), lambda: fwd(True, False),
             lambda: bwd("y", True), lambda: bwd("beta", False), lambda: bwd(None, False)]
    for k, run in enumerate(cases):
        with o.option("STREAM_FORM", 0):
            ref = run()
        got = run()
        torch.cuda.synchronize()
        for a, b in zip(got, ref):
            if torch.is_tensor(a):
                assert torch.equal(a, b), k
            else:
                assert a == b, (k, a, b)


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("shape,N", [((3, 20, 20, 64), 256), ((2, 9, 9, 128), 32), ((2, 40, 40, 32), 64), ((1, 10, 10, 256), 64)])
def test_batchnorm_backward_reduced_in_the_consuming_1x1_convolution(ops, shape, N, res, monkeypatch):
    """relu(bn(x) [+ r]) -> 1x1 convolution: with bwd_link=True the BatchNorm's backward sums come out of the convolution's
    data-gradient epilogue (tris_gemm_bnbwd_f32) instead of a reduction pass of their own; every gradient must match both the
    torch reference and the unfused path, and the fused entry point must really have run where the shape allows it"""
    from tris_amd import _lib
    C = shape[-1]
    x, g, b, w = leaf(*shape), leaf(C), leaf(C), leaf(N, C, scale=0.2)
    x.data = x.data * 2 + 1
    r = leaf(*shape, seed=5) if res else None
    y = F.batch_norm(x.permute(0, 3, 1, 2), torch.zeros(C), torch.ones(C), g, b, True, 0.1, 1e-5).permute(0, 2, 3, 1)
    y = F.relu(y + r if res else y)
    z = y @ w.t()
    (z * z).sum().backward()

    def run(link):
        monkeypatch.setattr(CFG, "bn_bwd_fuse", bool(link))
        gx, gg, gb, gw = gpu_leaf(x), gpu_leaf(g), gpu_leaf(b), gpu_leaf(w)
        gr = gpu_leaf(r) if res else None
        gy = ops.batch_norm(gx, gg, gb, torch.zeros(C).cuda(), torch.ones(C).cuda(), gr, True, True, bwd_link=True)
        assert hasattr(gy, "_bn_link") == link
        gz = ops.linear(gy, gw)
        (gz * gz).sum().backward()
        return gz, gx.grad, gg.grad, gb.grad, gw.grad, (gr.grad if res else None)
    calls = []
    real = _lib.call

    def spy(name, *a):
        if name == "tris_gemm_bnbwd_f32":
            calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(ops, "call", spy)
    fills = []
    real_fill = ops._BnBwdLink.fill
    monkeypatch.setattr(ops._BnBwdLink, "fill", lambda self, *a: (fills.append(1), real_fill(self, *a))[1])
    fused = run(True)
    M = x.numel() // C
    assert len(calls) == 1
    assert len(fills) == (1 if M >= 128 else 0)     # (fewer rows than one tile: the entry point declines, the two passes run)
    plain = run(False)
    assert len(calls) == 1 and len(fills) <= 1
    for name, a, b_, ref in zip(("z", "dx", "dgamma", "dbeta", "dw", "dresid"), fused, plain, (z, x.grad, g.grad, b.grad, w.grad,
                                                                                               r.grad if res else None)):
        if ref is None:
            continue
        close(a, ref, 5e-4, name=name + " (fused) vs torch")
        close(a, b_, 2e-5, name=name + " fused vs separate passes")


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("shape,Cout", [((2, 16, 16, 64), 64), ((3, 20, 20, 32), 64), ((1, 12, 12, 128), 32)])
def test_batchnorm_backward_reduced_in_the_consuming_3x3_convolution(ops, shape, Cout, lazy, monkeypatch):
    """relu(bn(x)) -> 3x3 convolution (stride 1), also with the BatchNorm folded into the convolution (lazy): the backward sums
    come out of the data-gradient epilogue (tris_conv3x3_dgrad_bnbwd_f32); gradients vs torch and vs the separate passes"""
    C = shape[-1]
    x, g, b = leaf(*shape), leaf(C), leaf(C)
    x.data = x.data * 2 + 1
    w = leaf(Cout, C, 3, 3, scale=0.1)
    y = F.relu(F.batch_norm(x.permute(0, 3, 1, 2), torch.zeros(C), torch.ones(C), g, b, True, 0.1, 1e-5))
    z = F.conv2d(y, w, padding=1).permute(0, 2, 3, 1)
    (z * z).sum().backward()
    fills = []
    real_fill = ops._BnBwdLink.fill
    monkeypatch.setattr(ops._BnBwdLink, "fill", lambda self, *a: (fills.append(1), real_fill(self, *a))[1])

    def run(link):
        monkeypatch.setattr(CFG, "bn_bwd_fuse", bool(link))
        gx, gg, gb = gpu_leaf(x), gpu_leaf(g), gpu_leaf(b)
        gw = w.detach().clone().cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        ok = lazy and ops.conv3x3_bnin_ok(gx.shape, Cout)
        gy = ops.batch_norm(gx, gg, gb, torch.zeros(C).cuda(), torch.ones(C).cuda(), None, True, True, lazy=ok, bwd_link=True)
        gz = ops.conv3x3(gy, gw)
        (gz * gz).sum().backward()
        return gz, gx.grad, gg.grad, gb.grad, gw.grad
    fused = run(True)
    M = x.numel() // C
    assert len(fills) == (1 if M >= 128 else 0)
    plain = run(False)
    assert len(fills) <= 1
    for name, a, b_, ref in zip(("z", "dx", "dgamma", "dbeta", "dw"), fused, plain, (z, x.grad, g.grad, b.grad, w.grad)):
        close(a, ref, 5e-4, name=name + " (fused) vs torch")
        close(a, b_, 2e-5, name=name + " fused vs separate passes")


@pytest.mark.parametrize("shape", [(2, 10, 10, 64), (3, 40, 36, 32), (2, 6, 8, 256), (1, 160, 160, 64)])
def test_batchnorm_relu_avgpool_as_one_op(ops, shape, monkeypatch):
    """avgpool2(relu(bn(x))) with the full-size activation never written (tris_bn_apply_pool_f32) and a backward that reads the
    pooled gradient in both passes: vs torch, and vs the two separate ops (config.cfg.bn_pool = False)"""
    C = shape[-1]
    x, g, b = leaf(*shape), leaf(C), leaf(C)
    x.data = x.data * 2 + 1
    y = F.avg_pool2d(F.relu(F.batch_norm(x.permute(0, 3, 1, 2), torch.zeros(C), torch.ones(C), g, b, True, 0.1, 1e-5)), 2)
    y = y.permute(0, 2, 3, 1)
    (y * y).sum().backward()

    def run(fused):
        monkeypatch.setattr(CFG, "bn_pool", bool(fused))
        gx, gg, gb = gpu_leaf(x), gpu_leaf(g), gpu_leaf(b)
        rm, rv = torch.zeros(C).cuda(), torch.ones(C).cuda()
        gy = ops.batch_norm(gx, gg, gb, rm, rv, None, True, True, pool=True)
        (gy * gy).sum().backward()
        return gy, gx.grad, gg.grad, gb.grad, rm, rv
    fused, plain = run(True), run(False)
    for name, a, b_, ref in zip(("y", "dx", "dgamma", "dbeta"), fused, plain, (y, x.grad, g.grad, b.grad)):
        close(a, ref, 5e-4, name=name + " vs torch")
        close(a, b_, 2e-6, name=name + " fused vs two ops")
    assert torch.equal(fused[4], plain[4]) and torch.equal(fused[5], plain[5])
    with torch.no_grad():   # eval mode: running statistics, two ops
        ye = F.avg_pool2d(F.relu(F.batch_norm(x.permute(0, 3, 1, 2), fused[4].cpu(), fused[5].cpu(), g, b, False, 0.1, 1e-5)), 2)
        close(ops.batch_norm(x.cuda(), g.detach().cuda(), b.detach().cuda(), fused[4], fused[5], None, True, False, pool=True),
              ye.permute(0, 2, 3, 1), name="eval")


def test_batchnorm_link_tolerates_a_second_consumer(ops):
    """bwd_link=True promises one autograd consumer; when the promise is broken (a second consumer's gradient is summed into the
    masked gradient by autograd) the BatchNorm backward notices that what arrives is not the product's tensor and runs its own
    two passes on the sum -- correct gradients, no error"""
    C = 64
    x, g, b, w = leaf(2, 16, 16, C), leaf(C), leaf(C), leaf(128, C, scale=0.2)
    y = F.relu(F.batch_norm(x.permute(0, 3, 1, 2), None, None, g, b, True, 0.1, 1e-5).permute(0, 2, 3, 1))
    ((y @ w.t()) ** 2).sum().add((y * 3.0).sum()).backward()
    gx, gg, gb, gw = gpu_leaf(x), gpu_leaf(g), gpu_leaf(b), gpu_leaf(w)
    gy = ops.batch_norm(gx, gg, gb, torch.zeros(C).cuda(), torch.ones(C).cuda(), None, True, True, bwd_link=True)
    out = (ops.linear(gy, gw) ** 2).sum() + (gy * 3.0).sum()
    out.backward()
    close(gx.grad, x.grad, 5e-4)
    close(gg.grad, g.grad, 5e-4)
    close(gb.grad, b.grad, 5e-4)
    close(gw.grad, w.grad)


def test_avgpool_layernorm_gelu(ops):
    x = leaf(2, 8, 6, 16)
    y = F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    y.backward(y.detach())
    gx = gpu_leaf(x)
    gy = ops.avgpool2(gx)
    gy.backward(gy.detach())
    close(gy, y)
    close(gx.grad, x.grad)
    for W in (512, 768, 100):
        x, g, b = leaf(37, W), leaf(W), leaf(W)
        y = F.layer_norm(x, (W,), g, b, 1e-5)
        (y * y).sum().backward()
        gx, gg, gb = gpu_leaf(x), gpu_leaf(g), gpu_leaf(b)
        gy = ops.layer_norm(gx, gg, gb)
        (gy * gy).sum().backward()
        close(gy, y)
        close(gx.grad, x.grad)
        close(gg.grad, g.grad)
        close(gb.grad, b.grad)
    x = leaf(33, 17)
    y = x * torch.sigmoid(1.702 * x)
    y.sum().backward()
    gx = gpu_leaf(x)
    gy = ops.quick_gelu(gx)
    gy.sum().backward()
    close(gy, y)
    close(gx.grad, x.grad)


def test_residual_gradient_box_through_layernorm(ops):
    """y = Linear(LN(x)) + x : the Linear's backward leaves the residual gradient in a GradBox and the LayerNorm
    backward kernel adds it while writing dX -- same gradients as torch, and the box is emptied."""
    for W in (512, 100):
        x, g, b, w, wb = leaf(37, W), leaf(W), leaf(W), leaf(W, W, scale=W ** -0.5), leaf(W)
        y = F.linear(F.layer_norm(x, (W,), g, b, 1e-5), w, wb) + x
        (y * y).sum().backward()
        gx, gg, gb, gw, gwb = (gpu_leaf(t) for t in (x, g, b, w, wb))
        box = ops.GradBox()
        gy = ops.linear(ops.layer_norm(gx, gg, gb, 1e-5, box), gw, gwb, resid=gx, grad_box_res=box)
        (gy * gy).sum().backward()
        assert box.consumed and box.value is None
        close(gy, y, 5e-4)
        for a, r, n in ((gx, x, "dx"), (gg, g, "dgamma"), (gb, b, "dbeta"), (gw, w, "dw"), (gwb, wb, "db")):
            close(a.grad, r.grad, 5e-4, n)


def test_transformer_block_gradients_do_not_depend_on_the_gradient_box(ops, monkeypatch):
    from tris_amd.CLIP.clip.model import ResidualAttentionBlock
    torch.manual_seed(3)
    blk = ResidualAttentionBlock(128, 2, attn_mask=True).cuda()   # head width 64, as every CLIP tower
    x0 = torch.randn(3, 20, 128, device="cuda")
    grads = []
    for flag in ("1", "0"):
        monkeypatch.setattr(CFG, "grad_box", flag == "1")
        blk.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = blk(blk(x))
        (y * y).mean().backward()
        grads.append([x.grad.clone()] + [p.grad.clone() for p in blk.parameters()])
    for a, b in zip(*grads):
        close(a, b, 1e-5)


@pytest.mark.parametrize("impl", ["mfma", "valu"])
@pytest.mark.parametrize("N,L,heads,causal", [(3, 20, 8, True), (2, 50, 12, False), (1, 64, 2, True), (2, 7, 1, False),
                                             (2, 65, 2, True), (1, 401, 3, False), (2, 130, 2, True), (1, 1, 1, True),
                                             (2, 16, 1, False), (1, 200, 1, False)])
def test_mha(ops, N, L, heads, causal, impl, monkeypatch):
    if impl == "valu" and L > 64:
        pytest.skip("the LDS-resident kernel holds the whole sequence: L <= 64")
    monkeypatch.setattr(CFG, "mha", impl)
    W = heads * 64
    qkv = leaf(N, L, 3 * W)
    q, k, v = qkv.split(W, dim=-1)
    q = q.view(N, L, heads, 64).transpose(1, 2)
    k = k.view(N, L, heads, 64).transpose(1, 2)
    v = v.view(N, L, heads, 64).transpose(1, 2)
    s = q @ k.transpose(-1, -2) / 8.0
    if causal:
        s = s + torch.full((L, L), float("-inf")).triu_(1)
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(N, L, W)
    (o * o).sum().backward()
    g = gpu_leaf(qkv)
    go = ops.mha(g, heads, causal)
    (go * go).sum().backward()
    close(go, o)
    close(g.grad, qkv.grad)
    if impl == "mfma":   # inside h2 the flash-style kernels run on the 16-bit MFMA from L = 32 on (csrc/attn_h2.hip)
        from tris_amd import ops as _o
        assert _o.MHA_STATS["last"] == ("h2" if (ops.get_gemm_mode() == "h2" and L >= 32) else "f32")


def test_embed_eot(ops):
    ids = torch.tensor([[49406, 5, 9, 49407, 0, 0], [49406, 9, 9, 9, 49407, 0], [49406, 7, 49407, 0, 0, 0]])
    tok, pos = leaf(49408, 64, scale=0.1), leaf(10, 64)
    x = tok[ids] + pos[:6]
    h = x[torch.arange(3), ids.argmax(-1)]
    ((x * x).sum() + (h * 3).sum()).backward()
    gt, gp = gpu_leaf(tok), gpu_leaf(pos)
    gx = ops.embed(ids.cuda(), gt, gp)
    gh = ops.eot_gather(ids.cuda(), gx)
    ((gx * gx).sum() + (gh * 3).sum()).backward()
    close(gx, x)
    close(gh, h)
    close(gt.grad, tok.grad)
    close(gp.grad, pos.grad)


@pytest.mark.parametrize("R,W,vocab", [(20480, 512, 3000), (16385, 768, 40), (50000, 64, 49408), (7, 512, 5)])
def test_embedding_row_list_scatter_beyond_one_bitmap(R, W, vocab):
    """tris_embed_rows_bwd_f32 on row lists longer than its LDS bitmap (16384 positions: 16 ranks x 64 sentences x 20 tokens of the
    sparse data-parallel exchange is 20480): the deterministic scatter walks the list in chunks -- same sums as index_add, and
    bit-identical from run to run"""
    from tris_amd import ops as o
    g = torch.Generator().manual_seed(R)
    ids = torch.randint(0, vocab, (R,), generator=g)
    ids[::7] = 1                                    # heavy repeats (SOT / EOT / padding in the real lists)
    rows = torch.randn(R, W, generator=g)
    want = torch.zeros(vocab, W).index_add_(0, ids, rows) * 0.25
    outs = []
    gi, gr = ids.cuda(), rows.cuda()
    for _ in range(2):
        d = torch.zeros(vocab, W, device="cuda")
        o.call("tris_embed_rows_bwd_f32", o.P(gi), o.P(gr), o.P(d), R, W, 0.25, o._stream())
        outs.append(d.cpu())
    assert torch.equal(outs[0], outs[1])
    close(outs[0], want, 2e-5)


def test_l2norm_softmax_instnorm_axpy(ops):
    x = leaf(50, 1024)
    y = x / x.norm(dim=-1, keepdim=True)
    (y * torch.arange(1024.0)).sum().backward()
    gx = gpu_leaf(x)
    gy = ops.l2norm(gx)
    (gy * torch.arange(1024.0).cuda()).sum().backward()
    close(gy, y)
    close(gx.grad, x.grad)
    for n in (48, 100, 130):
        x = leaf(20, n)
        y = torch.softmax(x / 32.0, -1)
        (y * y).sum().backward()
        gx = gpu_leaf(x)
        gy = ops.softmax(gx, 1 / 32.0)
        (gy * gy).sum().backward()
        close(gy, y)
        close(gx.grad, x.grad)
    for relu in (True, False):
        x, g, b = leaf(3, 100, 128), leaf(128), leaf(128)
        y = F.instance_norm(x.permute(0, 2, 1).reshape(3, 128, 10, 10), None, None, g, b, True, 0.1, 1e-5)
        y = (F.relu(y) if relu else y).reshape(3, 128, 100).permute(0, 2, 1)
        (y * y).sum().backward()
        gx, gg, gb = gpu_leaf(x), gpu_leaf(g), gpu_leaf(b)
        gy = ops.instance_norm(gx, gg, gb, relu)
        (gy * gy).sum().backward()
        close(gy, y)
        close(gx.grad, x.grad, 5e-4)
        close(gg.grad, g.grad, 5e-4)
        close(gb.grad, b.grad, 5e-4)
    a, b = leaf(7, 9), leaf(7, 9, seed=3)
    y = 0.1 * a + b
    y.sum().backward()
    ga, gb = gpu_leaf(a), gpu_leaf(b)
    gy = ops.axpy(ga, gb, 0.1)
    gy.sum().backward()
    close(gy, y)
    close(ga.grad, a.grad)
    close(gb.grad, b.grad)


@pytest.mark.parametrize("hi,wi,ho,wo,align", [(10, 10, 320, 320, False), (320, 320, 224, 224, True),
                                                (32, 32, 45, 61, True), (7, 9, 20, 13, False), (40, 40, 11, 17, True)])
def test_resize(ops, hi, wi, ho, wo, align):
    x = leaf(2, 3, hi, wi)
    y = F.interpolate(x, (ho, wo), mode="bilinear", align_corners=align)
    (y * y).sum().backward()
    gx = gpu_leaf(x)
    gy = ops.resize_bilinear(gx, (ho, wo), align)
    (gy * gy).sum().backward()
    close(gy, y)
    close(gx.grad, x.grad)


def _ref_heads(score, h, w, S, fp=3.0, fc=0.01):
    B, P, N = score.shape
    st = score.transpose(1, 2).reshape(B, N, h, w)
    st = torch.cat([torch.ones_like(st[:, :1]), st], 1)
    masks = torch.softmax(st, 1).view(B, N + 1, -1)
    feats = st.view(B, N + 1, -1)
    mm = masks.mean(-1)
    cls = (feats.mean(-1) + feats.max(-1).values + torch.pow(1 - mm, fp) * torch.log(fc + mm))[:, 1:]
    diag = torch.stack([score[i, :, i].view(1, h, w) for i in range(B)], 0)
    seg = F.interpolate(diag, size=(S, S), mode="bilinear", align_corners=False)
    return cls, torch.diagonal(mm[:, 1:]), F.relu(seg), torch.sigmoid(seg)


@pytest.mark.parametrize("B,h,w,S", [(4, 10, 10, 320), (3, 5, 5, 64), (48, 10, 10, 320), (48, 20, 20, 320)])
def test_score_heads(ops, B, h, w, S):
    score = leaf(B, h * w, B, scale=3.0)
    cls, fg, r, s = _ref_heads(score, h, w, S)
    wr, ws = torch.randn(r.shape, generator=torch.Generator().manual_seed(1)), torch.randn(s.shape, generator=torch.Generator().manual_seed(2))
    ((cls * cls).sum() + (r * wr).sum() + (s * ws).sum()).backward()
    g = gpu_leaf(score)
    gcls, gfg, gr, gs = ops.score_heads(g, h, w, S, True)
    ((gcls * gcls).sum() + (gr * wr.cuda()).sum() + (gs * ws.cuda()).sum()).backward()
    close(gcls, cls, name="cls")
    close(gfg, fg, name="cls_fg")
    close(gr, r, name="relu")
    close(gs, s, name="sig")
    close(g.grad, score.grad, 5e-4, name="dscore")
    with torch.no_grad():
        close(ops.score_heads(g, h, w, S, False), r, name="eval")


def test_fg_patches_and_vit_assemble(ops):
    cam, img = leaf(2, 1, 64, 64), leaf(2, 3, 64, 64)
    fg = cam * img
    ref = fg.reshape(2, 3, 2, 32, 2, 32).permute(0, 2, 4, 1, 3, 5).reshape(2, 4, 3 * 32 * 32)
    (ref * ref).sum().backward()
    gc = gpu_leaf(cam)
    out = ops.fg_patches(gc, img.detach().cuda(), 32)
    (out * out).sum().backward()
    close(out, ref)
    close(gc.grad, cam.grad)
    emb, cls, pos = leaf(2, 4, 96), leaf(96), leaf(5, 96)
    x = torch.cat([cls.expand(2, 1, 96), emb], 1) + pos
    (x * x).sum().backward()
    ge = gpu_leaf(emb)
    gx = ops.vit_assemble(ge, cls.detach().cuda(), pos.detach().cuda())
    (gx * gx).sum().backward()
    close(gx, x)
    close(ge.grad, emb.grad)


@pytest.mark.parametrize("K", [3, 0])
def test_stage1_loss(ops, K):
    B, E = 6, 512
    cls, fi, ft = leaf(B, B, scale=2.0), leaf(B, E), leaf(B, E, seed=1)
    ft.data[:3] += 2.0 * fi.data[:3]  # some clearly positive cosines (un-clamped branch)
    fneg = leaf(B, K, E, seed=2) if K else None
    a = fi / fi.norm(dim=-1, keepdim=True)
    t = ft / ft.norm(dim=-1, keepdim=True)
    l1 = -(torch.log((a * t).sum(-1).clamp(0.0001, 0.9999))).mean()
    l5 = torch.zeros(())
    if K:
        n = fneg / fneg.norm(dim=-1, keepdim=True)
        l5 = (-(torch.log(1 - (a[:, None] * n).sum(-1)))).mean(1).mean()
    l4 = F.multilabel_soft_margin_loss(cls, torch.eye(B))
    loss = l1 + 5 * l4 + 2 * l5
    loss.backward()
    gc, gi = gpu_leaf(cls), gpu_leaf(fi)
    out = ops.stage1_loss(gc, gi, ft.detach().cuda(), fneg.detach().cuda() if K else None, 1.0, 5.0, 2.0)
    out[0].backward()
    close(out, torch.stack([loss, l1, l4, l5]), name="losses")
    close(gc.grad, cls.grad, name="dcls")
    close(gi.grad, fi.grad, name="dfi")
    # a general upstream gradient of (total, l1, l4, l5): the kernels fold the loss weights into it themselves
    up = torch.tensor([0.7, -1.3, 0.25, 2.0])
    cls.grad = fi.grad = None
    a2, c2 = fi.detach().clone().requires_grad_(True), cls.detach().clone().requires_grad_(True)
    an = a2 / a2.norm(dim=-1, keepdim=True)
    r1 = -(torch.log((an * t.detach()).sum(-1).clamp(0.0001, 0.9999))).mean()
    r5 = (-(torch.log(1 - (an[:, None] * n.detach()).sum(-1)))).mean(1).mean() if K else torch.zeros(())
    r4 = F.multilabel_soft_margin_loss(c2, torch.eye(B))
    (torch.stack([r1 + 5 * r4 + 2 * r5, r1, r4, r5]) * up).sum().backward()
    gc2, gi2 = gpu_leaf(cls), gpu_leaf(fi)
    out2 = ops.stage1_loss(gc2, gi2, ft.detach().cuda(), fneg.detach().cuda() if K else None, 1.0, 5.0, 2.0)
    (out2 * up.cuda()).sum().backward()
    close(gc2.grad, c2.grad, name="dcls (general upstream gradient)")
    close(gi2.grad, a2.grad, name="dfi (general upstream gradient)")


def test_axpy_broadcast_scale_exp_concat_token0(ops):
    """the small ops that replaced torch element-wise launches on the training path (model_stage1.py:74, 77-78; train_stage1.py:342;
    CLIP/clip/model.py:443), forward and backward against torch"""
    B, N, C = 5, 7, 64
    a, b = leaf(B, N, C), leaf(N, C, seed=3)
    ref = 0.1 * a + b.unsqueeze(0)
    w = leaf(B, N, C, seed=9).detach()
    (ref * w).sum().backward()
    ga, gb = gpu_leaf(a), gpu_leaf(b)
    out = ops.axpy_bcast(ga, gb, 0.1)
    (out * w.cuda()).sum().backward()
    close(out, ref, name="axpy_bcast")
    close(ga.grad, a.grad, name="da")
    close(gb.grad, b.grad, name="db (summed over the broadcast dimension)")
    # score * exp(logit_scale)
    x, ls = leaf(3, 50, 11), torch.tensor(2.659, requires_grad=True)
    e = ls.exp()
    y = x * e
    wy = leaf(3, 50, 11, seed=4).detach()
    (y * wy).sum().backward()
    gx, gls = gpu_leaf(x), gpu_leaf(ls)
    gy, ge = ops.scale_exp(gx, gls)
    (gy * wy.cuda()).sum().backward()
    close(gy, y, name="scale_exp")
    close(ge, e, name="exp(logit_scale)")
    close(gx.grad, x.grad, name="dx")
    close(gls.grad, ls.grad, 1e-5 * float(ls.grad.abs()) + 1e-6, name="dlogit_scale")
    # gradient through the returned scale as well
    gls2 = gpu_leaf(ls)
    gy2, ge2 = ops.scale_exp(gx.detach(), gls2)
    (gy2.sum() + 3.0 * ge2).backward()
    ls2 = ls.detach().clone().requires_grad_(True)
    ((x.detach() * ls2.exp()).sum() + 3.0 * ls2.exp()).backward()
    close(gls2.grad, ls2.grad, 1e-5 * float(ls2.grad.abs()) + 1e-6, name="dlogit_scale (both outputs)")
    # int64 concat
    i1, i2 = torch.randint(0, 49408, (4, 20)), torch.randint(0, 49408, (12, 20))
    assert torch.equal(ops.concat_i64(i1.cuda(), i2.cuda()).cpu(), torch.cat([i1, i2], 0))
    # class token
    t = leaf(4, 50, 96)
    wt = leaf(4, 96, seed=2).detach()
    (t[:, 0, :] * wt).sum().backward()
    gt = gpu_leaf(t)
    o0 = ops.token0(gt)
    (o0 * wt.cuda()).sum().backward()
    close(o0, t[:, 0, :], name="token0")
    close(gt.grad, t.grad, name="dtoken0")


def test_adamw_matches_torch(ops):
    from tris_amd.optim import FusedAdamW
    torch.manual_seed(0)
    ps = [torch.randn(33, 7), torch.randn(64, 16, 3, 3).contiguous(memory_format=torch.channels_last), torch.randn(5)]
    ref = [p.clone().requires_grad_(True) for p in ps]
    ours = [torch.nn.Parameter(p.clone().cuda()) for p in ps]
    o_ref = torch.optim.AdamW([{"params": ref[:2], "lr": 5e-6}, {"params": ref[2:]}], lr=5e-5, weight_decay=0.01)
    o_our = FusedAdamW([{"params": ours[:2], "lr": 5e-6}, {"params": ours[2:]}], lr=5e-5, weight_decay=0.01)
    for step in range(3):
        for r, o in zip(ref, ours):
            g = torch.randn(r.shape, generator=torch.Generator().manual_seed(step * 10 + r.dim()))
            r.grad = g.clone()
            o.grad.copy_(g.cuda())
        o_ref.step()
        o_our.step()
    for r, o in zip(ref, ours):
        close(o, r, 1e-6)


def test_eval_post(ops):
    from oracle import tris_oracle as O
    g = torch.Generator().manual_seed(3)
    m = F.relu(torch.randn(1, 1, 320, 320, generator=g))
    m[0, 0, :40] = 0
    tgt = torch.zeros(427, 640, dtype=torch.bool)
    tgt[100:300, 50:400] = True
    I, U, mask, cam = O.eval_postprocess(m, tgt)
    iu, gcam = ops.eval_post(m.cuda(), tgt.to(torch.uint8).cuda())
    iu = iu.tolist()
    close(gcam, cam, 1e-5)
    assert abs(iu[0] - I) <= 2 and abs(iu[1] - U) <= 2  # exact up to pixels sitting on the 1e-9 threshold
    assert gcam.flatten()[iu[2]].item() == pytest.approx(float(cam.max()), abs=1e-6)


@pytest.mark.parametrize("B,P,N,C", [(3, 100, 5, 1024), (48, 100, 48, 1024), (1, 100, 1, 1024), (2, 97, 64, 512), (5, 8, 3, 512),
                                     (7, 104, 33, 1024), (40, 100, 33, 1024), (64, 100, 48, 512), (33, 57, 17, 1024),
                                     (60, 103, 64, 1024)])
def test_xattn_single_launch_kernels_match_the_two_launch_pair(ops, monkeypatch, B, P, N, C):
    """The two persistent single-launch forms -- csrc/xattn_px.hip (cut by pixel rows, S <= 8 workgroups of 512 threads per image,
    one in-kernel hand-off of the sentence -> pixel logits) and csrc/xattn_fused.hip (eight channel slices per image, reduce-scatter
    + all-gather of the partial logits) -- against an fp64 reference and against the two-launch pair, including the saved
    probabilities the backward pass reads; five calls in a row exercise the device-side epoch; no wait may have timed out.  The
    shapes cover S = 4 .. 8, one and two pixel tiles per workgroup, uneven pixel / channel-unit ranges, N = 1 .. 64, C = 512 | 1024."""
    g = torch.Generator().manual_seed(B * 1000 + P + N)
    Qv, Kv, Vv = (torch.randn(B, P, C, generator=g).cuda() * 1.5 for _ in range(3))
    Qt, Kt, Vt = (torch.randn(N, C, generator=g).cuda() * 1.5 for _ in range(3))
    sc = 1.0 / math.sqrt(C)
    Av = torch.softmax(Qv.cpu().double() @ Kt.cpu().double().t() * sc, dim=2)
    At = torch.softmax(Qt.cpu().double() @ Kv.cpu().double().transpose(1, 2) * sc, dim=2)
    rv, rl = Av @ Vt.cpu().double(), At @ Vv.cpu().double()
    outs = {}
    for form in ("pair", "slices", "px"):
        monkeypatch.setattr(CFG, "xattn_fused", form != "pair")
        monkeypatch.setattr(CFG, "xattn_px", form == "px")
        assert ops.query("tris_xattn_fused_ws_bytes", B, N, C) > 0 and ops.query("tris_xattn_px_ws_bytes", B, N, C) > 0
        ops.profile_begin()
        for _ in range(5):
            q = [t.clone().requires_grad_(True) for t in (Qv, Kv, Vv, Qt, Kt, Vt)]
            nv, nl = ops.xattn(*q)
        kinds = {r[0] for r in ops.profile_end() if r[0].startswith("xattn")}
        if form == "px" and ops.get_gemm_mode() != "f32" and B * max((P + 31) // 32, C // 256) <= 256:   # inside the pixel-row form's domain: it must have run
            assert kinds == {"xattn_fwd_px"}, kinds
            # ... in the arithmetic of the step: two fp16 pieces inside h2, three bf16 pieces otherwise
            assert int(ops.query("tris_xattn_px_last_form")) == (2 if ops.get_gemm_mode() == "h2" else 1)
        (nv.sum() + nl.sum()).backward()
        outs[form] = (nv.detach(), nl.detach(), [t.grad for t in q])
        close(nv.detach().cpu(), rv.float(), 2e-5, name=f"new_vis {form}")
        close(nl.detach().cpu(), rl.float(), 2e-5, name=f"new_lan {form}")
    assert not ops.xattn_timed_out()
    for form in ("slices", "px"):
        for a, b in zip(outs["pair"][2], outs[form][2]):   # the backward reads Av / AtT saved by whichever forward ran
            close(a, b, 2e-4, name=f"gradient through the saved probabilities ({form})")


def test_xattn_pixel_row_launch_replays_from_a_graph(ops):
    """The persistent cross-attention launch keeps its epoch and flags in device memory: captured once, it must replay with NEW
    operand values each time (the sentence planes are rebuilt by the captured preparation launch) and hand the same results as
    the eager call; no wait may time out."""
    if ops.get_gemm_mode() == "f32":
        pytest.skip("the single-launch forms are split-bf16 kernels")
    B, P, N, C = 48, 100, 48, 1024
    g = torch.Generator().manual_seed(11)
    mk = lambda *sh: torch.randn(*sh, generator=g).cuda()
    Qv, Kv, Vv, Qt, Kt, Vt = mk(B, P, C), mk(B, P, C), mk(B, P, C), mk(N, C), mk(N, C), mk(N, C)
    side = torch.cuda.Stream()
    with torch.no_grad():
        with torch.cuda.stream(side):
            for _ in range(2):
                ops.xattn(Qv, Kv, Vv, Qt, Kt, Vt)     # (allocations, sync words of this stream)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            nv, nl = ops.xattn(Qv, Kv, Vv, Qt, Kt, Vt)
        for it in range(3):
            for t in (Qv, Kv, Vv, Qt, Kt, Vt):
                t.copy_(torch.randn(t.shape, generator=g).cuda() * (1.0 + it))
            graph.replay()
            torch.cuda.synchronize()
            ev, el = ops.xattn(Qv, Kv, Vv, Qt, Kt, Vt)
            assert torch.equal(nv, ev) and torch.equal(nl, el), f"replay {it}"
    assert not ops.xattn_timed_out()


def test_xattn_forward_and_backward_replay_from_a_graph(ops):
    """Forward AND backward persistent launches share the sync words (epoch, flags): captured together in one graph they must replay
    with new operand values and hand the gradients of the eager call, bit for bit; no wait may time out."""
    if ops.get_gemm_mode() == "f32":
        pytest.skip("the single-launch forms are split-bf16 / h2 kernels")
    B, P, N, C = 48, 100, 48, 1024
    g = torch.Generator().manual_seed(5)
    mk = lambda *sh: torch.randn(*sh, generator=g).cuda().requires_grad_(True)
    q = [mk(B, P, C), mk(B, P, C), mk(B, P, C), mk(N, C), mk(N, C), mk(N, C)]
    wv, wl = torch.randn(B, P, C, generator=g).cuda(), torch.randn(B, N, C, generator=g).cuda()

    def fb():
        nv, nl = ops.xattn(*q)
        return torch.autograd.grad([nv, nl], q, [wv, wl])
    side = torch.cuda.Stream()
    ops.profile_begin()
    with torch.cuda.stream(side):
        for _ in range(2):
            fb()
    side.synchronize()
    kinds = {r[0] for r in ops.profile_end()}
    assert {"xattn_fwd_px", "xattn_bwd_px"} <= kinds, kinds      # (both persistent launches are what runs at this shape)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        grads = fb()
    for it in range(3):
        with torch.no_grad():
            for t in q + [wv, wl]:
                t.copy_(torch.randn(t.shape, generator=g).cuda() * (1.0 + it))
        graph.replay()
        torch.cuda.synchronize()
        want = fb()
        for a_, b_ in zip(grads, want):
            assert torch.equal(a_, b_), f"replay {it}"
    assert not ops.xattn_timed_out()


@pytest.mark.parametrize("B,P,N,C", [(3, 100, 5, 1024), (48, 100, 48, 1024), (1, 100, 1, 1024), (2, 37, 64, 128), (2, 25, 17, 64),
                                     (7, 104, 33, 1024), (33, 57, 17, 1024), (40, 97, 64, 512), (60, 103, 64, 1024), (5, 8, 3, 512)])
def test_xattn_fused(ops, B, P, N, C):
    Qv, Kv, Vv = leaf(B, P, C, seed=1), leaf(B, P, C, seed=2), leaf(B, P, C, seed=3)
    Qt, Kt, Vt = leaf(N, C, seed=4), leaf(N, C, seed=5), leaf(N, C, seed=6)
    sc = 1.0 / math.sqrt(C)
    Av = torch.softmax(Qv @ Kt.t() * sc, dim=2)
    At = torch.softmax(Qt @ Kv.transpose(1, 2) * sc, dim=2)
    nv, nl = Av @ Vt, At @ Vv
    wv = torch.randn(nv.shape, generator=torch.Generator().manual_seed(7))
    wl = torch.randn(nl.shape, generator=torch.Generator().manual_seed(8))
    ((nv * wv).sum() + (nl * wl).sum()).backward()
    g = [gpu_leaf(t) for t in (Qv, Kv, Vv, Qt, Kt, Vt)]
    ops.profile_begin()
    gnv, gnl = ops.xattn(*g)
    ((gnv * wv.cuda()).sum() + (gnl * wl.cuda()).sum()).backward()
    kinds = {r[0] for r in ops.profile_end()}
    if "xattn_fwd_px" in kinds:   # the pixel-row forward ran: so must the pixel-row backward (one persistent launch, csrc/xattn_px.hip)
        assert "xattn_bwd_px" in kinds, kinds
        assert not ops.xattn_timed_out()
    close(gnv, nv, name="new_vis")
    close(gnl, nl, name="new_lan")
    for a, b, name in zip(g, (Qv, Kv, Vv, Qt, Kt, Vt), ("dQv", "dKv", "dVv", "dQt", "dKt", "dVt")):
        close(a.grad, b.grad, 5e-4, name=name)


@pytest.mark.parametrize("kind,shape", [("conv3", (2, 20, 20, 32, 64)), ("conv3", (3, 24, 24, 64, 160)), ("conv1", (2, 16, 16, 64, 256)),
                                        ("conv1", (1, 12, 12, 256, 64)), ("stem", (3, 64, 48, 3, 32))])
def test_fused_bn_statistics_in_conv_epilogue(ops, kind, shape):
    """conv -> train-mode BN with the statistics taken from the GEMM epilogue == the two-kernel path."""
    B, H, W, Cin, Cout = shape
    x = torch.randn(B, H, W, Cin, generator=torch.Generator().manual_seed(1)).cuda() * 2 + 1
    k = 1 if kind == "conv1" else 3
    stride = 2 if kind == "stem" else 1     # the stem's first convolution (Cin = 3, stride 2): its own kernel and statistics
    w = (torch.randn(Cout, Cin, k, k, generator=torch.Generator().manual_seed(2)) * 0.1).contiguous(
        memory_format=torch.channels_last).cuda()
    g, b = torch.rand(Cout).cuda() + 0.5, torch.randn(Cout).cuda()

    def run(stats):
        rm, rv = torch.zeros(Cout).cuda(), torch.ones(Cout).cuda()
        y = ops.conv3x3(x, w, stride, stats=stats) if k == 3 else ops.linear(x, w, None, stats=stats)
        assert hasattr(y, "_bn_part") == stats
        return ops.batch_norm(y, g, b, rm, rv, None, True, True), rm, rv
    with torch.no_grad():
        (y0, rm0, rv0), (y1, rm1, rv1) = run(False), run(True)
    close(y1, y0, 1e-5, name="bn out")
    close(rm1, rm0, 1e-6, name="running_mean")
    close(rv1, rv0, 1e-5, name="running_var")


@pytest.mark.parametrize("M,N,K,tA,tB", [(2400, 768, 3072, False, True), (960, 512, 512, False, True),
                                         (1024, 256, 19200, True, False), (19200, 1024, 256, False, True),
                                         (300, 100, 4096, False, False), (5000, 32, 576, False, True),
                                         (4096, 32, 1024, False, False), (3000, 28, 512, True, False),
                                         # k-major operands over a k extent that is NOT a multiple of 32 (the weight gradients of a
                                         # ViT-B/16 trunk: 48 x 401 tokens): the fast kernel over K rounded up, tail rows read as zeros
                                         (768, 768, 19248, True, False), (512, 256, 200, True, False), (256, 64, 1203, True, False)])
def test_gemm_autotune_every_candidate_and_the_cached_choice(ops, M, N, K, tA, tB):
    """The first-encounter autotuner launches every admissible (tile, split-K) pair on the caller's buffers: after the
    tuning call AND on the cached path the result must be the product; each tile shape is also forced individually."""
    import os
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn((K, M) if tA else (M, K), generator=g)
    B = torch.randn((N, K) if tB else (K, N), generator=g)
    ref = ((A.t() if tA else A).double() @ (B.t() if tB else B).double()).float()
    dA, dB = A.cuda(), B.cuda()

    def run():
        C = torch.full((M, N), float("nan"), device="cuda")
        ops.gemm(dA, dB, C, M, N, K, dA.shape[1], dB.shape[1], N, tA, tB)
        return C.cpu()
    scale = float(ref.abs().max())
    ops.set_autotune(True)
    try:
        first, cached = run(), run()
    finally:
        ops.set_autotune(False)
    assert float((first - ref).abs().max()) <= 2e-4 * scale and float((cached - ref).abs().max()) <= 2e-4 * scale
    # (128x32 applies to N <= 32 only, 256x128 to the pipelined x3 loop with N > 64: otherwise the cost model's choice)
    for tile in ("128x128", "128x64", "64x64", "128x32", "256x128"):
        with ops.option("FORCE_TILE", tile):
            out = run()
        assert float((out - ref).abs().max()) <= 2e-4 * scale, tile


def test_side_streams_are_probed_onto_their_own_hardware_queues():
    """HIP maps streams onto 4 hardware queues round-robin in creation order; streams created by somebody else (a collective
    backend) can put a side stream on the compute stream's queue, where it no longer overlaps anything.  ops._calibrated_streams
    probes candidates with a device-side sleep: whatever was created before, the streams it hands out run concurrently with
    the compute stream and with each other."""
    from tris_amd import ops as o
    decoys = [torch.cuda.Stream() for _ in range(3)]           # shift the round-robin: the 4th new stream wraps onto queue 0
    for d in decoys:
        with torch.cuda.stream(d):
            torch.zeros(1, device="cuda").add_(1)
    torch.cuda.synchronize()
    o._CAL.clear()
    picked = o._calibrated_streams(torch.cuda.current_device())
    assert len(picked) >= 2, picked
    x = torch.zeros(64, device="cuda")

    def overlap(a, b):
        torch.cuda.synchronize()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        with torch.cuda.stream(a):
            e0.record()
            torch.cuda._sleep(3000000)
            e1.record()
        with torch.cuda.stream(b):
            x.add_(1.0)
            e2.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e2) < 0.5 * e0.elapsed_time(e1)
    main = torch.cuda.current_stream()
    for i, a in enumerate(picked):
        assert overlap(main, a), f"picked stream {i} shares the compute stream's hardware queue"
        for b in picked[i + 1:]:
            assert overlap(a, b)


def test_fusion_gradient_boxes_equal_autograd_sums(ops):
    """norm_vis / norm_lan feed three projections of the cross-modal fusion and the 0.1 residual mix: with gradient boxes each
    projection's data-gradient product adds the running sum in its epilogue (model/attn.py forward_cl, model_stage1.py
    forward_cached); with TRIS_GRAD_BOX=0 autograd sums the four terms with element-wise passes.  Same gradients either way."""
    import tris_amd.ops as o
    from tris_amd.model.attn import bilateral_prompt
    from tris_amd.utils.synth import seed_fill
    B, Pp, N, C = 3, 100, 5, 128
    fuse = bilateral_prompt(C, lan_chans=C).cuda().train()
    seed_fill(fuse.state_dict(), 77)
    g = torch.Generator().manual_seed(5)
    vis0, lan0 = torch.randn(B, Pp, C, generator=g), torch.randn(N, C, generator=g)
    wv, wl = torch.randn(B, Pp, C, generator=g).cuda(), torch.randn(B, N, C, generator=g).cuda()

    def run(boxes):
        with CFG.override(grad_box=boxes):
            vis, lan = vis0.clone().cuda().requires_grad_(True), lan0.clone().cuda().requires_grad_(True)
            nv, nl = o.l2norm(vis), o.l2norm(lan)
            grad = boxes
            bv = o.GradBox() if grad else None
            bl = o.GradBox() if grad else None
            new_vis, new_lan = fuse.forward_cl(nv, nl, box_vis=bv, box_lan=bl)
            ov = o.axpy(new_vis, nv, 0.1, grad_box_b=bv)
            ol = o.axpy_bcast(new_lan, nl, 0.1, grad_box_b=bl)
            for p_ in fuse.parameters():
                p_.grad = None
            ((ov * wv).sum() + (ol * wl).sum()).backward()
            torch.cuda.synchronize()
            if boxes:   # every box was filled and consumed: no gradient fell back to autograd's own sum
                assert bv.value is None and bl.value is None
            return vis.grad.clone(), lan.grad.clone(), [p_.grad.clone() for p_ in fuse.parameters()]
    a, b = run(True), run(False)
    close(a[0], b[0], 2e-6 * float(b[0].abs().max()) + 1e-9, name="d vis")
    close(a[1], b[1], 2e-6 * float(b[1].abs().max()) + 1e-9, name="d lan")
    for x, y in zip(a[2], b[2]):
        close(x, y, 2e-6 * float(y.abs().max()) + 1e-9, name="d parameter")


@pytest.mark.parametrize("M,W", [(2400, 768), (37, 64), (50, 48)])
def test_mlp_with_quickgelu_in_the_epilogues(ops, M, W):
    """transformer MLP (CLIP/clip/model.py:361-376): c_fc + QuickGELU in one launch that also stores the pre-activation, the
    QuickGELU backward in c_proj's data-gradient epilogue (tris_gemm_epilogue_next).  (50, 48): K % 32 != 0 -- the armed product
    declines and the unfused passes run; same numbers."""
    import tris_amd.ops as o
    x, w1, b1 = leaf(M, W), leaf(4 * W, W, scale=0.05), leaf(4 * W, scale=0.1)
    w2, b2 = leaf(W, 4 * W, scale=0.05, seed=1), leaf(W, scale=0.1, seed=1)
    h = x @ w1.t() + b1
    y = (h * torch.sigmoid(1.702 * h)) @ w2.t() + b2 + x
    wy = leaf(M, W, seed=7).detach()
    (y * wy).sum().backward()
    g = [gpu_leaf(t) for t in (x, w1, b1, w2, b2)]
    f = o.linear_qgelu(g[0], g[1], g[2])
    link = f._act_link
    gy = o.linear(f, g[3], g[4], g[0], 0, act_link=True)
    (gy * wy.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert link.applied == (W % 32 == 0)     # the fused backward ran exactly where the fast kernel serves the product
    close(gy, y, name="y")
    for a, b_, n in zip(g, (x, w1, b1, w2, b2), ("dx", "dw1", "db1", "dw2", "db2")):
        close(a.grad, b_.grad, 2e-5 if M > 1000 else TOL, name=n)


def test_gemm_epilogue_streams_nontemporal_equals_default(ops):
    """a product whose epilogue streams (C + residual) exceed the memory-side cache stores / loads them with the nontemporal
    policy (gemm_conv.hip stream_nt, option STREAM_FORM): same values bit for bit"""
    import tris_amd.ops as o
    M, N, K = 307200, 256, 64
    g = torch.Generator(device="cuda").manual_seed(3)
    A, W = torch.randn(M, K, device="cuda", generator=g), torch.randn(N, K, device="cuda", generator=g) * 0.1
    R = torch.randn(M, N, device="cuda", generator=g)
    assert 2 * M * N * 4 > 256 << 20
    outs = []
    for sf in (0, None):
        with o.option("STREAM_FORM", sf):
            C = torch.empty(M, N, device="cuda")
            o.gemm(A, W, C, M, N, K, K, K, N, False, True, resid=R, ldr=N)
            outs.append(C)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    ref = (A[:512].double() @ W.double().t() + R[:512].double()).float()
    close(outs[1][:512], ref, 1e-4, name="rows vs fp64")
