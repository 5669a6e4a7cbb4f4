"""Bilateral cross attention on the device against fp64 with the element-wise bounds of tests/oracle_xattn.py (derived there, checked on
the CPU by tests/test_xattn_host.py): the three forward entry points and the pixel-row backward on buffers the test owns -- guard rows
around every output, NaN behind every input, the probability scratch pre-filled with a sentinel --, the chain backward and the whole
ops.xattn autograd path, which kernel ops.xattn dispatches, and tris_softmax_col_bwd_f32.  The ratios err / bound measured on the
MI355X are in profiles/xattn_parity_floor.txt (`python tests/test_gpu_xattn.py > profiles/xattn_parity_floor.txt`).

Every test that launches a persistent kernel first looks at ops.xattn_timed_out(): the word is sticky, a timed-out wait is a finding,
and nothing is launched on top of one."""
import contextlib
import math
import os
import sys

import pytest
import torch

import oracle_xattn as O
from test_gpu_mha import SENT, H2Words, guarded_input, guarded_output, guards_intact, stream

gpu = pytest.mark.gpu

DECLINED = -2
INVALID = 1              # hipErrorInvalidValue
# (form, arithmetic) of the forward entry points; h2_amax_x64: amax words 64 times too large (any upper bound is a valid word)
FORWARDS = [("pair", "f32"), ("pair", "x3"), ("slices", "x3"), ("px", "x3"), ("px", "h2"), ("px", "h2_amax_x64")]
MODE = {"f32": "f32", "x3": "x3", "h2": "h2", "h2_amax_x64": "h2"}
ENTRY = {"pair": "tris_xattn_fwd_f32", "slices": "tris_xattn_fused_fwd_f32", "px": "tris_xattn_px_fwd_f32"}
PATHS = [("pair+chain", "f32"), ("pair+chain", "x3"), ("pair+chain", "h2"), ("px+px", "x3"), ("px+px", "h2")]


def lib():
    from tris_amd import _lib
    return _lib.load()


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@contextlib.contextmanager
def arithmetic(arith):
    """the dense-product mode of `arith`; h2: a fresh pool of amax words (H2Words) -> the words object, else None"""
    from tris_amd import ops
    if MODE[arith] == "h2":
        with H2Words() as h2:
            yield h2
        return
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(MODE[arith])
    try:
        yield None
    finally:
        torch.cuda.synchronize()
        ops.set_gemm_mode(prev)


@contextlib.contextmanager
def pinned(case):
    """XATTN_PX_SLOTS of the case for the scope; the plan must then be the oracle's cut"""
    from tris_amd import ops
    B, P, N, C, pin = case
    ops.set_option("XATTN_PX_SLOTS", pin if pin else None)
    try:
        S = int(ops.query("tris_xattn_px_slots", B, P, C, cus()))
        assert S == O.plan_slots(B, P, C, cus(), pin) == len(O.cut(case)), (case, S, cus())
        yield S
    finally:
        ops.set_option("XATTN_PX_SLOTS", None)


def upload(kind, case):
    """-> {name: [rows, C] view on the device, NaN behind it}, and the buffers (kept alive)"""
    x, _ = O.case_of(kind, case)
    views, bufs = {}, []
    for name, t in x.items():
        buf, v = guarded_input(t.reshape(-1, t.shape[-1]))
        views[name] = v
        bufs.append(buf)
    return views, bufs


def persistent_guard():
    from tris_amd import ops
    assert not ops.xattn_timed_out(), "a wait inside an earlier persistent launch timed out: nothing is launched on top of it"


def forward(form, d, case, h2=None, mul=1.0):
    """one launch of ENTRY[form] on fresh guarded outputs -> (rc, {new_vis, new_lan, probs [B, 4, P, N]} device views); guards checked"""
    from tris_amd import ops
    from tris_amd._lib import call
    B, P, N, C, _ = case
    vb, nv = guarded_output(B * P, C)
    lb, nl = guarded_output(B * N, C)
    pb, pr = guarded_output(B * 4 * P, N)
    ptr = lambda n: d[n].data_ptr()
    args = [ptr(n) for n in ("Qv", "Kv", "Vv", "Qt", "Kt", "Vt")] + [nv.data_ptr(), nl.data_ptr(), pr.data_ptr(), B, P, N, C]
    keep = None
    if form != "pair":
        persistent_guard()
        nbytes = int(ops.query(f"tris_xattn_{'px' if form == 'px' else 'fused'}_ws_bytes", B, N, C))
        ws = torch.empty(nbytes // 4 + 4, device="cuda", dtype=torch.float32) if nbytes > 0 else None   # (0: the shape is not supported)
        sync = ops._xattn_sync(torch.device("cuda", torch.cuda.current_device()), B)
        args += [ws.data_ptr() if nbytes > 0 else None, max(nbytes, 0), sync.data_ptr()]
        keep = (ws, sync)
        if h2 is not None:
            call("tris_xattn_amax_next", *[h2.of(d[n], mul) for n in ("Qv", "Kv", "Vv", "Qt", "Kt", "Vt")])
    rc = getattr(lib(), ENTRY[form])(*args, stream())
    torch.cuda.synchronize()
    del keep
    if form != "pair":
        assert not ops.xattn_timed_out(), (form, case, "a wait timed out")
    assert all(guards_intact(b) for b in (vb, lb, pb)), (form, case, "a guard row was written")
    return rc, dict(new_vis=nv, new_lan=nl, probs=pr.view(B, 4, P, N), bufs=(vb, lb, pb))


def px_backward(d, case, probs, h2=None, mul=1.0):
    """tris_xattn_px_bwd_f32 on the probabilities of a forward -> (rc, {dQv, dKv, dVv, dS [3, B, P, N], amax: three decoded words})"""
    from tris_amd import ops
    from tris_amd._lib import call
    B, P, N, C, _ = case
    persistent_guard()
    outs = {n: guarded_output(B * P, C) for n in ("dQv", "dKv", "dVv")}
    sb, dS = guarded_output(3 * B * P, N)
    words = [torch.zeros(ops.H2_SUB, device="cuda", dtype=torch.int32) for _ in range(3)]
    nbytes = int(ops.query("tris_xattn_px_bwd_ws_bytes", B, N, C))
    assert nbytes > 0, case
    ws = torch.empty(nbytes // 4 + 4, device="cuda", dtype=torch.float32)
    sync = ops._xattn_sync(torch.device("cuda", torch.cuda.current_device()), B)
    if h2 is not None:
        call("tris_xattn_amax_next", *[h2.of(d[n], mul) for n in ("d_vis", "Vv", "d_lan", "Qt", "Kt", "Vt")])
    rc = lib().tris_xattn_px_bwd_f32(*[d[n].data_ptr() for n in ("d_vis", "d_lan", "Vv", "Qt", "Kt", "Vt")], probs.data_ptr(),
                                     *[outs[n][1].data_ptr() for n in ("dQv", "dKv", "dVv")], dS.data_ptr(), B, P, N, C, ws.data_ptr(),
                                     ws.numel() * 4, sync.data_ptr(), *[w.data_ptr() for w in words], stream())
    torch.cuda.synchronize()
    assert not ops.xattn_timed_out(), (case, "a wait timed out")
    assert all(guards_intact(b) for b, _ in outs.values()) and guards_intact(sb), (case, "a guard row was written")
    res = {n: v.view(B, P, C) for n, (_, v) in outs.items()}
    res.update(dS=dS.view(3, B, P, N), amax=[float(w.view(torch.float32).max()) for w in words])
    return rc, res


def fwd_bound(form, arith, kind, case):
    mul = 64.0 if arith == "h2_amax_x64" else 1.0
    fwd = O.pair_arith(MODE[arith], case) if form == "pair" else MODE[arith]
    return O.bound_of(kind, case, fwd, "chain", "x3", mul, 8 if form == "slices" else 4)


def run_forward(form, arith, kind, case):
    """-> ({output: err / bound} or None where the form declines, outputs on the CPU) after the checks that do not depend on the bound:
    return code and arithmetic, finite, guard rows, planes 1 and 3, two launches bit for bit"""
    from tris_amd import ops
    B, P, N, C, _ = case
    _, ref = O.case_of(kind, case)
    d, bufs = upload(kind, case)
    mul = 64.0 if arith == "h2_amax_x64" else 1.0
    inside = form == "pair" or case in O.PERSISTENT
    with arithmetic(arith) as h2, (pinned(case) if form == "px" and inside else contextlib.nullcontext()):
        rc, first = forward(form, d, case, h2 if form == "px" else None, mul)
        if not inside:
            assert rc == DECLINED, (form, arith, case, rc)
            assert all(bool((b == SENT).all()) for b in first["bufs"]), (form, case, "a declined call wrote an output")
            return None, None
        assert rc == 0, (form, arith, case, rc)
        if form == "px":
            assert int(ops.query("tris_xattn_px_last_form")) == (2 if MODE[arith] == "h2" else 1), (arith, case)
        rc, again = forward(form, d, case, h2 if form == "px" else None, mul)
        assert rc == 0
    for name in ("new_vis", "new_lan", "probs"):
        assert torch.equal(first[name], again[name]), (form, arith, kind, case, name, "two launches differ")
    pr = first["probs"]
    if form != "pair":
        assert bool((pr[:, 1] == SENT).all()) and bool((pr[:, 3] == SENT).all()), (form, case, "planes 1 / 3 were written")
    got = dict(new_vis=first["new_vis"].view(B, P, C).cpu(), new_lan=first["new_lan"].view(B, N, C).cpu(), Av=pr[:, 0].cpu(),
               AtT=pr[:, 2].cpu())
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), (form, arith, kind, case, name, "not finite")
    if N == 1:
        assert bool((got["Av"] == 1).all()), (form, arith, case)
    return O.ratios(got, ref, fwd_bound(form, arith, kind, case)), got


@gpu
@pytest.mark.parametrize("kind", O.KINDS)
@pytest.mark.parametrize("form,arith", FORWARDS)
def test_forward_against_fp64(form, arith, kind):
    """the three forward entry points over the whole case list: new_vis, new_lan and the saved Av / AtT within the bound element by
    element; outside a persistent form's domain the call declines and writes nothing"""
    worst = {}
    for case in O.CASES:
        r, _ = run_forward(form, arith, kind, case)
        if r is None:
            continue
        print(f"{form} {arith} {kind} {case}: " + " ".join(f"{n} {v:.3f}" for n, v in r.items()))
        worst = {n: max(worst.get(n, 0.0), v) for n, v in r.items()}
        assert max(r.values()) <= 1.0, (form, arith, kind, case, r)
    print(f"{form} {arith} {kind}: worst err / bound {worst}")


def run_px_backward(arith, kind, case):
    """forward and backward of the pixel-row form in `arith` -> ({output: err / bound}, outputs on the CPU)"""
    B, P, N, C, _ = case
    x, ref = O.case_of(kind, case)
    d, bufs = upload(kind, case)
    with arithmetic(arith) as h2, pinned(case):
        rc, f = forward("px", d, case, h2)
        assert rc == 0, (arith, case, rc)
        rc, first = px_backward(d, case, f["probs"], h2)
        assert rc == 0, (arith, case, rc)
        rc, again = px_backward(d, case, f["probs"], h2)
        assert rc == 0
    for name in ("dQv", "dKv", "dVv", "dS"):
        assert torch.equal(first[name], again[name]), (arith, kind, case, name, "two launches differ")
    assert torch.equal(first["dS"][2], f["probs"][:, 0]), (arith, case, "dS plane 2 is not the saved Av")
    got = {n: first[n].cpu() for n in ("dQv", "dKv", "dVv")}
    got.update(dS1=first["dS"][0].cpu(), dS2=first["dS"][1].cpu())
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), (arith, kind, case, name, "not finite")
    for name, word in zip(("dQv", "dKv", "dVv"), first["amax"]):       # a word that is too small overflows the fp16 consumer
        assert word >= float(got[name].abs().max()), (arith, kind, case, name, word, float(got[name].abs().max()))
    if kind == "zero_rows":
        rows = O.zero_pixels(case)
        assert bool((got["dQv"][:, rows] == 0).all()) and bool((got["dS1"][:, rows] == 0).all()), (arith, case)
        assert bool((got["dS2"][:, :, 0] == 0).all()), (arith, case)
    if N == 1:
        assert bool((got["dS1"] == 0).all()) and bool((got["dQv"] == 0).all()), (arith, case)
    return O.ratios(got, ref, O.bound_of(kind, case, arith, "px", arith)), got


@gpu
@pytest.mark.parametrize("kind", O.KINDS)
@pytest.mark.parametrize("arith", ["x3", "h2"])
def test_pixel_row_backward_against_fp64(arith, kind):
    """tris_xattn_px_bwd_f32 on the probabilities its own forward wrote: dQv, dKv, dVv, dS1, dS2 within the bound, the Av copy bit for
    bit, exact zeros for zero_rows and N = 1, the amax words it leaves not below what it wrote"""
    worst = {}
    for case in O.PERSISTENT:
        r, _ = run_px_backward(arith, kind, case)
        print(f"px backward {arith} {kind} {case}: " + " ".join(f"{n} {v:.3f}" for n, v in r.items()))
        worst = {n: max(worst.get(n, 0.0), v) for n, v in r.items()}
        assert max(r.values()) <= 1.0, (arith, kind, case, r)
    print(f"px backward {arith} {kind}: worst err / bound {worst}")


def expected_kernels(case, mode, fused, px, bwd_px):
    """which launches ops.xattn issues, from the documented domains (include/tris_hip.h)"""
    B, P, N, C, pin = case
    if mode != "f32" and fused and px and O.plan_slots(B, P, C, cus(), pin) > 0:
        return {"xattn_fwd_px", "xattn_bwd_px"} if bwd_px else {"xattn_fwd_px"}
    if mode != "f32" and fused and C in (512, 1024) and 8 <= P <= 104 and N <= 64 and B * 8 <= cus():
        return {"xattn_fwd_fused"}
    return {"xattn_fwd_pair"}


def run_autograd(path, mode, kind, case, flags=None):
    """ops.xattn forward and backward with the explicit d_vis, d_lan of the oracle -> (outputs on the CPU, the xattn launches recorded)"""
    from tris_amd import ops
    from tris_amd.config import cfg as CFG
    x, _ = O.case_of(kind, case)
    px = path == "px+px"
    flags = flags or dict(xattn_fused=px, xattn_px=px, xattn_bwd_px=px, xattn_h2=True)
    prev = ops.get_gemm_mode()
    pin = pinned(case) if case in O.PERSISTENT else contextlib.nullcontext()
    try:
        ops.set_gemm_mode(mode)
        ops.h2_begin_step()
        ops.h2_end_step()
        with CFG.override(**flags), pin:
            if flags["xattn_fused"] and mode != "f32":
                persistent_guard()
            q = [x[n].cuda().requires_grad_(True) for n in ("Qv", "Kv", "Vv", "Qt", "Kt", "Vt")]
            ops.profile_begin()
            nv, nl = ops.xattn(*q)
            grads = torch.autograd.grad([nv, nl], q, [x["d_vis"].cuda(), x["d_lan"].cuda()])
            kinds = {r[0] for r in ops.profile_end() if r[0].startswith("xattn")}
            form = int(ops.query("tris_xattn_px_last_form"))
        torch.cuda.synchronize()
        assert not ops.xattn_timed_out(), (path, mode, case)
    finally:
        ops.set_gemm_mode(prev)
    got = dict(new_vis=nv.detach().cpu(), new_lan=nl.detach().cpu())
    got.update({n: g.cpu() for n, g in zip(O.GRADS, grads)})
    return got, kinds, form


@gpu
@pytest.mark.parametrize("kind", O.KINDS)
@pytest.mark.parametrize("path,mode", PATHS)
def test_autograd_paths_against_fp64(path, mode, kind):
    """the whole ops.xattn path -- the pair with the chain backward in f32, x3 and h2, the pixel-row forward with the pixel-row backward
    in x3 and h2 -- with explicit d_vis, d_lan: both outputs and all six gradients within the bound, exact zeros for zero_rows"""
    worst = {}
    for case in (O.PERSISTENT if path == "px+px" else O.CASES):
        _, ref = O.case_of(kind, case)
        got, kinds, form = run_autograd(path, mode, kind, case)
        if path == "px+px":
            assert kinds == {"xattn_fwd_px", "xattn_bwd_px"}, (mode, case, kinds)
            assert form == (2 if mode == "h2" else 1), (mode, case, form)
            bound = O.bound_of(kind, case, mode, "px", mode)
        else:
            assert kinds == {"xattn_fwd_pair"}, (mode, case, kinds)
            bound = O.bound_of(kind, case, O.pair_arith(mode, case), "chain", mode)
        for name, t in got.items():
            assert bool(torch.isfinite(t).all()), (path, mode, kind, case, name, "not finite")
        if kind == "zero_rows":
            assert bool((got["dQv"][:, O.zero_pixels(case)] == 0).all()), (path, mode, case)
        r = O.ratios(got, ref, bound)
        print(f"{path} {mode} {kind} {case}: " + " ".join(f"{n} {v:.3f}" for n, v in r.items()))
        worst = {n: max(worst.get(n, 0.0), v) for n, v in r.items()}
        assert max(r.values()) <= 1.0, (path, mode, kind, case, r)
    print(f"{path} {mode} {kind}: worst err / bound {worst}")


@gpu
@pytest.mark.parametrize("mode", ["f32", "x3", "h2"])
def test_dispatch(mode):
    """which kernel ops.xattn runs, per case and configuration, computed from the documented domains: asserted unconditionally.  The f32
    mode takes the pair whatever the configuration says"""
    for case in O.CASES:
        for fused, px, bwd_px, h2 in ((True, True, True, True), (True, True, False, True), (True, False, True, True),
                                      (False, True, True, True), (True, True, True, False)):
            flags = dict(xattn_fused=fused, xattn_px=px, xattn_bwd_px=bwd_px, xattn_h2=h2)
            _, kinds, form = run_autograd("px+px", mode, "randn", case, flags)
            want = expected_kernels(case, mode, fused, px, bwd_px)
            assert kinds == want, (mode, case, flags, kinds, want)
            if "xattn_fwd_px" in want:
                assert form == (2 if mode == "h2" and h2 else 1), (mode, case, flags, form)
    if mode == "f32":
        assert all(expected_kernels(c, "f32", True, True, True) == {"xattn_fwd_pair"} for c in O.CASES)
    else:
        assert all("xattn_fwd_px" in expected_kernels(c, mode, True, True, True) for c in O.PERSISTENT)
        assert all(expected_kernels(c, mode, True, False, True) == {"xattn_fwd_fused"} for c in O.PERSISTENT)
        assert all(expected_kernels(c, mode, True, True, True) == {"xattn_fwd_pair"} for c in O.PAIR_ONLY)


COL_SHAPES = [(2, 8, 1), (2, 33, 17), (2, 104, 64), (1, 130, 5)]


def run_col_bwd(B, P, N):
    g = torch.Generator().manual_seed(4100 + 131 * P + N)
    Y = torch.softmax(3.0 * torch.randn(B, P, N, generator=g), 1)
    dY = torch.randn(B, P, N, generator=g)
    scale = 1.0 / math.sqrt(512.0)
    ref, bound = O.col_bwd_reference(Y, dY, float(torch.tensor(scale, dtype=torch.float32)))
    _, dy = guarded_input(dY.view(B * P, N))
    _, y = guarded_input(Y.view(B * P, N))
    ob, out = guarded_output(B * P, N)
    rc = lib().tris_softmax_col_bwd_f32(dy.data_ptr(), y.data_ptr(), out.data_ptr(), B, P, N, scale, stream())
    torch.cuda.synchronize()
    assert rc == 0 and guards_intact(ob), (B, P, N, rc)
    got = out.view(B, P, N).cpu()
    assert bool(torch.isfinite(got).all())
    return O.ratios(dict(dX=got), dict(dX=ref), dict(dX=bound))["dX"]


@gpu
def test_softmax_col_bwd_against_fp64():
    """the soft-max backward over the pixel axis of the chain backward, on its own: within its derived bound (a P-term sum, three
    roundings), guard rows intact; N = 65 is refused before any launch"""
    for B, P, N in COL_SHAPES:
        r = run_col_bwd(B, P, N)
        print(f"softmax_col_bwd B {B} P {P} N {N}: err / bound {r:.3f}")
        assert r <= 1.0, (B, P, N, r)
    B, P, N = 2, 8, 65
    _, y = guarded_input(torch.full((B * P, N), 1.0 / P))
    out = torch.full((B * P, N), SENT, device="cuda")
    rc = lib().tris_softmax_col_bwd_f32(y.data_ptr(), y.data_ptr(), out.data_ptr(), B, P, N, 1.0, stream())
    torch.cuda.synchronize()
    assert rc == INVALID and bool((out == SENT).all())


# ---- the record: python tests/test_gpu_xattn.py > profiles/xattn_parity_floor.txt on the MI355X --------------------------------------
def main():
    print("# Cross-attention kernels (csrc/xattn.hip, xattn_fused.hip, xattn_px.hip) against fp64: the largest err / bound over the case")
    print("# list of tests/oracle_xattn.py per form, arithmetic, output and input kind, MI355X.  The bounds are the element-wise ones")
    print("# derived in tests/oracle_xattn.py; tests/test_gpu_xattn.py asserts ratio <= 1.  h2_amax_x64: amax words 64 times too large.")
    print("# form | arithmetic | output | err / bound per kind: " + " | ".join(O.KINDS))
    table = {}

    def note(form, arith, kind, r):
        for name, v in r.items():
            table[(form, arith, name, kind)] = max(table.get((form, arith, name, kind), 0.0), v)

    for kind in O.KINDS:
        for form, arith in FORWARDS:
            for case in (O.CASES if form == "pair" else O.PERSISTENT):
                note(f"forward {form}", arith, kind, run_forward(form, arith, kind, case)[0])
        for arith in ("x3", "h2"):
            for case in O.PERSISTENT:
                note("backward px", arith, kind, run_px_backward(arith, kind, case)[0])
        for path, mode in PATHS:
            for case in (O.PERSISTENT if path == "px+px" else O.CASES):
                _, ref = O.case_of(kind, case)
                got, _, _ = run_autograd(path, mode, kind, case)
                bound = O.bound_of(kind, case, mode, "px", mode) if path == "px+px" else \
                    O.bound_of(kind, case, O.pair_arith(mode, case), "chain", mode)
                note(f"ops.xattn {path}", mode, kind, O.ratios(got, ref, bound))
    for form, arith, name in dict.fromkeys(k[:3] for k in table):
        print(f"{form:<20} | {arith:<11} | {name:<7} | " + " | ".join(f"{table[(form, arith, name, kind)]:.3f}" for kind in O.KINDS))
    print("#\n# tris_softmax_col_bwd_f32\n# B | P | N | err / bound")
    for B, P, N in COL_SHAPES:
        print(f"{B} | {P} | {N} | {run_col_bwd(B, P, N):.3f}")
    top = {}
    for (form, arith, name, kind), v in table.items():
        top[(form, arith)] = max(top.get((form, arith), 0.0), v)
    print("#\n# largest ratio per form and arithmetic\n# form | arithmetic | err / bound")
    for (form, arith), v in top.items():
        print(f"{form:<20} | {arith:<11} | {v:.3f}")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
