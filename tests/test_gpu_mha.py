"""The three self-attention forms on the device against fp64 with the element-wise bounds of tests/oracle_mha.py (derived there,
checked on the CPU by tests/test_mha_host.py): the six C entry points on buffers the test owns -- guard rows around every output,
NaN behind every input --, the dispatch of ops.mha, and the argument contracts.  The ratios err / bound measured on the MI355X are
in profiles/mha_parity_floor.txt (`python tests/test_gpu_mha.py > profiles/mha_parity_floor.txt`)."""
import contextlib
import os
import sys

import pytest
import torch

import oracle_mha as O

gpu = pytest.mark.gpu

SENT = -7777.25          # sentinel of the buffers the tests own: a kernel that writes where it must not changes it
GUARD = 64               # guard rows: a whole key block read past the end would land in them
IMPLS = ["valu", "f32", "h2", "h2_amax_x64"]
FORM = {"valu": "valu", "f32": "f32", "h2": "h2", "h2_amax_x64": "h2"}
INVALID = 1              # hipErrorInvalidValue


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded_input(t):
    """t [rows, width] on the device, followed by GUARD rows of NaN -> (buffer, view of the rows)"""
    buf = torch.full((t.shape[0] + GUARD, t.shape[1]), float("nan"), device="cuda")
    buf[:t.shape[0]] = t.cuda()
    return buf, buf[:t.shape[0]]


def guarded_output(rows, width):
    buf = torch.full((rows + 2 * GUARD, width), SENT, device="cuda")
    return buf, buf[GUARD:GUARD + rows]


def guards_intact(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


class H2Words:
    """amax words the way MhaMfmaFn obtains them: ops._h2_amax inside the h2 arithmetic, on a fresh pool; restored on exit"""

    def __enter__(self):
        from tris_amd import ops
        self.ops, self.prev, self.keep = ops, ops.get_gemm_mode(), []
        ops.set_gemm_mode("h2")
        ops.h2_begin_step()
        ops.h2_end_step()
        return self

    def of(self, t, mul=1.0):
        t = t if mul == 1.0 else (t * mul).contiguous()
        self.keep.append(t)
        word = self.ops._h2_amax(t)
        assert word is not None
        return word

    def __exit__(self, *a):
        torch.cuda.synchronize()
        self.ops.set_gemm_mode(self.prev)


def launch(impl, qkv, dout, N, L, heads, causal, words):
    """one forward and one backward of `impl` on fresh guarded outputs -> dict of device tensors (oracle_mha.OUTPUTS layout)"""
    from tris_amd._lib import call
    W = heads * O.HD
    ob, out = guarded_output(N * L, W)
    gb, dqkv = guarded_output(N * L, 3 * W)
    lb, lse = guarded_output(N * heads * L, 1)
    db, delta = guarded_output(N * heads * L, 1)
    P = lambda t: t.data_ptr()
    if impl == "valu":
        call("tris_mha_fwd_f32", P(qkv), P(out), N, L, W, heads, causal, stream())
        call("tris_mha_bwd_f32", P(qkv), P(dout), P(dqkv), N, L, W, heads, causal, stream())
    elif impl == "f32":
        call("tris_mha_mfma_fwd_f32", P(qkv), P(out), P(lse), N, L, W, heads, causal, stream())
        call("tris_mha_mfma_bwd_f32", P(qkv), P(out), P(dout), P(lse), P(delta), P(dqkv), N, L, W, heads, causal, stream())
    else:
        call("tris_mha_h2_fwd_f32", P(qkv), P(out), P(lse), words[0], N, L, W, heads, causal, stream())
        call("tris_mha_h2_bwd_f32", P(qkv), P(out), P(dout), P(lse), P(delta), P(dqkv), words[0], words[1], N, L, W, heads, causal,
             stream())
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b in (ob, gb, lb, db)), "a guard row was written"
    if impl == "valu":
        assert bool((lb == SENT).all()) and bool((db == SENT).all())
    d3 = dqkv.view(N, L, 3, W)
    res = dict(out=out.view(N, L, W), dq=d3[:, :, 0], dk=d3[:, :, 1], dv=d3[:, :, 2])
    if impl != "valu":
        res.update(lse=lse.view(N, heads, L), delta=delta.view(N, heads, L))
    return res


def run_case(impl, kind, L, heads, causal):
    """-> ({output: err / bound}, outputs on the CPU) of one case, after the checks that do not depend on the bound: finite, guard rows,
    two launches bit for bit"""
    qkv, dout, ref, bnd = O.case(kind, L, heads, causal)
    N, W = O.NB, heads * O.HD
    mul = 64.0 if impl == "h2_amax_x64" else 1.0
    bound = bnd[FORM[impl]] if mul == 1.0 else O.bounds_h2(qkv, dout, heads, causal, amax_mul=mul)
    qb, d_qkv = guarded_input(qkv.view(N * L, 3 * W))
    gb, d_dout = guarded_input(dout.view(N * L, W))
    with (H2Words() if FORM[impl] == "h2" else contextlib.nullcontext()) as h2:
        words = (h2.of(d_qkv, mul), h2.of(d_dout, mul)) if h2 is not None else None
        first = launch(impl, d_qkv, d_dout, N, L, heads, causal, words)
        again = launch(impl, d_qkv, d_dout, N, L, heads, causal, words)
    for name in first:
        assert torch.equal(first[name], again[name]), (impl, kind, L, heads, causal, name, "two launches differ")
    got = {k: v.cpu() for k, v in first.items()}
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), (impl, kind, L, heads, causal, name, "not finite")
    return O.ratios(got, ref, bound), got


def cases_of(impl):
    return [c for c in O.CASES if impl != "valu" or c[0] <= 64]


@gpu
@pytest.mark.parametrize("kind", O.KINDS)
@pytest.mark.parametrize("impl", IMPLS)
def test_attention_against_fp64(impl, kind):
    """every case of the list: out, lse, dq, dk, dv (and delta for the flash forms) within the bound element by element, finite, guard
    rows intact, the NaN behind qkv and dout never reaches a result, two launches identical; zero_rows: exact zeros in dq.
    h2_amax_x64: amax words of 64 qkv and 64 dout (any upper bound is a valid word) under the bound for that amax."""
    worst = {}
    for L, heads, causal in cases_of(impl):
        r, got = run_case(impl, kind, L, heads, causal)
        print(f"{impl} {kind} L {L} heads {heads} causal {causal}: " + " ".join(f"{n} {v:.3f}" for n, v in r.items()))
        for name, v in r.items():
            worst[name] = max(worst.get(name, 0.0), v)
        if kind == "zero_rows":
            assert bool((got["dq"][:, O.zero_row_set(L)] == 0).all()), (impl, L, heads, causal)
        assert max(r.values()) <= 1.0, (impl, kind, L, heads, causal, r)
    print(f"{impl} {kind}: worst err / bound {worst}")


@gpu
def test_ops_mha_dispatch_and_parity():
    """ops.mha at the thresholds: L < 40 -> the LDS-resident kernel unless cfg.mha = "mfma"; L > 64 -> flash whatever cfg.mha says;
    inside flash the h2 kernels from L = 32 on in the h2 arithmetic; the autograd result within the bounds of the form that ran"""
    from tris_amd import ops
    from tris_amd.config import cfg as CFG
    table = {"auto": lambda L: "valu" if L < 40 else "mfma", "valu": lambda L: "valu" if L <= 64 else "mfma", "mfma": lambda L: "mfma"}
    prev = ops.get_gemm_mode()
    try:
        for mode in ("x3", "h2", "f32"):
            ops.set_gemm_mode(mode)
            ops.h2_begin_step()
            ops.h2_end_step()
            for pick in ("auto", "valu", "mfma"):
                for L in (31, 32, 39, 40, 64, 65):
                    heads, causal = 3, L % 2
                    qkv, dout, ref, bnd = O.case("randn", L, heads, causal)
                    with CFG.override(mha=pick):
                        want = ops._mha_impl(L)
                        assert want == table[pick](L), (pick, L)
                        x = qkv.cuda().requires_grad_(True)
                        ops.MHA_STATS["last"] = None
                        y = ops.mha(x, heads, bool(causal))
                        y.backward(dout.cuda())
                    cls = type(y.grad_fn).__name__
                    assert cls == ("MhaFnBackward" if want == "valu" else "MhaMfmaFnBackward"), (mode, pick, L, cls)
                    if want == "valu":
                        form = "valu"
                        assert ops.MHA_STATS["last"] is None
                    else:
                        form = "h2" if (mode == "h2" and L >= 32) else "f32"
                        assert ops.MHA_STATS["last"] == form, (mode, pick, L)
                    W = heads * O.HD
                    got = dict(out=y.detach().cpu(), dq=x.grad[..., :W].cpu(), dk=x.grad[..., W:2 * W].cpu(), dv=x.grad[..., 2 * W:].cpu())
                    r = O.ratios(got, ref, bnd[form])
                    assert max(r.values()) <= 1.0, (mode, pick, L, form, r)
    finally:
        ops.set_gemm_mode(prev)


@gpu
def test_argument_contracts():
    """every validation of the six entry points: the call returns hipErrorInvalidValue before any launch, the outputs keep the
    sentinel.  Pointers are only ever offset where the entry point checks them -- no kernel runs on a pointer it does not support."""
    from tris_amd import _lib
    lib = _lib.load()
    N, L, heads = 2, 16, 1
    W = heads * O.HD
    qkv, dout = O.inputs("randn", L, heads, 0)
    _, d_qkv = guarded_input(qkv.view(N * L, 3 * W))
    _, d_dout = guarded_input(dout.view(N * L, W))
    outs = {n: torch.full(s, SENT, device="cuda") for n, s in dict(out=(N * L + 1, W), dqkv=(N * L, 3 * W), lse=(N * heads * L,),
                                                                   delta=(N * heads * L,)).items()}
    with H2Words() as h2:
        wq, wg = h2.of(d_qkv), h2.of(d_dout)
        q, g, o, dq, ls, dl = (t.data_ptr() for t in (d_qkv, d_dout, outs["out"], outs["dqkv"], outs["lse"], outs["delta"]))
        st = stream()
        good = dict(N=N, L=L, W=W, heads=heads, qkv=q, dout=g, out=o, wq=wq, wg=wg)
        bad = dict(W=dict(W=W + 64), L0=dict(L=0), N0=dict(N=0), L65=dict(L=65), qkv=dict(qkv=q + 4), dout=dict(dout=g + 4),
                   out=dict(out=o + 4), wq=dict(wq=None), wg=dict(wg=None))
        entry = {
            "tris_mha_fwd_f32": (lambda a: (a["qkv"], a["out"], a["N"], a["L"], a["W"], a["heads"], 0, st), ["W", "L0", "L65"]),
            "tris_mha_bwd_f32": (lambda a: (a["qkv"], a["dout"], dq, a["N"], a["L"], a["W"], a["heads"], 0, st), ["W", "L0", "L65"]),
            "tris_mha_mfma_fwd_f32": (lambda a: (a["qkv"], a["out"], ls, a["N"], a["L"], a["W"], a["heads"], 0, st), ["W", "L0", "N0", "qkv"]),
            "tris_mha_mfma_bwd_f32": (lambda a: (a["qkv"], a["out"], a["dout"], ls, dl, dq, a["N"], a["L"], a["W"], a["heads"], 0, st),
                                      ["W", "L0", "N0", "qkv", "dout", "out"]),
            "tris_mha_h2_fwd_f32": (lambda a: (a["qkv"], a["out"], ls, a["wq"], a["N"], a["L"], a["W"], a["heads"], 0, st),
                                    ["W", "L0", "N0", "qkv", "wq"]),
            "tris_mha_h2_bwd_f32": (lambda a: (a["qkv"], a["out"], a["dout"], ls, dl, dq, a["wq"], a["wg"], a["N"], a["L"], a["W"], a["heads"],
                                               0, st), ["W", "L0", "N0", "qkv", "dout", "out", "wq", "wg"]),
        }
        for name, (args, checks) in entry.items():
            for c in checks:
                rc = getattr(lib, name)(*args({**good, **bad[c]}))
                torch.cuda.synchronize()
                assert rc == INVALID, (name, c, rc)
                assert all(bool((t == SENT).all()) for t in outs.values()), (name, c, "an output was written")
        # (the same arguments without a defect are accepted: the table above tests the checks, not a typo in it)
        for name, (args, _) in entry.items():
            if "bwd" not in name:
                assert getattr(lib, name)(*args(good)) == 0, name
        for name, (args, _) in entry.items():
            if "bwd" in name:
                assert getattr(lib, name)(*args(good)) == 0, name
        torch.cuda.synchronize()


# ---- the record: python tests/test_gpu_mha.py > profiles/mha_parity_floor.txt on the MI355X ---------------------------------------
def rowwise(got, ref):
    """largest relative error of a query's 64 channels in the 2-norm, over the rows whose reference is at least 1e-6 of the largest
    row of their head (a causal first query's dq is zero up to the fp64 rounding of the reference)"""
    e = (got.double() - ref).view(*ref.shape[:-1], -1, O.HD).norm(dim=-1)
    n = ref.view(*ref.shape[:-1], -1, O.HD).norm(dim=-1)
    ok = (n > 0) & (n >= 1e-6 * n.amax((0, 1), keepdim=True))
    return float((e[ok] / n[ok]).max()) if bool(ok.any()) else 0.0


def main():
    print("# Self-attention kernels (csrc/attn.hip, attn_mfma.hip, attn_h2.hip) against fp64: the largest err / bound per implementation,")
    print("# output, input kind, L and mask, MI355X, N 2, heads 3 (heads 1 where marked).  The bounds are the element-wise ones derived in")
    print("# tests/oracle_mha.py; tests/test_gpu_mha.py asserts ratio <= 1.  h2_amax_x64: amax words 64 times too large.")
    print("# implementation | output | kind | L | causal | err / bound")
    top, rows = {}, []
    for impl in IMPLS:
        for kind in O.KINDS:
            for L, heads, causal in cases_of(impl):
                r, got = run_case(impl, kind, L, heads, causal)
                for name, v in r.items():
                    print(f"{impl:<11} | {name:<5} | {kind:<10} | {L}{' (1 head)' if heads == 1 else ''} | {causal} | {v:.3f}")
                    top[(impl, name)] = max(top.get((impl, name), 0.0), v)
                if heads == 3 and impl != "h2_amax_x64" and L in (17, 64, 129 if impl != "valu" else 63):
                    qkv, dout, ref, _ = O.case(kind, L, heads, causal)
                    aten = O.restate_fp32(qkv, dout, heads, causal)
                    for name in ("out", "dq", "dk", "dv"):
                        rows.append((impl, name, kind, L, causal, rowwise(got[name], ref[name]), rowwise(aten[name], ref[name])))
    print("#\n# largest ratio per implementation and output\n# implementation | output | err / bound")
    for (impl, name), v in top.items():
        print(f"{impl:<11} | {name:<5} | {v:.3f}")
    print("#\n# Reported, not asserted: the largest row-wise relative error (2-norm over a query's 64 channels of one head) beside ATen's")
    print("# fp32 evaluation of the same formulas on the CPU, same inputs.\n# implementation | output | kind | L | causal | err_hip | err_aten32")
    for impl, name, kind, L, causal, a, b in rows:
        print(f"{impl:<11} | {name:<5} | {kind:<10} | {L} | {causal} | {a:.3e} | {b:.3e}")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
