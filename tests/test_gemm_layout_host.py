"""The yardstick of tests/test_gpu_gemm_layout.py, checked without a GPU: the flat-index reference of tests/oracle_gemm_layout.py
against torch's own matmul on strided views of the same buffers (two independent statements of the header's addressing), the
poisoning, the window / outside partition, and the kernel class every case is predicted to reach -- pinned as plain data, so that a
change of the table cannot silently drain a class."""
from collections import Counter

import numpy as np
import pytest
import torch

import oracle_gemm_layout as G

CASES = G.cases()
BY_NAME = {c.name: c for c in CASES}

# predicted kernel class per case: <kernel>[+kv]/<epilogue> or <kernel>|slab><reduce kernel>/<its store>  (oracle_gemm_layout.predict)
PINNED = {
    "L0-130x68x96-NT": "fast/vec", "L0-200x136x64-NN": "fast/vec", "L0-64x64x32-TT": "fast/vec", "L0-100x48x100-TN": "fast+kv/vec",
    "L0-129x33x96-NT": "fast/scalar", "L0-7x5x27-NT": "generic", "L0-3x136x64-NT": "generic",
    "L0-200x136x4096-NT-ws4": "fast|slab>reduce4/vec", "L0-200x136x4096-NT-ws16": "fast|slab>wide/vec",
    "L0-132x33x4096-NT-ws16": "fast|slab>reduce1/scalar", "L0-64x64x4096-TN-ws16": "fast|slab>wide/vec",
    "L0-50x30x4100-NT-ws16": "generic|slab>reduce1/scalar",
    "L1-130x68x96-NT": "fast/vec", "L1-200x136x64-NN": "fast/vec", "L1-64x64x32-TT": "fast/vec", "L1-100x48x100-TN": "fast+kv/vec",
    "L1-129x33x96-NT": "fast/scalar", "L1-7x5x27-NT": "generic", "L1-3x136x64-NT": "generic",
    "L1-200x136x4096-NT-ws4": "fast|slab>reduce4/vec", "L1-200x136x4096-NT-ws16": "fast|slab>wide/vec",
    "L1-132x33x4096-NT-ws16": "fast|slab>reduce1/scalar", "L1-64x64x4096-TN-ws16": "fast|slab>wide/vec",
    "L1-50x30x4100-NT-ws16": "generic|slab>reduce1/scalar",
    "L2-130x68x96-NT": "generic", "L2-200x136x64-NN": "generic", "L2-64x64x32-TT": "generic", "L2-100x48x100-TN": "generic",
    "L2-129x33x96-NT": "generic", "L2-7x5x27-NT": "generic", "L2-3x136x64-NT": "generic",
    "L2-200x136x4096-NT-ws4": "generic|slab>reduce4/scalar", "L2-200x136x4096-NT-ws16": "generic|slab>wide/scalar",
    "L2-132x33x4096-NT-ws16": "generic|slab>reduce1/scalar", "L2-64x64x4096-TN-ws16": "generic|slab>wide/scalar",
    "L2-50x30x4100-NT-ws16": "generic|slab>reduce1/scalar",
    "L3-130x68x96-NT": "generic", "L3-200x136x64-NN": "generic", "L3-64x64x32-TT": "generic", "L3-100x48x100-TN": "generic",
    "L3-129x33x96-NT": "generic", "L3-7x5x27-NT": "generic", "L3-3x136x64-NT": "generic",
    "L3-200x136x4096-NT-ws4": "generic|slab>reduce1/scalar", "L3-200x136x4096-NT-ws16": "generic|slab>reduce1/scalar",
    "L3-132x33x4096-NT-ws16": "generic|slab>reduce1/scalar", "L3-64x64x4096-TN-ws16": "generic|slab>reduce1/scalar",
    "L3-50x30x4100-NT-ws16": "generic|slab>reduce1/scalar",
    "L4-130x68x96-NT": "fast/scalar", "L4-200x136x64-NN": "fast/scalar", "L4-64x64x32-TT": "fast/scalar",
    "L4-100x48x100-TN": "fast+kv/scalar", "L4-129x33x96-NT": "fast/scalar", "L4-7x5x27-NT": "generic", "L4-3x136x64-NT": "generic",
    "L4-200x136x4096-NT-ws4": "fast|slab>reduce4/scalar", "L4-200x136x4096-NT-ws16": "fast|slab>wide/scalar",
    "L4-132x33x4096-NT-ws16": "fast|slab>reduce1/scalar", "L4-64x64x4096-TN-ws16": "fast|slab>wide/scalar",
    "L4-50x30x4100-NT-ws16": "generic|slab>reduce1/scalar",
    "B3-100x64x64-NT-sharedA": "fast/vec", "B3-100x64x64-NT-sharedA-oddsCsR": "fast/scalar",
}

# the classes the GPU test exists for: each must keep at least two cases
REQUIRED = ["fast/vec", "fast/scalar", "generic", "fast+kv/vec", "fast|slab>reduce4/vec", "fast|slab>wide/vec",
            "fast|slab>reduce1/scalar", "generic|slab>reduce1/scalar"]
REQUIRED_PREFIX = ["fast+kv/", "generic|slab>", "|slab>reduce4/scalar", "|slab>wide/scalar", "|slab>reduce1/scalar"]


def test_every_case_reaches_its_pinned_class():
    assert sorted(PINNED) == sorted(BY_NAME)
    got = {c.name: G.predict(c) for c in CASES}
    assert got == PINNED, {k: (got[k], PINNED[k]) for k in got if got[k] != PINNED[k]}


def test_every_class_has_two_cases():
    count = Counter(PINNED.values())
    for cls in REQUIRED:
        assert count[cls] >= 2, (cls, count[cls])
    for part in REQUIRED_PREFIX:
        assert sum(v for k, v in count.items() if part in k) >= 2, part
    # odd leading dimensions and misaligned bases put EVERY product on the generic kernel's scalar loaders
    assert all(v.startswith("generic") for k, v in PINNED.items() if k[:2] in ("L2", "L3"))


def test_epilogue_options_rotate_through_every_layout():
    for lname in G.LAYOUTS:
        cs = [c for c in CASES if c.layout == lname and c.batch == 1]
        assert {c.bias_mode for c in cs} == {0, 1, 2}
        assert {c.act for c in cs} == {0, 1, 2}
        assert {c.resid for c in cs} == {False, True}
        assert {c.alpha for c in cs} == {1.0, 0.5}


def test_layouts_are_the_stated_ones():
    c = BY_NAME["L1-130x68x96-NT"]
    assert (c.lda, c.ldb, c.ldc, c.ldr) == (96 + 4, 96 + 8, 68 + 4, 68 + 8)
    c = BY_NAME["L2-200x136x64-NN"]
    assert (c.lda, c.ldb, c.ldc, c.ldr) == (64 + 1, 136 + 3, 136 + 1, 136 + 2)
    c = BY_NAME["L2-100x48x100-TN"]
    assert (c.lda, c.ldb) == (100 + 1, 48 + 3)
    c = BY_NAME["L4-64x64x32-TT"]
    assert (c.lda, c.ldb, c.ldc, c.ldr) == (64, 32, 65, 67) and c.mis == ("bias",)
    c = BY_NAME["L3-129x33x96-NT"]
    assert (c.lda, c.ldb, c.ldc, c.ldr) == (96, 96, 33, 33) and set(c.mis) == {"A", "B", "C", "resid"}
    b = BY_NAME["B3-100x64x64-NT-sharedA"]
    assert b.sA == 0 and b.sB == 64 * 64 + 8 and b.sC == 6400 + 12 and b.sR == 6400 + 4
    b = BY_NAME["B3-100x64x64-NT-sharedA-oddsCsR"]
    assert b.sC % 2 == 1 and b.sR % 2 == 1
    assert BY_NAME["L0-200x136x4096-NT-ws4"].ws_bytes() == 4 * 4 * 200 * 136


def _strided(buf, off, shape, strides):
    return torch.as_strided(torch.from_numpy(buf), shape, strides, off).double()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_reference_agrees_with_matmul_on_strided_views(case):
    bufs = G.lay_out(case, seed=11)
    ref64 = G.reference(case, bufs, torch.float64)
    ref32 = G.reference(case, bufs, torch.float32)
    off, (Bn, M, N, K) = bufs["off"], (case.batch, case.M, case.N, case.K)
    A = _strided(bufs["A"], off["A"], (Bn, M, K), (case.sA, 1, case.lda) if case.tA else (case.sA, case.lda, 1))
    B = _strided(bufs["B"], off["B"], (Bn, K, N), (case.sB, 1, case.ldb) if case.tB else (case.sB, case.ldb, 1))
    x = case.alpha * (A @ B)
    if case.bias_mode == 1:
        x = x + _strided(bufs["bias"], off["bias"], (N,), (1,))
    elif case.bias_mode == 2:
        x = x + _strided(bufs["bias"], off["bias"], (M,), (1,))[:, None]
    pre = x
    x = torch.relu(x) if case.act == 1 else x * torch.sigmoid(1.702 * x) if case.act == 2 else x
    if case.resid:
        x = x + _strided(bufs["resid"], off["resid"], (Bn, M, N), (case.sR, case.ldr, 1))
    scale = float(x.abs().max())
    assert torch.isfinite(ref64).all() and torch.isfinite(ref32).all()          # no NaN of the padding reaches the reference
    assert float((ref64 - x).abs().max()) <= 1e-12 * scale
    assert float((G.reference(case, bufs, torch.float64, pre_activation=True) - pre).abs().max()) <= 1e-12 * scale
    e32 = float((ref32.double() - ref64).abs().max())
    assert 0.0 < e32 < 1e-4 * scale                                                   # the yardstick is non-zero (and fp32-sized)


@pytest.mark.parametrize("case", [c for c in CASES if c.layout in ("L2", "L3") or c.batch > 1][::4], ids=repr)
def test_poison_surrounds_every_window(case):
    bufs = G.lay_out(case, seed=5)
    for name, idx in (("A", G.index_a(case)), ("B", G.index_b(case))) + ((("resid", G.index_r(case)),) if case.resid else ()) + \
            ((("bias", G.index_bias(case)),) if case.bias_mode else ()):
        buf = bufs[name]
        inside = np.zeros(buf.shape[0], bool)
        inside[idx.reshape(-1)] = True
        assert np.isfinite(buf[inside]).all() and np.isnan(buf[~inside]).all(), name
        assert idx.min() >= G.GUARD and buf.shape[0] - 1 - idx.max() >= G.GUARD, name
        assert (idx.min() % 4 == 1) == (name in case.mis), name
    assert (bufs["C"].view(np.uint32) == G.SENTINEL_BITS).all() and np.isfinite(G.sentinel())
    if case.slabs:
        assert np.isnan(bufs["ws"]).all() and bufs["ws"].shape[0] * 4 >= case.ws_bytes() + 4 * G.GUARD


@pytest.mark.parametrize("case", [BY_NAME["L2-129x33x96-NT"], BY_NAME["L3-7x5x27-NT"], BY_NAME["B3-100x64x64-NT-sharedA-oddsCsR"]], ids=repr)
def test_window_and_outside_partition_the_buffer(case):
    cbuf = np.arange(G.lay_out(case, seed=1)["C"].shape[0], dtype=np.float32)
    w, o = G.window(case, cbuf), G.outside(case, cbuf)
    assert w.shape == (case.batch, case.M, case.N)
    assert w.size + o.size == cbuf.size
    assert sorted(np.concatenate([w.reshape(-1), o]).tolist()) == cbuf.tolist()
    assert w[case.batch - 1, case.M - 1, case.N - 1] == G.GUARD + (1 if "C" in case.mis else 0) + (case.batch - 1) * case.sC + \
        (case.M - 1) * case.ldc + case.N - 1


def test_col_workspace_bytes_of_a_narrow_matrix():
    """tris_col_workspace_bytes is a host function and a caller sizes the workspace of tris_colsum_f32 with it for ANY width: for
    fewer than four columns it used to divide by zero (the process died with SIGFPE)"""
    from tris_amd import _lib
    for N in (1, 2, 3):
        assert _lib.query("tris_col_workspace_bytes", 4097, N) > 0
    assert _lib.query("tris_col_workspace_bytes", 4097, 4) == 3 * 2 * 4 * 8      # three partial rows of (sum, sum of squares) doubles


def test_colsum_table_and_reference():
    for N in G.COLSUM_N_VEC:
        assert [G.colsum_predict(N, f) for f in G.COLSUM_FORMS] == ["vector", "vector", "scalar", "scalar"]
    for N in G.COLSUM_N_SCALAR:
        assert {G.colsum_predict(N, f) for f in G.COLSUM_FORMS} == {"scalar"}
    for form in G.COLSUM_FORMS:
        buf, off, ld = G.colsum_lay_out(255, 12, form, seed=2)
        r64 = G.colsum_reference(buf, off, 255, 12, ld, torch.float64)
        view = torch.as_strided(torch.from_numpy(buf), (255, 12), (ld, 1), off).double()
        assert float((r64 - view.sum(0)).abs().max()) <= 1e-12 * float(r64.max()) and torch.isfinite(r64).all()
        assert float(r64.min()) > 100.0          # N(1, 1): the sums do not cancel
        assert np.isnan(buf).sum() == buf.shape[0] - 255 * 12
