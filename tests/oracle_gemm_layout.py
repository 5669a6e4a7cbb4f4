"""Reference of tris_gemm_f32 / tris_colsum_f32 on NON-PACKED operands, written from include/tris_hip.h and not from the kernels.

The header promises, for every batch b,

    C[b] = act(alpha * opA(A[b]) . opB(B[b]) + bias) + resid[b]
    opA: transA=0 -> A[m*lda+k], 1 -> A[k*lda+m];  opB: transB=0 -> B[k*ldb+n], 1 -> B[n*ldb+k]
    bias_mode 1: bias[n], 2: bias[m];  act 0 none, 1 ReLU, 2 QuickGELU x*sigmoid(1.702x)

with its own leading dimension for C (ldc) and for the residual (ldr) and batch strides sA / sB / sC / sR.  `lay_out` places every
operand of a case inside a larger flat fp32 buffer -- guards in front and behind, rows `ld` apart, batches a stride apart, the
window optionally one float past a 16-byte boundary -- and poisons everything that is not a logical element: NaN around A, B, bias
and resid, one fixed finite bit pattern everywhere in C, NaN in the split-K workspace.  `reference` evaluates the formula by
explicit flat indexing (index tensors built from m*lda+k, never a view), in fp64 and in fp32 on the CPU.  A kernel that reads one
element past a row or a buffer multiplies a NaN in; one that writes outside the M x N x batch window changes a sentinel.

`predict` restates, from the header-level predicates alone (alignment, leading dimensions modulo 4, the shape rules of the fast
kernel and of the split-K choice), which kernel class serves a case; tests/test_gemm_layout_host.py pins the outcome per case."""
import numpy as np
import torch

GUARD = 64                       # floats in front of and behind every window (a multiple of 4: the window keeps the base's alignment)
SENTINEL_BITS = 0x42F6E979       # 123.456..: what C (and pre_out) hold wherever the product must not write
NAN_BITS = 0x7FC00000


def sentinel():
    return np.array([SENTINEL_BITS], np.uint32).view(np.float32)[0]


# ---- layouts: additions to the packed leading dimensions (lda, ldb, ldc, ldr) and which windows start one float past a boundary ----
LAYOUTS = {
    "L0": dict(add=(0, 0, 0, 0), mis=()),                          # packed: control
    "L1": dict(add=(4, 8, 4, 8), mis=()),                          # padded, every 16-byte path kept
    "L2": dict(add=(1, 3, 1, 2), mis=()),                          # odd leading dimensions: scalar loaders, generic kernel, scalar epilogue
    "L3": dict(add=(0, 0, 0, 0), mis=("A", "B", "C", "resid")),    # packed widths, misaligned bases
    "L4": dict(add=(0, 0, 1, 3), mis=("bias",)),                   # A, B aligned and packed; odd output side only: fast kernel, scalar epilogue
}

# (M, N, K, transA, transB): the smallest products that still reach each branch
PRODUCTS = [
    (130, 68, 96, 0, 1),
    (200, 136, 64, 0, 0),
    (64, 64, 32, 1, 1),
    (100, 48, 100, 1, 0),      # both operands k-major, K % 32 != 0: the fast kernel over K rounded up to 128 (rows past K read as zero)
    (129, 33, 96, 0, 1),       # N % 4 != 0
    (7, 5, 27, 0, 1),          # generic kernel: K % 32 != 0
    (3, 136, 64, 0, 1),        # generic kernel: M < 4
]
# split-K (K >= 4096 with a caller-owned workspace): (M, N, K, transA, transB, slabs the workspace has room for)
SPLIT_PRODUCTS = [
    (200, 136, 4096, 0, 1, 4),     # splitk_reduce_kernel<4>
    (200, 136, 4096, 0, 1, 16),    # the wide reduce
    (132, 33, 4096, 0, 1, 16),     # splitk_reduce_kernel<1>
    (64, 64, 4096, 1, 0, 16),
    (50, 30, 4100, 0, 1, 16),      # the generic kernel, split
]


class Case:
    def __init__(self, name, M, N, K, tA, tB, layout, batch=1, slabs=0, bias_mode=0, act=0, resid=False, alpha=1.0,
                 shared_a=False, gaps=(0, 0, 0, 0)):
        self.name, self.M, self.N, self.K, self.tA, self.tB, self.layout = name, M, N, K, int(tA), int(tB), layout
        self.batch, self.slabs, self.bias_mode, self.act, self.resid, self.alpha = batch, slabs, bias_mode, act, bool(resid), alpha
        add = LAYOUTS[layout]["add"]
        self.mis = LAYOUTS[layout]["mis"]
        self.lda = (M if tA else K) + add[0]
        self.ldb = (K if tB else N) + add[1]
        self.ldc = N + add[2]
        self.ldr = N + add[3]
        rows_a, rows_b = (K if tA else M), (N if tB else K)
        # batch strides: the extent of one matrix plus the case's gap; shared_a: every batch reads the same A (stride 0)
        self.sA = 0 if (shared_a or batch == 1) else rows_a * self.lda + gaps[0]
        self.sB = 0 if batch == 1 else rows_b * self.ldb + gaps[1]
        self.sC = 0 if batch == 1 else M * self.ldc + gaps[2]
        self.sR = 0 if batch == 1 else M * self.ldr + gaps[3]

    def __repr__(self):
        return self.name

    def ws_bytes(self):
        return self.slabs * 4 * self.M * self.N


def cases():
    """the table of tests/test_gpu_gemm_layout.py: every product under every layout, the epilogue options rotated so that every
    value of each appears under every layout, plus the batched product (shared A, gaps between the batches; once with odd sC / sR)"""
    out = []
    for li, lname in enumerate(LAYOUTS):
        prods = [p + (0,) for p in PRODUCTS] + list(SPLIT_PRODUCTS)
        for pi, (M, N, K, tA, tB, slabs) in enumerate(prods):
            out.append(Case(f"{lname}-{M}x{N}x{K}-{'T' if tA else 'N'}{'T' if tB else 'N'}" + (f"-ws{slabs}" if slabs else ""),
                            M, N, K, tA, tB, lname, slabs=slabs, bias_mode=pi % 3, act=(pi // 3 + li) % 3, resid=(pi + li) % 2 == 0,
                            alpha=1.0 if (pi // 2 + li) % 2 == 0 else 0.5))
    out.append(Case("B3-100x64x64-NT-sharedA", 100, 64, 64, 0, 1, "L0", batch=3, bias_mode=1, act=2, resid=True, alpha=0.5,
                    shared_a=True, gaps=(0, 8, 12, 4)))
    out.append(Case("B3-100x64x64-NT-sharedA-oddsCsR", 100, 64, 64, 0, 1, "L0", batch=3, bias_mode=2, act=1, resid=True, alpha=1.0,
                    shared_a=True, gaps=(0, 8, 5, 7)))
    return out


# ---- flat indices of the logical elements (the header's formulas, nothing else) ------------------------------------------------
def _off(case, which):
    return GUARD + (1 if which in case.mis else 0)


def index_a(case):
    b, m, k = np.meshgrid(np.arange(case.batch), np.arange(case.M), np.arange(case.K), indexing="ij")
    return _off(case, "A") + b * case.sA + (k * case.lda + m if case.tA else m * case.lda + k)


def index_b(case):
    b, k, n = np.meshgrid(np.arange(case.batch), np.arange(case.K), np.arange(case.N), indexing="ij")
    return _off(case, "B") + b * case.sB + (n * case.ldb + k if case.tB else k * case.ldb + n)


def index_c(case):
    b, m, n = np.meshgrid(np.arange(case.batch), np.arange(case.M), np.arange(case.N), indexing="ij")
    return _off(case, "C") + b * case.sC + m * case.ldc + n


def index_r(case):
    b, m, n = np.meshgrid(np.arange(case.batch), np.arange(case.M), np.arange(case.N), indexing="ij")
    return _off(case, "resid") + b * case.sR + m * case.ldr + n


def index_bias(case):
    return _off(case, "bias") + np.arange(case.N if case.bias_mode == 1 else case.M)


def _poisoned(idx, values, fill_bits=NAN_BITS):
    """a flat fp32 buffer: GUARD floats (at least) on either side of the window that `idx` spans, `values` at idx, poison elsewhere"""
    n = int(idx.max()) + 1 + GUARD
    n += (-n) % 4
    buf = np.full(n, fill_bits, np.uint32).view(np.float32)
    if values is not None:
        buf[idx.reshape(-1)] = values.reshape(-1)
    return buf


def lay_out(case, seed):
    """-> dict of flat fp32 numpy buffers A, B, C, (bias), (resid), (ws) and the offsets (in floats) at which the windows start.
    Operands: A ~ N(0, 1), B ~ N(0, 0.1) (inside fp16's range: the h2 arithmetic runs with unit scales), bias, resid ~ N(0, 1)."""
    g = np.random.default_rng(seed)
    ia, ib = index_a(case), index_b(case)
    # a shared A (stride 0) is ONE matrix: draw it once (the indices of every batch coincide)
    va = g.standard_normal(ia[:1].shape if case.sA == 0 else ia.shape).astype(np.float32)
    bufs = {"A": _poisoned(ia[:1] if case.sA == 0 else ia, va),
            "B": _poisoned(ib, (0.1 * g.standard_normal(ib.shape)).astype(np.float32)),
            "C": _poisoned(index_c(case), None, SENTINEL_BITS)}
    if case.bias_mode:
        ibias = index_bias(case)
        bufs["bias"] = _poisoned(ibias, g.standard_normal(ibias.shape).astype(np.float32))
    if case.resid:
        ir = index_r(case)
        bufs["resid"] = _poisoned(ir, g.standard_normal(ir.shape).astype(np.float32))
    if case.slabs:
        bufs["ws"] = np.full(case.slabs * case.M * case.N + GUARD, NAN_BITS, np.uint32).view(np.float32)
    bufs["off"] = {w: _off(case, w) for w in ("A", "B", "C", "bias", "resid")}
    return bufs


def _act(x, act):
    if act == 1:
        return torch.clamp_min(x, 0)
    if act == 2:
        return x / (1 + torch.exp(-torch.tensor(1.702, dtype=x.dtype) * x))
    return x


def reference(case, bufs, dtype, pre_activation=False):
    """the header's formula on the gathered elements, every step in `dtype` (torch.float64 | torch.float32) on the CPU -> [batch, M, N];
    pre_activation: the value BEFORE the activation and the residual (what tris_gemm_epilogue_next's pre_out receives)"""
    A = torch.from_numpy(bufs["A"])[torch.from_numpy(index_a(case))].to(dtype)        # [batch, M, K]
    B = torch.from_numpy(bufs["B"])[torch.from_numpy(index_b(case))].to(dtype)        # [batch, K, N]
    x = torch.matmul(A, B) * torch.tensor(case.alpha, dtype=dtype)
    if case.bias_mode:
        bias = torch.from_numpy(bufs["bias"])[torch.from_numpy(index_bias(case))].to(dtype)
        x = x + (bias[None, None, :] if case.bias_mode == 1 else bias[None, :, None])
    if pre_activation:
        return x
    x = _act(x, case.act)
    if case.resid:
        x = x + torch.from_numpy(bufs["resid"])[torch.from_numpy(index_r(case))].to(dtype)
    return x


def window(case, cbuf):
    """the M x N x batch window of a C buffer (flat numpy fp32) -> [batch, M, N]"""
    return cbuf[index_c(case)]


def outside(case, cbuf):
    """every element of a C buffer that is not in the window (flat)"""
    keep = np.ones(cbuf.shape[0], bool)
    keep[index_c(case).reshape(-1)] = False
    return cbuf[keep]


# ---- which kernel class serves a case: the header-level predicates only -----------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def predict(case, armed=False):
    """-> e.g. 'fast/vec', 'fast/scalar', 'generic', 'fast+kv/vec', 'fast|slab>reduce4/vec', 'generic|slab>reduce1/scalar'.
    Alignment of a window = alignment of its offset (every buffer's base is 16-byte aligned)."""
    al = lambda w: _off(case, w) % 4 == 0
    M, N, K = case.M, case.N, case.K
    vec_a = al("A") and case.lda % 4 == 0 and case.sA % 4 == 0
    vec_b = al("B") and case.ldb % 4 == 0 and case.sB % 4 == 0
    fast_a = vec_a and (not case.tA or M % 4 == 0)
    fast_b = vec_b and (case.tB or N % 4 == 0)
    kv = bool(case.tA and not case.tB and K % 32 != 0 and K > 32 and fast_a and fast_b and M >= 4 and N >= 4 and not armed)
    if kv:
        K = (K + 31) // 32 * 32
    fast = fast_a and fast_b and K % 32 == 0 and M >= 4 and N >= 4
    head = ("fast" if fast else "generic") + ("+kv" if kv else "")
    splitk = 1
    if case.batch == 1 and case.slabs and K >= 4096 and not armed:
        bm = bn = 64
        if N <= 64:
            bm = 128 if M >= 128 else 64
        elif M >= 128 and N >= 128:
            bm = bn = 128
        splitk = min(_cdiv(512, _cdiv(M, bm) * _cdiv(N, bn)), K // 256, case.ws_bytes() // (4 * M * N))
        if splitk >= 2:
            kalign = 32 if fast else 16
            splitk = _cdiv(K, _cdiv(_cdiv(K, splitk), kalign) * kalign)
        else:
            splitk = 1
    res_ok = not case.resid or (al("resid") and case.ldr % 4 == 0)
    if splitk > 1:     # (the workspace is 16-byte aligned: the caller's choice)
        if N % 4 == 0 and al("C"):
            red = "wide" if (splitk >= 8 and M * N // 4 < 128 * 256) else "reduce4"
            return f"{head}|slab>{red}/{'vec' if case.ldc % 4 == 0 else 'scalar'}"
        return f"{head}|slab>reduce1/scalar"
    if not fast:
        return head        # (the generic kernel has one, scalar, epilogue)
    vec_c = (N % 4 == 0 and al("C") and case.ldc % 4 == 0 and case.sC % 4 == 0 and res_ok and (not case.resid or case.sR % 4 == 0)
             and (case.bias_mode != 1 or al("bias")))
    return f"{head}/{'vec' if vec_c else 'scalar'}"


def fused_finish_applies(case):
    """may tris_splitk_tickets_next fold the reduce of this split-K case into the product's launch?  (fast kernel, at most 16 slices;
    where the wide reduce would run, only with the vector form of the finish)"""
    p = predict(case)
    if not p.startswith("fast") or "|slab>" not in p:
        return False
    al = lambda w: _off(case, w) % 4 == 0
    vec_fin = (case.N % 4 == 0 and al("C") and case.ldc % 4 == 0 and (not case.resid or (al("resid") and case.ldr % 4 == 0))
               and (case.bias_mode != 1 or al("bias")))
    return ">wide" not in p or vec_fin


# ---- column sums ------------------------------------------------------------------------------------------------------------------
COLSUM_M = [1, 255, 2500, 4097]           # 2500: more than one partial row of the vector kernel at every N below (checked on the GPU)
COLSUM_N_VEC = [4, 12, 68, 1028]
COLSUM_N_SCALAR = [1, 7, 33]
COLSUM_FORMS = ["packed", "ld+4", "ld+1", "misaligned"]


def colsum_lay_out(M, N, form, seed):
    """X ~ N(1, 1) (the sums do not cancel) as M rows `ld` apart inside a NaN buffer -> (buffer, offset, ld)"""
    ld = N + (4 if form == "ld+4" else 1 if form == "ld+1" else 0)
    off = GUARD + (1 if form == "misaligned" else 0)
    g = np.random.default_rng(seed)
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    idx = off + m * ld + n
    return _poisoned(idx, (1.0 + g.standard_normal(idx.shape)).astype(np.float32)), off, ld


def colsum_reference(buf, off, M, N, ld, dtype):
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    return torch.from_numpy(buf)[torch.from_numpy(off + m * ld + n)].to(dtype).sum(0)


def colsum_predict(N, form):
    """'vector' (fp64 partials, 16-byte loads) or 'scalar' (one thread per column)"""
    ld = N + (4 if form == "ld+4" else 1 if form == "ld+1" else 0)
    return "scalar" if (N % 4 or ld % 4 or form == "misaligned") else "vector"
