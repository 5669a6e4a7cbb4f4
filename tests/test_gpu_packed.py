"""Kernel-level tests of the packed text rows (tris_amd/csrc/attn.hip "packed text rows") and of the row limit they put on the dense
products and the LayerNorm forward (tris_rows_limit_thread): the plan exactly, the gather kernels bit for bit, the attention against
fp64 and against the padded kernel, every arithmetic / tile / split-K form of the product under a limit with NaN behind it, and the
frozen text tower packed against padded -- eager, poisoned and replayed from a hipGraph across a changing limit.

The tests print the worst figure they met (pytest -s): error / bound for the attention, error / largest reference magnitude for the
products and the tower."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from tris_amd.config import cfg as CFG

gpu = pytest.mark.gpu

SENT = -7777.25          # sentinel of the buffers the tests own: a kernel that writes where it must not changes it
EOT, SOT = 49407, 49406
U = 2.0 ** -24           # unit round-off of fp32
TOL = 2e-4               # products against fp64: tests/test_gpu_ops.py::test_gemm_autotune_every_candidate_and_the_cached_choice
TOWER_TOL = 2e-5         # packed against padded: tests/test_gpu_parity.py::test_packed_text_pass_equals_the_padded_pass


def ceil256(x):
    return (x + 255) // 256 * 256


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- 1. the plan -----------------------------------------------------------------------------------------------------------------
def plan_reference(ids):
    """include/tris_hip.h "packed text rows": [0] rows in use P, [1] P rounded up to 256, [2 + n] first row of sentence n (n = 0 .. N),
    then the source token n L + l of every packed row, -1 from P to R - 1 (R = N L rounded up to 256).  A sentence ends at its largest
    id, first occurrence."""
    ids = np.asarray(ids)
    N, L = ids.shape
    R = ceil256(N * L)
    lens = np.argmax(ids, axis=1) + 1
    first = np.concatenate([[0], np.cumsum(lens)])
    P = int(first[-1])
    plan = np.empty(3 + N + R, dtype=np.int32)
    plan[0], plan[1] = P, ceil256(P)
    plan[2:3 + N] = first
    rows = np.full(R, -1, dtype=np.int32)
    for n in range(N):
        rows[first[n]:first[n + 1]] = n * L + np.arange(lens[n])
    plan[3 + N:] = rows
    return plan


def ids_from_lengths(lens, L, seed=0, junk=False):
    """[len(lens), L] token ids: SOT, words, EOT at position len - 1, zeros (junk: ids below EOT) behind it"""
    rng = np.random.RandomState(seed)
    ids = np.zeros((len(lens), L), dtype=np.int64)
    for n, l in enumerate(lens):
        ids[n, :l - 1] = rng.randint(1, 40000, l - 1)
        if l > 1:
            ids[n, 0] = SOT
        ids[n, l - 1] = EOT
        if junk:
            ids[n, l:] = rng.randint(1, EOT, L - l)
    return ids


@functools.lru_cache(maxsize=None)
def plan_cases():
    rng = np.random.RandomState(3)
    c = {
        "1x1": ids_from_lengths([1], 1),
        "1x20": ids_from_lengths([11], 20),
        "3x2 SOT EOT": ids_from_lengths([2, 2, 2], 2),
        "7x20 ragged": ids_from_lengths([1, 2, 20, 7, 13, 5, 19], 20),
        "257x20": ids_from_lengths(list(rng.randint(1, 21, 257)), 20, seed=1),
        "300x5": ids_from_lengths(list(rng.randint(1, 6, 300)), 5, seed=2),
        "13x64": ids_from_lengths([1, 64, 2, 33, 7, 63, 20, 1, 50, 64, 3, 17, 41], 64, seed=3),
        "64x64 full": ids_from_lengths([64] * 64, 64, seed=4),                 # P = 4096 = R
        "32x20 len 8": ids_from_lengths([8] * 32, 20, seed=5),                 # P = 256 < R = 768
        "32x20 len 8, one 9": ids_from_lengths([8] * 17 + [9] + [8] * 14, 20, seed=6),   # P = 257, plan[1] = 512
        "junk behind EOT": ids_from_lengths([1, 2, 20, 7, 13, 5, 19], 20, seed=7, junk=True),
    }
    eq = ids_from_lengths([5, 9, 3, 20], 20, seed=8)
    eq[2, :] = 777                                                              # a row of all-equal ids: its length is 1
    c["all-equal row"] = eq
    return c


PLAN_SHAPES = {"1x1": (1, 1), "1x20": (1, 20), "3x2 SOT EOT": (3, 2), "7x20 ragged": (7, 20), "257x20": (257, 20), "300x5": (300, 5),
               "13x64": (13, 64), "64x64 full": (64, 64), "32x20 len 8": (32, 20), "32x20 len 8, one 9": (32, 20),
               "junk behind EOT": (7, 20), "all-equal row": (4, 20)}


def test_plan_reference_invariants():
    """the helper itself: plan[2 + N] = P, the row map is a bijection onto the kept tokens, plan[1] <= R, the listed extents"""
    cases = plan_cases()
    assert set(cases) == set(PLAN_SHAPES)
    for name, ids in cases.items():
        N, L = ids.shape
        assert (N, L) == PLAN_SHAPES[name]
        R = ceil256(N * L)
        plan = plan_reference(ids)
        P = int(plan[0])
        assert plan.shape == (3 + N + R,) and plan[2] == 0 and plan[2 + N] == P, name
        assert plan[1] % 256 == 0 and P <= plan[1] < P + 256 and plan[1] <= R, name
        rows = plan[3 + N:]
        assert (rows[P:] == -1).all() and (rows[:P] >= 0).all(), name
        kept = sorted(n * L + l for n in range(N) for l in range(int(np.argmax(ids[n])) + 1))
        assert sorted(rows[:P].tolist()) == kept and len(set(rows[:P].tolist())) == P, name
        assert (np.diff(plan[2:3 + N]) >= 1).all(), name
    P_of = lambda k: int(plan_reference(cases[k])[0])
    assert P_of("64x64 full") == 4096 and P_of("32x20 len 8") == 256 and P_of("3x2 SOT EOT") == 6
    assert tuple(plan_reference(cases["32x20 len 8, one 9"])[:2]) == (257, 512)
    assert plan_reference(cases["all-equal row"])[2:7].tolist() == [0, 5, 14, 15, 35]
    assert np.array_equal(plan_reference(cases["junk behind EOT"])[:10], plan_reference(ids_from_lengths([1, 2, 20, 7, 13, 5, 19], 20))[:10])


@gpu
@pytest.mark.parametrize("case", sorted(PLAN_SHAPES))
def test_text_pack_plan_is_the_reference_plan(case):
    """tris_text_pack_plan_i64 == plan_reference, every word: one sentence, one token, sentence loops past the 256 threads, P on the
    256-row granule and one past it, P = R, ties, junk behind EOT"""
    from tris_amd import ops as O
    ids = plan_cases()[case]
    got = O.text_pack_plan(torch.from_numpy(ids).cuda()).cpu()
    assert torch.equal(got, torch.from_numpy(plan_reference(ids))), case


# ---- 2. embed_packed, eot_gather_packed ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("W", [64, 512, 768])
@pytest.mark.parametrize("case", ["7x20 ragged", "32x20 len 8", "32x20 len 8, one 9", "64x64 full", "all-equal row"])
def test_embed_packed_and_eot_gather_packed_exactly(case, W):
    """rows < P: tok[id] + pos[l] in fp32 (one rounding: bit for bit); P .. plan[1] - 1: zero; >= plan[1]: never written.  The gather
    returns each sentence's last row (a one-token sentence; the last sentence: row P - 1).  Plans with plan[1] < R ("32x20 ..."),
    plan[1] = R ("7x20", "64x64 full") and P on the granule ("32x20 len 8", "64x64 full")."""
    from tris_amd._lib import call
    V = 1024
    ids = plan_cases()[case]
    ids = np.where(ids == EOT, V - 1, ids % (V - 1))     # (a small table: the plan only sees the order of the ids)
    N, L = ids.shape
    R = ceil256(N * L)
    ref_plan = plan_reference(ids)
    P, P2 = int(ref_plan[0]), int(ref_plan[1])
    g = torch.Generator().manual_seed(W + N)
    tok, pos = torch.randn(V, W, generator=g), torch.randn(L, W, generator=g) * 0.3
    d_ids, d_tok, d_pos = torch.from_numpy(ids).cuda(), tok.cuda(), pos.cuda()
    plan = torch.full((3 + N + R,), -5, dtype=torch.int32, device="cuda")
    call("tris_text_pack_plan_i64", d_ids.data_ptr(), N, L, plan.data_ptr(), stream())
    assert torch.equal(plan.cpu(), torch.from_numpy(ref_plan))
    out = torch.full((R, W), SENT, device="cuda")
    call("tris_embed_packed_fwd_f32", d_ids.data_ptr(), d_tok.data_ptr(), d_pos.data_ptr(), plan.data_ptr(), out.data_ptr(), N, L, W,
         stream())
    src = torch.from_numpy(ref_plan[3 + N:3 + N + P].astype(np.int64))
    want = tok[torch.from_numpy(ids).reshape(-1)[src]] + pos[src % L]
    got = out.cpu()
    assert torch.equal(got[:P], want)
    assert bool((got[P:P2] == 0).all()) and bool((got[P2:] == SENT).all())
    last = torch.from_numpy(ref_plan[3:3 + N].astype(np.int64)) - 1
    assert int(last[-1]) == P - 1
    eot = torch.full((N, W), SENT, device="cuda")
    call("tris_eot_gather_packed_f32", out.data_ptr(), plan.data_ptr(), eot.data_ptr(), N, W, stream())
    assert torch.equal(eot.cpu(), got[last])


# ---- 3. mha_packed ---------------------------------------------------------------------------------------------------------------
MHA_SETS = {20: [(5, [1, 2, 20, 7, 13]),                                   # R = 256 = plan[1]
                 (40, [1, 2, 20, 5, 7, 3, 6, 4] * 5),                      # R = 1024, P = 240: plan[1] = 256
                 (40, [1, 2, 20, 13, 17, 9, 11, 15] * 5)],                 # R = 1024, P = 440: plan[1] = 512
            64: [(5, [1, 2, 64, 33, 7])]}                                  # R = 512, P = 107: plan[1] = 256; 68 864 B of dynamic LDS
MHA_CASES = [(1, 20), (8, 20), (12, 64), (2, 64)]


def attention(x, heads, causal):
    """one sentence x [L, 3 W] (q | k | v, heads of 64) in x's own precision -> out [L, W], and in fp64 the issue's bound
    (2 ds_i + (2 L + 8) u) sum_j p_ij |v_jd|,  ds_i = 66 u max_j (sum_d |q_id| |k_jd|) / 8:
    64 products and the scale multiply, doubled by the exponential; the sum, the division and the PV sum."""
    L, W = x.shape[0], x.shape[1] // 3
    q, k, v = (x[:, i * W:(i + 1) * W].reshape(L, heads, 64).transpose(0, 1) for i in range(3))
    s = (q @ k.transpose(1, 2)) * 0.125
    sa = q.abs() @ k.abs().transpose(1, 2)
    if causal:
        keep = torch.ones(L, L, dtype=torch.bool).tril()
        s, sa = s.masked_fill(~keep, float("-inf")), sa.masked_fill(~keep, 0.0)
    p = torch.softmax(s, -1)
    out = (p @ v).transpose(0, 1).reshape(L, W)
    ds = 66 * U * sa.max(-1).values / 8
    bound = ((2 * ds[..., None] + (2 * L + 8) * U) * (p @ v.abs())).transpose(0, 1).reshape(L, W)
    return out, bound


@functools.lru_cache(maxsize=None)
def mha_inputs(heads, Lmax, causal, which):
    """-> ids, lens, qkv [R, 3 W] fp32 (NaN from row P on), the fp64 result [P, W], its bound [P, W]; built once per case"""
    N, lens = MHA_SETS[Lmax][which]
    assert len(lens) == N and max(lens) == Lmax and {1, 2} <= set(lens)
    W, R, P = heads * 64, ceil256(N * Lmax), sum(lens)
    gain = (1.0, 3.0)[(heads + which) % 2]
    g = torch.Generator().manual_seed(heads * 100 + Lmax + which)
    qkv = torch.randn(R, 3 * W, generator=g) * gain
    qkv[P:] = float("nan")
    ref, bound, r0 = [], [], 0
    for l in lens:
        o, b = attention(qkv[r0:r0 + l].double(), heads, causal)
        ref.append(o)
        bound.append(b)
        r0 += l
    return ids_from_lengths(lens, Lmax, seed=which), lens, qkv, torch.cat(ref), torch.cat(bound)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("heads,Lmax", MHA_CASES)
def test_attention_bound_holds_for_the_plain_fp32_restatement(heads, Lmax, causal):
    """a bound the plain reference breaks is a wrong bound: torch's fp32 evaluation of the same formula, at the inputs the GPU test uses"""
    worst = 0.0
    for which in range(len(MHA_SETS[Lmax])):
        _, lens, qkv, ref, bound = mha_inputs(heads, Lmax, causal, which)
        r0 = 0
        for l in lens:
            o, _ = attention(qkv[r0:r0 + l], heads, causal)
            worst = max(worst, float(((o.double() - ref[r0:r0 + l]).abs() / bound[r0:r0 + l]).max()))
            r0 += l
    print(f"fp32 restatement, heads {heads} Lmax {Lmax} causal {causal}: worst |err| / bound = {worst:.4f}")
    assert worst <= 1.0


@gpu
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("heads,Lmax", MHA_CASES)
def test_mha_packed_against_fp64_and_the_padded_kernel(heads, Lmax, causal):
    """tris_mha_packed_fwd_f32 on buffers the test owns: every sentence within the bound of its fp64 attention although the qkv rows
    from P on are NaN (no sentence may read them); rows P .. plan[1] - 1 of out zero, rows >= plan[1] untouched; two launches give the
    same bits; and sentence n's rows are BIT FOR BIT ops.mha (the LDS-resident kernel, cfg.mha = "valu") of that sentence alone -- the
    two kernels perform the same operations in the same order."""
    from tris_amd import ops as O
    from tris_amd._lib import call
    W = heads * 64
    worst = 0.0
    for which in range(len(MHA_SETS[Lmax])):
        ids, lens, qkv, ref, bound = mha_inputs(heads, Lmax, causal, which)
        N, R, P = len(lens), qkv.shape[0], sum(lens)
        plan = O.text_pack_plan(torch.from_numpy(ids).cuda())
        ref_plan = plan_reference(ids)
        assert torch.equal(plan.cpu(), torch.from_numpy(ref_plan))
        P2 = int(ref_plan[1])
        d_qkv = qkv.cuda()
        outs = []
        for _ in range(2):
            out = torch.full((R, W), SENT, device="cuda")
            call("tris_mha_packed_fwd_f32", d_qkv.data_ptr(), out.data_ptr(), plan.data_ptr(), N, Lmax, W, heads, int(causal), stream())
            outs.append(out)
        assert torch.equal(outs[0], outs[1])
        got = outs[0].cpu()
        assert bool(torch.isfinite(got).all())
        ratio = float(((got[:P].double() - ref).abs() / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (which, ratio)
        assert bool((got[P:P2] == 0).all()) and bool((got[P2:] == SENT).all()), which
        with torch.no_grad(), CFG.override(mha="valu"):
            r0 = 0
            for n, l in enumerate(lens):
                alone = O.mha(d_qkv[r0:r0 + l][None], heads, causal)[0]
                assert torch.equal(alone, outs[0][r0:r0 + l]), (which, n, l)
                r0 += l
    print(f"mha_packed, heads {heads} Lmax {Lmax} causal {causal}: worst |err| / bound = {worst:.4f}")


# ---- 4. the row limit on the dense products and the LayerNorm forward ------------------------------------------------------------
_VARIANT = {"x3-classic": ("FORCE_PIPE", 0), "h2-pipe": ("PIPE", 1)}


@pytest.fixture(scope="module", params=["x3", "x3-classic", "h2", "h2-pipe", "f32"])
def ops(request):
    """the three arithmetics of the dense-product core, x3 and h2 under both loop structures (tests/test_gpu_ops.py's fixture)"""
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
    """(the per-test option reset of conftest.py would drop the module-scoped fixture's option: put it back.)  The product tests run
    the cost model's choice (no autotuning) and start on a fresh amax pool, so that no h2 tag is lost to a pool restart mid-test."""
    if "ops" in request.fixturenames:
        from tris_amd import _lib, ops as o
        v = _VARIANT.get(request.node.callspec.params.get("ops"))
        if v is not None:
            o.set_option(*v)
        was = _lib.load().tris_get_autotune()
        o.set_autotune(False)
        o.h2_begin_step()
        o.h2_end_step()
        yield
        o.set_autotune(bool(was))
    else:
        yield


def limit_word(limit, rows=None):
    """what ops.rows_limit reads: an int32 device array whose word 1 is the limit (word 0: rows in use)"""
    return torch.tensor([limit if rows is None else rows, limit], dtype=torch.int32, device="cuda")


@contextlib.contextmanager
def limited(o, limit):
    """ops.rows_limit(limit) for the scope (None: no limit); the device word stays alive until the scope ends"""
    if limit is None:
        yield
        return
    word = limit_word(limit)
    with o.rows_limit(word):
        yield
    del word


@functools.lru_cache(maxsize=None)
def product_data(M, N, K):
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K)
    d = {"A": torch.randn(M, K, generator=g), "B": torch.randn(N, K, generator=g) * 0.05, "bias": torch.randn(N, generator=g),
         "R": torch.randn(M, N, generator=g), "X": torch.randn(M, min(K, 512), generator=g) * 2 + 0.5,
         "g": 1 + 0.1 * torch.randn(min(K, 512), generator=g), "b": 0.1 * torch.randn(min(K, 512), generator=g),
         "up": torch.randn(K, 512, generator=g) * 0.05 if K > 512 else None}
    return {k: (None if v is None else v.cuda()) for k, v in d.items()}


def nan_tail(t, limit):
    t = t.clone()
    t[limit:] = float("nan")
    return t


def operand_a(o, d, M, K, limit, under_limit):
    """The A operand of a product under `limit`.  x3 / f32: random rows, NaN from the limit on.  h2: A must carry the amax word a
    real pass would give it -- taken over the rows in use only -- so it is PRODUCED under the same limit from an X whose rows behind
    the limit are NaN: by ops.layer_norm, and for K > 1024 (the LayerNorm kernel's width limit; the text tower's K = 2048 operand
    is c_fc's output) by a QuickGELU product of that LayerNorm's output, as in the block.  The unlimited twin (under_limit False)
    repeats rows 0 .. limit - 1 behind the limit: the same values, so the same amax and the same operand scale."""
    lim = min(limit, M)
    if not o.h2_on():
        return nan_tail(d["A"], lim) if under_limit else d["A"]
    X = d["X"].clone()
    if under_limit:
        X[lim:] = float("nan")
    else:
        X[lim:] = X[torch.arange(lim, M, device="cuda") % lim]
    with limited(o, limit if under_limit else None), torch.no_grad():
        A = o.layer_norm(X, d["g"], d["b"])
        if K > 512:
            h, A = A, torch.full((M, K), float("nan"), device="cuda")
            o.gemm(h, d["up"], A, M, K, 512, 512, 512, K, False, True, act=2)
    assert o._h2_tag_slot(A) is not None       # (the product below runs in h2, not in the x3 of an untagged operand)
    return A


WORST = {}


def check_product(o, M, N, K, limit, resid, act, tag=""):
    """one product under `limit` against the same call without one and against fp64; returns the limited C"""
    d = product_data(M, N, K)
    lim = min(limit, M)
    out = {}
    for under in (False, True):
        A = operand_a(o, d, M, K, limit, under)
        R = None if not resid else (nan_tail(d["R"], lim) if under else d["R"])
        C = torch.full((M, N), float("nan"), device="cuda")
        with limited(o, limit if under else None):
            o.gemm(A, d["B"], C, M, N, K, K, K, N, False, True, bias=d["bias"], bias_mode=1, resid=R, ldr=N, act=act)
        out[under] = (A, C)
    A, C = out[True]
    assert torch.equal(C[:lim], out[False][1][:lim]), (tag, limit)
    assert bool(torch.isnan(C[lim:]).all()), (tag, limit, "rows behind the limit were written")
    ref = A[:lim].double().cpu() @ d["B"].double().cpu().t() + d["bias"].double().cpu()
    if act == 2:
        ref = ref * torch.sigmoid(1.702 * ref)
    if resid:
        ref = ref + d["R"][:lim].double().cpu()
    got = C[:lim].cpu()
    assert bool(torch.isfinite(got).all()), (tag, limit)
    rel = float((got.double() - ref).abs().max() / ref.abs().max())
    WORST[o.get_gemm_mode()] = max(WORST.get(o.get_gemm_mode(), 0.0), rel)
    print(f"product {tag} M{M} N{N} K{K} limit {limit} [{o.get_gemm_mode()}]: max err / max |ref| = {rel:.3e}")
    assert rel <= TOL, (tag, limit, rel)
    return C


@gpu
@pytest.mark.parametrize("M,N,K,resid,act,limits", [(1024, 1536, 512, False, 0, (256, 768, 1024)),
                                                    (1024, 512, 512, True, 0, (256, 768, 1024)),
                                                    (1024, 2048, 512, False, 2, (256, 768, 1024)),
                                                    (1024, 512, 2048, True, 0, (256, 768, 1024)),
                                                    (512, 128, 4096, False, 0, (256, 768, 1024)),
                                                    (300, 512, 512, False, 0, (512,))])
def test_products_under_a_row_limit(ops, M, N, K, resid, act, limits):
    """The text tower's products (row-major A x W^T + bias, M = 1024: in_proj, out_proj + residual, c_fc + QuickGELU, c_proj + residual),
    a long-K product and a limit beyond M, with C pre-filled with NaN and A / the residual NaN behind the limit: rows below the limit
    are bit for bit the unlimited call's and within 2e-4 of the fp64 product's largest magnitude, rows behind it are never written.

    What heuristic_cfg chooses (no autotuning) for the c_proj product M 1024, N 512, K 2048: K < 4096, so the cost model runs over
    tiles x slices {1, 2, 3, 4, 6}; its minimum is the 64 x 64 tile with TWO K slices in every arithmetic (x3 / h2: 45.5 k model
    cycles against 47.3 k for 128 x 64 in four slices; f32: 60.5 k against 60.8 k) -- 256 workgroups and the one-thread-per-four-
    columns reduce (splitk_reduce_kernel<4>: fewer than 8 slices).  The long-K product M 512, N 128, K 4096 takes the long-K branch:
    128 x 128 tiles, 4 tiles, min(512 / 4, 4096 / 256) = 16 slices, and -- 16 >= 8 slices of a 512 x 128 output -- the wide reduce."""
    for limit in limits:
        check_product(ops, M, N, K, limit, resid, act)
    print(f"worst so far {WORST}")


@gpu
@pytest.mark.parametrize("tile", ["128x128", "128x64", "64x64", "256x128"])
def test_every_tile_under_a_row_limit(ops, tile):
    """each tile shape forced on the in_proj product at limit 256 (the 256-row tile exists in the pipelined loop only: elsewhere
    run_cfg turns it into 128 rows)"""
    with ops.option("FORCE_TILE", tile):
        check_product(ops, 1024, 1536, 512, 256, False, 0, tag=tile)


@gpu
def test_both_splitk_reduce_kernels_under_a_row_limit(ops):
    """run_cfg sums the slabs with splitk_reduce_wide_kernel when `(N & 3) == 0 && splitk >= 8 && M N / 4 < 128 * 256` (aligned
    buffers, option REDUCE_WIDE != 0), else with splitk_reduce_kernel.  The long-K product (16 slices, M N / 4 = 16 384) meets it; the
    c_proj product (2 slices) does not; and with REDUCE_WIDE = 0 the long-K product goes through the other kernel as well -- its 16
    slabs are then summed in another order, so its bits differ from the wide kernel's, which shows that both ran."""
    check_product(ops, 1024, 512, 2048, 256, True, 0, tag="narrow")
    wide = check_product(ops, 512, 128, 4096, 256, False, 0, tag="wide")
    with ops.option("REDUCE_WIDE", 0):
        narrow = check_product(ops, 512, 128, 4096, 256, False, 0, tag="REDUCE_WIDE=0")
    assert not torch.equal(wide[:256], narrow[:256])


def fused_splitk_under_a_limit(o, M, N, K, limit):
    from tris_amd import _lib
    d = product_data(M, N, K)
    A = operand_a(o, d, M, K, limit, True)
    R = nan_tail(d["R"], limit)
    out, took = {}, {}
    for fused in (True, False):
        o.set_option("FUSE_SPLITK", None if fused else "0")
        n0 = _lib.query("tris_splitk_fused_launches")
        C = torch.full((M, N), float("nan"), device="cuda")
        with CFG.override(fuse_splitk=True), limited(o, limit):
            o.gemm(A, d["B"], C, M, N, K, K, K, N, False, True, bias=d["bias"], bias_mode=1, resid=R, ldr=N, act=2)
        torch.cuda.synchronize()
        took[fused] = _lib.query("tris_splitk_fused_launches") - n0
        out[fused] = C
    o.set_option("FUSE_SPLITK", None)
    print(f"fused split-K M{M} N{N} K{K} limit {limit}: fused launches {took}")
    assert torch.equal(out[True][:limit], out[False][:limit])
    assert bool(torch.isnan(out[True][limit:]).all()) and bool(torch.isfinite(out[True][:limit]).all())
    assert int(o.splitk_tickets().abs().sum()) == 0          # tiles that left took no ticket
    return took


@gpu
def test_fused_splitk_finish_under_a_row_limit_long_k_shape(ops):
    """The long-K product M 512, N 128, K 4096 armed with a ticket array (cfg.fuse_splitk) under limit 256: 16 slices of a small output,
    the class whose separate reduce launch is splitk_reduce_wide_kernel.  The fused finish sums the slabs in that kernel's order
    (GemmParams.fin_groups), so the result is the two-launch form's bit for bit; nothing is written behind the limit, the tickets are
    zero afterwards (tiles that left took none) and the launch counter advances by one."""
    took = fused_splitk_under_a_limit(ops, 512, 128, 4096, 256)
    assert took == {True: 1, False: 0}, took


@gpu
@pytest.mark.parametrize("limit", [768, 2048])
def test_fused_splitk_finish_under_a_row_limit(ops, limit):
    """M 2048, N 512, K 4096 (128 x 128 tiles, 64 of them, 8 slices: tests/test_gpu_ops.py's fused shape) under a limit: tiles behind
    the limit leave before they take a ticket; the counter advances, the bits are the reduce launch's, the tickets return to zero"""
    took = fused_splitk_under_a_limit(ops, 2048, 512, 4096, limit)
    assert took == {True: 1, False: 0}, took


@gpu
def test_transposed_and_batched_products_ignore_the_limit(ops):
    """the documented exceptions: under a live limit a transA product and a batch = 3 product compute every row"""
    g = torch.Generator().manual_seed(21)
    M, N, K = 512, 192, 256
    At, A3 = torch.randn(K, M, generator=g), torch.randn(3, M, K, generator=g)
    B, B3 = torch.randn(N, K, generator=g) * 0.1, torch.randn(3, N, K, generator=g) * 0.1
    dAt, dA3, dB, dB3 = At.cuda(), A3.cuda(), B.cuda(), B3.cuda()
    with limited(ops, 256):
        C = torch.full((M, N), float("nan"), device="cuda")
        ops.gemm(dAt, dB, C, M, N, K, M, K, N, True, True)
        Cb = torch.full((3, M, N), float("nan"), device="cuda")
        ops.gemm(dA3, dB3, Cb, M, N, K, K, K, N, False, True, batch=3, sA=M * K, sB=N * K, sC=M * N)
    for got, ref in ((C, At.double().t() @ B.double().t()), (Cb, A3.double() @ B3.double().transpose(1, 2))):
        got = got.cpu()
        assert bool(torch.isfinite(got).all())
        assert float((got.double() - ref).abs().max()) <= TOL * float(ref.abs().max())


@gpu
def test_the_limit_is_cleared_on_exit(ops):
    """after the `with` block -- left normally or by an exception -- the same call writes every row again"""
    d = product_data(1024, 512, 512)
    if ops.h2_on():
        assert ops._h2_amax(d["A"]) is not None      # (h2: A carries a word of this step, as every operand of the packed pass does)

    def run():
        C = torch.full((1024, 512), float("nan"), device="cuda")
        ops.gemm(d["A"], d["B"], C, 1024, 512, 512, 512, 512, 512, False, True, bias=d["bias"], bias_mode=1)
        return C
    full = run()
    assert bool(torch.isfinite(full).all())
    with limited(ops, 256):
        part = run()
    assert torch.equal(part[:256], full[:256]) and bool(torch.isnan(part[256:]).all())
    assert torch.equal(run(), full)
    with pytest.raises(ZeroDivisionError):
        with limited(ops, 256):
            1 / 0
    assert torch.equal(run(), full)


@gpu
@pytest.mark.parametrize("W", [512, 768])
def test_layernorm_forward_under_a_row_limit(W):
    """raw tris_layernorm_fwd_f32 with Y, mean and rstd owned by the test, X NaN behind the limit: rows below the limit are the
    unlimited launch's bits, everything behind it is untouched"""
    from tris_amd import ops as O
    from tris_amd._lib import call
    rows = 1024
    g = torch.Generator().manual_seed(W)
    X = (torch.randn(rows, W, generator=g) * 3 + 1).cuda()
    gam, bet = (1 + 0.1 * torch.randn(W, generator=g)).cuda(), (0.1 * torch.randn(W, generator=g)).cuda()

    def run(x, limit):
        Y, mean, rstd = (torch.full(s, SENT, device="cuda") for s in ((rows, W), (rows,), (rows,)))
        with limited(O, limit):
            call("tris_layernorm_fwd_f32", x.data_ptr(), gam.data_ptr(), bet.data_ptr(), Y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                 rows, W, 1e-5, stream())
        return Y, mean, rstd
    full = run(X, None)
    assert all(bool(torch.isfinite(t).all()) for t in full)
    for limit in (256, 768, 1024):
        got = run(nan_tail(X, limit), limit)
        for a, b in zip(got, full):
            assert torch.equal(a[:limit], b[:limit]), limit
            assert bool((a[limit:] == SENT).all()), limit


@gpu
def test_untagged_operand_under_a_row_limit_gets_no_amax_prepass():
    """h2: an A operand WITHOUT an amax word of the live step must not get the pre-pass of ops._h2_amax under a live limit --
    tris_amax_bits_f32 over all of A reads the rows behind the limit, here NaN, into the scale of the rows in use (measured without
    the guard in ops.gemm: max err / max |ref| = 0.78).  ops.gemm runs such a product in x3: finite, within tolerance, nothing
    written behind the limit, and its output carries a word again.  The packed tower pass itself never brings such an operand
    (last test of this file); a caller of ops.gemm with an operand of its own can."""
    from tris_amd import ops as O
    prev = O.get_gemm_mode()
    O.set_gemm_mode("h2")
    try:
        O.h2_begin_step()
        O.h2_end_step()
        M, N, K, limit = 1024, 512, 512, 256
        d = product_data(M, N, K)
        A = nan_tail(d["A"], limit)
        assert O._h2_tag_slot(A) is None
        C = torch.full((M, N), float("nan"), device="cuda")
        with limited(O, limit):
            O.gemm(A, d["B"], C, M, N, K, K, K, N, False, True, bias=d["bias"], bias_mode=1)
        ref = d["A"][:limit].double().cpu() @ d["B"].double().cpu().t() + d["bias"].double().cpu()
        got = C[:limit].cpu()
        assert bool(torch.isfinite(got).all()) and bool(torch.isnan(C[limit:]).all())
        rel = float((got.double() - ref).abs().max() / ref.abs().max())
        print(f"untagged A under a limit: max err / max |ref| = {rel:.3e}")
        assert rel <= TOL
        assert O._h2_tag_slot(C) is not None
    finally:
        O.set_gemm_mode(prev)


# ---- 5. the tower ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def aux():
    import warnings
    from tris_amd.CLIP import clip
    from tris_amd.train_stage1 import freeze_aux
    from tris_amd.utils.synth import seed_fill
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, _ = clip.load("ViT-B-32", device="cuda", txt_length=20)
    seed_fill(a.state_dict(), 4321)
    return freeze_aux(a)


@pytest.fixture(params=["x3", "h2"])
def arith(request):
    from tris_amd import ops as O
    prev = O.get_gemm_mode()
    O.set_gemm_mode(request.param)
    O.h2_begin_step()        # (a fresh amax pool: no restart in the middle of a pass, so two passes take the same arithmetic)
    O.h2_end_step()
    yield request.param
    O.set_gemm_mode(prev)


TN, TL, TR, TW = 26, 20, 768, 512
LENS_A = [2, 3, 4, 5, 6, 7, 8, 9] * 3 + [2, 9]                      # P = 143: plan[1] = 256
LENS_B = [20] * 22 + [19, 19, 19, 18]                               # P = 515: plan[1] = 768 = R


def tower_ids():
    a, b = ids_from_lengths(LENS_A, TL, seed=11), ids_from_lengths(LENS_B, TL, seed=12)
    assert tuple(plan_reference(a)[:2]) == (143, 256) and tuple(plan_reference(b)[:2]) == (515, 768) and ceil256(TN * TL) == TR
    return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()


def padded(aux, ids):
    with CFG.override(text_pack=False):
        return aux.encode_text_hidden(ids)


def rel_err(got, ref):
    return float((got - ref).abs().max()) / float(ref.abs().max())


def poison():
    """NaN-filled tensors of the packed buffers' sizes, freed again: the caching allocator hands these blocks to the pass's
    torch.empty.  Best effort -- returns whether a fresh torch.empty((R, W)) came back NaN."""
    junk = [torch.full((TR, w), float("nan"), device="cuda") for w in (TW, 3 * TW, 4 * TW) for _ in range(6)]
    torch.cuda.synchronize()
    del junk
    probe = torch.empty((TR, TW), device="cuda")
    hit = bool(torch.isnan(probe).all())
    del probe
    return hit


@gpu
def test_tower_packed_equals_padded_at_both_limits(aux, arith):
    """encode_text_hidden packed against cfg.text_pack = False for short sentences (plan[1] = 256 of R = 768 rows) and long ones
    (plan[1] = R); with NaN planted in the memory the packed buffers are about to get, the result is the unpoisoned one bit for bit"""
    with torch.no_grad():
        for name, ids in zip("AB", tower_ids()):
            ref = padded(aux, ids)
            got = aux.encode_text_hidden(ids)
            rel = rel_err(got, ref)
            hit = poison()
            again = aux.encode_text_hidden(ids)
            print(f"tower [{arith}] set {name}: packed vs padded max err / max |ref| = {rel:.3e}; poisoned torch.empty came back NaN: {hit}")
            assert bool(torch.isfinite(got).all()) and rel <= TOWER_TOL, (name, rel)
            assert torch.equal(again, got), name


@gpu
def test_tower_graph_replay_across_a_changing_limit(aux, arith):
    """GraphedFrozenText replays follow the ids' own limit (the plan is rebuilt on the device inside the graph): recorded on full-length
    sentences (the class's default), on set A (limit 256) and on set B (limit 768 = R), every replay stays within the tolerance of its
    own padded reference, and A after a B replay is the first A bit for bit"""
    from tris_amd.graphs import GraphedFrozenText
    A, B = tower_ids()
    with torch.no_grad():
        refA, refB = padded(aux, A), padded(aux, B)
        worst = 0.0
        for rec in (None, A, B):
            g = GraphedFrozenText(aux, TN, TL, ids=rec)
            a0, b0, a1 = g(A), g(B), g(A)
            torch.cuda.synchronize()
            for got, ref in ((a0, refA), (b0, refB), (a1, refA)):
                assert bool(torch.isfinite(got).all())
                worst = max(worst, rel_err(got, ref))
                assert rel_err(got, ref) <= TOWER_TOL
            assert torch.equal(a1, a0)
    print(f"tower graph replay [{arith}]: worst max err / max |ref| = {worst:.3e}")


@gpu
def test_tower_survives_an_amax_pool_restart_inside_the_packed_pass(aux):
    """h2, eager: with fewer words left in the per-step pool (4096) than the packed pass takes under its limit (7 per block + 1 = 85),
    the pool restarts inside the pass -- ops._h2_slot never hands the main pool's caller None -- and every tag written before is void.
    No A operand is caught by that: each is written and tagged by the launch right before the product that reads it, and the
    restart happens while that product's OUTPUT is marked, after A's word was looked up.  So no amax pre-pass runs over rows behind
    the limit (NaN is planted there), and the pass equals the padded one.  (The captured passes own a private pool of 512 words,
    cleared in the capture: it is never full, and a full private pool hands out None to the pre-pass as well.)"""
    from tris_amd import ops as O
    prev = O.get_gemm_mode()
    O.set_gemm_mode("h2")
    try:
        A, _ = tower_ids()
        with torch.no_grad():
            ref = padded(aux, A)
            O.h2_begin_step()
            O.h2_end_step()
            while O._H2.next < O.H2_SLOTS - 40:
                O._h2_slot()
            step = O._H2.step
            hit = poison()
            got = aux.encode_text_hidden(A)
            assert O._H2.step != step          # (the pool did restart inside the pass)
            rel = rel_err(got, ref)
            print(f"pool restart inside the packed pass: max err / max |ref| = {rel:.3e}; poisoned torch.empty came back NaN: {hit}")
            assert bool(torch.isfinite(got).all()) and rel <= TOWER_TOL
    finally:
        O.set_gemm_mode(prev)
