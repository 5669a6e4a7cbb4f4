"""Launch trace of the dense-product dispatch (tris_amd/ops.py: gemm, h2_pp, LinearFn, LinearQGeluFn, MatmulFn, BmmFn, Conv3x3Fn).

`python tools/product_launch_trace.py` runs every case of CASES twice on the GPU and writes tests/golden/product_launch_trace.json:
case id -> {"calls": the entry-point calls of the case in issue order, "sha256": a digest of what the case computed, or null}.
tests/test_gpu_product_dispatch.py runs the same cases and compares with that file.  The file is made from the code whose behaviour is
to be kept; a refactor never regenerates it.  The hand-offs between a Bottleneck's BatchNorms and its products are the cases of
tools/bn_launch_trace.py and are not repeated here.

Calls are stored as tools/bn_launch_trace.py stores them (its docstring), with one addition: where include/tris_hip.h declares the last
parameter of an entry point as `void* stream`, that position holds the STREAM the call went to -- 0 for the stream current when the case
began, 1, 2, ... for other streams in order of first appearance in the case (weight gradients and bias column sums go to a side stream).

Pointers are only null / non-null in the trace, which cannot tell P(w) from P(cl_weight(w)) or an activation from its byte mask.  So
every case also leaves a sha256 over the bytes of its forward output, its input gradients and its parameter gradients (arena views
included), read after wgrad_join and a synchronize.  A case whose digest does not repeat between the two runs on the recording code
itself is stored without one (null) and compared by its calls alone.

Every case is a batch of 2 and a step of its own, in h2 with operand planes unless it says otherwise, with the autotuner off and the
switches of tris_amd.config that the family reads pinned to their defaults, whatever the environment says."""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "product_launch_trace.json")

import torch  # noqa: E402

from tools.bn_launch_trace import DEFAULTS as BN_DEFAULTS, _classify, _step, recording  # noqa: E402

DEFAULTS = dict(BN_DEFAULTS, mlp_fuse=True, wgrad_stream=True, text_pack=True, mha="auto", mha_h2=True)


def _streamed():
    """names of the entry points whose last parameter is `void* stream`"""
    from tris_amd._lib import HEADER
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {m.group(1) for m in re.finditer(r"\b(?:int|long)\s+(tris_\w+)\s*\(([^)]*)\)\s*;", src)
            if re.search(r"void\s*\*\s*stream\s*$", m.group(2).strip())}


def _classifier(base):
    """_classify, with the stream position as the index of the stream (0: `base`, the raw handle current when the case began)"""
    streamed, seen = _streamed(), {base or 0: 0}

    def classify(name, args):
        out = _classify(name, args)
        if name in streamed:
            out[-1] = seen.setdefault(args[-1] or 0, len(seen))
        return out
    return classify


# ------------------------------------------------------------------------------------------------------------------ the cases
# A case returns (output, inputs, parameters): what its digest is taken over -- the output, then .grad of the inputs and parameters
def _leaf(*shape, seed, scale=1.0):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return (scale * torch.randn(*shape, device="cuda", generator=gen)).requires_grad_()


def _param(*shape, seed, scale=0.1, sunk=False):
    p = torch.nn.Parameter(_leaf(*shape, seed=seed, scale=scale).detach())
    return _sink(p) if sunk else p


def _sink(p):
    """the parameter's gradient goes straight into its (arena) view (tools/bn_launch_trace.py case_linked)"""
    p.grad = torch.zeros_like(p)
    p._tris_sink = True
    return p


def _run(ops, fwd, inputs=(), params=(), backward=True):
    got = []

    def keep():
        got.append(fwd())
        return got[0]
    if backward:
        _step(ops, keep)
    else:
        with torch.no_grad():
            _step(ops, keep, backward=False)
    return got[0], inputs, params


def _block(sunk=False):
    from tris_amd.CLIP.clip.model import ResidualAttentionBlock
    torch.manual_seed(31)
    net = ResidualAttentionBlock(64, 1, attn_mask=True).cuda().train()      # (the attention kernels serve heads of 64 channels)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    if sunk:
        for p in net.parameters():
            _sink(p)
    return net


def _ids():
    """two sentences of 4 and 7 tokens (start ... end, the end token being the largest id) in rows of 8"""
    ids = torch.zeros(2, 8, dtype=torch.int64)
    ids[0, :4] = torch.tensor([49406, 320, 1125, 49407])
    ids[1, :7] = torch.tensor([49406, 320, 1125, 539, 518, 2368, 49407])
    return ids.cuda()


def case_block_train(ops, sunk=False):
    net, x = _block(sunk), _leaf(2, 8, 64, seed=32)
    return _run(ops, lambda: net(x), [x], list(net.parameters()))


def case_block_eval(ops, how):
    net = _block()
    if how == "packed":
        ids, x = _ids(), _leaf(ops.packed_rows(2, 8), 64, seed=33).detach()

        def fwd():
            plan = ops.text_pack_plan(ids)
            with ops.rows_limit(plan):
                return net.forward_packed(x, plan, 2, 8)[:11]      # (the rows in use: the ones behind them are never written)
        return _run(ops, fwd, backward=False)
    x = _leaf(2, 8, 64, seed=33).detach()
    return _run(ops, (lambda: net.forward_token0(x)) if how == "token0" else (lambda: net(x)), backward=False)


def case_text_proj(ops):
    """tris_amd/model/attn.py forward_cl: three ReLU projections of one `lan`, their data gradients chained through GradBoxes"""
    lan = _leaf(2, 3, 64, seed=41)
    w = [_param(64, 64, seed=42 + i) for i in range(3)]
    b = [_param(64, seed=45 + i) for i in range(3)]
    t1, t2 = ops.GradBox(), ops.GradBox()

    def fwd():
        q = ops.linear(lan, w[0], b[0], None, 1, grad_box=t1)
        k = ops.linear(lan, w[1], b[1], None, 1, grad_box=t2, grad_box_out=t1)
        v = ops.linear(lan, w[2], b[2], None, 1, grad_box=None, grad_box_out=t2)
        return q + k + v
    return _run(ops, fwd, [lan], w + b)


def case_matmul(ops, tB, sunk):
    A, B = _leaf(2, 3, 64, seed=51), _param(*((32, 64) if tB else (64, 32)), seed=52, sunk=sunk)
    return _run(ops, lambda: ops.matmul(A, B, tB), [A], [B])


def case_bmm(ops, tB, shared):
    A = _leaf(3, 64, seed=53) if shared else _leaf(2, 3, 64, seed=53)
    B = _leaf(*((2, 32, 64) if tB else (2, 64, 32)), seed=54)
    return _run(ops, lambda: ops.bmm(A, B, tB, 0.5), [A, B])


def _conv_w(cout, cin, seed):
    return _param(cout, cin, 3, 3, seed=seed).detach().contiguous(memory_format=torch.channels_last).requires_grad_()


def case_batch_invariant(ops, what):
    """what: a matmul of 1, 3 (padded to four rows) or 4 rows, a conv3x3 or a linear, inside ops.batch_invariant()"""
    if what == "conv3x3":
        x, w = _leaf(2, 16, 16, 32, seed=61).detach(), _conv_w(32, 32, 62).detach()
        fwd = lambda: ops.conv3x3(x, w, 1)
    elif what == "linear":
        x, w, b = _leaf(2, 3, 64, seed=61).detach(), _param(32, 64, seed=62), _param(32, seed=63)
        fwd = lambda: ops.linear(x, w, b)
    else:
        A, B = _leaf(what, 64, seed=61).detach(), _leaf(64, 32, seed=62, scale=0.1).detach()
        fwd = lambda: ops.matmul(A, B)

    def scoped():
        with ops.batch_invariant():
            return fwd()
    return _run(ops, scoped, backward=False)


def case_conv_stem(ops):
    """stride 2 from 3 channels with the statistics epilogue; the image needs no gradient"""
    x, w = _leaf(2, 16, 16, 3, seed=71).detach(), _conv_w(32, 3, 72)
    return _run(ops, lambda: ops.conv3x3(x, w, 2, stats=True), [], [w])


def case_conv(ops, shape, stats):
    B, H, W, Cin, Cout = shape
    x, w = _leaf(B, H, W, Cin, seed=73), _conv_w(Cout, Cin, 74)
    return _run(ops, lambda: ops.conv3x3(x, w, 1, stats=stats), [x], [w])


def case_gemm_blind(ops):
    """ops.gemm under ops.rows_limit with an operand of the caller's own that carries no amax word (_rows_limit_blind)"""
    ids = _ids()
    A, B = _leaf(256, 64, seed=81).detach(), _leaf(32, 64, seed=82, scale=0.1).detach()
    C = torch.zeros(256, 32, device="cuda")

    def fwd():
        plan = ops.text_pack_plan(ids)
        with ops.rows_limit(plan):
            return ops.gemm(A, B, C, 256, 32, 64, 64, 64, 32, False, True)
    return _run(ops, fwd, backward=False)


def case_gemm_convert(ops):
    """cfg.gemm_convert: a frozen tower's Linear whose weight is marked as the ViT's are; 128 rows of 64"""
    x, w, b = _leaf(2, 64, 64, seed=91).detach(), _param(64, 64, seed=92), _param(64, seed=93)
    w._tris_linear_w = True
    return _run(ops, lambda: ops.linear(x, w, b), backward=False)


def case_fuse_splitk(ops):
    """cfg.fuse_splitk: 512 rows, K 4096 -> 128 (a product the static cost model splits along K), with its backward"""
    x, w, b = _leaf(2, 256, 4096, seed=94), _param(128, 4096, seed=95, scale=0.02), _param(128, seed=96)
    return _run(ops, lambda: ops.linear(x, w, b), [x], [w, b])


CONV, CONV_ODD = (2, 16, 16, 32, 32), (2, 10, 10, 64, 64)    # (CONV_ODD: 200 pixels, a weight-gradient reduction that is no multiple of 32)

# case id -> (cfg switches off the defaults, arithmetic, function, arguments)
CASES = {
    "block": ({}, "h2", case_block_train, ()),
    "block-no-mlp-fuse": ({"mlp_fuse": False}, "h2", case_block_train, ()),
    "block-no-grad-box": ({"grad_box": False}, "h2", case_block_train, ()),
    "block-sunk": ({}, "h2", case_block_train, (True,)),
    "block-sunk-no-side-param-grads": ({"side_param_grads": False}, "h2", case_block_train, (True,)),
    "block-no-side-param-grads": ({"side_param_grads": False}, "h2", case_block_train, ()),
    "block-x3": ({}, "x3", case_block_train, ()),
    "block-no-planes": ({"h2_planes": False}, "h2", case_block_train, ()),
    "block-eval": ({}, "h2", case_block_eval, ("forward",)),
    "block-eval-token0": ({}, "h2", case_block_eval, ("token0",)),
    "block-eval-packed": ({}, "h2", case_block_eval, ("packed",)),
    "text-proj": ({}, "h2", case_text_proj, ()),
    "matmul": ({}, "h2", case_matmul, (False, False)),
    "matmul-tb": ({}, "h2", case_matmul, (True, False)),
    "matmul-sunk": ({}, "h2", case_matmul, (False, True)),
    "matmul-tb-sunk": ({}, "h2", case_matmul, (True, True)),
    "bmm": ({}, "h2", case_bmm, (False, False)),
    "bmm-tb": ({}, "h2", case_bmm, (True, False)),
    "bmm-shared": ({}, "h2", case_bmm, (False, True)),
    "bmm-tb-shared": ({}, "h2", case_bmm, (True, True)),
    "invariant-matmul-m1": ({}, "h2", case_batch_invariant, (1,)),
    "invariant-matmul-m3": ({}, "h2", case_batch_invariant, (3,)),
    "invariant-matmul-m4": ({}, "h2", case_batch_invariant, (4,)),
    "invariant-conv3x3": ({}, "h2", case_batch_invariant, ("conv3x3",)),
    "invariant-linear": ({}, "h2", case_batch_invariant, ("linear",)),
    "conv-stem": ({}, "h2", case_conv_stem, ()),
    "conv": ({}, "h2", case_conv, (CONV, False)),
    "conv-stats": ({}, "h2", case_conv, (CONV, True)),
    "conv-x3": ({}, "x3", case_conv, (CONV, False)),
    "conv-stats-x3": ({}, "x3", case_conv, (CONV, True)),
    "conv-no-planes": ({"h2_planes": False}, "h2", case_conv, (CONV, False)),
    "conv-stats-no-planes": ({"h2_planes": False}, "h2", case_conv, (CONV, True)),
    "conv-odd-pixels": ({}, "h2", case_conv, (CONV_ODD, False)),
    "gemm-rows-limit-blind": ({}, "h2", case_gemm_blind, ()),
    "gemm-convert": ({"gemm_convert": 1}, "h2", case_gemm_convert, ()),
    "fuse-splitk": ({"fuse_splitk": True}, "h2", case_fuse_splitk, ()),
}


def _digest(out, inputs, params):
    h = hashlib.sha256()
    for t in [out] + [t.grad for t in list(inputs) + list(params)]:
        h.update(b"none" if t is None else t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def run_case(cid):
    """-> (the classified calls of case `cid`, the digest of what it computed)"""
    from tris_amd import ops
    from tris_amd.config import cfg
    switches, arith, fn, args = CASES[cid]
    prev, calls = ops.get_gemm_mode(), []
    ops.set_gemm_mode(arith)
    ops.set_autotune(False)
    arenas, ops._H2_ARENAS[:] = ops._H2_ARENAS[:], []     # (an optimiser somebody else left alive adds its per-step launches to every step)
    try:
        with cfg.override(**dict(DEFAULTS, **switches)), recording(calls, _classifier(ops._stream())):
            res = fn(ops, *args)
    finally:
        ops._H2_ARENAS[:] = arenas
        ops.set_autotune(os.environ.get("TRIS_AUTOTUNE", "1")[:1] != "0")    # (the library's own reading of the environment)
        ops.set_gemm_mode(prev)
        torch.cuda.synchronize()
    assert ops.pl_word(res[0]) is None, cid
    return calls, _digest(*res)


def main(out=FIXTURE):
    lines, loose = [], []
    for cid in CASES:
        (calls, d1), (again, d2) = run_case(cid), run_case(cid)
        assert calls == again, f"{cid}: the calls of two runs on the same code differ"
        if d1 != d2:
            loose.append(cid)
        lines.append(f"{json.dumps(cid)}: {json.dumps({'calls': calls, 'sha256': d1 if d1 == d2 else None})}")
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")
    print(f"{out}: {len(lines)} cases, digests that did not repeat: {loose or 'none'}")


if __name__ == "__main__":
    main(*sys.argv[1:2])
