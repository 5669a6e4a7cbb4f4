"""Launch trace of the h2 step lifecycle (tris_amd/ops.py: the amax pool, its steps, private and retired pools, the constant words, the
arenas' per-step launches and the plane tags).

`python tools/h2_step_trace.py` runs every case of CASES twice on the GPU and writes tests/golden/h2_step_trace.json: case id ->
{"calls": the entry-point calls of the case in issue order, "sha256": a digest of what the case computed, or null}.
tests/test_gpu_h2_step.py runs the same cases and compares with that file.  The file is made from the code whose behaviour is to be
kept; a refactor never regenerates it.

Calls are stored as tools/bn_launch_trace.py stores them (its docstring), with one addition: a pointer that lies inside an amax pool is
stored as the WORD it names -- ["pool", i] in the pool of the running step, ["retired", k, i] in the k-th youngest retired pool,
["private", i] in a private pool (the step's own pool is still "pool" inside the region) and ["const", i] among the constant words,
with i = (address - base of that pool) // (4 * H2_SUB) and the bases read from ops.h2_pool_state() as the call is made.  Between the
calls a case leaves rows ["#state", next, base, step changed since the last row, retired pools]: what the tests of the pool observe.

Every case is a batch of 2, in h2 with operand planes, with the autotuner off, no optimiser arena but its own, an empty pool of constant
words and the switches of tris_amd.config pinned as tools/product_launch_trace.py pins them, whatever the environment says; it begins
behind an empty explicit step (next == base == 0, nothing retired)."""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "h2_step_trace.json")

import torch  # noqa: E402

from tools.bn_launch_trace import _classify, recording  # noqa: E402
from tools.product_launch_trace import DEFAULTS  # noqa: E402


class _Trace:
    """the classifier of one case and its "#state" rows"""

    def __init__(self, ops):
        self.ops, self.calls, self.main, self.step = ops, [], None, ops.h2_pool_state()["step"]

    def classify(self, name, args):
        from tris_amd._lib import DECLS
        ops, out, s = self.ops, _classify(name, args), self.ops.h2_pool_state()
        if not s["private"]:
            self.main = s["pool"]
        pools = [(["private"] if s["private"] else ["pool"], s["pool"], s["limit"] or ops.H2_SLOTS), (["const"], s["const"], ops.H2_CONST_SLOTS)]
        pools += [(["retired", k], p, ops.H2_SLOTS) for k, p in enumerate(reversed(s["retired"]))]
        if s["private"]:
            pools.append((["pool"], self.main, ops.H2_SLOTS))
        for j, (t, v) in enumerate(zip(DECLS[name][1], args)):
            if t is ctypes.c_void_p and isinstance(v, int) and v:
                for label, base, words in pools:
                    if base is not None and 0 <= v - base < 4 * ops.H2_SUB * words:
                        out[j + 1] = label + [(v - base) // (4 * ops.H2_SUB)]
        return out

    def state(self):
        s = self.ops.h2_pool_state()
        self.calls.append(["#state", s["next"], s["base"], int(s["step"] != self.step), len(s["retired"])])
        self.step = s["step"]


# ------------------------------------------------------------------------------------------------------------------ the cases
# A case gets (ops, trace) and returns the tensors its digest is taken over
def _leaf(*shape, seed, scale=1.0, relu=False):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = scale * torch.randn(*shape, device="cuda", generator=gen)
    return (torch.relu(x) if relu else x).requires_grad_()


def _bottleneck(stride, seed):
    """Bottleneck(64, 16, stride), for [2, 8, 8, 64] maps (tools/bn_launch_trace.py _block)"""
    from tris_amd.CLIP.clip.model import Bottleneck
    torch.manual_seed(seed)
    net = Bottleneck(64, 16, stride).cuda().train()
    with torch.no_grad():
        for n_, p in net.named_parameters():
            if p.dim() == 1:
                p.copy_(1 + 0.2 * torch.randn_like(p) if n_.endswith("weight") else 0.1 * torch.randn_like(p))
    return net


def _attention_block(seed):
    """ResidualAttentionBlock(64, 1), for [2, 8, 64] tokens (tools/product_launch_trace.py _block)"""
    from tris_amd.CLIP.clip.model import ResidualAttentionBlock
    torch.manual_seed(seed)
    net = ResidualAttentionBlock(64, 1, attn_mask=True).cuda().train()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return net


def _loss(ops, y):
    return (ops.unplanes(y) * torch.linspace(-1, 1, y.shape[-1], device="cuda")).sum()


def _grads(net, *inputs):
    return [t.grad for t in inputs] + [p.grad for p in net.parameters()]


def case_arena(ops, tr, superseded=False):
    """an explicit step over a registered arena of a 3x3 weight, a 1x1 weight of 64 x 64 and a 1-D parameter: the three per-arena
    launches, the parameters on words 0 .. 2, the first activation on word 3 -- in the second step as in the first.  superseded: a
    second arena over the same parameters; only that one is walked"""
    from tris_amd.optim import Arena
    net, x = _bottleneck(2, 11), _leaf(2, 8, 8, 64, seed=12, relu=True)
    params = [net.conv2.weight, net.downsample[1].weight, net.bn1.weight]
    assert ops._pl_weight_ok(params[0]) and ops._pl_weight_t_ok(params[1]) and not ops._pl_weight_t_ok(params[0])
    arenas = [Arena(params) for _ in range(2 if superseded else 1)]
    for a in arenas:
        ops.h2_register_arena(a)
    for _ in range(1 if superseded else 2):
        ops.h2_begin_step()
        assert ops.h2_step_arenas() == arenas[-1:]
        tr.state()
        y = net(x)
        _loss(ops, y).backward()
        ops.wgrad_join()
        ops.h2_end_step()
        tr.state()
    return [ops.unplanes(y)] + _grads(net, x)


def case_two_forwards(ops, tr):
    """tests/test_gpu_planes.py::test_two_forwards_then_one_backward_outside_an_explicit_step: the first forward's pool is retired,
    the backward over both losses reads its words there, the next explicit begin drops it"""
    net = _bottleneck(1, 21)
    x1, x2 = _leaf(2, 8, 8, 64, seed=22, relu=True), _leaf(2, 8, 8, 64, seed=23, scale=3.0, relu=True)
    assert ops._h2_slot() is not None      # (something was handed out since the last begin: the next forward starts a step)
    losses = []
    for x in (x1, x2):
        assert ops.h2_auto_step()
        tr.state()
        losses.append(_loss(ops, net(x)))
    tr.state()
    (losses[0] + losses[1]).backward()
    ops.wgrad_join()
    tr.state()
    ops.h2_begin_step()
    tr.state()
    ops.h2_end_step()
    return [l.detach() for l in losses] + _grads(net, x1, x2)


def case_private_pool(ops, tr):
    """a private pool of 4 words inside an explicit step over a small arena: two products of three words each -- the second one's B gets
    None and the product runs in x3, unmarked -- and the step's own hand-out goes on where it was"""
    from tris_amd.optim import Arena
    arena = Arena([torch.nn.Parameter(_leaf(64, seed=31).detach())])
    ops.h2_register_arena(arena)
    A1, B1, A2, B2 = (_leaf(*s, seed=32 + i, scale=sc).detach() for i, (s, sc) in enumerate((((2, 3, 64), 1.0), ((64, 32), 0.1)) * 2))
    with torch.no_grad():
        ops.h2_begin_step()
        y0 = ops.ew("TRIS_EW_SCALE", A1, None, 2.0)
        tr.state()
        before = [ops.h2_pool_state()[k] for k in ("next", "step", "pool")], ops.h2_step_arenas()
        region = ops.h2_private_pool(slots=4)
        with region:
            region.reset()
            tr.state()
            c1, c2 = ops.matmul(A1, B1), ops.matmul(A2, B2)
            tr.state()
            assert ops._h2_slot() is None
        assert ([ops.h2_pool_state()[k] for k in ("next", "step", "pool")], ops.h2_step_arenas()) == before and before[1] == [arena]
        tr.state()
        y1 = ops.ew("TRIS_EW_SCALE", y0, None, 2.0)
        ops.h2_end_step()
    tr.state()
    return [c1, c2, y1]


def case_pool_full(ops, tr):
    """tests/test_gpu_packed.py::test_tower_survives_an_amax_pool_restart_inside_the_packed_pass in small: two words left in an explicit
    step, three marked launches -- the third one's word is the first of a new step, explicit as the one it replaces (a forward that
    asks h2_auto_step behind it begins none) -- and a product of an output tagged before the restart with one tagged after it"""
    x, w = _leaf(6, 64, seed=41).detach(), _leaf(64, 32, seed=42, scale=0.1).detach()
    with torch.no_grad():
        ops.h2_begin_step()
        while ops.h2_pool_state()["next"] < ops.H2_SLOTS - 2:
            ops._h2_slot()
        tr.state()
        y = [x]
        for _ in range(3):
            y.append(ops.ew("TRIS_EW_SCALE", y[-1], None, 0.5))
            tr.state()
        assert ops.h2_step_open() and not ops.h2_auto_step()
        c = ops.matmul(y[3], y[2], True), ops.matmul(y[3], w)
        ops.h2_end_step()
    tr.state()
    return y[1:] + list(c)


def case_frozen(ops, tr):
    """a frozen Linear weight on planes (cfg.gemm_convert, tools/product_launch_trace.py case_gemm_convert): first use -- its constant
    word and its planes --, reuse without a launch for either, then an in-place write: the same word refreshed, the planes rebuilt
    once, and reused again"""
    x, w, b = _leaf(2, 64, 64, seed=51).detach(), torch.nn.Parameter(_leaf(64, 64, seed=52, scale=0.1).detach()), torch.nn.Parameter(_leaf(64, seed=53).detach())
    w._tris_linear_w = True
    out = []
    with torch.no_grad():
        ops.h2_begin_step()
        for k in range(4):
            if k == 2:
                w.mul_(2.0)
            out.append(ops.linear(x, w, b))
            tr.state()
        ops.h2_end_step()
    return out


def case_unarmed(ops, tr):
    """products inside h2_paused and under a thread mode run unarmed and take no word; the same pass behind them is armed"""
    net, x = _attention_block(61), _leaf(2, 8, 64, seed=62).detach()
    out = []
    with torch.no_grad():
        ops.h2_begin_step()
        with ops.h2_paused():
            out.append(net(x))
        tr.state()
        prev = ops._set_thread_mode("x3")
        try:
            out.append(net(x))
        finally:
            ops._set_thread_mode(prev)
        tr.state()
        out.append(net(x))
        ops.h2_end_step()
    tr.state()
    return out


def case_orphan_plane_gradient(ops, tr):
    """a gradient written as planes that no plane-aware backward takes: the end of the autograd pass raises and leaves no entry"""
    class Orphan(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.view_as(x)

        @staticmethod
        def backward(ctx, g):
            return ops.pl_grad_out(torch.zeros_like(g), ops._h2_slot())
    x = _leaf(2, 8, seed=71)
    ops.h2_begin_step()
    try:
        Orphan.apply(x).sum().backward()
        raised = False
    except RuntimeError as e:
        raised = "plane gradients without a plane-aware consumer" in str(e)
    ops.h2_end_step()
    assert raised and not ops._PL_GRAD
    tr.state()
    assert len(tr.calls) == 1, tr.calls
    return []


# case id -> (cfg switches off the defaults, function, arguments)
CASES = {
    "arena-two-steps": ({}, case_arena, ()),
    "arena-superseded": ({}, case_arena, (True,)),
    "two-forwards-one-backward": ({}, case_two_forwards, ()),
    "private-pool": ({}, case_private_pool, ()),
    "pool-full": ({}, case_pool_full, ()),
    "frozen-parameter": ({"gemm_convert": 1}, case_frozen, ()),
    "paused-and-thread-mode": ({}, case_unarmed, ()),
    "orphan-plane-gradient": ({}, case_orphan_plane_gradient, ()),
}


def _digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(b"none" if t is None else t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def run_case(cid):
    """-> (the classified calls and state rows of case `cid`, the digest of what it computed)"""
    from tris_amd import ops
    from tris_amd.config import cfg
    switches, fn, args = CASES[cid]
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode("h2")
    ops.set_autotune(False)
    arenas, ops._H2_ARENAS[:] = ops._H2_ARENAS[:], []     # (an optimiser somebody else left alive adds its per-step launches to every step)
    try:
        with cfg.override(**dict(DEFAULTS, **switches)), ops.h2_fresh_consts():
            ops.h2_begin_step()
            ops.h2_end_step()
            tr = _Trace(ops)
            with recording(tr.calls, tr.classify):
                res = fn(ops, tr, *args)
            ops.wgrad_join()
            torch.cuda.synchronize()
            digest = _digest(res)
    finally:
        ops._H2_ARENAS[:] = arenas
        ops.set_autotune(os.environ.get("TRIS_AUTOTUNE", "1")[:1] != "0")    # (the library's own reading of the environment)
        ops.set_gemm_mode(prev)
        torch.cuda.synchronize()
    return tr.calls, digest


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
