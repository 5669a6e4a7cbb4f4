"""Launch trace of the BatchNorm dispatch (tris_amd/ops.py: BatchNormFn, its hand-offs to LinearFn / Conv3x3Fn, BnPreluFn).

`python tools/bn_launch_trace.py` runs every case of CASES on the GPU and writes tests/golden/bn_launch_trace.json: case id -> the
list of entry-point calls the case made through ops.call and ops._declinable (the latter carries the pooled-residual product), in
issue order.  tests/test_gpu_bn_dispatch.py runs the same cases and compares with that file, so a change of the Python dispatch that
adds, drops, reorders or re-parametrises a launch shows.  The file is made from the code whose behaviour is to be kept; a refactor
never regenerates it.

A call is stored as [name, arg, arg, ...] with the arguments classified by tris_amd._lib.DECLS[name]: a pointer position (the stream
and a byref included) only as 0 (null) or 1; int / long positions by value; float positions by their fp32 value.  Pointers differ
from run to run; nothing else did between two runs on the same code, so no other field is left out.

Every case is a batch of 2 and a step of its own, in h2 with operand planes unless it says otherwise, with the autotuner off (the
cost model then picks the tiles, and the number of partial-sum rows follows from the tile) and the BatchNorm-related switches of
tris_amd.config pinned to their defaults, whatever the environment says."""
import contextlib
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "bn_launch_trace.json")

import torch  # noqa: E402

DEFAULTS = dict(h2_planes=True, bn_pair=True, bn_pair_parts="fwd,pool", bn_pool=True, bn_bitmask=True, bn_bwd_fuse=True, grad_box=True,
                syncbn_bound=True, side_param_grads=True, fuse_splitk=False, gemm_convert=0)


def _classify(name, args):
    from tris_amd._lib import DECLS
    out = [name]
    for t, v in zip(DECLS[name][1], args):
        if t is ctypes.c_void_p:
            out.append(0 if v is None or (isinstance(v, int) and v == 0) else 1)
        elif t is ctypes.c_float:
            out.append(ctypes.c_float(v).value)
        else:
            out.append(int(v))
    assert len(out) == len(args) + 1, (name, len(args))
    return out


@contextlib.contextmanager
def recording(calls, classify=_classify):
    """every ops.call / ops._declinable of the scope, classified, appended to `calls`"""
    from tris_amd import ops
    call, declinable = ops.call, ops._declinable
    ops.call = lambda name, *a: (calls.append(classify(name, a)), call(name, *a))[1]
    ops._declinable = lambda name, *a: (calls.append(classify(name, a)), declinable(name, *a))[1]
    try:
        yield calls
    finally:
        ops.call, ops._declinable = call, declinable


# ------------------------------------------------------------------------------------------------------------------ the cases
def _block(inplanes, planes, stride, seed):
    """(as tests/test_gpu_bn_pair.py builds its blocks)"""
    from tris_amd.CLIP.clip.model import Bottleneck
    torch.manual_seed(seed)
    net = Bottleneck(inplanes, planes, stride).cuda().train()
    with torch.no_grad():
        for n_, p in net.named_parameters():
            if p.dim() == 1:
                p.copy_(1 + 0.2 * torch.randn_like(p) if n_.endswith("weight") else 0.1 * torch.randn_like(p))
    return net


def _step(ops, fwd, backward=True):
    ops.h2_begin_step()
    y = ops.unplanes(fwd())
    if backward:
        (y * torch.linspace(-1, 1, y.shape[-1], device="cuda")).sum().backward()
        ops.wgrad_join()
    ops.h2_end_step()
    torch.cuda.synchronize()


def _input(hw, C, seed):
    torch.manual_seed(seed)
    return torch.relu(torch.randn(2, hw, hw, C, device="cuda")).requires_grad_()


def _syncbn_stub(net):
    """a SyncBatchNorm group of one rank without a mailbox (tests/test_gpu_bn_pair.py::_forward_calls), backward included"""
    from tris_amd import comm
    from tris_amd.CLIP.clip.model import BatchNorm2d
    saved = {k: getattr(comm, k) for k in ("world_size", "syncbn_mailbox", "syncbn_all_gather_into", "syncbn_all_reduce_sum")}
    comm.world_size = lambda g: 1
    comm.syncbn_mailbox = lambda g, n: None
    comm.syncbn_all_gather_into = lambda out, src, group=None: out.copy_(src)
    comm.syncbn_all_reduce_sum = lambda t, group=None: t
    group = object()
    for m in net.modules():
        if isinstance(m, BatchNorm2d):
            m.process_group = group
    return lambda: [setattr(comm, k, v) for k, v in saved.items()]


def case_block(ops, stride, train=True, group=False):
    net = _block(64, 32, stride, 11)
    x = _input(16, 64, 12)
    undo = _syncbn_stub(net) if group else (lambda: None)
    try:
        if train:
            _step(ops, lambda: net(x))
        else:
            net.eval()
            with torch.no_grad():
                _step(ops, lambda: net(x), backward=False)
    finally:
        undo()


def case_linked(ops, sunk=False):
    b1, b2 = _block(64, 32, 2, 21), _block(128, 32, 1, 22)
    if sunk:   # every parameter gradient goes straight into its (arena) view: the arena-direct branches
        for p in list(b1.parameters()) + list(b2.parameters()):
            p.grad = torch.zeros_like(p)
            p._tris_sink = True
    x = _input(32, 64, 23)
    _step(ops, lambda: b2(b1(x, link_out=True)))


def case_lazy(ops, shape):
    """conv3x3(stats) -> batch_norm(relu, lazy, bwd_link) -> conv3x3 (shapes of tests/test_gpu_ops.py's lazy test); where
    conv3x3_bnin_ok says no the second convolution writes the BatchNorm's output after all"""
    B, H, W, Cin, Cout = shape
    gen = torch.Generator(device="cuda").manual_seed(H + Cin)
    x = torch.randn(B, H, W, Cin, device="cuda", generator=gen).requires_grad_()
    w0, w1 = ((0.1 * torch.randn(co, Cin, 3, 3, device="cuda", generator=gen)).contiguous(memory_format=torch.channels_last)
              .requires_grad_() for co in (Cin, Cout))
    g, b = (1 + 0.2 * torch.randn(Cin, device="cuda", generator=gen)).requires_grad_(), torch.zeros(Cin, device="cuda", requires_grad=True)
    rm, rv = torch.zeros(Cin, device="cuda"), torch.ones(Cin, device="cuda")

    def fwd():
        a = ops.batch_norm(ops.conv3x3(x, w0, 1, stats=True), g, b, rm, rv, None, True, True, lazy=True, bwd_link=True)
        assert hasattr(a, "_bn_lazy")
        return ops.conv3x3(a, w1, 1)
    _step(ops, fwd)


def case_refusal(ops, why):
    """tests/test_gpu_bn_pair.py::test_a_batchnorm_that_cannot_pair_writes_the_shortcut_after_all, the switch on"""
    B, H, W, C = 2, 6, 10, 64
    gen = torch.Generator(device="cuda").manual_seed(C)
    x3, xs = (torch.randn(B, H, W, C, device="cuda", generator=gen).requires_grad_() for _ in range(2))
    g3, gs = ((1 + 0.2 * torch.randn(C, device="cuda", generator=gen)).requires_grad_() for _ in range(2))
    b3, bs = ((0.1 * torch.randn(C, device="cuda", generator=gen)).requires_grad_() for _ in range(2))
    rm, rv, rm_s, rv_s = torch.zeros(C).cuda(), torch.ones(C).cuda(), torch.zeros(C).cuda(), torch.ones(C).cuda()

    def fwd():
        idn = ops.batch_norm(xs, gs, bs, rm_s, rv_s, training=True, pair=True)
        assert hasattr(idn, "_bn_pair")
        return ops.batch_norm(x3, g3, b3, rm, rv, resid=idn, relu=why != "no_relu", training=True, planes=why != "no_planes")
    _step(ops, fwd)


def case_bn_prelu(ops, how):
    """how: "part" (train mode behind conv3x3(stats=True): the partials of its epilogue), "pass" (train mode, a statistics pass),
    "eval".  [2, 16, 16, 32] -> 32: 512 rows of 32 channels, within the statistics epilogue's preconditions (Cin % 32, 128 rows)"""
    B, H, W, C = 2, 16, 16, 32
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(B, H, W, C, device="cuda", generator=gen).requires_grad_()
    w = (0.1 * torch.randn(C, C, 3, 3, device="cuda", generator=gen)).contiguous(memory_format=torch.channels_last).requires_grad_()
    g, b = (1 + 0.2 * torch.randn(C, device="cuda", generator=gen)).requires_grad_(), torch.zeros(C, device="cuda", requires_grad=True)
    a = torch.tensor([0.27], device="cuda", requires_grad=True)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")

    def fwd():
        y = ops.conv3x3(x, w, 1, stats=how == "part")
        assert hasattr(y, "_bn_part") == (how == "part")
        return ops.bn_prelu(y, g, b, rm, rv, a, how != "eval")
    _step(ops, fwd)


OK_SHAPE, NO_SHAPE = (2, 16, 32, 32, 32), (2, 10, 10, 64, 64)   # (conv3x3_bnin_ok: yes / no)

# case id -> (cfg switches off the defaults, arithmetic, function, arguments)
CASES = {
    "block-s1": ({}, "h2", case_block, (1,)),
    "block-s2": ({}, "h2", case_block, (2,)),
    "linked": ({}, "h2", case_linked, ()),
    "linked-parts-fwd-pool-bwd": ({"bn_pair_parts": "fwd,pool,bwd"}, "h2", case_linked, ()),
    "linked-no-bitmask": ({"bn_bitmask": False}, "h2", case_linked, ()),
    "linked-no-bwd-fuse": ({"bn_bwd_fuse": False}, "h2", case_linked, ()),
    "linked-no-grad-box": ({"grad_box": False}, "h2", case_linked, ()),
    "linked-sunk": ({}, "h2", case_linked, (True,)),
    "linked-sunk-parts-fwd-pool-bwd": ({"bn_pair_parts": "fwd,pool,bwd"}, "h2", case_linked, (True,)),
    "block-s2-no-pair": ({"bn_pair": False}, "h2", case_block, (2,)),
    "block-s2-no-pool": ({"bn_pool": False}, "h2", case_block, (2,)),
    "block-s2-no-planes": ({"h2_planes": False}, "h2", case_block, (2,)),
    "block-s2-x3": ({}, "x3", case_block, (2,)),
    "block-s2-syncbn": ({}, "h2", case_block, (2, True, True)),
    "block-s2-eval": ({}, "h2", case_block, (2, False)),
    "block-s2-eval-x3": ({}, "x3", case_block, (2, False)),
    "lazy-folded": ({}, "h2", case_lazy, (OK_SHAPE,)),
    "lazy-written-after-all": ({}, "h2", case_lazy, (NO_SHAPE,)),
    "refusal-no-planes": ({}, "h2", case_refusal, ("no_planes",)),
    "refusal-no-relu": ({}, "h2", case_refusal, ("no_relu",)),
    "bn-prelu-part": ({}, "h2", case_bn_prelu, ("part",)),
    "bn-prelu-pass": ({}, "h2", case_bn_prelu, ("pass",)),
    "bn-prelu-eval": ({}, "h2", case_bn_prelu, ("eval",)),
}


def run_case(cid):
    """-> the classified calls of case `cid`"""
    from tris_amd import ops
    from tris_amd.config import cfg
    switches, arith, fn, args = CASES[cid]
    assert ops.conv3x3_bnin_ok(OK_SHAPE[:4], OK_SHAPE[4]) and not ops.conv3x3_bnin_ok(NO_SHAPE[:4], NO_SHAPE[4])
    prev, calls = ops.get_gemm_mode(), []
    ops.set_gemm_mode(arith)
    ops.set_autotune(False)
    try:
        with cfg.override(**dict(DEFAULTS, **switches)), recording(calls):
            fn(ops, *args)
    finally:
        ops.set_autotune(os.environ.get("TRIS_AUTOTUNE", "1")[:1] != "0")    # (the library's own reading of the environment)
        ops.set_gemm_mode(prev)
        torch.cuda.synchronize()
    return calls


def main(out=FIXTURE):
    traces = {cid: run_case(cid) for cid in CASES}
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(cid)}: {json.dumps(calls)}" for cid, calls in traces.items()) + "\n}\n")
    print(f"{out}: {len(traces)} cases, {sum(map(len, traces.values()))} calls")


if __name__ == "__main__":
    main(*sys.argv[1:2])
