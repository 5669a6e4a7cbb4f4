"""Host-side operators of the TRIS Stage-1 hot path: thin autograd wrappers over the C ABI (include/tris_hip.h).

PyTorch supplies device memory, the current HIP stream and the autograd tape -- plumbing.  Every
numeric op below is a kernel from libtris_hip.so; there is no eager / CPU fallback and CPU tensors
are rejected loudly.

Layout conventions: activations are channels-last, i.e. an image tensor is a contiguous
[B, H, W, C] array; conv weights keep the reference's [Cout, Cin, kh, kw] *shape* in
torch.channels_last memory so state dicts stay compatible.

Weight gradients: a parameter may carry a "gradient sink" (`p.grad` is a view into a flat arena,
see tris_amd.optim).  Backward kernels then write the weight gradient straight into that arena
(each parameter is used once per step) and return None to autograd.
"""
import ctypes
import math
import contextlib
import os
import weakref
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import CONSTS, call, query
from .config import cfg

EW = CONSTS


class NoGpuError(RuntimeError):
    pass


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """raw handle of the current HIP stream (the launch path calls this ~1500 times per step: the raw accessor avoids building a
    torch.cuda.Stream object each time)"""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise NoGpuError("tris_amd ops run on MI355X only (got a CPU tensor); there is no CPU fallback")
        if t.dtype != torch.float32 and t.dtype != torch.int64 and t.dtype != torch.uint8:
            raise TypeError(f"unsupported dtype {t.dtype}")


def P(t, off=0):
    return None if t is None else t.data_ptr() + 4 * off


_WS = {}


def workspace(nbytes):
    """Scratch arena per (device, stream): kernels on one stream run in order, so serial reuse is safe; work issued on
    a second stream (the text encoders overlap the RN50 trunk, tris_amd.model.model_stage1) gets its own arena."""
    key = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    cur = _WS.get(key)
    if cur is None or cur.numel() * 4 < nbytes:
        n = max(int(nbytes), 256 << 20)
        cur = torch.empty(n // 4 + 1, dtype=torch.float32, device="cuda")
        _WS[key] = cur
    return cur


_TICKETS = {}
TICKET_SLOTS = 1 << 14


def splitk_tickets():
    """ticket array of the fused split-K finish (tris_splitk_tickets_next) for the current (device, stream): zero when created, left
    zero by every launch; products launched on one stream run in order, so they share it"""
    key = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    cur = _TICKETS.get(key)
    if cur is None:
        if torch.cuda.is_current_stream_capturing():
            return None        # (never allocated under capture: the product then takes the two-launch form)
        cur = _TICKETS[key] = torch.zeros(TICKET_SLOTS, dtype=torch.int32, device="cuda")
    return cur


# ---- arithmetic of the dense products --------------------------------------------------------------------------------------
# 'h2' (default since round 5 -- the arithmetic bench.py reports and the trainer runs are one and the same): two fp16 pieces per
#   operand (the residual pre-scaled by 2^11), three f16 MFMAs per product, one power-of-two scale per TENSOR formed on the device from
#   its largest magnitude: fp32-class accuracy over a 2^27 dynamic range inside a tensor, half the matrix work of x3
#   (csrc/x3_split.h, "h2 products" below).  A product whose operands have no amax runs in x3.
# 'x3': split-bf16 -- three bf16 pieces per fp32 operand, six bf16 MFMAs per product, fp32 accumulate: fp32-class accuracy at ~2.6x
#   the f32-MFMA rate; also what the kernel library itself runs when a product is not armed for h2.
# 'f32': the f32-input MFMA (bit-equal to an fmaf chain).
_ARITH = "h2"     # (TRIS_GEMM_MODE at import overrides; the library's own default for unarmed products is x3 either way)


def set_gemm_mode(mode):
    """'x3' | 'h2' | 'f32' (env TRIS_GEMM_MODE at import).  h2 is per product on top of x3: the library's own default
    arithmetic (tris_set_gemm_mode) stays x3 for whatever cannot run in h2."""
    global _ARITH
    assert mode in ("f32", "x3", "h2"), mode
    call("tris_set_gemm_mode", 0 if mode == "f32" else 1)
    _ARITH = mode


def get_gemm_mode():
    return _ARITH


_TLS = __import__("threading").local()


def _set_thread_mode(mode):
    """per-thread arithmetic override of the dense products (None = none; 'f32' | 'x3'); returns the previous override"""
    prev = getattr(_TLS, "mode", None)
    _TLS.mode = mode
    call("tris_set_gemm_mode_thread", -1 if mode is None else {"f32": 0, "x3": 1}[mode])
    return prev


def _thread_mode_is_set():
    return getattr(_TLS, "mode", None) is not None


def set_autotune(on):
    """per-shape (tile, split-K) autotuning of the GEMM core on/off (include/tris_hip.h: tris_set_autotune)"""
    call("tris_set_autotune", int(bool(on)))


def set_option(name, value):
    """developer option of the kernel library (include/tris_hip.h tris_set_option): FORCE_TILE, FORCE_PIPE, CONV_DIRECT,
    WGRAD_DIRECT, BN_FOLD, TUNE_LOG, ...; value None restores the default"""
    call("tris_set_option", name.encode(), None if value is None else str(value).encode())


class option:
    """`with ops.option("CONV_DIRECT", 0): ...` -- a library option for a scope (tests)"""

    def __init__(self, name, value, restore=None):
        self.name, self.value, self.restore = name, value, restore

    def __enter__(self):
        set_option(self.name, self.value)

    def __exit__(self, *exc):
        set_option(self.name, self.restore)
        return False


if os.environ.get("TRIS_GEMM_MODE"):
    set_gemm_mode(os.environ["TRIS_GEMM_MODE"])


def cl_weight(w):
    """Conv weight in the kernel layout [Cout][kh][kw][Cin] (= channels_last memory)."""
    if w.dim() == 4 and not w.is_contiguous(memory_format=torch.channels_last):
        return w.contiguous(memory_format=torch.channels_last)
    return w


# ----------------------------------------------------------------------------------------------- weight-gradient stream
# Weight gradients are consumed only by the optimiser (or the data-parallel reducer), never by the rest of backward.
# They are issued on their own HIP stream so a wgrad (split-K, often HBM-bound in the early layers) overlaps the dgrad /
# BatchNorm-backward chain that continues on the main stream.  `wgrad_join()` makes the current stream wait for them.
_WG = {}


# Side streams under stream capture: a capture that forks (event record on the capturing stream, wait on the side stream) and
# joins again before it ends records the side streams' launches as parallel branches of the graph.  The small inference graphs
# (tris_amd.graphs.GraphedStage1Eval) stay single-stream; the captured training step switches this on around its capture.
_CAPTURE_STREAMS = False


def streams_allowed():
    """may work be forked onto a side stream here?  (not under a stream capture, unless the capture asked for it)"""
    return _CAPTURE_STREAMS or not torch.cuda.is_current_stream_capturing()


# Segmented capture (tris_amd.graphs.SegmentedTrainStep): the step is captured as a chain of SINGLE-STREAM hipGraphs (the form
# the ROCm runtime launches through its packet path), cut at autograd boundaries; weight-gradient work is not forked onto its
# stream from inside a capture but handed to the capturing object, which records it as a graph of its own for that stream.
_SEG = None


def cut(x):
    """Autograd segment boundary.  A no-op (returns x) except while a segmented capture is being recorded: there the returned
    tensor is a fresh leaf on x's storage, and the capture drives the backward segment by segment (x <- leaf.grad)."""
    if _SEG is None or not x.requires_grad or not torch.is_grad_enabled():
        return x
    return _SEG.cut(x)


def _wgrad_enabled():
    if _SEG is not None:
        return True
    return cfg.wgrad_stream and streams_allowed()


# ---- side streams on their own hardware queues ------------------------------------------------------------------------------
# The HIP runtime maps streams onto a small number of hardware queues (GPU_MAX_HW_QUEUES, 4 by default) round-robin in creation
# order, and two streams on one queue run one after the other.  Which queue a new stream gets depends on how many streams the
# process created before -- a collective backend that creates three or four of its own is enough to put the text or the
# weight-gradient stream on the COMPUTE stream's queue, and the overlap this path is built on silently disappears (measured:
# +3.7 ms per step as soon as an RCCL communicator exists, reproduced without RCCL by creating three dummy streams first;
# DESIGN.md "Streams").  So the side streams are not taken as they come: a handful of candidates is created and PROBED -- a
# device-side sleep on one stream, a tiny kernel on the other, HIP-event timestamps tell whether they overlapped -- and the
# first ones that run concurrently with the compute stream and with each other are kept.
_CAL = {}


def _calibrated_streams(dev):
    """up to three streams of device `dev` that the hardware runs concurrently with the current stream and with each other"""
    if dev in _CAL:
        return _CAL[dev]
    if torch.cuda.is_current_stream_capturing():
        return []               # (no probing under stream capture; not remembered)
    picked = []
    if cfg.stream_probe and hasattr(torch.cuda, "_sleep"):
        main = torch.cuda.current_stream(dev)
        scratch = torch.zeros(64, device=f"cuda:{dev}")

        def overlap(a, b):
            torch.cuda.synchronize(dev)
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            with torch.cuda.stream(a):
                e0.record()
                torch.cuda._sleep(6000000)      # ~2.5 ms on the device
                e1.record()
            with torch.cuda.stream(b):
                scratch.add_(1.0)
                e2.record()
            torch.cuda.synchronize(dev)
            return e0.elapsed_time(e2) < 0.5 * e0.elapsed_time(e1)
        try:
            torch.cuda._sleep(1000)
            for _ in range(10):
                c = torch.cuda.Stream(device=dev)
                with torch.cuda.stream(c):      # first use of a stream creates its queue (milliseconds): not part of the probe
                    scratch.add_(1.0)
                if overlap(main, c) and all(overlap(x, c) for x in picked):
                    picked.append(c)
                    if len(picked) == 3:
                        break
        except Exception:       # the probe is an optimisation: any failure falls back to plain streams
            picked = []
    _CAL[dev] = picked
    return picked


_COMPUTE_STREAM = {}


def compute_stream(dev=None):
    """one non-default stream per device to compute on (torch.cuda.set_stream(ops.compute_stream())): on this runtime the process's
    default stream runs exclusively with respect to hipGraphs launched on other streams, so a step that replays its text towers
    from graphs must not compute on it (bench.py, train_stage1.main; data-parallel runs get theirs from place_streams)"""
    dev = torch.cuda.current_device() if dev is None else dev
    s = _COMPUTE_STREAM.get(dev)
    if s is None:
        s = _COMPUTE_STREAM[dev] = torch.cuda.Stream(device=dev)
    return s


def place_streams(group=None):
    """Data-parallel start-up (call once on every rank right after init_process_group, before anything else touches the
    device): sort out which stream runs on which of the four hardware queues WITH the collective backend in the picture.
    torch's NCCL/RCCL process group runs its kernels on a stream of its own whose queue nobody chooses -- if that is the
    compute stream's queue, every gradient all-reduce sits in front of the compute kernels until the peers arrive (measured
    with one rank: a collective issued while the compute stream sleeps completes only after the sleep), and the reducer's
    overlap is gone without any error.  Probes (device sleep + tiny kernel / tiny all-reduce, HIP-event timestamps) find the
    queue classes of a few candidate streams and the class of the backend's stream; compute, text and weight-gradient streams
    are then taken from three classes the backend is NOT on.  Every rank issues the same fixed number of probe collectives.
    Returns the stream the caller should make current (torch.cuda.set_stream) for all further work, or None to stay."""
    import torch.distributed as dist
    dev = torch.cuda.current_device()
    if not cfg.stream_probe or not hasattr(torch.cuda, "_sleep"):
        return None
    null = torch.cuda.current_stream(dev)
    scratch = torch.zeros(64, device=f"cuda:{dev}")
    cands = [null]
    torch.cuda._sleep(1000)
    for _ in range(7):
        c = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(c):
            scratch.add_(1.0)
        cands.append(c)
    torch.cuda.synchronize(dev)

    def probe(a, b, op):
        """does `op`, issued on b, finish while a is still asleep?"""
        torch.cuda.synchronize(dev)
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        with torch.cuda.stream(a):
            e0.record()
            torch.cuda._sleep(6000000)
            e1.record()
        with torch.cuda.stream(b):
            op()
            e2.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e2) < 0.5 * e0.elapsed_time(e1)
    reps, cls = [], []                      # one representative stream per hardware-queue class
    for c in cands:
        k = next((i for i, r in enumerate(reps) if r is c or not probe(r, c, lambda: scratch.add_(1.0))), None)
        if k is None:
            reps.append(c)
            k = len(reps) - 1
        cls.append(k)
    backend_cls = None
    if dist.is_initialized() and dist.get_backend(group) == "nccl":   # (no condition on what THIS rank found: same collectives everywhere)
        buf = torch.zeros(256, device=f"cuda:{dev}")
        for _ in range(2):                  # communicator / stream set-up is not part of the probe
            dist.all_reduce(buf, group=group)
        torch.cuda.synchronize(dev)
        for k in range(4):                  # a FIXED number of collectives on every rank, whatever the probes find locally
            r = reps[k % len(reps)]
            issue = reps[(k + 1) % len(reps)]

            def coll():
                w = dist.all_reduce(buf, group=group, async_op=True)
                w.wait()
            dist.barrier(group=group)       # ranks start each probe together: a late peer must not look like a shared queue
            if not probe(r, issue, coll) and backend_cls is None and k < len(reps):
                backend_cls = k
    if cfg.stream_probe_log:
        print(f"[place_streams] queue classes of the candidates {cls}, collective backend on class {backend_cls}", flush=True)
    free = [k for k in range(len(reps)) if k != backend_cls]
    if len(free) < 3:                       # fewer queues than roles: leave everything as the runtime handed it out
        return None
    order = ([cls[0]] if cls[0] in free else []) + [k for k in free if k != cls[0]]   # keep the current stream if it may stay
    compute, text, wgrad = reps[order[0]], reps[order[1]], reps[order[2]]
    # the reducer's ISSUE stream carries only event records / waits (the backend's own stream runs the kernels), but a wait
    # parked in a hardware queue blocks whatever is behind it there: it goes on the backend's queue, never the compute one's
    used = {cls[cands.index(compute)], cls[cands.index(text)], cls[cands.index(wgrad)]}
    issue = next((c for c, k in zip(cands, cls) if k == backend_cls), None)
    if issue is None:
        issue = next((c for c, k in zip(cands, cls) if k not in used), wgrad)
    _CAL[dev] = [text, wgrad, issue]
    _WG.pop(dev, None)
    for key in [k for k in _SIDE_STREAMS if k[0] == dev]:
        _SIDE_STREAMS.pop(key)
    return None if compute is null else compute


def _new_side_stream(dev, slot):
    """slot 0 = text towers, 1 = weight gradients, 2 = gradient reducer: distinct probed streams where the hardware has them"""
    pool = _calibrated_streams(dev)
    return pool[slot] if slot < len(pool) else torch.cuda.Stream(device=dev)


def _wgrad_stream():
    dev = torch.cuda.current_device()
    if dev not in _WG:
        _WG[dev] = _new_side_stream(dev, 1)
    return _WG[dev]


def on_wgrad_stream(fn, *tensors, sink=None):
    """Run `fn()` (kernel launches only) on the weight-gradient stream after everything queued so far on the current
    stream; `tensors` are the buffers it reads (kept alive for the side stream via record_stream); sink: the gradient-arena
    view it writes."""
    if _SEG is not None:
        return _SEG.defer(fn, tensors, sink)
    if not _wgrad_enabled():
        return fn()
    main, side = torch.cuda.current_stream(), _wgrad_stream()
    side.wait_stream(main)
    with torch.cuda.stream(side):
        r = fn()
    for t in tensors:
        if t is not None:
            t.record_stream(side)
    return r


_SIDE_STREAMS = {}


def side_stream(name):
    """Named auxiliary HIP stream of the current device (e.g. "text": the text encoders overlap the RN50 trunk)."""
    key = (torch.cuda.current_device(), name)
    if key not in _SIDE_STREAMS:
        slot = {"text": 0, "reduce": 2}.get(name)
        _SIDE_STREAMS[key] = _new_side_stream(key[0], slot) if slot is not None else torch.cuda.Stream(device=key[0])
    return _SIDE_STREAMS[key]


def wgrad_join(into=None):
    """Make a stream (default: the current one) wait for every auxiliary stream that may still be producing gradients (the
    weight-gradient stream and the named side streams): call before anything consumes the gradient arenas (optimiser,
    all-reduce).  `into`: the stream that should wait -- the data-parallel reducer passes its own stream so that the COMPUTE
    stream is not stalled in the middle of backward."""
    if _SEG is not None:
        return  # segmented capture: the streams are joined between the graphs, by the object that replays them
    if not _WG and not _SIDE_STREAMS:
        return  # nothing was ever issued on an auxiliary stream (also: host-only / CPU test contexts)
    cur = torch.cuda.current_stream() if into is None else into
    dev = torch.cuda.current_device()
    if dev in _WG and _WG[dev] != cur:
        cur.wait_stream(_WG[dev])
    for (d, _), st in _SIDE_STREAMS.items():
        if d == dev and st != cur:
            cur.wait_stream(st)


def _sink(p):
    """The arena view a weight gradient should be written into, or None (=> return it to autograd)."""
    if p is not None and getattr(p, "_tris_sink", False):
        return p.grad
    return None


def _emit(p, make, needs, reads=None):
    """Produce a parameter gradient: into the sink (return None) or as a fresh tensor.  reads: the tensors `make` reads -- a gradient
    that lands in the arena and that nothing downstream of the backward pass waits for (a bias or norm-parameter column sum) is then
    issued on the weight-gradient stream like the weight gradients themselves, off the compute stream's chain (cfg.side_param_grads)."""
    if not needs:
        return None
    s = _sink(p)
    if s is not None:
        if reads is not None and cfg.side_param_grads:
            on_wgrad_stream(lambda: make(s), *reads, sink=s)
        else:
            make(s)
        return None
    out = torch.empty_like(p, memory_format=torch.preserve_format)
    make(out)
    return out


# ----------------------------------------------------------------------------------------------- profiling hook
# bench.py measures the dominant kernel family live: when enabled, every MFMA GEMM / implicit-GEMM conv launch is
# bracketed by HIP events on the launch stream and logged with its algorithmic FLOPs.
_PROF = None
_PROF_SHAPES = False


def profile_begin():
    global _PROF
    _PROF = []


def profile_end():
    """-> list of (kind, flops, milliseconds, algorithmic bytes)"""
    global _PROF
    rec, _PROF = _PROF, None
    torch.cuda.synchronize()
    return [(k, f, a.elapsed_time(b), nb) for k, f, a, b, nb in rec]


def _shape_tag(text):
    return text if _PROF_SHAPES else None


def _timed(kind, flops, fn, tag=None, nbytes=0):
    """nbytes: ALGORITHMIC HBM bytes of the launch -- every operand read once, every output written once"""
    if _PROF is None:
        return fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    if r is not False:   # (False = the entry point declined the shape: nothing was launched)
        _PROF.append((kind if tag is None else f"{kind}:{tag}", flops, a, b, nbytes))
    return r


# ----------------------------------------------------------------------------------------------- raw launches
# Batch-invariant arithmetic (evaluation): with it on, the result of every output ROW of a dense product is independent of how
# many other rows share the launch.  What can differ between launches of different M is (a) split-K (a different partition of
# the K sum) and (b) the direct vs implicit 3x3 convolution (different K order); tile shapes and the classic / pipelined loops
# walk K in the same order and are bitwise neutral.  `batch_invariant()` switches (a) and (b) off for its scope, so that
# tris_amd.validate can batch images and sentences and still return exactly the numbers of the one-at-a-time loop.
_BATCH_INVARIANT = 0


class batch_invariant:
    def __enter__(self):
        global _BATCH_INVARIANT
        _BATCH_INVARIANT += 1
        if _BATCH_INVARIANT == 1:
            call("tris_set_conv_direct_thread", 0)     # this thread's products only; nothing process-wide is touched
        # h2 scales every operand by a power of two derived from the amax of the WHOLE tensor: a row's rounding depends on which other
        # rows share the launch, so h2 cannot be batch-invariant (measured in round 6: one of 128 hit-tests flipped between group
        # sizes).  Inside this scope products run in the split-bf16 x3 arithmetic -- exact pieces, no data-dependent scale, row results
        # independent of the batch -- which is also the faster one at evaluation sizes (no amax words to produce or read).
        _H2.paused += 1
        return self

    def __exit__(self, *exc):
        global _BATCH_INVARIANT
        _BATCH_INVARIANT -= 1
        _H2.paused -= 1
        if _BATCH_INVARIANT == 0:
            call("tris_set_conv_direct_thread", -1)
        return False


def gemm(A, B, C, M, N, K, lda, ldb, ldc, tA, tB, batch=1, sA=0, sB=0, sC=0, bias=None, bias_mode=0, resid=None,
         ldr=0, sR=0, act=0, alpha=1.0, use_ws=True, pre_out=None, dact=None, w_a=False, w_b=False, w_bt=False, mark=True,
         resid_pool=None):
    """resid_pool = (H, W) (tris_gemm_resid_pool_next): resid is the gradient of the 2x2 average pool of the [.., H, W] map the rows
    of C stand for; the call returns False -- nothing launched -- where the fast kernel does not serve the product (caller falls back).
    pre_out / dact (tris_gemm_epilogue_next): also store the pre-activation value / multiply the result by quickgelu'(dact);
    the call then returns False -- nothing launched -- when the fast kernel does not serve the operands (caller falls back).
    w_a / w_b: that operand is a convolution weight, which exists as operand planes when the other operand is a plane tensor.
    mark=False: no product will read C as an operand (a weight gradient written into the optimiser's arena): the launch -- and the
    split-K reduce behind it -- does not carry the amax by-product (the reduce was 65 % longer with it)."""
    _chk(A, B, C, bias, resid)
    if pre_out is not None or dact is not None or batch != 1 or _BATCH_INVARIANT:
        A, B = unplanes(A), unplanes(B)
    if pre_out is not None or dact is not None:
        return _gemm_epilogue(A, B, C, M, N, K, lda, ldb, ldc, tA, tB, batch, bias, bias_mode, resid, ldr, sR, act, alpha, pre_out, dact)
    if _BATCH_INVARIANT and batch == 1 and not tA and M < 4 and lda == K and ldc == N and (resid is None or ldr == N) and bias_mode != 2:
        return _gemm_padded(A, B, C, M, N, K, ldb, tB, bias, bias_mode, resid, act, alpha, use_ws)
    ws = workspace(0) if (use_ws and batch == 1 and not _BATCH_INVARIANT) else None   # (no workspace = no split-K)
    blind = _rows_limit_blind(A, tA, batch)
    if (w_b and batch == 1 and not tA and M >= cfg.gemm_convert and cfg.gemm_convert > 0 and K % 32 == 0 and lda == K and getattr(B, "_tris_linear_w", False)
            and planes_on() and pl_word(A) is None and A.is_contiguous() and A.data_ptr() % 16 == 0 and _pl_weight_ok(B) and not blind):
        A = _a_planes(A, M, K)
    if blind or batch != 1:     # (a batched product's operands were rebuilt above)
        pp = _Operands(P(A), P(unplanes(B)), False, False)
    else:
        pp = h2_pp(A, B, w_a=w_a, w_b=w_b, k_red=K, w_bt=w_bt and not tB)
    if pp.b_t:    # B = W [K][N] arrived as the planes of its transpose [N][K]
        tB, ldb = True, K
    if mark:
        h2_mark_next(C)  # (h2: the product also leaves the amax of what it writes -- another product may consume C directly)
    if ws is not None and cfg.fuse_splitk:
        tk = splitk_tickets()
        if tk is not None:
            call("tris_splitk_tickets_next", tk.data_ptr(), tk.numel())
    if resid_pool is not None:
        call("tris_gemm_resid_pool_next", resid_pool[0], resid_pool[1])

    def launch():
        return (_declinable if resid_pool is not None else call)(
            "tris_gemm_f32", pp.a, pp.b, P(C), M, N, K, lda, ldb, ldc, int(tA), int(tB), batch, sA, sB, sC, P(bias), bias_mode, P(resid),
            ldr, sR, act, float(alpha), P(ws), 0 if ws is None else ws.numel() * 4, _stream())
    ran = _timed("gemm", 2.0 * M * N * K * batch, launch,
                 tag=(f"{'T' if tA else 'N'}{'T' if tB else 'N'} M{M} N{N} K{K} b{batch}" if _PROF_SHAPES else None),
                 nbytes=4.0 * ((M * K if (sA == 0 and batch > 1) else batch * M * K) + batch * K * N
                               + batch * M * N * (2 if resid is not None else 1)))
    return False if ran is False else C


def _gemm_epilogue(A, B, C, M, N, K, lda, ldb, ldc, tA, tB, batch, bias, bias_mode, resid, ldr, sR, act, alpha, pre_out, dact):
    """ops.gemm with pre_out / dact: True if the fast kernel ran, False -- nothing launched -- if it does not serve the product"""
    if _BATCH_INVARIANT or batch != 1:
        return False
    h2_arm(A, B)
    h2_mark_next(C)
    call("tris_gemm_epilogue_next", P(pre_out), P(dact))

    def launch():
        return _declinable("tris_gemm_f32", P(A), P(B), P(C), M, N, K, lda, ldb, ldc, int(tA), int(tB), 1, 0, 0, 0, P(bias), bias_mode,
                           P(resid), ldr, sR, act, float(alpha), None, 0, _stream())
    return _timed("gemm", 2.0 * M * N * K, launch, nbytes=4.0 * (M * K + K * N + M * N * (2 + int(resid is not None))))


def _gemm_padded(A, B, C, M, N, K, ldb, tB, bias, bias_mode, resid, act, alpha, use_ws):
    """ops.gemm, batch-invariant, fewer than four rows: such products run a different (generic) kernel than larger ones, so they are
    padded to four rows -- a sentence evaluated alone goes through the same arithmetic as one evaluated in a batch"""
    A4 = A.new_zeros(4, K)
    A4[:M].copy_(A.reshape(M, K))
    R4 = None
    if resid is not None:
        R4 = resid.new_zeros(4, N)
        R4[:M].copy_(resid.reshape(M, N))
    C4 = C.new_empty(4, N)
    gemm(A4, B, C4, 4, N, K, K, ldb, N, False, tB, bias=bias, bias_mode=bias_mode, resid=R4, ldr=N, act=act, alpha=alpha, use_ws=use_ws)
    C.reshape(M, N).copy_(C4[:M])
    return C


def colsum(X, M, N, out):
    ws = workspace(query("tris_col_workspace_bytes", M, N))
    call("tris_colsum_f32", P(X), M, N, N, P(out), P(ws), _stream())
    return out


def ew(op, A, B=None, s=0.0, out=None):
    _chk(A, B)
    out = torch.empty_like(A) if out is None else out
    h2_mark_next(out)
    call("tris_elementwise_f32", EW[op], P(A), P(B), P(out), A.numel(), float(s), _stream())
    return out


def nchw_to_nhwc(x):
    _chk(x)
    if x.dim() == 4 and x.permute(0, 2, 3, 1).is_contiguous():   # already channels-last in memory (tris_amd.dataset.hbm)
        return x.permute(0, 2, 3, 1)
    x = x.contiguous()
    B, C, H, W = x.shape
    y = torch.empty(B, H, W, C, device=x.device, dtype=x.dtype)
    call("tris_nchw_to_nhwc_f32", P(x), P(y), B, C, H, W, _stream())
    return y


# ----------------------------------------------------------------------------------------------- fused BN statistics
# A conv forward can emit the BatchNorm batch statistics of its output from the GEMM epilogue (tris_*_bnstat_f32).
# The fp64 partials travel from the conv Function to the BatchNorm Function as an attribute of the output tensor
# (`y._bn_part`, set inside the Function's forward: the object returned by apply() is that same tensor).
# The other records between the autograd nodes of the BatchNorm family (field order as the tests index them): `y._bn_lazy`, `y._bn_pair`
# (ops.batch_norm: y is unwritten, its one consumer normalises x itself; bound / word: amax word of an upper bound of the would-be
# contents, bound None outside h2; state: what the pair's two backward nodes talk through) and what _BnBwdLink.take() returns (the
# product's partial rows of the two sums, the amax word of the masked gradient, cfg.bn_pair: the rows of the shortcut's third sum)
_BN = [(f, torch.Tensor) for f in ("x", "mean", "invstd", "gamma", "beta")]   # (a BatchNorm: its input, statistics and parameters)
_BnPart = NamedTuple("_BnPart", [("part", torch.Tensor), ("rows", int)])
_BnLazy = NamedTuple("_BnLazy", _BN + [("bound", Optional[int])])
_BnPair = NamedTuple("_BnPair", _BN + [("word", int), ("state", object)])
_BnTaken = NamedTuple("_BnTaken", [("part", torch.Tensor), ("rows", int), ("dzw", Optional[int]), ("part2", Optional[torch.Tensor])])


class _BnPairState:
    """dx_pl, needs: what bn3's backward needs to know of its shortcut BatchNorm's (dx goes out as planes; needs_input_grad of x, gamma,
    beta); done = (dxs, in_arena_s, sums_s): where it leaves dx and the sums it formed for it"""
    __slots__ = ("dx_pl", "needs", "done")

    def __init__(self, dx_pl, needs):
        self.dx_pl, self.needs, self.done = dx_pl, needs, None


# What rides on a tensor across an autograd node that is an identity (SegmentedStep.cut, GradReducer.boundary): the hand-offs to the
# tensor's consumer and its plane / amax tags.  (`_bn_part` is read by the very next op; `_bn_pair` must not pass: carry)
RIDERS = ("_bn_link", "_bn_lazy", "_pl", "_h2")


def carry(src, dst):
    """dst is src behind an identity node: hand over what rides on src.  -> dst  (Not a `_bn_pair` stand-in: it holds no data, whoever
    reads dst without the hand-over reads garbage, and only a BatchNorm takes it.)"""
    if getattr(src, "_bn_pair", None) is not None:
        raise RuntimeError("the unwritten output of a paired shortcut BatchNorm goes to the block's bn3 and nowhere else")
    for attr in RIDERS:
        v = getattr(src, attr, None)
        if v is not None:
            setattr(dst, attr, v)
    return dst


def _part_rows(M, C, device):
    """what the statistics / BatchNorm-backward epilogue of an [M, C] product writes: fp64 partial rows (two sums per channel and 128 rows)
    and the word it leaves their number in (0: the entry point declined the shape, nothing was launched)"""
    return torch.empty(((M + 127) // 128) * 2 * C, device=device, dtype=torch.float64), ctypes.c_int(0)


def _launch_with_stats(y, M, N, launch, stats=True):
    """launch(part, rows) writes y [M, N]; stats: and leaves the BatchNorm statistics of y as partial rows -> y._bn_part"""
    if not stats:
        return launch(None, None)
    part, rows = _part_rows(M, N, y.device)
    launch(part, ctypes.byref(rows))
    if rows.value > 0:
        y._bn_part = _BnPart(part, rows.value)


def _bn_bwd_bufs(M, C, device, pair=None):
    """-> (part, rows, part2, dzw) of a data gradient that reduces for the BatchNorm behind it (_BnBwdLink): _part_rows, the rows of a paired
    shortcut BatchNorm's third sum (pair: its `_bn_pair`) and, with operand planes, the amax word of the masked gradient"""
    part, rows = _part_rows(M, C, device)
    return part, rows, (torch.empty_like(part) if pair is not None else None), (_h2_slot() if planes_on() else None)


def _declinable(name, *args):
    """call an entry point that may decline a shape: True if it ran, False if it returned TRIS_DECLINED (caller falls back)"""
    err = getattr(_lib.load(), name)(*args)
    if err == -2:   # TRIS_DECLINED
        return False
    if err != 0:
        raise _lib.TrisHipError(f"{name} failed with hipError_t {err}")
    return True


class GradBox:
    """Hand-off of a residual-branch gradient inside one block.  In `out = relu(bn3(f(x)) + x)` the tensor x has two
    consumers (f's first conv and the residual input of bn3); autograd would sum their two gradients with an extra
    elementwise pass over the activation.  Instead bn3's backward -- which always runs before the first conv's, because
    the latter depends on it through f -- leaves its residual gradient here, and the first conv's data-gradient GEMM adds
    it in its epilogue (`resid`).  Used by the identity Bottlenecks of the RN50 trunk.

    In the down-sampling Bottlenecks the second consumer of x is the shortcut (avg-pool / 1x1 conv); its backward normally
    runs before conv1's too (autograd schedules later-created nodes first) but nothing guarantees it, so the depositor
    checks `consumed` and simply returns its gradient to autograd if conv1 has already run.
    `pool` = (H, W): the value is the gradient of the 2x2 average pool of x (a stride-2 shortcut, cfg.bn_pair), a quarter of the size;
    conv1's epilogue reads it at the pooled pixel (tris_gemm_resid_pool_next) instead of a full-size expansion written for it."""
    __slots__ = ("value", "consumed", "pool")

    def __init__(self):
        self.value = None
        self.consumed = False
        self.pool = None

    def deposit(self, g):
        """-> True if the gradient was taken over (the caller must then return None for that input)"""
        if self.consumed or self.value is not None:
            return False
        self.value = g
        return True


# ----------------------------------------------------------------------------------------------- Linear / 1x1 conv
# ---- "h2" products (ops.set_gemm_mode("h2") / TRIS_GEMM_MODE=h2) -------------------------------------------
# Every product of the GEMM / convolution family with two fp16 pieces per operand and three f16 MFMAs (half the matrix work of
# x3).  fp16 holds 11 significand bits per piece but only 5 exponent bits, so every operand is scaled by a power of two derived --
# inside the kernel -- from the largest magnitude of its tensor; the residual piece is stored pre-scaled by 2^11, which keeps the
# representation fp32-class over a 2^27 range inside a tensor (csrc/x3_split.h).  The amax is a word in a pool, written
#   * by the pass that PRODUCES the tensor (BatchNorm apply / backward apply, LayerNorm, elementwise: h2_mark_next, no extra traffic),
#   * for all parameters of an optimiser arena by ONE launch per step; for other parameters (a frozen model) once, into a pool of
#     constants, until the parameter is written to,
#   * for a BatchNorm + ReLU folded into its consuming convolution -- a tensor that never exists -- as an upper bound from the affine
#     parameters (h2_bound_next),
#   * otherwise by a small pre-pass (tensors up to 128 MB).
# A product whose operands have no amax runs in x3.  A "step" is the life of the pool's words: h2_begin_step() clears the pool
# (train_step calls it; any other entry -- an evaluation forward, a lone op in a test -- starts one on first use or when the pool
# is full).
class _H2State:
    """the state of the amax pools: one instance, _H2, every field declared here with its default"""
    __slots__ = ("pool", "next", "base", "step", "paused", "in_step", "auto_lock", "auto_grad", "auto_pools", "private", "limit", "arenas",
                 "plane_numel", "const", "const_next", "const_tags")

    def __init__(self):
        self.pool, self.next, self.base, self.step = None, 0, -1, 0   # the step's words, the next one to hand out, the first one behind the arenas', the step id
        self.paused = 0                                               # depth of h2_paused / batch_invariant scopes
        self.in_step = self.auto_lock = self.auto_grad = False        # inside an explicit step / h2_auto_lock; the step is a gradient-mode forward's own
        self.auto_pools = {}                                          # step id -> retired pool, oldest first (H2_AUTO_KEEP)
        self.private, self.limit = False, None                        # inside h2_private_pool, and its number of words
        self.arenas, self.plane_numel = [], {}                        # the arenas the step tagged; word -> elements of the plane tensors written in it
        self.const, self.const_next, self.const_tags = None, 0, {}    # the constant words: id(parameter) -> _ConstWord

    def swap(self, **new):
        """set the fields named -> what restore() puts back: those fields and no other"""
        saved = {k: getattr(self, k) for k in new}
        self.restore(new)
        return saved

    def restore(self, saved):
        for k, v in saved.items():
            setattr(self, k, v)


_H2 = _H2State()
_H2_STEP_IDS = [0]       # step ids are unique across the main pool and private pools: a tag never matches another pool's step
# What rides on tensors and parameters.  Each is written in ONE place: t._h2 by h2_tag, t._pl by pl_tag, p._plw / p._plwt by h2_begin_step
_AmaxTag = NamedTuple("_AmaxTag", [("step", int), ("word", int), ("version", int)])          # t._h2: t's amax is in `word` while t is unwritten
_PlaneTag = NamedTuple("_PlaneTag", [("step", int), ("word", int), ("ptr", int)])            # t._pl: t's bytes are planes scaled by `word`
_WeightPlanes = NamedTuple("_WeightPlanes", [("step", int), ("ptr", int), ("word", int)])    # p._plw / p._plwt: an arena parameter's (transposed) planes
_PlaneGrad = NamedTuple("_PlaneGrad", [("step", int), ("word", int), ("shape", tuple)])      # _PL_GRAD entries
H2_SLOTS = 4096          # amax words per step; a word is H2_SUB unsigned words (csrc/amax.h amax_raise)
H2_SUB = 2048
H2_CONST_SLOTS = 1024
H2_PREPASS_MAX = 1 << 25
H2_AUTO_KEEP = 4         # retired pools of gradient-mode forwards issued outside an explicit step (h2_begin_step)


def h2_on():
    return _ARITH == "h2" and not _H2.paused and not _thread_mode_is_set()


_H2_ARENAS = []   # weak references to the optimiser arenas whose parameters get their amax from ONE launch per step


def h2_register_arena(arena):
    """an optimiser arena (tris_amd.optim.Arena: .p flat parameter buffer, .params, .offsets).  Its parameters are updated in
    place by kernels that do not bump torch's version counters, so they never get a CONSTANT amax word (_h2_const_slot)."""
    r = weakref.ref(arena)
    _H2_ARENAS.append(r)
    for p in arena.params:
        p._tris_arena = r       # (the LATEST arena a parameter was put into: an optimiser built later supersedes an earlier one)


def _h2_live_arenas():
    """the registered arenas that still own their parameters (an optimiser object that was superseded by a newer one over the same
    parameters, or is only kept alive by a reference cycle, is not one), newest first, as many as fit half the pool"""
    out, words = [], 0
    for r in reversed(list(_H2_ARENAS)):
        a = r()
        if a is None or not a.params or getattr(a.params[0], "_tris_arena", None) is not r:
            _H2_ARENAS.remove(r)
        elif _H2.pool is not None and a.p.device == _H2.pool.device and words + len(a.params) <= H2_SLOTS // 2:
            out.append(a)
            words += len(a.params)
    return out


# _ArenaPlanes: the parameters of an optimiser arena that exist as operand planes too (csrc/planes.h) -- `idx` --, their segment tables on the
# device and the plane buffer (None: no such parameter).  _ArenaWords: what the per-step launches of one arena read, built once per arena:
# the offsets and sizes of its parameters on the device and, from the first step with operand planes on, the planes of its convolution
# weights (`pl`) and of its 1x1 weights TRANSPOSED (`plt`: their data gradient dX = dY . W is then the forward's row-major A x B^T product)
_ArenaPlanes = NamedTuple("_ArenaPlanes", [("idx", list), ("seg", tuple), ("buf", Optional[torch.Tensor]), ("attr", str)])
_ArenaWords = NamedTuple("_ArenaWords", [("seg", tuple), ("pl", Optional[_ArenaPlanes]), ("plt", Optional[_ArenaPlanes])])
_ARENA_WORDS = weakref.WeakKeyDictionary()


def _arena_words(a):
    mk = lambda v: torch.tensor(v, device=a.p.device, dtype=torch.int64)
    planes = lambda attr, idx, *cols: _ArenaPlanes(idx, tuple(mk([c(i) for i in idx]) for c in cols) if idx else None,
                                                   torch.zeros_like(a.p) if idx else None, attr)
    r = _ARENA_WORDS.get(a) or _ArenaWords((mk(list(a.offsets)), mk([p.numel() for p in a.params])), None, None)
    if r.pl is None and cfg.h2_planes:
        idx = [i for i, p in enumerate(a.params) if _pl_weight_ok(p)]
        idt = [i for i in idx if _pl_weight_t_ok(a.params[i])]
        r = r._replace(pl=planes("_plw", idx, lambda i: a.offsets[i], lambda i: a.params[i].numel(), lambda i: i),
                       plt=planes("_plwt", idt, lambda i: a.offsets[i], lambda i: a.params[i].shape[0], lambda i: a.params[i].shape[1], lambda i: i))
    _ARENA_WORDS[a] = r
    return r


def h2_weights_amax(arenas=None, tag=False):
    """(re)compute the amax words of the arenas' parameters -- the first words of the pool, in order -- and with them their planes: for
    each arena its record, then up to three launches.  arenas: the list a captured step recorded (its launches read those words);
    default: the live registered ones.  tag (h2_begin_step): the parameters are tagged with their words and planes.  -> the words used"""
    base = 0
    for a in (_h2_live_arenas() if arenas is None else arenas):
        r, words = _arena_words(a), _H2.pool.data_ptr() + 4 * H2_SUB * base
        call("tris_amax_segments_f32", P(a.p), *(t.data_ptr() for t in r.seg), len(a.params), words, _stream())
        for pl, entry in ((r.pl, "tris_h2_planes_segments_f32"), (r.plt, "tris_h2_planes_t_segments_f32")) if cfg.h2_planes else ():
            if pl.idx:
                call(entry, P(a.p), *(t.data_ptr() for t in pl.seg), len(pl.idx), words, P(pl.buf), _stream())
            for i in (pl.idx if tag else ()):
                setattr(a.params[i], pl.attr, _WeightPlanes(_H2.step, pl.buf.data_ptr() + 4 * a.offsets[i], words + 4 * H2_SUB * i))
                _H2.plane_numel[words + 4 * H2_SUB * i] = a.params[i].numel()
        for i, p in enumerate(a.params if tag else ()):
            h2_tag(p, words + 4 * H2_SUB * i)
        base += len(a.params)
    return base


def _pl_weight_t_ok(p):
    """a 1x1-convolution weight [Cout, Cin, 1, 1] whose transposed planes exist (64 x 64 tiles of the transposing pass)"""
    if p.dim() == 2:     # a Linear weight [N, K] of a tower whose products run on planes (VisionTransformer marks them)
        return cfg.gemm_convert > 0 and getattr(p, "_tris_linear_w", False) and p.shape[0] % 64 == 0 and p.shape[1] % 64 == 0
    return p.dim() == 4 and p.shape[2] * p.shape[3] == 1 and p.shape[0] % 64 == 0 and p.shape[1] % 64 == 0


def _pl_weight_ok(p):
    """a parameter that dense products of the trunk read as fp16 operand planes: a convolution weight [Cout, Cin, kh, kw] whose
    contiguous dimension (Cin: channels_last memory) is a multiple of 8"""
    if p.dim() == 2:     # (round 6) a Linear weight [N, K], K contiguous: the same geometry as a 1x1 convolution's
        return cfg.gemm_convert > 0 and getattr(p, "_tris_linear_w", False) and p.shape[1] % 8 == 0 and p.is_contiguous()
    return p.dim() == 4 and p.shape[1] % 8 == 0 and (p.is_contiguous(memory_format=torch.channels_last) or p.shape[2] * p.shape[3] == 1)


def _a_planes(A, M, K):
    """(round 6, cfg.gemm_convert) The row-major A operand [M, K] of a large product against a weight that exists as planes, converted
    to planes ONCE in a pass of its own (tris_h2_planes_f32: 4 bytes read + 4 written per element) so that the product runs on the
    LDS-DMA loop with no split in its K loop -- every column tile of the product would otherwise re-split the same rows (a ViT-B/16
    trunk product has 6 ... 24 of them).  Measured per shape in profiles/r6_vit_planes_bench.txt (x1.2 ... 1.57 for the product, 5 ... 13 us
    for the pass at 2400 rows).  Returns the plane tensor (tagged with A's amax word) or A itself where A has no word."""
    slot = _h2_amax(A)
    if slot is None:
        return A
    t = torch.empty_like(A)
    call("tris_h2_planes_f32", P(A), P(t), A.numel(), slot, _stream())
    PL_STATS["converted"] += 1
    return pl_tag(t, slot)


def _h2_new_step_id():
    _H2_STEP_IDS[0] += 1
    return _H2_STEP_IDS[0]


def h2_begin_step(explicit=True):
    """A fresh amax pool (one memset) + the weights' amaxes (one launch per optimiser arena).  Returns the pool (None when the
    arithmetic is not h2).  Whatever was issued earlier on a side stream may still read the words about to be cleared: the
    current stream first waits for the side streams.  explicit: the caller brackets a whole step (h2_end_step closes it)."""
    if _ARITH != "h2":
        return None
    _H2.in_step = bool(explicit)
    wgrad_join()
    dev = torch.device("cuda", torch.cuda.current_device())
    # A forward issued OUTSIDE an explicit step with gradients on may still have its autograd graph -- and the plane tensors saved in
    # it -- alive when the next such forward begins (gradient accumulation, a drop-in user summing the losses of two forwards before
    # one backward: legal PyTorch).  Its pool is then RETIRED, not cleared: the words stay what the saved plane tensors were written
    # under (pl_word accepts the H2_AUTO_KEEP most recent retired steps) and the new forward gets a fresh pool.
    live = _H2.auto_pools
    if _H2.pool is None or _H2.pool.device != dev:
        _H2.pool = torch.zeros(H2_SLOTS * H2_SUB, device=dev, dtype=torch.int32)
        live.clear()
    elif not explicit and _H2.auto_grad and not _H2.private and not torch.cuda.is_current_stream_capturing():
        live[_H2.step] = _H2.pool
        while len(live) > H2_AUTO_KEEP:
            live.pop(next(iter(live)))
        _H2.pool = torch.zeros(H2_SLOTS * H2_SUB, device=dev, dtype=torch.int32)
    else:
        if explicit:
            live.clear()
        _H2.pool.zero_()
    _H2.auto_grad = (not explicit) and torch.is_grad_enabled() and not _H2.private
    _H2.step = _h2_new_step_id()
    _H2.plane_numel = {}
    _PL_GRAD.clear()
    _H2.arenas = _h2_live_arenas() if not _H2.private else []
    _H2.next = _H2.base = h2_weights_amax(_H2.arenas, tag=True)
    return _H2.pool


def h2_end_step():
    """the explicit step ends: the words stay valid until the next begin; forwards issued outside a step start their own again"""
    _H2.in_step = False


def h2_step_open():
    """inside an explicit step or a private pool: whoever asks must not begin a step of its own"""
    return _H2.in_step or _H2.private


def h2_step_arenas():
    """the arenas whose parameters the open step tagged (a captured step keeps them for h2_weights_amax)"""
    return list(_H2.arenas)


def h2_pool_state():
    """a snapshot for tools/h2_step_trace.py: where the pools lie (the retired ones oldest first), the hand-out counters and the step id"""
    ptr = lambda t: None if t is None else t.data_ptr()
    return {"pool": ptr(_H2.pool), "retired": [ptr(p) for p in _H2.auto_pools.values()], "const": ptr(_H2.const), "private": _H2.private,
            "limit": _H2.limit, "next": _H2.next, "base": _H2.base, "step": _H2.step}


@contextlib.contextmanager
def h2_fresh_consts():
    """a scope with a pool of constant words of its own (launch traces: which word a parameter gets does not depend on what ran before)"""
    saved = _H2.swap(const=None, const_next=0, const_tags={})
    try:
        yield
    finally:
        _H2.restore(saved)


def h2_auto_step():
    """Called where a training forward STARTS (TRIS.forward, ModifiedResNet.forward_cl).  With operand planes a forward must not
    straddle two pools -- a plane tensor is only meaningful with the word of the pool it was written under -- so a forward issued
    OUTSIDE an explicit step (train_step brackets its own with h2_begin_step / h2_end_step) begins a fresh step of its own instead
    of running into a half-used pool that restarts mid-way.  No-op inside an explicit step, when planes are off, and when nothing
    has been handed out since the last begin.  Returns True if a step was begun (the caller's nested forwards must not begin another:
    h2_auto_lock)."""
    if not planes_on() or _H2.in_step or _H2.auto_lock or _H2.private:
        return False
    if _H2.pool is not None and _H2.next == _H2.base:
        return False
    h2_begin_step(explicit=False)
    return True


class h2_auto_lock:
    """inside: nested forwards do not begin a step of their own (TRIS.forward around its trunk call)"""

    def __enter__(self):
        self.prev = _H2.auto_lock
        _H2.auto_lock = True

    def __exit__(self, *a):
        _H2.auto_lock = self.prev


class h2_step:
    """with h2_step(): the region is one h2 step -- begun here unless a step is already open (an enclosing train step, a private
    pool) or the arithmetic is not h2, and closed on exit.  explicit=False: begun like a forward issued outside a step (its pool is
    retired, not cleared, while an autograd graph may still hold its words) and not closed."""

    def __init__(self, explicit=True):
        self.explicit, self.mine = explicit, False

    def __enter__(self):
        self.mine = h2_on() and not h2_step_open()
        if self.mine:
            h2_begin_step(explicit=self.explicit)
        return self

    def __exit__(self, *exc):
        if self.mine and self.explicit:
            h2_end_step()
        return False


class h2_private_pool:
    """Products launched inside take their per-step amax words from a pool of their own, cleared on entry: a region that is
    captured into a hipGraph of its own and replayed outside the steps it was recorded in (the frozen aux text tower) must not
    hold words of the per-step pool.  Parameters inside get constant words (they must not be arena parameters of a live step)."""

    def __init__(self, slots=512):
        self.slots, self.pool = slots, None

    def __enter__(self):
        self.active = _ARITH == "h2"
        if not self.active:
            return self
        dev = torch.device("cuda", torch.cuda.current_device())
        if self.pool is None or self.pool.device != dev:
            self.pool = torch.zeros(self.slots * H2_SUB, device=dev, dtype=torch.int32)
        self.pool.zero_()
        self.saved = _H2.swap(pool=self.pool, next=0, step=_h2_new_step_id(), arenas=[], private=True, limit=self.slots)
        return self

    def reset(self):
        """clear the words and hand them out from the first again (call it as the first thing INSIDE a capture of the region: the
        memset is then part of the graph, and the words are handed out in the same order at every recording)"""
        if self.active:
            self.pool.zero_()
            _H2.next, _H2.step = 0, _h2_new_step_id()

    def __exit__(self, *exc):
        if self.active:
            _H2.restore(self.saved)
        return False


class h2_paused:
    """products launched inside run in x3"""

    def __enter__(self):
        _H2.paused += 1

    def __exit__(self, *a):
        _H2.paused -= 1


def _h2_slot():
    limit = _H2.limit or H2_SLOTS
    if _H2.pool is None or (_H2.next >= limit and not _H2.private):
        h2_begin_step(explicit=_H2.in_step)          # first use outside a training step, or the pool is full: a new step
    i = _H2.next
    if i >= limit:
        return None              # (a private pool is never restarted: its region would lose words it still reads)
    _H2.next = i + 1
    return _H2.pool.data_ptr() + 4 * H2_SUB * i


def h2_mark_next(t):
    """call right BEFORE the launch that writes `t` (BatchNorm apply-type passes, LayerNorm, elementwise): that launch also
    leaves t's amax in a pool word"""
    if t is None or not h2_on():
        return
    slot = _h2_slot()
    if slot is None:
        return
    call("tris_amax_next", slot)
    h2_tag(t, slot)


def h2_tag(t, word, step=None):
    """THE writer of t._h2: t's amax is in `word` of the running step (step: of that one -- a tag put back) until t is written to"""
    t._h2 = _AmaxTag(_H2.step if step is None else step, word, t._version)


def _h2_tag_slot(t):
    tag = getattr(t, "_h2", None)
    if tag is not None and tag.step == _H2.step and tag.version == t._version:
        return tag.word
    return None


# The two caches of parameters outside the optimiser arenas, both keyed by id(parameter): its constant amax word and its planes
_ConstWord = NamedTuple("_ConstWord", [("version", int), ("ptr", int), ("word", int), ("ref", weakref.ref)])
_ConstPlanes = NamedTuple("_ConstPlanes", [("version", int), ("ptr", int), ("word", int), ("planes", torch.Tensor), ("ref", weakref.ref)])


def _still_is(entry, t):
    """is this cache entry (of id(t)) still THIS live parameter at this address?  (an id is handed out again once its object is gone)"""
    return entry is not None and entry.ptr == t.data_ptr() and entry.ref() is t


def _h2_const_slot(t):
    """amax word of a parameter outside the optimiser arenas (a frozen model's): computed once, valid until it is written to"""
    tag = _H2.const_tags.get(id(t))
    if _still_is(tag, t) and _H2.const is not None and _H2.const.device == t.device:
        if tag.version != t._version:
            # written to since (load_state_dict, seed_fill): refresh the SAME word on the stream -- a hipGraph that recorded its address
            # (the frozen aux text tower, the evaluation graphs) goes on reading a valid amax, and no new slot is used up
            i = (tag.word - _H2.const.data_ptr()) // (4 * H2_SUB)
            _H2.const[i * H2_SUB:(i + 1) * H2_SUB].zero_()
            call("tris_amax_bits_f32", P(t), t.numel(), tag.word, _stream())
            _H2.const_tags[id(t)] = tag._replace(version=t._version)
        return tag.word
    if _H2.const is None or _H2.const.device != t.device:
        _H2.const = torch.zeros(H2_CONST_SLOTS * H2_SUB, device=t.device, dtype=torch.int32)
        _H2.const_next = 0
        _H2.const_tags.clear()
    if _H2.const_next >= H2_CONST_SLOTS:
        return None
    slot = _H2.const.data_ptr() + 4 * H2_SUB * _H2.const_next
    _H2.const_next += 1
    call("tris_amax_bits_f32", P(t), t.numel(), slot, _stream())
    _H2.const_tags[id(t)] = _ConstWord(t._version, t.data_ptr(), slot, weakref.ref(t))
    return slot


def _h2_amax(t):
    slot = _h2_tag_slot(t)
    if slot is not None:
        return slot
    dense = t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))
    if not (t.numel() <= H2_PREPASS_MAX and dense and t.data_ptr() % 16 == 0 and t.numel() > 0):
        return None
    if isinstance(t, torch.nn.Parameter) and not getattr(t, "_tris_arena", False):
        slot = _h2_const_slot(t)
        if slot is not None:
            return slot
    slot = _h2_slot()
    if slot is None:
        return None
    call("tris_amax_bits_f32", P(t), t.numel(), slot, _stream())
    try:
        h2_tag(t, slot)
    except AttributeError:
        pass
    return slot


def h2_arm(A, B, a_slot=None, b_slot=None):
    """before a dense product of A and B: run it in h2 if both operands have an amax (one shot, this thread).  a_slot / b_slot: the
    operand's amax word where the tensor itself is not at hand (a BatchNorm folded into the consuming convolution)"""
    if not h2_on():
        return False
    a = a_slot if a_slot is not None else (_h2_amax(A) if A is not None else None)
    b = None
    if a is not None:
        b = b_slot if b_slot is not None else (_h2_amax(B) if B is not None else None)
    if a is None or b is None:
        return False
    call("tris_h2_next", a, b, 0.0, 0.0)
    return True


# ---- operand planes (csrc/planes.h, DESIGN.md "operand planes") --------------------------------------------------------------
# In h2 the activations of the RN50 trunk between a BatchNorm and the convolutions that read it, the gradients between a BatchNorm
# backward and the convolution backward that reads it, and the convolution weights exist as fp16 PIECE PLANES: float32 tensors in
# torch's eyes whose bytes are the two fp16 pieces of every element, scaled by the power of two their amax word implies.  The tensor
# carries `_pl`, a _PlaneTag; only the ops below that say so accept one, everything else must see `unplanes(t)`.
PL_STATS = {"unplanes": 0, "dx_planes": 0, "dy_planes": 0, "products": 0, "mixed": 0, "converted": 0}


_HAS_GPU = None


def planes_on():
    global _HAS_GPU
    if _HAS_GPU is None:
        _HAS_GPU = torch.cuda.is_available()     # (host-logic tests run the model's control flow on CPU stand-ins)
    return _HAS_GPU and cfg.h2_planes and h2_on() and not _BATCH_INVARIANT


def pl_word(t):
    """amax word of a plane tensor (None: `t` is an ordinary fp32 tensor)"""
    tag = getattr(t, "_pl", None) if t is not None else None
    if tag is None:
        return None
    if (tag.step != _H2.step and tag.step not in _H2.auto_pools) or tag.ptr != t.data_ptr():
        raise RuntimeError("a plane tensor outlived the step whose amax pool scales it")
    return tag.word


def _pl_write(t, step, word, ptr):
    """THE writer of t._pl, and of the amax tag that goes with it"""
    t._pl = _PlaneTag(step, word, ptr)
    h2_tag(t, word, step)
    return t


def pl_tag(t, word):
    _H2.plane_numel[word] = t.numel()
    return _pl_write(t, _H2.step, word, t.data_ptr())


def h2_range_report(threshold=0.01):
    """Range tell-tale of the plane tensors WRITTEN since the last h2_begin_step (host sync; csrc/planes.h): an element is held with
    its full 22 bits only down to 2^-27 of its tensor's scaled bound; the writing passes count the non-zero elements below that floor.
    -> {"plane_tensors", "elements", "elements_below_floor", "max_fraction_below_floor", "out_of_range_operands"} where the last is the
    number of tensors with more than `threshold` of their elements in the absolute-accuracy regime (bench.py prints it as
    h2_out_of_range_operands; the B = 48 parity test asserts 0)."""
    numel, pool = _H2.plane_numel, _H2.pool
    if pool is None or not numel:
        return {"plane_tensors": 0, "elements": 0, "elements_below_floor": 0, "max_fraction_below_floor": 0.0, "out_of_range_operands": 0}
    torch.cuda.synchronize()
    base = pool.data_ptr()
    words = sorted(numel)
    idx = torch.tensor([(w - base) // (4 * H2_SUB) for w in words], device=pool.device, dtype=torch.int64)
    cnt = pool.view(-1, H2_SUB)[idx][:, 1::16].to(torch.int64).sum(1).cpu().tolist()
    fr = [c / max(numel[w], 1) for c, w in zip(cnt, words)]
    return {"plane_tensors": len(words), "elements": int(sum(numel.values())), "elements_below_floor": int(sum(cnt)),
            "max_fraction_below_floor": max(fr), "out_of_range_operands": sum(1 for f in fr if f > threshold)}


def _unplanes_raw(t, cache=True):
    w = pl_word(t)
    c = getattr(t, "_pl_f32", None) if cache else None
    if c is None:
        c = torch.empty_like(t)
        call("tris_h2_unplanes_f32", P(t), P(c), t.numel(), w, _stream())
        h2_tag(c, w)   # (the word bounds the rebuilt values as well)
        if cache:
            t._pl_f32 = c
        PL_STATS["unplanes"] += 1
    return c


class _UnplanesFn(torch.autograd.Function):
    """differentiable form of unplanes: the gradient of the rebuilt tensor IS the gradient of the plane tensor (fp32 either way)"""

    @staticmethod
    def forward(ctx, t):
        return _unplanes_raw(t, cache=False)

    @staticmethod
    def backward(ctx, g):
        return g


def unplanes(t):
    """the fp32 tensor a plane tensor stands for (its h2 operand rounding: 22 significand bits); fp32 tensors pass through"""
    if pl_word(t) is None:
        return t
    if t.requires_grad and torch.is_grad_enabled():
        return _UnplanesFn.apply(t)
    return _unplanes_raw(t)


_PL_CONST = {}   # id(parameter) -> _ConstPlanes: parameters outside the optimiser arenas


def _pl_weight(w):
    """(pointer to the planes of a convolution weight, its amax word) or None"""
    tag = getattr(w, "_plw", None)
    if tag is not None and tag.step == _H2.step:
        return tag.ptr, tag.word
    if not _pl_weight_ok(w):
        return None
    word = _h2_amax(w)
    if word is None:
        return None
    c = _PL_CONST.get(id(w))
    if _still_is(c, w) and c.version == w._version and c.word == word:
        return c.planes.data_ptr(), word
    wc = cl_weight(w)
    pl = torch.empty(wc.numel(), device=w.device, dtype=torch.float32)
    call("tris_h2_planes_f32", wc.data_ptr(), P(pl), wc.numel(), word, _stream())
    if len(_PL_CONST) > 4096:
        _PL_CONST.clear()
    _PL_CONST[id(w)] = _ConstPlanes(w._version, w.data_ptr(), word, pl, weakref.ref(w))
    return pl.data_ptr(), word


def _retag(t, tag):
    """a tensor that comes back from ctx.saved_tensors keeps its plane tag (set again in case autograd re-wrapped the object)"""
    if tag is not None and t is not None and getattr(t, "_pl", None) is None:
        _pl_write(t, *tag)
    return t


_PL_GRAD = {}   # data_ptr -> _PlaneGrad: gradients a BatchNorm backward wrote as planes, until their one consumer takes them


_PL_GRAD_CB = [False]


def _pl_grad_end_of_backward():
    """ runs when the autograd pass that registered plane gradients ends: an entry that is still there found no
    plane-aware consumer -- its bytes were read as fp32 by whoever took the tensor, and the address-keyed tag would wait for an
    unrelated gradient that reuses the address.  Never silent: drop the entries and raise."""
    _PL_GRAD_CB[0] = False
    if _PL_GRAD:
        left = [(hex(k), v.shape) for k, v in _PL_GRAD.items()]
        _PL_GRAD.clear()
        raise RuntimeError(f"plane gradients without a plane-aware consumer at the end of backward: {left[:4]}")


def pl_grad_out(t, word):
    pl_tag(t, word)
    _PL_GRAD[t.data_ptr()] = _PlaneGrad(_H2.step, word, tuple(t.shape))
    PL_STATS["dx_planes"] += 1
    if not _PL_GRAD_CB[0]:
        try:   # (inside an autograd pass: BatchNormFn.backward calls this)
            torch.autograd.Variable._execution_engine.queue_callback(_pl_grad_end_of_backward)
            _PL_GRAD_CB[0] = True
        except RuntimeError:
            pass
    return t


def pl_grad_in(dy):
    """the gradient a backward is handed: tag it as a plane tensor if a BatchNorm backward wrote it as one (one consumer: the entry
    is taken).  Returns dy."""
    ent = _PL_GRAD.pop(dy.data_ptr(), None)
    if ent is not None and ent.step == _H2.step and ent.shape == tuple(dy.shape):
        if getattr(dy, "_pl", None) is None:
            _pl_write(dy, ent.step, ent.word, dy.data_ptr())
        PL_STATS["dy_planes"] += 1
    elif getattr(dy, "_pl", None) is not None:
        raise RuntimeError("a plane gradient reached a second consumer")
    return dy


# _Operands: what h2_pp hands the caller of a dense product -- the pointers of A and B to give the entry point, whether the product just
# armed takes planes, and whether B (a 1x1 weight used as [k][n]) arrived as the planes of its TRANSPOSE: the product then runs with B as [n][k]
_Operands = NamedTuple("_Operands", [("a", Optional[int]), ("b", Optional[int]), ("planes", bool), ("b_t", bool)])


def h2_pp(A, B, a_slot=None, b_slot=None, y_planes=False, w_a=False, w_b=False, k_red=32, w_bt=False, y_mask=False):
    """Arm the next dense product for h2 (as h2_arm) and return the _Operands to hand to the entry point.  With
    operand planes on: if one operand IS a plane tensor and the other one is too, or is a convolution weight (w_a / w_b: that
    operand is a parameter), the product runs on planes; a plane tensor next to an fp32 operand is rebuilt (counted in PL_STATS).
    k_red: the reduction length of the product -- the plane kernels (the fast kernels) need a multiple of 32; anything else (the weight
    gradients of a 10 x 10 map at batch 2: 200 pixels) runs on the rebuilt tensors through the generic kernel.
    w_bt: B is a 1x1 weight used as [k][n] (a data gradient): if its TRANSPOSED planes exist the caller gets those (_Operands.b_t)."""
    if A is None or B is None or a_slot is not None or b_slot is not None or not planes_on() or k_red % 32 != 0:
        if pl_word(A) is not None or pl_word(B) is not None:
            A, B = unplanes(A), unplanes(B)
        h2_arm(A, B, a_slot, b_slot)
        return _Operands(P(A), P(B), False, False)
    wa, wb = pl_word(A), pl_word(B)
    if wa is not None or wb is not None:
        pa = (P(A), wa) if wa is not None else (_pl_weight(A) if w_a else None)
        pb = (P(B), wb) if wb is not None else (_pl_weight(B) if w_b else None)
        b_t = False
        if w_bt and wb is None and pa is not None:
            tt = getattr(B, "_plwt", None)
            if tt is not None and tt.step == _H2.step:
                pb, b_t = (tt.ptr, tt.word), True
        if pa is not None and pb is not None:
            call("tris_h2_next_planes", pa[1], pb[1], (1 if y_planes else 0) | (2 if b_t else 0) | (4 if y_mask else 0))
            PL_STATS["products"] += 1
            return _Operands(pa[0], pb[0], True, b_t)
        PL_STATS["mixed"] += 1
        A, B = unplanes(A), unplanes(B)
    h2_arm(A, B)
    return _Operands(P(A), P(B), False, False)


class _BnBwdLink:
    """Hand-off between a train-mode BatchNorm(+ReLU) and the 1x1 convolution / Linear that consumes its output.

    The BatchNorm backward needs sum(dz), sum(dz * xhat) over the whole batch before it can form dx -- a reduction pass over dy
    and x of its own (col_partial_kernel<1>).  Where dy is produced by a 1x1-convolution data gradient, that GEMM's epilogue has
    every dy value in registers: tris_gemm_bnbwd_f32 masks it there, stores the masked gradient dz and leaves the two sums as
    per-tile fp64 partial rows, and the BatchNorm backward is the apply pass alone.  Forward: BatchNormFn.forward hangs a link on
    its output tensor, ops.linear picks it up from its input.  Backward: LinearFn.backward fills it (dz tensor, partial rows),
    BatchNormFn.backward uses it iff the gradient it is handed IS that tensor, unmodified (same storage, same version counter:
    a second consumer's gradient accumulated into it by autograd changes one of the two) -- otherwise the usual two passes run
    on whatever arrived, which is why the masked gradient is only ever produced when the BatchNorm is known to be behind it.
    The model marks the BatchNorms whose output has exactly one autograd consumer (Bottleneck: bn2 -> conv3; bn3 -> the next
    block's conv1, the residual branch rides a GradBox) with bwd_link=True."""
    __slots__ = ("x", "mean", "invstd", "gamma", "beta", "from_y", "dz", "part", "rows", "dzw", "mask", "pair", "part2")

    def __init__(self, x, mean, invstd, gamma, beta, from_y):
        # (no reference to the BatchNorm's OUTPUT, which carries this object: the consumer has that tensor as its own input)
        self.x, self.mean, self.invstd, self.gamma, self.beta, self.from_y = x, mean, invstd, gamma, beta, from_y
        self.dz = self.part = self.dzw = None
        self.rows = 0
        self.mask = None      # (cfg.bn_bitmask) the ReLU mask of the BatchNorm's plane output, one byte per 8 channels (tris_bn_mask_next)
        # (cfg.bn_pair) bn3 of a down-sampling Bottleneck: the `_bn_pair` hand-over of its shortcut BatchNorm, which receives the same
        # masked gradient -- the product also reduces sum(dz * xhat_s) (tris_gemm_bnbwd_x2_next), into part2
        self.pair = self.part2 = None

    def fill(self, dz, part, rows, dzw=None, part2=None):
        # (identity of the gradient tensor, not a reference to it: autograd hands a sole-owner gradient on without a copy)
        # dzw: amax word of the masked gradient (operand planes: the bound of the BatchNorm's dx is formed from it)
        self.dz, self.part, self.rows, self.dzw = (dz.data_ptr(), dz._version, tuple(dz.shape)), part, rows, dzw
        self.part2 = part2

    def take(self, dy):
        """_BnTaken if dy IS the masked gradient this link's product left (same storage, version and shape); None if no product
        filled the link -- or if what arrives is something else: a second consumer's gradient was added to it by autograd (a
        down-sampling block whose shortcut backward ran late, a model that uses the BatchNorm output twice).  The caller then runs
        the usual two passes on whatever arrived, which is correct for any sum of gradients (the ReLU mask is idempotent: masking
        an already-masked term again changes nothing).  One use."""
        dz, part, rows, dzw, part2 = self.dz, self.part, self.rows, self.dzw, self.part2
        self.dz = self.part = self.dzw = self.part2 = None
        if dz is None or (dy.data_ptr(), dy._version, tuple(dy.shape)) != dz:
            return None
        return _BnTaken(part, rows, dzw, part2)


# ---- the steps of a Linear / 1x1 convolution and what the dense-product Functions share (LinearFn, LinearQGeluFn, Conv3x3Fn)
# _LinOpts: what ops.linear tells LinearFn beyond the tensors autograd must see (one argument of apply).  act: 0 none | 1 ReLU | 2 QuickGELU
# (forward-only); stats: leave the BatchNorm statistics of the output; grad_box / grad_box_out / grad_box_res (GradBox): where a later layer
# left a gradient of x / where dx goes / where the residual's gradient goes; bn_link (_BnBwdLink), act_link (_ActLink): what x is the output of
_LinOpts = NamedTuple("_LinOpts", [("act", int), ("stats", bool), ("grad_box", object), ("grad_box_out", object), ("grad_box_res", object),
                                   ("bn_link", object), ("act_link", object)])


def _bn_link_of(x):
    """the `_bn_link` riding on x, if the consumer's data gradient may reduce for that BatchNorm"""
    link = getattr(x, "_bn_link", None)
    return link if (link is not None and torch.is_grad_enabled() and x.requires_grad and cfg.bn_bwd_fuse) else None


def _lin_fwd_stats(x, w, y, M, N, K, part, rows):
    def launch():
        pp = h2_pp(x, w, w_b=True, k_red=K)
        call("tris_gemm_bnstat_f32", pp.a, pp.b, P(y), M, N, K, part.data_ptr(), rows, _stream())
    _timed("gemm", 2.0 * M * N * K, launch, nbytes=4.0 * (M * K + K * N + M * N), tag=_shape_tag(f"bnstat M{M} N{N} K{K}"))


def _grad_forms(dy, x, x_pl, fp32_dy, planes_x=False):
    """-> dy, x: the gradient a product's backward is handed and the input it saved (plane tag x_pl) in the forms its kernels read: dy fp32 if
    fp32_dy (or, planes_x, if x is no plane tensor); a plane x next to an fp32 dy rebuilt (vis_project: the weight gradient reads that)"""
    dy = pl_grad_in(dy.contiguous())
    _retag(x, x_pl)
    if pl_word(dy) is not None and (fp32_dy or (planes_x and pl_word(x) is None)):
        dy = unplanes(dy)
    if pl_word(dy) is None:
        x = unplanes(x)
    return dy, x


def _lin_resid_grad(dy, box, needed, wgrad_reads_dy):
    """the gradient of a residual added in the forward's epilogue: dy itself; None if not needed or taken over by `box`"""
    if not needed:
        return None
    if box is not None and box.deposit(dy):
        return None    # picked up by the block's LayerNorm backward (read-only there: no copy needed)
    if _wgrad_enabled() and wgrad_reads_dy:
        # dy is about to be read by the weight-gradient stream; autograd may accumulate IN PLACE into a gradient
        # tensor it is handed back (InputBuffer steals sole-owner tensors), so the residual branch gets its own copy
        return dy.clone()
    return dy


def _box_take(box):
    """empty the GradBox of a product's input -> (extra, pool): a residual-branch gradient left by a later layer of the same block, to
    be added in the data gradient's epilogue, and (H, W) if it is given as the gradient of its 2x2 average pool (GradBox.pool)"""
    extra = pool = None
    if box is not None:
        box.consumed = True
        if box.value is not None:
            extra, pool, box.value, box.pool = box.value, box.pool, None, None
    return extra, pool


def _lin_dgrad_bnbwd(dy, x, w, dx, dims, link, extra, pool):
    """dx = mask(dy . W + extra) with the sums of the BatchNorm backward behind x as partial rows (tris_gemm_bnbwd_f32), the link filled.
    -> False, nothing launched, where the form does not apply or the entry point declines the shape"""
    M, N, K = dims
    ypl = link.from_y and pl_word(x) is not None   # (the BatchNorm's output as planes: only a plane product masks from it)
    if ypl and pl_word(dy) is None:
        return False
    pr2 = link.pair if (cfg.bn_pair and "bwd" in cfg.bn_pair_parts and planes_on()) else None
    part, rows, part2, dzw = _bn_bwd_bufs(M, K, x.device, pr2)     # (part2: the shortcut BatchNorm's sum(dz * xhat_s), same rows)
    bits = ypl and link.mask is not None

    def launch():
        pp = h2_pp(dy, w, w_b=True, y_planes=ypl, k_red=N, w_bt=True, y_mask=bits)
        if dzw is not None:
            call("tris_amax_next", dzw)
        by = (P(x) if (pp.planes or not ypl) else P(unplanes(x))) if link.from_y else None
        if bits and pp.planes:
            by = link.mask.data_ptr()       # (the product took planes and was armed with flag 4: bn_y is the byte mask)
        if pool is not None:
            call("tris_gemm_resid_pool_next", pool[0], pool[1])
        if part2 is not None:
            call("tris_gemm_bnbwd_x2_next", P(pr2.x), P(pr2.mean), P(pr2.invstd), part2.data_ptr())
        call("tris_gemm_bnbwd_f32", pp.a, pp.b, P(dx), M, K, N, P(extra), K, P(link.x), by,
             P(link.mean), P(link.invstd), P(link.gamma), P(link.beta), part.data_ptr(), ctypes.byref(rows), _stream())
        return rows.value > 0     # (False: the entry point declined the shape, nothing was launched)
    ran = _timed("gemm_bnbwd", 2.0 * M * N * K, launch, tag=_shape_tag(f"M{M} N{K} K{N}"),
                 nbytes=4.0 * (M * N + N * K + M * K * (2 + int(link.from_y) + int(extra is not None))))
    if ran:
        link.fill(dx, part, rows.value, dzw, part2)
    return ran


def _lin_dgrad(dy, x, w, dx, dims, link, alink, box, extra, pool):
    """dx = dy . W (+ extra) in the first of four forms that applies -> "bnbwd" | "qgelu" | "pool" | "plain", the one that ran"""
    M, N, K = dims
    # x is the output of a BatchNorm(+ReLU) that has no other consumer: mask dx and reduce it for that BatchNorm's backward in this
    # product's epilogue (_BnBwdLink).  With a gradient box whose value has NOT arrived yet (the other consumer's backward is still to
    # run and will hand its term to autograd) the sums would miss that term: the plain data gradient runs and the BatchNorm backward
    # does its own reduction
    if link is not None and (box is None or extra is not None) and _lin_dgrad_bnbwd(dy, x, w, dx, dims, link, extra, pool):
        return "bnbwd"
    # x = QuickGELU(pre) with this product as its only consumer (linear_qgelu): the data gradient comes out of the epilogue already
    # multiplied by quickgelu'(pre); the producer's backward is told so
    if alink is not None and extra is None and gemm(dy, w, dx, M, K, N, N, K, K, False, False, dact=alink.pre) is not False:
        alink.applied = True
        return "qgelu"
    if pool is not None:
        if gemm(dy, w, dx, M, K, N, N, K, K, False, False, resid=extra, ldr=K, w_b=True, w_bt=True, resid_pool=pool) is not False:
            return "pool"
        extra = _avgpool2_bwd(extra, x.shape)    # (a product the fast kernel does not serve: the expansion after all)
    gemm(dy, w, dx, M, K, N, N, K, K, False, False, resid=extra, ldr=K, w_b=True, w_bt=True)
    return "plain"


def _wgrad(p, make, needs, *reads):
    """The weight gradient of a product, make(out) launching it: into p's sink on the weight-gradient stream (-> None; reads: every tensor
    the launch reads), else as _emit hands it to autograd."""
    sk = _sink(p) if needs else None
    if sk is None:
        return _emit(p, make, needs)
    on_wgrad_stream(lambda: make(sk), *reads, sink=sk)
    return None


def _bias_grad(p, dy, M, N, needs):
    """the gradient of a bias added to the rows of an [M, N] product: the column sum of dy (p None: there was no bias)"""
    return None if p is None else _emit(p, lambda o: colsum(dy, M, N, o), needs, reads=(dy,))


class LinearFn(torch.autograd.Function):
    """y = act(x . W^T + b) + resid  with W [N, K] (nn.Linear) or [N, K, 1, 1] (1x1 conv on channels-last)."""

    @staticmethod
    def forward(ctx, x, w, b, resid, o):
        _chk(x, w, b, resid)
        ctx.opts = o
        ctx.bn_link = o.bn_link if (o.bn_link is not None and x.is_contiguous() and o.bn_link.x.shape == x.shape) else None
        x = x.contiguous()
        K = x.shape[-1]
        N = w.numel() // K
        M = x.numel() // K
        y = torch.empty(*x.shape[:-1], N, device=x.device, dtype=torch.float32)
        if resid is not None:
            resid = resid.contiguous()
        if o.stats and b is None and resid is None and o.act == 0:
            _launch_with_stats(y, M, N, lambda part, rows: _lin_fwd_stats(x, w, y, M, N, K, part, rows))
        else:
            gemm(x, w, y, M, N, K, K, K, N, False, True, bias=b, bias_mode=1 if b is not None else 0, resid=resid,
                 ldr=N, act=o.act, w_b=True)
        ctx.dims, ctx.params, ctx.x_pl = (M, N, K), (w, b), getattr(x, "_pl", None)
        ctx.has_b, ctx.has_r = b is not None, resid is not None
        ctx.save_for_backward(x, w, b, y if o.act == 1 else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        o, needs = ctx.opts, ctx.needs_input_grad
        if o.act == 2:
            raise RuntimeError("fused QuickGELU epilogue is forward-only; use QGeluFn when gradients are needed")
        if o.act == 1 and ctx.has_r:
            raise RuntimeError("relu + residual epilogue is forward-only")
        x, w, b, y = ctx.saved_tensors
        (pw, pb), (M, N, K) = ctx.params, ctx.dims
        # (bias / residual / ReLU backward read the gradient element-wise: never on the trunk's path)
        dy, x = _grad_forms(dy, x, ctx.x_pl, ctx.has_r or ctx.has_b or o.act == 1)
        d_res = _lin_resid_grad(dy, o.grad_box_res, ctx.has_r and needs[3], needs[1])
        if o.act == 1:
            dy = ew("TRIS_EW_RELU_BWD", dy, y)
        extra, pool = _box_take(o.grad_box)
        dx = None
        if needs[0]:
            dx = torch.empty_like(x)
            _lin_dgrad(dy, x, w, dx, ctx.dims, ctx.bn_link, o.act_link, o.grad_box, extra, pool)
        elif extra is not None:
            raise RuntimeError("a residual gradient was handed to a layer whose input needs no gradient")
        if dx is not None and o.grad_box_out is not None and o.grad_box_out.deposit(dx):
            dx = None   # the block's first conv adds it in its data-gradient epilogue
        dw = _wgrad(pw, lambda out: gemm(dy, x, out, N, K, M, N, K, K, True, False, mark=False), needs[1], dy, x)
        db = _bias_grad(pb, dy, M, N, needs[2])
        return dx, dw, db, d_res, None


def linear(x, w, b=None, resid=None, act=0, stats=False, grad_box=None, grad_box_out=None, grad_box_res=None, act_link=False):
    """act_link=True: x is the output of linear_qgelu and THIS product is its only consumer -- the QuickGELU backward rides this
    product's data-gradient epilogue (the caller vouches for the single consumer)"""
    alink = getattr(x, "_act_link", None) if (act_link and torch.is_grad_enabled() and x.requires_grad) else None
    return LinearFn.apply(x, w, b, resid, _LinOpts(act, stats, grad_box, grad_box_out, grad_box_res, _bn_link_of(x), alink))


class _ActLink:
    """QuickGELU hand-off between linear_qgelu (producer: holds the pre-activation) and the Linear that consumes its output:
    `applied` is set by the consumer's backward when its data gradient already carries quickgelu'(pre)."""
    __slots__ = ("pre", "applied")

    def __init__(self, pre):
        self.pre, self.applied = pre, False


class LinearQGeluFn(torch.autograd.Function):
    """QuickGELU(x . W^T + b) in one launch (CLIP/clip/model.py:361-376: c_fc + gelu of the transformer MLP): the epilogue stores the
    activated value AND the pre-activation its backward needs."""

    @staticmethod
    def forward(ctx, x, w, b):
        _chk(x, w, b)
        x = x.contiguous()
        K = x.shape[-1]
        N = w.numel() // K
        M = x.numel() // K
        y = torch.empty(*x.shape[:-1], N, device=x.device, dtype=torch.float32)
        pre = torch.empty_like(y)
        if gemm(x, w, y, M, N, K, K, K, N, False, True, bias=b, bias_mode=1 if b is not None else 0, act=2, pre_out=pre) is False:
            gemm(x, w, pre, M, N, K, K, K, N, False, True, bias=b, bias_mode=1 if b is not None else 0)
            ew("TRIS_EW_QGELU", pre, out=y)
        ctx.dims, ctx.params = (M, N, K), (w, b)
        ctx.link = y._act_link = _ActLink(pre)
        ctx.save_for_backward(x, w, pre)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, pre = ctx.saved_tensors
        (pw, pb), (M, N, K) = ctx.params, ctx.dims
        dy = dy.contiguous()
        dpre = dy if ctx.link.applied else ew("TRIS_EW_QGELU_BWD", dy, pre)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            gemm(dpre, w, dx, M, K, N, N, K, K, False, False)
        dw = _wgrad(pw, lambda out: gemm(dpre, x, out, N, K, M, N, K, K, True, False, mark=False), ctx.needs_input_grad[1], dpre, x)
        db = _bias_grad(pb, dpre, M, N, ctx.needs_input_grad[2])
        return dx, dw, db


def linear_qgelu(x, w, b=None):
    return LinearQGeluFn.apply(x, w, b)     # (the returned tensor carries `_act_link`, set inside forward)


class MatmulFn(torch.autograd.Function):
    """C = A . B (tB False, B [K,N]) or A . B^T (tB True, B [N,K]); A [..., K] flattened to 2-D."""

    @staticmethod
    def forward(ctx, A, B, tB):
        _chk(A, B)
        A, B = A.contiguous(), B.contiguous()
        K = A.shape[-1]
        M = A.numel() // K
        N = B.shape[0] if tB else B.shape[1]
        C = torch.empty(*A.shape[:-1], N, device=A.device, dtype=torch.float32)
        gemm(A, B, C, M, N, K, K, B.shape[1], N, False, tB)
        ctx.tB, ctx.dims = tB, (M, N, K)
        ctx.params = (B,)
        ctx.save_for_backward(A, B)
        return C

    @staticmethod
    def backward(ctx, dC):
        A, B = ctx.saved_tensors
        M, N, K = ctx.dims
        dC = dC.contiguous()
        dA = dB = None
        if ctx.needs_input_grad[0]:
            dA = torch.empty_like(A)
            if ctx.tB:   # dA = dC . B   (B [N,K])
                gemm(dC, B, dA, M, K, N, N, K, K, False, False)
            else:        # dA = dC . B^T (B [K,N])
                gemm(dC, B, dA, M, K, N, N, N, K, False, True)
        if ctx.needs_input_grad[1]:
            if ctx.tB:   # dB [N,K] = dC^T . A
                dB = _emit(ctx.params[0], lambda o: gemm(dC, A, o, N, K, M, N, K, K, True, False, mark=False), True)
            else:        # dB [K,N] = A^T . dC
                dB = _emit(ctx.params[0], lambda o: gemm(A, dC, o, K, N, M, K, N, N, True, False, mark=False), True)
        return dA, dB, None


def matmul(A, B, tB=False):
    return MatmulFn.apply(A, B, tB)


class BmmFn(torch.autograd.Function):
    """C[b] = A[b] . op(B[b]);  A may be 2-D (shared by every batch).  A [Bt,M,K]|[M,K]; B [Bt,N,K] (tB) | [Bt,K,N]."""

    @staticmethod
    def forward(ctx, A, B, tB, alpha):
        _chk(A, B)
        A, B = A.contiguous(), B.contiguous()
        Bt = B.shape[0]
        shared = A.dim() == 2
        M, K = A.shape[-2], A.shape[-1]
        N = B.shape[1] if tB else B.shape[2]
        C = torch.empty(Bt, M, N, device=B.device, dtype=torch.float32)
        gemm(A, B, C, M, N, K, K, B.shape[2], N, False, tB, batch=Bt, sA=0 if shared else M * K,
             sB=B.shape[1] * B.shape[2], sC=M * N, alpha=alpha)
        ctx.cfg = (tB, alpha, shared, Bt, M, N, K)
        ctx.save_for_backward(A, B)
        return C

    @staticmethod
    def backward(ctx, dC):
        A, B = ctx.saved_tensors
        tB, alpha, shared, Bt, M, N, K = ctx.cfg
        dC = dC.contiguous()
        sA = 0 if shared else M * K
        dA = dB = None
        if ctx.needs_input_grad[0]:
            dAp = torch.empty(Bt, M, K, device=B.device, dtype=torch.float32)
            if tB:   # dA[b] = dC[b] . B[b]       (B[b] is [N,K])
                gemm(dC, B, dAp, M, K, N, N, K, K, False, False, batch=Bt, sA=M * N, sB=N * K, sC=M * K, alpha=alpha)
            else:    # dA[b] = dC[b] . B[b]^T     (B[b] is [K,N])
                gemm(dC, B, dAp, M, K, N, N, N, K, False, True, batch=Bt, sA=M * N, sB=K * N, sC=M * K, alpha=alpha)
            if shared:
                dA = torch.empty(M, K, device=B.device, dtype=torch.float32)
                colsum(dAp, Bt, M * K, dA)
            else:
                dA = dAp
        if ctx.needs_input_grad[1]:
            dB = torch.empty_like(B)
            if tB:   # dB[b] [N,K] = dC[b]^T . A[b]
                gemm(dC, A, dB, N, K, M, N, K, K, True, False, batch=Bt, sA=M * N, sB=sA, sC=N * K, alpha=alpha)
            else:    # dB[b] [K,N] = A[b]^T . dC[b]
                gemm(A, dC, dB, K, N, M, K, N, N, True, False, batch=Bt, sA=sA, sB=M * N, sC=K * N, alpha=alpha)
        return dA, dB, None, None


def bmm(A, B, tB=False, alpha=1.0):
    return BmmFn.apply(A, B, tB, alpha)


# ----------------------------------------------------------------------------------------------- 3x3 conv
# _ConvOpts: what ops.conv3x3 tells Conv3x3Fn beyond the tensors autograd must see (one argument of apply).
# bn_link: x is the output of a BatchNorm + ReLU with no other consumer (_BnBwdLink): the data gradient reduces that BatchNorm's backward
# sums in its epilogue.  lazy (_BnLazy): `x` is the NOT-YET-WRITTEN output buffer of a BatchNorm + ReLU over lazy.x
# (batch_norm(..., lazy=True)); the direct kernels normalise x_raw while they stage it and `x` is never written -- or, when they cannot
# serve the shape after all, it is written first and everything proceeds as usual.  (h2: the unwritten buffer carries the amax word of
# an upper bound of its would-be contents, BatchNormFn.forward.)
_ConvOpts = NamedTuple("_ConvOpts", [("stride", int), ("stats", bool), ("lazy", Optional[_BnLazy]), ("bn_link", object)])


def _conv_pp(a, w_param, w_cl):
    """_Operands of a 3x3 product (activation or gradient `a`, weight parameter `w_param` whose kernel layout is `w_cl`)"""
    pp = h2_pp(a, w_param, w_b=True)
    return pp if pp.b != P(w_param) else pp._replace(b=P(w_cl))


def _conv_fwd(x, w_param, w, stride, stats, lazy=None):
    """y = conv3x3(x), stats: with the BatchNorm statistics of y.  lazy: x is unwritten -- y = conv3x3(relu(bn(lazy.x))), the BatchNorm
    folded into the direct kernel's staging (stride 1, conv3x3_bnin_ok)"""
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    y = torch.empty(B, Ho, Wo, Cout, device=x.device, dtype=torch.float32)

    def launch(part, rows):
        def run():
            if lazy is not None:
                if lazy.bound is not None:      # (None outside h2)
                    h2_arm(None, w_param, a_slot=lazy.bound)
                return call("tris_conv3x3_fwd_bnin_f32", P(lazy.x), P(lazy.mean), P(lazy.invstd), P(lazy.gamma), P(lazy.beta), P(w), P(y),
                            B, H, W, Cin, Cout, None if part is None else part.data_ptr(), rows, _stream())
            pp = _conv_pp(x, w_param, w)
            if part is None:
                call("tris_conv3x3_fwd_f32", pp.a, pp.b, P(y), B, H, W, Cin, Cout, stride, _stream())
            else:
                call("tris_conv3x3_fwd_bnstat_f32", pp.a, pp.b, P(y), B, H, W, Cin, Cout, stride, part.data_ptr(), rows, _stream())
        form = "bnin " if lazy is not None else ("" if part is None else "bnstat ")
        _timed("conv3x3_fwd", 2.0 * B * Ho * Wo * Cout * 9 * Cin, run, nbytes=4.0 * (B * H * W * Cin + B * Ho * Wo * Cout + 9 * Cin * Cout),
               tag=_shape_tag(f"{form}B{B} {H}x{W} {Cin}->{Cout}" + ("" if lazy is not None else f" s{stride}")))
    _launch_with_stats(y, B * Ho * Wo, Cout, launch, stats)
    return y


def _conv_dgrad(dy, w_param, w, dx, link):
    """dx = the data gradient of a stride-1 conv3x3.  link (_BnBwdLink or None): masked and reduced for the BatchNorm + ReLU behind x in the
    epilogue (as _lin_dgrad_bnbwd) and the link filled -- unless the entry point declines the shape: then the plain form, as without a link"""
    B, H, W, Cin = dx.shape
    Cout = w.shape[0]
    fl, tag = 2.0 * B * H * W * Cout * 9 * Cin, _shape_tag(f"B{B} {H}x{W} {Cin}<-{Cout}")
    if link is not None:
        part, rows, _, dzw = _bn_bwd_bufs(B * H * W, Cin, dx.device)

        def fused():
            pp = _conv_pp(dy, w_param, w)
            if dzw is not None:
                call("tris_amax_next", dzw)
            call("tris_conv3x3_dgrad_bnbwd_f32", pp.a, pp.b, P(dx), B, H, W, Cin, Cout, P(link.x), P(link.mean), P(link.invstd),
                 P(link.gamma), P(link.beta), part.data_ptr(), ctypes.byref(rows), _stream())
            return rows.value > 0
        if _timed("conv3x3_dgrad_bnbwd", fl, fused, tag=tag, nbytes=4.0 * (B * H * W * (Cout + 2 * Cin) + 9 * Cin * Cout)):
            link.fill(dx, part, rows.value, dzw)
            return

    def plain():
        pp = _conv_pp(dy, w_param, w)
        call("tris_conv3x3_dgrad_f32", pp.a, pp.b, P(dx), B, H, W, Cin, Cout, _stream())
    _timed("conv3x3_dgrad", fl, plain, tag=tag, nbytes=4.0 * (B * H * W * (Cout + Cin) + 9 * Cin * Cout))


def _conv_wgrad(dy, x, o, stride, bn=(), h2_in=None):
    """the weight gradient into o [Cout, 3, 3, Cin].  bn = (mean, invstd, gamma, beta): x is the raw input of a BatchNorm + ReLU folded
    into the forward (h2_in: the amax word of its would-be output) -- folded here as well, or materialised after all"""
    B, H, W, Cin = x.shape
    Cout = o.shape[0]
    ws = workspace(0)
    fl = 2.0 * dy.shape[0] * dy.shape[1] * dy.shape[2] * Cout * 9 * Cin
    nb = 4.0 * (B * H * W * Cin + dy.numel() + 9 * Cin * Cout)
    if bn and conv3x3_bnin_ok(x.shape, Cout):
        mean, invstd, gamma, beta = bn

        def folded():
            if h2_in is not None:
                h2_arm(dy, None, b_slot=h2_in)
            call("tris_conv3x3_wgrad_bnin_f32", P(x), P(mean), P(invstd), P(gamma), P(beta), P(dy), P(o), B, H, W, Cin, Cout,
                 P(ws), ws.numel() * 4, _stream())
        return _timed("conv3x3_wgrad", fl, folded, nbytes=nb, tag=_shape_tag(f"bnin B{B} {H}x{W} {Cin}->{Cout}"))
    xin = _bn_write(x, *bn, torch.empty_like(x), True) if bn else x    # (materialise relu(bn(x)) after all)

    def plain():
        pp = h2_pp(dy, xin, k_red=dy.shape[0] * dy.shape[1] * dy.shape[2])
        call("tris_conv3x3_wgrad_f32", pp.b, pp.a, P(o), B, H, W, Cin, Cout, stride, P(ws), ws.numel() * 4, _stream())
    return _timed("conv3x3_wgrad", fl, plain, nbytes=nb, tag=_shape_tag(f"B{B} {H}x{W} {Cin}->{Cout} s{stride}"))


class Conv3x3Fn(torch.autograd.Function):
    """x [B,H,W,Cin] channels-last, w [Cout,Cin,3,3] in channels_last memory, pad 1, stride 1|2."""

    @staticmethod
    def forward(ctx, x, w, o):
        _chk(x, w)
        link, lazy = o.bn_link, o.lazy
        ctx.bn_link = link if (link is not None and o.stride == 1 and not link.from_y and x.is_contiguous() and link.x.shape == x.shape) else None
        x = x.contiguous()
        ctx.params = (w,)
        w = cl_weight(w)
        ctx.stride, ctx.h2_in = o.stride, None
        ctx.lazy = lazy is not None and o.stride == 1 and conv3x3_bnin_ok(x.shape, w.shape[0])
        if ctx.lazy:
            ctx.h2_in = lazy.bound
            ctx.save_for_backward(lazy.x, w, lazy.mean, lazy.invstd, lazy.gamma, lazy.beta)
            return _conv_fwd(x, ctx.params[0], w, 1, o.stats, lazy)
        if lazy is not None:
            _bn_write(lazy.x, lazy.mean, lazy.invstd, lazy.gamma, lazy.beta, x, True)
        if pl_word(x) is not None and (x.shape[3] % 32 != 0 or o.stride != 1):
            x = unplanes(x)        # (the fast kernels' gather needs 32-channel pieces; the stem's strided first convolution reads the image)
        ctx.x_pl = getattr(x, "_pl", None)
        ctx.save_for_backward(x, w)
        return _conv_fwd(x, ctx.params[0], w, o.stride, o.stats)

    @staticmethod
    def backward(ctx, dy):
        x, w, *bn = ctx.saved_tensors      # (lazy: x is the raw input of the folded BatchNorm, bn its mean, invstd, gamma, beta)
        wp = ctx.params[0]
        # (the BatchNorm-folded forms and the stem's first convolution read an fp32 gradient)
        dy, x = _grad_forms(dy, x, None if ctx.lazy else ctx.x_pl, ctx.lazy or w.shape[0] % 32 != 0, planes_x=True)
        dx = None
        if ctx.needs_input_grad[0]:
            if ctx.stride != 1:
                raise NotImplementedError("dgrad of the strided stem conv is never needed (its input is the image)")
            dx = torch.empty_like(x)
            _conv_dgrad(dy, wp, w, dx, ctx.bn_link)
        # (every tensor the deferred launch READS is named: a segmented capture keeps them alive and keeps the early part of AdamW away
        # from the parameters among them -- the folded BatchNorm's gamma / beta)
        dw = _wgrad(wp, lambda out: _conv_wgrad(dy, x, out, ctx.stride, bn, ctx.h2_in), ctx.needs_input_grad[1], dy, x, *bn)
        return dx, dw, None


def conv3x3_bnin_ok(xshape, Cout):
    """can conv3x3(relu(bn(x))) run with the BatchNorm folded into the direct kernels (forward AND weight gradient)?"""
    B, H, W, Cin = xshape
    return bool(query("tris_conv3x3_bnin_ok", B, H, W, Cin, Cout))


def conv3x3(x, w, stride=1, stats=False):
    return Conv3x3Fn.apply(x, w, _ConvOpts(stride, stats, getattr(x, "_bn_lazy", None), _bn_link_of(x)))


# ----------------------------------------------------------------------------------------------- BatchNorm
# _BnOpts: what ops.batch_norm tells BatchNormFn beyond the tensors autograd must see (one argument of apply; ops.batch_norm).
_BnOpts = NamedTuple("_BnOpts", [("relu", bool), ("training", bool), ("momentum", float), ("eps", float), ("group", object),
                                 ("part", Optional[_BnPart]), ("grad_box", object), ("lazy", bool), ("bwd_link", bool), ("pool", bool),
                                 ("planes", bool), ("dx_planes", bool), ("pair", bool)])
# _BnPlan: what BatchNormFn.forward decides -- from its options, the shapes, cfg and planes_on() -- before it launches anything.
# use_pl / dx_pl: the output is written as operand planes / the input gradient will be; pair_out: the output is not written, what
# comes back is the stand-in carrying `_bn_pair`; pair_in (bn3 of that block): the residual is such a stand-in and this pass normalises
# the shortcut itself; lazy: y stays UNWRITTEN -- its only consumer (a 3x3 convolution with direct kernels) normalises x while staging it
_BnPlan = NamedTuple("_BnPlan", [("use_pl", bool), ("dx_pl", bool), ("pair_out", bool), ("pair_in", Optional[_BnPair]), ("lazy", bool)])
_Bn = NamedTuple("_Bn", _BN)
# _BnBwd: the BatchNorm one backward pass works on and the constants of that pass (x is [M, C]; pool: the forward was BatchNorm + ReLU +
# AvgPool2d(2), dy is the POOLED gradient; xmax = sqrt(count - 1), Samuelson's bound of |xhat|)
_BnBwd = NamedTuple("_BnBwd", _BN + [("M", int), ("C", int), ("pool", bool), ("inv_cnt", float), ("xmax", float)])


def _bn_plan(o, x, resid):
    C = x.shape[-1]
    fits = bool(o.training and C % 8 == 0 and 2048 % C == 0 and planes_on())
    use_pl = bool(o.planes and fits)
    lazy = o.lazy and not use_pl
    pair_out = bool(o.pair and cfg.bn_pair and "fwd" in cfg.bn_pair_parts and fits and o.group is None and resid is None and not o.relu
                    and not o.pool and not lazy and not use_pl)
    pr = getattr(resid, "_bn_pair", None) if resid is not None else None
    take = pr is not None and use_pl and o.group is None and o.relu and not o.pool and pr.x.shape == x.shape
    return _BnPlan(use_pl, bool(o.dx_planes and fits), pair_out, pr if take else None, bool(lazy and o.training and o.relu and resid is None))


def _bn_bound_words(resid, pr):
    """-> (w, rw): a fresh amax word for the bound of a plane output, and the word of the residual it is added to -- its plane word,
    the bound of a paired shortcut, else its amax (a by-product or a pre-pass); (None, None) where either is not to be had"""
    w, rw = _h2_slot(), None
    if pr is not None:
        rw = pr.word
    elif resid is not None:
        rw = pl_word(resid)
        rw = _h2_amax(resid) if rw is None else rw
    return (w, rw) if w is not None and (resid is None or rw is not None) else (None, None)


def _bn_local_stats(x, part, eps, momentum, dst, rm, rv, bound=None):
    """this rank's statistics of x into dst, running statistics rm / rv updated (None: not here): finalized from the partial sums out of
    the producing conv's epilogue -- bound = (gamma, beta, xmax, resid word, word): that launch also leaves the bound of the plane
    output in `word` -- or by a statistics pass"""
    M, C = x.numel() // x.shape[-1], x.shape[-1]
    if part is not None and bound is not None:
        gamma, beta, xmax, rw, w = bound
        call("tris_bn_finalize_bound_f32", part.part.data_ptr(), part.rows, M, C, eps, momentum, P(dst), P(rm), P(rv), P(gamma), P(beta),
             xmax, rw, w, _stream())
    elif part is not None:
        call("tris_bn_finalize_f32", part.part.data_ptr(), part.rows, M, C, eps, momentum, P(dst), P(rm), P(rv), _stream())
    else:
        ws = workspace(query("tris_col_workspace_bytes", M, C))
        call("tris_bn_stats_f32", P(x), M, C, eps, momentum, P(dst), P(rm), P(rv), P(ws), _stream())


def _bn_statistics(o, plan, x, stats, gamma, beta, rmean, rvar, resid, world, xmax):
    """train mode: local statistics, or combined over the `world` ranks of o.group through the SyncBN mailbox or a c10d gather.
    -> (word, rw): the plane output's bound word and its residual's word where the finalizing launch formed the bound too"""
    M, C = x.numel() // x.shape[-1], x.shape[-1]
    word = rw = None
    if o.group is None:
        if o.part is not None and (plan.use_pl or plan.pair_out):
            # partial sums from the producing conv's epilogue; the same launch leaves the bound of the plane output
            # (pair_out: the bound of the shortcut's value, which bn3's launch chains into its own as add_word)
            word, rw = _bn_bound_words(resid, plan.pair_in)
        _bn_local_stats(x, o.part, o.eps, o.momentum, stats, rmean, rvar, None if word is None else (gamma, beta, xmax, rw, word))
        return word, rw
    from . import comm
    mb = comm.syncbn_mailbox(o.group, 3 * C)
    if mb is not None:   # one launch: peer-mailbox exchange + combine (+ running statistics)
        loc = torch.empty(3 * C, device=x.device, dtype=torch.float32)
        _bn_local_stats(x, o.part, o.eps, o.momentum, loc, None, None)
        if plan.use_pl and cfg.syncbn_bound:   # ... + the bound word of the plane output (what tris_bn_out_bound2_f32 would launch for)
            word, rw = _bn_bound_words(resid, plan.pair_in)
        if word is not None:
            mb.bn_combine_bound(loc, C, M, o.eps, o.momentum, stats, rmean, rvar, gamma, beta, xmax, rw, word)
        else:
            mb.bn_combine(loc, C, M, o.eps, o.momentum, stats, rmean, rvar)
    else:
        _bn_local_stats(x, o.part, o.eps, o.momentum, stats, None, None)
        allv = torch.empty(world * 3 * C, device=x.device, dtype=torch.float32)
        comm.syncbn_all_gather_into(allv, stats, group=o.group)   # the stats block travels as is
        call("tris_bn_sync_combine_f32", P(allv), world, C, M, o.eps, o.momentum, P(stats), P(rmean), P(rvar), _stream())
    return word, rw


def _bn_write(x, mean, invstd, gamma, beta, y, relu, resid=None):
    """the plain apply pass: y = relu?(bn(x) + resid?) written in fp32, its amax a by-product of the launch.  -> y"""
    h2_mark_next(y)
    call("tris_bn_apply_f32", P(x), P(mean), P(invstd), P(gamma), P(beta), P(resid), P(y), x.numel() // x.shape[-1], x.shape[-1],
         int(relu), _stream())
    return y


def _bn_apply(o, plan, bn, resid, y, word, rw):
    """the apply pass in the forms that write y: operand planes under the bound `word` (+ pool, + the paired shortcut), fp32 (+ pool);
    lazy: none.  -> the ReLU mask bytes of a plane output whose consumer will mask with them"""
    x, pr, y_mask, p = bn.x, plan.pair_in, None, [P(t) for t in bn]
    M, C = x.numel() // x.shape[-1], x.shape[-1]
    if plan.use_pl and o.pool:
        call("tris_bn_apply_pool_pl_f32", *p, P(y), word, x.shape[0], x.shape[1], x.shape[2], C, _stream())
    elif plan.use_pl:
        if cfg.bn_bitmask and o.bwd_link and o.relu and resid is not None:
            # out = relu(bn(x) + identity) with ONE consumer whose data-gradient epilogue will mask with it (_BnBwdLink.from_y):
            # the pass also leaves the mask as one byte per 8 channels, so that epilogue reads a bit, not the plane element
            y_mask = torch.empty(M * C // 8, device=x.device, dtype=torch.uint8)
            call("tris_bn_mask_next", y_mask.data_ptr())
        if pr is not None:   # relu(bn3(x) + bn_s(xs)): the shortcut's BatchNorm in the same pass
            call("tris_bn_apply_pair_pl_f32", *p, P(pr.x), P(pr.mean), P(pr.invstd), P(pr.gamma), P(pr.beta), P(y), word, M, C, _stream())
        else:
            rk = 0 if resid is None else (2 if pl_word(resid) is not None else 1)
            call("tris_bn_apply_pl_f32", *p, P(resid), rk, rw if rk == 2 else None, P(y), word, M, C, int(o.relu), _stream())
    elif o.pool:
        h2_mark_next(y)
        call("tris_bn_apply_pool_f32", *p, P(y), x.shape[0], x.shape[1], x.shape[2], C, _stream())
    elif not plan.lazy:
        _bn_write(*bn, y, o.relu, resid)
    if plan.use_pl:
        pl_tag(y, word)
    return y_mask


def _bn_bwd_reduce(b, dy, y, mask_x, p_dz, p_dzx, dzw, dz_out):
    """sum(dz), sum(dz * xhat) in a pass of their own over dy (no product left them behind; pooled: the mask from x); dz_out: the
    pass also writes the masked gradient dz there"""
    ws, px = workspace(query("tris_col_workspace_bytes", b.M, b.C)), (P(b.x), P(b.mean), P(b.invstd))
    if dzw is not None:
        call("tris_amax_next", dzw)
    if b.pool:
        call("tris_bn_bwd_reduce_pool_f32", P(dy), *px, *b.x.shape[:3], b.C, p_dz, p_dzx, P(ws), P(b.gamma), P(b.beta), _stream())
    elif pl_word(y) is not None and not mask_x:
        call("tris_bn_bwd_reduce_pl_f32", P(dy), P(y), *px, b.M, b.C, p_dz, p_dzx, P(ws), P(dz_out), _stream())
    else:
        call("tris_bn_bwd_reduce_f32", P(dy), None if mask_x else P(y), *px, b.M, b.C, p_dz, p_dzx, P(ws),
             P(b.gamma) if mask_x else None, P(b.beta) if mask_x else None, P(dz_out), _stream())


def _bn_bwd_apply(b, g, ymask, dz_out, beta_m, dx, p_dz, p_dzx, dzw, word, dx_pl):
    """dx from the (masked or to-be-masked) gradient g; dx_pl: as operand planes, where the convolution before takes them, under the
    bound `word` (None: no finalizer has formed it, a launch of its own does)"""
    px = (P(b.x), P(b.mean), P(b.invstd), P(b.gamma))
    if dx_pl:
        if word is None:
            word = _h2_slot()
            call("tris_bn_bwd_bound_f32", P(b.gamma), P(b.invstd), p_dz, p_dzx, b.C, b.inv_cnt, b.xmax, dzw, word, _stream())
        if b.pool:
            call("tris_bn_bwd_apply_pool_pl_f32", P(g), *px, P(b.beta), p_dz, p_dzx, b.inv_cnt, P(dx), word, *b.x.shape[:3], b.C, _stream())
        else:
            if ymask is not None and pl_word(ymask) is None:
                raise RuntimeError("operand planes: the ReLU mask of a plane-output BatchNorm must come from plane y")
            call("tris_bn_bwd_apply_pl_f32", P(g), P(ymask), *px, p_dz, p_dzx, b.inv_cnt, P(dx), word, P(dz_out), b.M, b.C, P(beta_m),
                 _stream())
        pl_grad_out(dx, word)
        return
    h2_mark_next(dx)
    if b.pool:
        call("tris_bn_bwd_apply_pool_f32", P(g), *px, P(b.beta), p_dz, p_dzx, b.inv_cnt, P(dx), *b.x.shape[:3], b.C, _stream())
    else:
        call("tris_bn_bwd_apply_f32", P(g), P(unplanes(ymask)) if ymask is not None else None, *px, p_dz, p_dzx, b.inv_cnt, P(dx),
             P(dz_out), b.M, b.C, P(beta_m), _stream())


def _bn_param_grads(ctx, sums, C):
    """(dgamma, dbeta) out of the two sums (sum(dz), sum(dz * xhat)) of a backward that did not write them into the arena"""
    return (_emit(ctx.params[0], lambda o: o.copy_(sums[C:]), ctx.needs_input_grad[1]),
            _emit(ctx.params[1], lambda o: o.copy_(sums[:C]), ctx.needs_input_grad[2]))




class BatchNormFn(torch.autograd.Function):
    """BatchNorm2d on channels-last x [..., C] with optional fused residual add and ReLU.

    training=True: batch statistics (+ running-stat update, + cross-rank combine when `group` is given =
    SyncBatchNorm).  training=False: running statistics (forward only)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, rmean, rvar, resid, o):
        """o: _BnOpts.  The steps: plan (_bn_plan), statistics (_bn_statistics), apply (_bn_apply), hand-offs"""
        _chk(x, gamma, beta, rmean, rvar, resid)
        x = x.contiguous()
        C = x.shape[-1]
        M = x.numel() // C
        plan = _bn_plan(o, x, resid)
        use_pl, pair_out, pr = plan.use_pl, plan.pair_out, plan.pair_in
        if pr is None and getattr(resid, "_bn_pair", None) is not None:
            # (this BatchNorm cannot take the pair: the shortcut's fp32 output is written first, as it used to be)
            q = resid._bn_pair
            resid = _bn_write(q.x, q.mean, q.invstd, q.gamma, q.beta, torch.empty_like(q.x), False)
        y = (torch.empty(x.shape[0], x.shape[1] // 2, x.shape[2] // 2, C, device=x.device, dtype=torch.float32) if o.pool
             else (None if pair_out else torch.empty_like(x)))
        if resid is not None and pr is None:
            resid = resid.contiguous()
        world = 1
        if o.training and o.group is not None:
            from . import comm
            world = comm.world_size(o.group)
        count = M * world  # DistributedSampler gives every rank the same per-step batch
        xmax = math.sqrt(max(count - 1, 1))   # (Samuelson: |xhat| <= sqrt(n - 1) -- what every bound of normalised values starts from)
        word = rw = None   # (operand planes: the output's bound word and its residual's, formed by the finalizer where it can)
        if o.training:
            stats = torch.empty(3 * C, device=x.device, dtype=torch.float32)
            word, rw = _bn_statistics(o, plan, x, stats, gamma, beta, rmean, rvar, resid, world, xmax)
            bn = _Bn(x, stats[:C], stats[C:2 * C], gamma, beta)
        else:
            bn = _Bn(x, rmean, torch.rsqrt(rvar + o.eps), gamma, beta)
        if not use_pl and resid is not None:
            resid = unplanes(resid)
        if (use_pl or pair_out) and word is None:
            # the scale must exist before the pass writes: Samuelson's bound of the normalised values from the affine parameters,
            # plus the bound (or amax) of the residual it is added to -- in a launch of its own where no finalizer formed it
            # (pair_out: statistics from a pass of their own, a convolution too small for the fused epilogue)
            word, rw = _bn_bound_words(resid, pr)
            if word is not None:
                call("tris_bn_out_bound2_f32", P(gamma), P(beta), C, xmax, rw, word, _stream())
            elif use_pl:
                raise RuntimeError("operand planes: no amax word for a BatchNorm output / its residual")
            else:                                      # (no amax word left in the pool: the shortcut is written after all)
                pair_out, y = False, torch.empty_like(x)
        ctx.pair_state = y_mask = None
        if pair_out:
            # neither allocated nor written: autograd needs a tensor of the output's shape to route bn3's residual gradient back here
            y = torch.empty(1, device=x.device, dtype=torch.float32).expand(x.shape)
            ctx.pair_state = _BnPairState(plan.dx_pl, tuple(ctx.needs_input_grad[:3]))
            y._bn_pair = _BnPair(*bn, word, ctx.pair_state)
        else:
            y_mask = _bn_apply(o, plan, bn, resid, y, word, rw)
        if plan.lazy:   # the hand-off to ops.conv3x3 rides on the (unwritten) output tensor itself
            # h2: the consuming convolution needs an operand scale for a tensor that never exists -- an upper bound of |relu(bn(x))|
            # from the affine parameters alone, as an amax word that travels with the hand-off (None: not h2)
            bound = _h2_slot() if h2_on() else None
            if bound is not None:
                call("tris_bn_out_bound_f32", P(gamma), P(beta), C, xmax, bound, _stream())
            y._bn_lazy = _BnLazy(*bn, bound)
        ctx.cfg = (M, C, bool(o.relu), resid is not None, count, o.group)
        ctx.grad_box, ctx.params, ctx.training = o.grad_box, (gamma, beta), bool(o.training)
        ctx.dx_pl, ctx.pool, ctx.pair, ctx.link = plan.dx_pl, bool(o.pool), pr, None
        ctx.y_pl = getattr(y, "_pl", None)
        if o.training:
            keep_y = o.relu and not o.pool and resid is not None
            ctx.save_for_backward(x, gamma, beta, bn.mean, bn.invstd, y if keep_y else None)
            if o.bwd_link and o.relu and not o.pool:
                # the consumer (ops.linear) may reduce this BatchNorm's backward sums in its data-gradient epilogue: _BnBwdLink
                ctx.link = y._bn_link = _BnBwdLink(*bn, keep_y)
                ctx.link.mask = y_mask if keep_y else None
                ctx.link.pair = pr if keep_y else None
        return y

    @staticmethod
    def backward(ctx, dy):
        """The steps: take the link; the two sums (finalized from the product's partial rows, or _bn_bwd_reduce); the SyncBN exchange or
        the parameter gradients; apply (_bn_bwd_apply, or the pair pass)"""
        if not ctx.training:
            raise NotImplementedError("BatchNorm in eval mode is forward-only on this path")
        x, gamma, beta, mean, invstd, y = ctx.saved_tensors
        M, C, relu, has_res, count, group = ctx.cfg
        st = ctx.pair_state
        if st is not None and st.done is not None:
            # the shortcut BatchNorm of a pair whose bn3 backward has done this one's as well (below): dx is written, the sums formed
            (dxs, in_arena_s, sums_s), st.done = st.done, None
            dg, db = (None, None) if in_arena_s else _bn_param_grads(ctx, sums_s, C)
            return dxs, dg, db, None, None, None, None
        dy = unplanes(pl_grad_in(dy.contiguous()))   # (the gradient of a BatchNorm OUTPUT is fp32 on every path of the trunk)
        _retag(y, ctx.y_pl)
        b = _BnBwd(x, mean, invstd, gamma, beta, M, C, ctx.pool, 1.0 / float(count), math.sqrt(max(count - 1, 1)))
        need_dx = ctx.needs_input_grad[0]
        dx_pl = ctx.dx_pl and planes_on()
        dzw = _h2_slot() if dx_pl else None    # amax word of the masked gradient dz: left by whichever pass reduces it
        dx = dg = db = d_res = None
        want_dz = has_res and ctx.needs_input_grad[5]
        if has_res and not relu:
            d_res, want_dz = (dy if want_dz else None), False
        # out = relu(bn(x) + resid): both branches see dz = dy * (out > 0); the mask is applied inside the reduce / apply
        # kernels and the apply kernel emits dz for the residual branch in the same pass
        sg, sb = _sink(ctx.params[0]), _sink(ctx.params[1])
        in_arena = (sg is not None and sb is not None and ctx.needs_input_grad[1] and ctx.needs_input_grad[2]
                    and sg.is_contiguous() and sb.is_contiguous())
        mb = None
        if group is not None and in_arena:
            from . import comm
            mb = comm.syncbn_mailbox(group, 2 * C)
        direct = in_arena and (group is None or mb is not None)
        # direct: the two LOCAL reductions ARE dbeta / dgamma, written straight into the gradient arena (mb: the sums over all ranks)
        sums = torch.empty(2 * C, device=x.device, dtype=torch.float32) if (mb is not None or not direct) else None
        p_dz, p_dzx = (P(sb), P(sg)) if direct else (P(sums), P(sums, C))
        # BatchNorm + ReLU without a residual: the mask is recomputed from x inside the kernels, y is not read
        mask_x = relu and not has_res and y is None
        # residual blocks (out = relu(bn(x) + identity)): the reduce pass writes the masked gradient dz -- which IS the identity
        # branch's gradient -- and the apply pass reads it back instead of masking dy from y a second time
        got = ctx.link.take(dy) if ctx.link is not None else None
        if got is not None and dx_pl:
            dzw = got.dzw if got.dzw is not None else _h2_amax(dy)
        dz_first = got is None and not ctx.pool and want_dz and relu and y is not None
        if dz_first:
            d_res = torch.empty_like(x)
        bound_word = None     # (operand planes: dx's bound word when the finalizer below formed it)
        if got is not None and dx_pl and mb is None and (direct or group is None) and need_dx:
            bound_word = _h2_slot()
        # cfg.bn_pair: the product that left bn3's sums also left sum(dz * xhat_s) of the shortcut BatchNorm, which receives the same
        # masked gradient: one finalizer launch for both, one apply pass that reads dz once and writes both input gradients
        pair, pair_word = ctx.pair, None
        if (pair is not None and got is not None and got.part2 is not None and bound_word is not None and group is None and want_dz
                and pair.state.dx_pl and all(pair.state.needs)):
            pair_word = _h2_slot()
        if pair_word is not None:
            sgs, sbs = _sink(pair.gamma), _sink(pair.beta)
            in_arena_s = sgs is not None and sbs is not None and sgs.is_contiguous() and sbs.is_contiguous()
            sums_s = None if in_arena_s else torch.empty(2 * C, device=x.device, dtype=torch.float32)
            ps_dz, ps_dzx = (P(sbs), P(sgs)) if in_arena_s else (P(sums_s), P(sums_s, C))
            call("tris_part_finalize_pair_f32", got.part.data_ptr(), got.part2.data_ptr(), got.rows, C, p_dz, p_dzx, ps_dz, ps_dzx, P(gamma),
                 P(invstd), P(pair.gamma), P(pair.invstd), b.inv_cnt, b.xmax, dzw, bound_word, pair_word, _stream())
        elif got is not None and bound_word is not None:
            call("tris_part_finalize_bound_f32", got.part.data_ptr(), got.rows, C, p_dz, p_dzx, P(gamma), P(invstd), b.inv_cnt, b.xmax, dzw,
                 bound_word, _stream())
        elif got is not None:
            # dy came out of the consuming 1x1 convolution's data gradient already MASKED, with the two sums as partial rows
            call("tris_part_finalize_f32", got.part.data_ptr(), got.rows, C, p_dz, p_dzx, _stream())
        else:
            _bn_bwd_reduce(b, dy, y, mask_x, p_dz, p_dzx, dzw, d_res if dz_first else None)
        if mb is not None:
            # SyncBatchNorm: the arena keeps this rank's dbeta / dgamma (the data-parallel reducer averages them like every
            # other gradient); the sums over ALL ranks that dX needs come from one peer-mailbox launch reading the arena
            if dx_pl and dzw is not None and need_dx and bound_word is None and cfg.syncbn_bound:
                bound_word = _h2_slot()
            if bound_word is not None and dx_pl and dzw is not None:   # the same launch leaves the bound word of dx
                mb.bn_bwd_exchange(sb, sg, sums, gamma, invstd, b.inv_cnt, b.xmax, dzw, bound_word)
            else:
                mb.exchange(sb, sums, 1, src1=sg)
            p_dz, p_dzx = P(sums), P(sums, C)
        elif not direct:
            dg, db = _bn_param_grads(ctx, sums, C)
            if group is not None:
                from . import comm
                comm.syncbn_all_reduce_sum(sums, group=group)
        if pair_word is not None:
            d_res = dy              # (what autograd routes to the shortcut BatchNorm's node; that node finds its work done)
            dx, dxs = torch.empty_like(x), torch.empty_like(x)
            call("tris_bn_bwd_apply_pair_pl_f32", P(dy), P(x), P(mean), P(invstd), P(gamma), p_dzx, P(pair.x), P(pair.mean), P(pair.invstd),
                 P(pair.gamma), ps_dzx, p_dz, b.inv_cnt, P(dx), bound_word, P(dxs), pair_word, M, C, _stream())
            pl_grad_out(dx, bound_word)
            pl_grad_out(dxs, pair_word)
            pair.state.done = (dxs, in_arena_s, sums_s)
        elif ctx.pool or got is not None or dz_first:
            if got is not None and want_dz:
                d_res = dy          # the masked gradient IS the identity branch's gradient
            if need_dx:
                dx = torch.empty_like(x)
                _bn_bwd_apply(b, d_res if dz_first else dy, None, None, None, dx, p_dz, p_dzx, dzw, bound_word, dx_pl)
        elif need_dx or want_dz:
            dx = torch.empty_like(x)
            if want_dz:
                d_res = torch.empty_like(x)
            _bn_bwd_apply(b, dy, None if mask_x else y, d_res if want_dz else None, beta if mask_x else None, dx, p_dz, p_dzx, dzw,
                          bound_word, dx_pl)
        if ctx.grad_box is not None and d_res is not None and ctx.grad_box.deposit(d_res):
            d_res = None   # handed to the block's first conv
        return dx, dg, db, None, None, d_res, None


def batch_norm(x, gamma, beta, rmean, rvar, resid=None, relu=False, training=True, momentum=0.1, eps=1e-5, group=None,
               grad_box=None, lazy=False, bwd_link=False, pool=False, planes=False, dx_planes=False, pair=False):
    """lazy=True (train-mode BatchNorm + ReLU whose ONLY consumer is ops.conv3x3, and conv3x3_bnin_ok said yes): the returned
    tensor is an unwritten buffer carrying `_bn_lazy`; pass it to ops.conv3x3 and nowhere else.
    planes / dx_planes (h2 with operand planes, train mode): the output is WRITTEN as fp16 operand planes -- the caller vouches that
    every consumer is a product, a plane-aware BatchNorm / pool, or goes through ops.unplanes -- and so is the input gradient (its one
    consumer is the backward of the convolution before).
    pair (the shortcut BatchNorm of a down-sampling Bottleneck; cfg.bn_pair): the output's ONLY reader is the block's bn3, as its
    residual -- where the plane path applies the statistics are formed here, the output is NOT written, and what comes back is an
    unallocated stand-in carrying `_bn_pair`; bn3's pass normalises the shortcut's raw input itself (tris_bn_apply_pair_pl_f32).
    pool: the output is avgpool2(relu(bn(x))) -- BatchNorm + ReLU + AvgPool2d(2) as one op, the full-size tensor never written (needs
    train mode, ReLU, no residual, an even map: otherwise the two ops one after the other)."""
    part = getattr(x, "_bn_part", None) if training else None
    bwd_link = bool(bwd_link and training and torch.is_grad_enabled() and x.requires_grad and cfg.bn_bwd_fuse)
    o = _BnOpts(relu, training, momentum, eps, group, part, grad_box, lazy, bwd_link, bool(pool), planes, dx_planes, pair)
    if pool and not (training and relu and resid is None and not lazy and x.dim() == 4 and x.shape[1] % 2 == 0
                     and x.shape[2] % 2 == 0 and cfg.bn_pool):
        return avgpool2(BatchNormFn.apply(x, gamma, beta, rmean, rvar, resid, o._replace(pool=False)))
    return BatchNormFn.apply(x, gamma, beta, rmean, rvar, resid, o)


class AvgPool2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, grad_box_out=None):
        _chk(x)
        ctx.grad_box_out = grad_box_out
        x = x.contiguous()
        B, H, W, C = x.shape
        y = torch.empty(B, H // 2, W // 2, C, device=x.device, dtype=torch.float32)
        w = pl_word(x)
        if w is not None and C % 8 == 0:   # planes in, planes out at the same scale (a mean never exceeds the bound of its terms)
            call("tris_avgpool2_fwd_pl_f32", P(x), P(y), w, B, H, W, C, _stream())
            pl_tag(y, w)
        else:
            call("tris_avgpool2_fwd_f32", P(unplanes(x)), P(y), B, H, W, C, _stream())
        ctx.shape = (B, H, W, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, H, W, C = ctx.shape
        dy = unplanes(pl_grad_in(dy.contiguous()))
        box = ctx.grad_box_out
        if (box is not None and cfg.bn_pair and "pool" in cfg.bn_pair_parts and planes_on() and C % 4 == 0 and H % 2 == 0 and W % 2 == 0 and dy.data_ptr() % 16 == 0
                and box.deposit(dy)):
            box.pool = (H, W)     # the pooled gradient itself: the block's first conv reads it in place (GradBox.pool)
            return None, None
        dx = _avgpool2_bwd(dy, (B, H, W, C))
        if box is not None and box.deposit(dx):
            dx = None
        return dx, None


def _avgpool2_bwd(dy, shape):
    B, H, W, C = shape
    dx = torch.empty(B, H, W, C, device=dy.device, dtype=torch.float32)
    call("tris_avgpool2_bwd_f32", P(dy), P(dx), B, H, W, C, _stream())
    return dx


def avgpool2(x, grad_box_out=None):
    return AvgPool2Fn.apply(x, grad_box_out)


# ----------------------------------------------------------------------------------------------- transformer pieces
class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g, b, eps, grad_box=None):
        _chk(x, g, b)
        ctx.grad_box = grad_box
        x = x.contiguous()
        W = x.shape[-1]
        rows = x.numel() // W
        y = torch.empty_like(x)
        st = torch.empty(2, rows, device=x.device, dtype=torch.float32)
        h2_mark_next(y)
        call("tris_layernorm_fwd_f32", P(x), P(g), P(b), P(y), P(st), P(st, rows), rows, W, eps, _stream())
        ctx.dims = (rows, W)
        ctx.params = (g, b)
        ctx.save_for_backward(x, g, b, st)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g, b, st = ctx.saved_tensors
        rows, W = ctx.dims
        dy = dy.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        box, extra = ctx.grad_box, None
        if box is not None:   # the block's residual gradient (left by the Linear that added x back): summed in this kernel
            box.consumed = True
            if box.value is not None:
                extra, box.value = box.value.contiguous(), None
                if dx is None:
                    raise RuntimeError("a residual gradient was handed to a LayerNorm whose input needs no gradient")
        need_p = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        ws = workspace(query("tris_layernorm_bwd_workspace_bytes", rows, W))
        sg, sb = _sink(ctx.params[0]), _sink(ctx.params[1])
        if need_p and sg is not None and sb is not None and sg.is_contiguous() and sb.is_contiguous():
            h2_mark_next(dx)
            call("tris_layernorm_bwd_f32", P(dy), P(x), P(g), P(st), P(st, rows), P(dx), P(sg), P(sb), rows, W, P(ws),
                 P(extra), _stream())
            return dx, None, None, None, None
        dgb = torch.empty(2, W, device=x.device, dtype=torch.float32) if need_p else None
        h2_mark_next(dx)
        call("tris_layernorm_bwd_f32", P(dy), P(x), P(g), P(st), P(st, rows), P(dx), P(dgb), P(dgb, W),
             rows, W, P(ws), P(extra), _stream())
        dg = _emit(ctx.params[0], lambda o: o.copy_(dgb[0]), ctx.needs_input_grad[1])
        db = _emit(ctx.params[1], lambda o: o.copy_(dgb[1]), ctx.needs_input_grad[2])
        return dx, dg, db, None, None


def layer_norm(x, g, b, eps=1e-5, grad_box=None):
    return LayerNormFn.apply(x, g, b, eps, grad_box)


class MhaFn(torch.autograd.Function):
    """qkv [N, L, 3W] -> [N, L, W]; heads of 64."""

    @staticmethod
    def forward(ctx, qkv, heads, causal):
        _chk(qkv)
        qkv = qkv.contiguous()
        N, L, W3 = qkv.shape
        W = W3 // 3
        out = torch.empty(N, L, W, device=qkv.device, dtype=torch.float32)
        h2_mark_next(out)
        call("tris_mha_fwd_f32", P(qkv), P(out), N, L, W, heads, int(causal), _stream())
        ctx.cfg = (N, L, W, heads, int(causal))
        ctx.save_for_backward(qkv)
        return out

    @staticmethod
    def backward(ctx, do):
        (qkv,) = ctx.saved_tensors
        N, L, W, heads, causal = ctx.cfg
        do = do.contiguous()
        dqkv = torch.empty_like(qkv)
        h2_mark_next(dqkv)
        call("tris_mha_bwd_f32", P(qkv), P(do), P(dqkv), N, L, W, heads, causal, _stream())
        return dqkv, None, None


MHA_STATS = {"last": None}     # arithmetic of the last flash-style forward: "h2" | "f32" (tests)


class MhaMfmaFn(torch.autograd.Function):
    """Flash-style attention on the f32 MFMA, any L (csrc/attn_mfma.hip); saves the per-query log-sum-exp."""

    @staticmethod
    def forward(ctx, qkv, heads, causal):
        _chk(qkv)
        qkv = qkv.contiguous()
        N, L, W3 = qkv.shape
        W = W3 // 3
        out = torch.empty(N, L, W, device=qkv.device, dtype=torch.float32)
        lse = torch.empty(N, heads, L, device=qkv.device, dtype=torch.float32)
        # inside an h2 step the products run on two fp16 pieces per operand (csrc/attn_h2.hip, 16-bit MFMA), scaled by qkv's amax word
        # (from L = 32 on: at the text encoder's L = 20 the split while staging costs more than the 16-bit MFMA saves, tools/mha_bench.py)
        w_qkv = _h2_amax(qkv) if (h2_on() and cfg.mha_h2 and L >= 32) else None
        h2_mark_next(out)
        if w_qkv is not None:
            _timed("mha_fwd", 4.0 * N * heads * L * L * 64 * (0.5 if causal else 1.0),
                   lambda: call("tris_mha_h2_fwd_f32", P(qkv), P(out), P(lse), w_qkv, N, L, W, heads, int(causal), _stream()))
        else:
            _timed("mha_fwd", 4.0 * N * heads * L * L * 64 * (0.5 if causal else 1.0),
                   lambda: call("tris_mha_mfma_fwd_f32", P(qkv), P(out), P(lse), N, L, W, heads, int(causal), _stream()))
        MHA_STATS["last"] = "h2" if w_qkv is not None else "f32"
        ctx.h2 = w_qkv is not None
        ctx.cfg = (N, L, W, heads, int(causal))
        ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    def backward(ctx, do):
        qkv, out, lse = ctx.saved_tensors
        N, L, W, heads, causal = ctx.cfg
        do = do.contiguous()
        dqkv = torch.empty_like(qkv)
        delta = torch.empty_like(lse)
        w_qkv = w_do = None
        if ctx.h2 and h2_on():
            w_qkv, w_do = _h2_amax(qkv), _h2_amax(do)
        h2_mark_next(dqkv)
        if w_qkv is not None and w_do is not None:
            call("tris_mha_h2_bwd_f32", P(qkv), P(out), P(do), P(lse), P(delta), P(dqkv), w_qkv, w_do, N, L, W, heads, causal, _stream())
        else:
            call("tris_mha_mfma_bwd_f32", P(qkv), P(out), P(do), P(lse), P(delta), P(dqkv), N, L, W, heads, causal, _stream())
        return dqkv, None, None


def _mha_impl(L):
    """'valu' = the LDS-resident kernel for L <= 64 (csrc/attn.hip), 'mfma' = the flash-style MFMA kernel (any L).
    TRIS_MHA=valu|mfma forces one; default 'auto' takes the measured faster one: at L = 20 (text) the op is an HBM stream
    of the packed QKV and the single-launch backward of the LDS-resident kernel wins (654 vs 806 us at N = 3840), from
    L = 50 (aux ViT) on the MFMA kernel does (fwd 47 vs 53 us, bwd 126 vs 159 us; L = 401: 73 / 84 TFLOP/s)."""
    import os
    mode = cfg.mha
    if L > 64 or mode == "mfma":
        return "mfma"
    if mode == "valu":
        return "valu"
    return "valu" if L < 40 else "mfma"


def mha(qkv, heads, causal):
    if _mha_impl(qkv.shape[1]) == "valu":
        return MhaFn.apply(qkv, heads, causal)
    return MhaMfmaFn.apply(qkv, heads, causal)


class QGeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return ew("TRIS_EW_QGELU", x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return ew("TRIS_EW_QGELU_BWD", dy.contiguous(), x)


def quick_gelu(x):
    return QGeluFn.apply(x)


class EmbedFn(torch.autograd.Function):
    """token_embedding(ids) + positional_embedding[:L]  (CLIP/clip/model.py:553-554).

    Backward: the positional gradient is a column sum; the token gradient is built from the ROW LIST (ids, d_out rows) by a
    deterministic kernel (tris_embed_rows_bwd_f32).  Data-parallel (`reducer` given and it takes the table): the list is handed
    to the reducer, which all-gathers the <= B*L rows of every rank and builds the SAME mean gradient on every rank -- 2 MB per
    rank on the wire instead of the dense 101 MB table."""

    @staticmethod
    def forward(ctx, ids, tok, pos, reducer=None):
        _chk(ids, tok, pos)
        ids = ids.contiguous()
        N, L = ids.shape
        W = tok.shape[1]
        out = torch.empty(N, L, W, device=tok.device, dtype=torch.float32)
        call("tris_embed_fwd_f32", P(ids), P(tok), P(pos), P(out), N, L, W, _stream())
        ctx.params = (tok, pos)
        ctx.reducer = reducer
        ctx.save_for_backward(ids, tok, pos)
        return out

    @staticmethod
    def backward(ctx, dout):
        ids, tok, pos = ctx.saved_tensors
        N, L = ids.shape
        W = tok.shape[1]
        dout = dout.contiguous()
        st = _sink(ctx.params[0]), _sink(ctx.params[1])
        dtok = st[0] if st[0] is not None else torch.empty_like(tok)
        dpos = st[1] if st[1] is not None else torch.empty_like(pos)
        dtok.zero_()
        dpos.zero_()
        call("tris_embed_bwd_f32", P(ids), P(dout), None, P(dpos), N, L, W, _stream())     # positional part
        red = ctx.reducer
        if red is not None and st[0] is not None and W % 4 == 0 and W <= 2048 and red.take_embedding_rows(ctx.params[0], ids.view(-1), dout.view(N * L, W), dtok):
            pass     # the reducer gathers every rank's rows and scatters them (scale 1 / world) into dtok
        elif W % 4 == 0 and W <= 2048:
            call("tris_embed_rows_bwd_f32", P(ids), P(dout), P(dtok), N * L, W, 1.0, _stream())
        else:
            call("tris_embed_bwd_f32", P(ids), P(dout), P(dtok), None, N, L, W, _stream())
        return None, (None if st[0] is not None else dtok), (None if st[1] is not None else dpos), None


def embed(ids, tok, pos, reducer=None):
    return EmbedFn.apply(ids, tok, pos, reducer)


class EotGatherFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, x):
        _chk(ids, x)
        ids, x = (None if ids is None else ids.contiguous()), x.contiguous()
        N, L, W = x.shape
        out = torch.empty(N, W, device=x.device, dtype=torch.float32)
        call("tris_eot_gather_fwd_f32", P(ids), P(x), P(out), N, L, W, _stream())
        ctx.save_for_backward(ids)
        ctx.dims = (N, L, W)
        return out

    @staticmethod
    def backward(ctx, dout):
        (ids,) = ctx.saved_tensors
        N, L, W = ctx.dims
        dx = torch.empty(N, L, W, device=dout.device, dtype=torch.float32)
        call("tris_eot_gather_bwd_f32", P(ids), P(dout.contiguous()), P(dx), N, L, W, _stream())
        return None, dx


def eot_gather(ids, x):
    return EotGatherFn.apply(ids, x)


# ---- packed text rows (csrc/attn.hip "packed text rows"; include/tris_hip.h) -- forward only, no autograd: the frozen aux tower
class rows_limit:
    """inside: this thread's tris_gemm_f32 (row-major A) and LayerNorm-forward launches skip rows >= plan[1] (a device word)"""

    def __init__(self, plan):
        self.ptr = plan.data_ptr() + 4

    def __enter__(self):
        call("tris_rows_limit_thread", self.ptr)
        _TLS.rows_limit = self.ptr      # (ops.gemm: no amax pre-pass over an operand whose rows behind the limit may hold anything)

    def __exit__(self, *exc):
        _TLS.rows_limit = None
        call("tris_rows_limit_thread", None)
        return False


def _rows_limit_blind(A, tA, batch):
    """A row limit is live, the product obeys it (row-major A, one batch) and A carries no amax word of this step: the h2 pre-pass
    (tris_amax_bits_f32 over ALL of A) would read the rows behind the limit, which a packed pass never writes -- torch.empty
    memory, possibly NaN or huge -- into the scale of the rows in use.  Such a product runs in x3 (no data-dependent scale); its
    output is tagged by its own launch, so the next product is back in h2.  CLIP.encode_text_hidden never gets here: every A of the
    packed pass is written by the launch right before the product that reads it and tagged there (LayerNorm, attention, product),
    over the rows in use only; this guards callers of ops.gemm that bring an operand of their own under ops.rows_limit."""
    return (getattr(_TLS, "rows_limit", None) is not None and batch == 1 and not tA and h2_on() and pl_word(A) is None
            and _h2_tag_slot(A) is None)


def packed_rows(N, L):
    """rows of every packed buffer: N L rounded up to the 256-row granule of the row limit"""
    return (N * L + 255) // 256 * 256


def text_packable(L):
    return not _BATCH_INVARIANT and 1 <= L <= 64


def text_pack_plan(ids):
    """ids int64 [N, L] -> plan (int32 device array: rows in use, row limit, first row of every sentence, source token of every row)"""
    N, L = ids.shape
    plan = torch.empty(3 + N + packed_rows(N, L), device=ids.device, dtype=torch.int32)
    call("tris_text_pack_plan_i64", P(ids), N, L, plan.data_ptr(), _stream())
    return plan


def embed_packed(ids, tok, pos, plan):
    N, L = ids.shape
    W = tok.shape[1]
    out = torch.empty(packed_rows(N, L), W, device=tok.device, dtype=torch.float32)
    call("tris_embed_packed_fwd_f32", P(ids), P(tok), P(pos), plan.data_ptr(), P(out), N, L, W, _stream())
    return out


def mha_packed(qkv, plan, N, L, heads, causal):
    """qkv [N L, 3 W] packed rows -> out [N L, W]; sentence n attends inside its own row range (L: the longest possible sentence)"""
    W = qkv.shape[-1] // 3
    out = torch.empty(qkv.shape[0], W, device=qkv.device, dtype=torch.float32)
    h2_mark_next(out)
    call("tris_mha_packed_fwd_f32", P(qkv), P(out), plan.data_ptr(), N, L, W, heads, int(causal), _stream())
    return out


def eot_gather_packed(x, plan, N):
    out = torch.empty(N, x.shape[-1], device=x.device, dtype=torch.float32)
    call("tris_eot_gather_packed_f32", P(x), plan.data_ptr(), P(out), N, x.shape[-1], _stream())
    return out


def token0(x):
    """x[:, 0, :] of [N, L, W] as a copy, with its own backward kernel (the ViT class token, CLIP/clip/model.py:443)"""
    return EotGatherFn.apply(None, x)


# ----------------------------------------------------------------------------------------------- CLIP attention pooling (inference)
ATTNPOOL_LMAX = CONSTS["TRIS_ATTNPOOL_LMAX"]


def _no_backward(name, *ts):
    """the attention pooling has no backward (nothing trains through it in the reference's scripts): refuse to drop a gradient silently"""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise NotImplementedError(f"ops.{name} is forward only (no backward kernel): call it under torch.no_grad() or detach its inputs")


def attnpool_tokens(c4_cl, pos, S):
    """The token matrix of AttentionPool2d (CLIP/clip/model.py:70-83) in one launch: c4_cl [B,h,w,C] channels-last (fp32 or operand
    planes), pos [S*S+1, C] -> T [B, hw+1, C]; row 0 = mean over the pixels + pos[0], row 1+i = pixel i + the S x S grid of pos[1:]
    resized bilinearly to h x w (F.interpolate's defaults).  Forward only."""
    _no_backward("attnpool_tokens", c4_cl, pos)
    if c4_cl.dim() != 4 or pos.dim() != 2:
        raise ValueError(f"ops.attnpool_tokens: c4_cl [B,h,w,C] and pos [S*S+1,C] expected, got {tuple(c4_cl.shape)} and {tuple(pos.shape)}")
    B, h, w, C = c4_cl.shape
    if C % 4 or C < 4:
        raise ValueError(f"ops.attnpool_tokens: C % 4 == 0 required, got C = {C}")
    if h * w + 1 > ATTNPOOL_LMAX:
        raise ValueError(f"ops.attnpool_tokens: L = h*w + 1 = {h * w + 1} exceeds the limit L <= {ATTNPOOL_LMAX}")
    if S < 1 or tuple(pos.shape) != (S * S + 1, C):
        raise ValueError(f"ops.attnpool_tokens: pos must be [S*S+1, C] = [{S * S + 1}, {C}], got {tuple(pos.shape)}")
    if B < 1 or B > 65535 or h < 1 or w < 1:
        raise ValueError(f"ops.attnpool_tokens: 1 <= B <= 65535 and a non-empty map required, got {tuple(c4_cl.shape)}")
    _chk(c4_cl, pos)
    with torch.no_grad():
        x = unplanes(c4_cl).contiguous()
        pos = pos.detach().contiguous()
        T = torch.empty(B, h * w + 1, C, device=x.device, dtype=torch.float32)
        call("tris_attnpool_tokens_f32", P(x), P(pos), P(T), B, h, w, C, S, _stream())
    return T


def attnpool_pool(T, U, scale):
    """The one-query attention of the folded global embedding: T [B,L,C] tokens, U [B,heads,C] (contiguous, or the
    transposed view of a dense head-major [heads,B,C] buffer -- what a per-head ops.bmm writes and reads: taken as it is, no copy) ->
    (P [B,heads,L] = softmax_j(scale * T[b,j] . U[b,h]), pooled [B,heads,C] = sum_j P[b,h,j] T[b,j], laid out in memory like U).
    Forward only."""
    _no_backward("attnpool_pool", T, U)
    if T.dim() != 3 or U.dim() != 3 or U.shape[0] != T.shape[0] or U.shape[2] != T.shape[2]:
        raise ValueError(f"ops.attnpool_pool: T [B,L,C] and U [B,heads,C] expected, got {tuple(T.shape)} and {tuple(U.shape)}")
    B, L, C = T.shape
    heads = U.shape[1]
    if C % 4 or C < 4:
        raise ValueError(f"ops.attnpool_pool: C % 4 == 0 required, got C = {C}")
    if L < 1 or L > ATTNPOOL_LMAX:
        raise ValueError(f"ops.attnpool_pool: L = {L} outside the limit 1 <= L <= {ATTNPOOL_LMAX}")
    if B < 1 or heads < 1:
        raise ValueError(f"ops.attnpool_pool: B >= 1 and heads >= 1 required, got {tuple(U.shape)}")
    _chk(T, U)
    with torch.no_grad():
        T = unplanes(T).contiguous()
        U = unplanes(U).detach()
        head_major = U.stride() == (C, B * C, 1)          # the [B,heads,C] view of a dense [heads,B,C] buffer
        if not head_major:
            U = U.contiguous()
        Pr = torch.empty(B, heads, L, device=T.device, dtype=torch.float32)
        pooled = torch.empty_strided((B, heads, C), U.stride(), device=T.device, dtype=torch.float32)
        call("tris_attnpool_pool_f32", P(T), P(U), U.stride(0), U.stride(1), float(scale), P(Pr), P(pooled), B, L, C, heads, _stream())
    return Pr, pooled


# ----------------------------------------------------------------------------------------------- heads
class L2NormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _chk(x)
        x = x.contiguous()
        C = x.shape[-1]
        rows = x.numel() // C
        y = torch.empty_like(x)
        inv = torch.empty(rows, device=x.device, dtype=torch.float32)
        call("tris_l2norm_fwd_f32", P(x), P(y), P(inv), rows, C, _stream())
        ctx.save_for_backward(y, inv)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, inv = ctx.saved_tensors
        dx = torch.empty_like(y)
        call("tris_l2norm_bwd_f32", P(dy.contiguous()), P(y), P(inv), P(dx), inv.numel(), y.shape[-1], _stream())
        return dx


def l2norm(x):
    return L2NormFn.apply(x)


class SoftmaxFn(torch.autograd.Function):
    """softmax(scale * x) over the last dim"""

    @staticmethod
    def forward(ctx, x, scale):
        _chk(x)
        x = x.contiguous()
        n = x.shape[-1]
        y = torch.empty_like(x)
        call("tris_softmax_fwd_f32", P(x), P(y), x.numel() // n, n, scale, _stream())
        ctx.scale = scale
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        n = y.shape[-1]
        dx = torch.empty_like(y)
        call("tris_softmax_bwd_f32", P(dy.contiguous()), P(y), P(dx), y.numel() // n, n, ctx.scale, _stream())
        return dx, None


def softmax(x, scale=1.0):
    return SoftmaxFn.apply(x, scale)


class InstNormFn(torch.autograd.Function):
    """InstanceNorm2d(affine) [+ReLU] on channels-last x [B, P, C]"""

    @staticmethod
    def forward(ctx, x, g, b, relu, eps):
        _chk(x, g, b)
        x = x.contiguous()
        B, Pp, C = x.shape
        y = torch.empty_like(x)
        st = torch.empty(2, B, C, device=x.device, dtype=torch.float32)
        h2_mark_next(y)     # (h2: the launch leaves y's amax -- its consumers are dense products)
        call("tris_instnorm_fwd_f32", P(x), P(g), P(b), P(y), P(st), P(st, B * C), B, Pp, C, eps, int(relu), _stream())
        ctx.relu = bool(relu)
        ctx.params = (g, b)
        ctx.save_for_backward(x, g, b, st, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g, b, st, y = ctx.saved_tensors
        B, Pp, C = x.shape
        dx = torch.empty_like(x)
        parts = torch.empty(2, B, C, device=x.device, dtype=torch.float32)
        h2_mark_next(dx)
        call("tris_instnorm_bwd_f32", P(dy.contiguous()), P(y), P(x), P(g), P(st), P(st, B * C), P(dx), P(parts),
             P(parts, B * C), B, Pp, C, int(ctx.relu), _stream())
        dg = _emit(ctx.params[0], lambda o: colsum(parts[0], B, C, o), ctx.needs_input_grad[1], reads=(parts,))
        db = _emit(ctx.params[1], lambda o: colsum(parts[1], B, C, o), ctx.needs_input_grad[2], reads=(parts,))
        return dx, dg, db, None, None


def instance_norm(x, g, b, relu=False, eps=1e-5):
    return InstNormFn.apply(x, g, b, relu, eps)


_XATTN_SYNC = {}
_XATTN_SPARE = {}      # device -> zeroed buffers allocated OUTSIDE any stream capture, for streams first seen under one
_XATTN_WORDS = 16 + 8 * 64


def _xattn_sync(dev, B):
    """the fused cross-attention kernel's device-side bookkeeping (launch epoch, finish ticket, time-out flag, publish flags):
    zeroed once, then owned by the kernel.  One buffer per (device, stream): launches on one stream are ordered.
    Nothing is allocated -- or cleared -- inside a stream capture: a capture runs on a stream of its own, so its first launch meets a
    stream without a buffer; a buffer created there would live in the graph's private pool and its zero-fill would be a graph node,
    i.e. every replay would clear the STICKY time-out word (sync[2]) before anyone looked at it.  Eager launches (the priming steps
    every capture is preceded by) keep spare buffers ready; a capture takes one of those."""
    key = (dev, torch.cuda.current_stream().cuda_stream)
    n = max(int(query("tris_xattn_fused_sync_words", B)), int(query("tris_xattn_px_sync_words", B)), _XATTN_WORDS)
    capturing = torch.cuda.is_current_stream_capturing()
    spare = _XATTN_SPARE.setdefault(dev, [])
    if not capturing:
        while len(spare) < 3 or any(b.numel() < n for b in spare):
            spare[:] = [b for b in spare if b.numel() >= n]
            spare.append(torch.zeros(n, device=dev, dtype=torch.int32))
    t = _XATTN_SYNC.get(key)
    if t is None or t.numel() < n:
        if capturing:
            fit = [b for b in spare if b.numel() >= n]
            if not fit:
                raise RuntimeError("fused cross attention: no sync buffer for a stream first seen under capture "
                                   "(run one eager step with the largest batch before capturing)")
            t = fit[0]
            spare.remove(t)
        else:
            t = torch.zeros(n, device=dev, dtype=torch.int32)
        _XATTN_SYNC[key] = t
    return t


def xattn_timed_out(collective=False):
    """True if a wait inside any fused cross-attention launch gave up (host sync).  The word is sticky: nothing but this process's
    exit clears it.  collective=True (every rank calls it at the same point): the answer is the group's, so that all ranks stop
    together instead of one raising while its peers wait for it in a collective."""
    hit = any(int(t[2].item()) != 0 for t in _XATTN_SYNC.values())
    if collective and torch.distributed.is_available() and torch.distributed.is_initialized():
        f = torch.tensor([1.0 if hit else 0.0], device="cuda" if torch.cuda.is_available() else "cpu")
        torch.distributed.all_reduce(f, op=torch.distributed.ReduceOp.MAX)
        hit = bool(f.item() > 0)
    return hit


def _xattn_arm(*six):
    """h2: the next pixel-row launch runs on two fp16 pieces per operand, scaled by the amax words of its six operands (a pre-pass where none is left)"""
    if h2_on() and cfg.xattn_h2:
        words = [_h2_amax(t) for t in six]
        if all(w is not None for w in words):
            call("tris_xattn_amax_next", *words)


class XAttnFn(torch.autograd.Function):
    """Fused bilateral cross attention (model/attn.py:117-128): forward = tris_xattn_fwd (two launches for the whole
    batch); backward = nine large single GEMMs on the saved probabilities + two softmax-backward kernels."""

    @staticmethod
    def forward(ctx, Qv, Kv, Vv, Qt, Kt, Vt):
        _chk(Qv, Kv, Vv, Qt, Kt, Vt)
        Qv, Kv, Vv, Qt, Kt, Vt = (t.contiguous() for t in (Qv, Kv, Vv, Qt, Kt, Vt))
        B, Pp, C = Qv.shape
        N = Qt.shape[0]
        dev = Qv.device
        new_vis = torch.empty(B, Pp, C, device=dev, dtype=torch.float32)
        new_lan = torch.empty(B, N, C, device=dev, dtype=torch.float32)
        probs = torch.empty(B, 4, Pp, N, device=dev, dtype=torch.float32)
        done = px_ran = False
        # ONE persistent launch where a kernel's domain covers the shape and all its workgroups are co-resident: cut by pixel rows
        # (csrc/xattn_px.hip, S <= 8 workgroups per image, one hand-off) or, failing that, by channel slices (csrc/xattn_fused.hip,
        # eight per image, three hand-offs); TRIS_XATTN_FUSED=0 forces the two-launch pair
        for kind, on in (("px", cfg.xattn_fused and cfg.xattn_px), ("fused", cfg.xattn_fused)):
            ws_bytes = query(f"tris_xattn_{kind}_ws_bytes", B, N, C) if on and not done else 0
            if ws_bytes > 0:
                ws = torch.empty(ws_bytes // 4 + 4, device=dev, dtype=torch.float32)
                sync = _xattn_sync(dev, B)
                if kind == "px":
                    _xattn_arm(Qv, Kv, Vv, Qt, Kt, Vt)
                done = _timed(f"xattn_fwd_{kind}", 8.0 * B * Pp * N * C, lambda: _declinable(
                    f"tris_xattn_{kind}_fwd_f32", P(Qv), P(Kv), P(Vv), P(Qt), P(Kt), P(Vt), P(new_vis), P(new_lan), P(probs), B,
                    Pp, N, C, P(ws), ws.numel() * 4, sync.data_ptr(), _stream()))
                px_ran = done and kind == "px"
        if not done:
            _timed("xattn_fwd_pair", 8.0 * B * Pp * N * C,
                   lambda: call("tris_xattn_fwd_f32", P(Qv), P(Kv), P(Vv), P(Qt), P(Kt), P(Vt), P(new_vis), P(new_lan),
                                P(probs), B, Pp, N, C, _stream()))
        ctx.dims = (B, Pp, N, C)
        ctx.px_form = px_ran
        ctx.save_for_backward(Qv, Kv, Vv, Qt, Kt, Vt, probs)
        return new_vis, new_lan

    @staticmethod
    def _backward_px(ctx, d_vis, d_lan):
        """the pixel-row form of the backward (csrc/xattn_px.hip): one persistent launch for dQv, dKv, dVv and the two soft-max
        backwards, then the three [N, C] sums over images and pixels as split-K products.  None: outside its domain."""
        Qv, Kv, Vv, Qt, Kt, Vt, probs = ctx.saved_tensors
        B, Pp, N, C = ctx.dims
        dev = Qv.device
        ws_bytes = query("tris_xattn_px_bwd_ws_bytes", B, N, C)
        if ws_bytes <= 0:
            return None
        ws = torch.empty(ws_bytes // 4 + 4, device=dev, dtype=torch.float32)
        sync = _xattn_sync(dev, B)
        dQv, dKv, dVv = (torch.empty(B, Pp, C, device=dev, dtype=torch.float32) for _ in range(3))
        dS = torch.empty(3, B * Pp, N, device=dev, dtype=torch.float32)
        _xattn_arm(d_vis, Vv, d_lan, Qt, Kt, Vt)
        slots = [_h2_slot() if h2_on() else None for _ in range(3)]   # the launch leaves the amax words of its three outputs
        if not _timed("xattn_bwd_px", 10.0 * B * Pp * N * C, lambda: _declinable(
                "tris_xattn_px_bwd_f32", P(d_vis), P(d_lan), P(Vv), P(Qt), P(Kt), P(Vt), P(probs), P(dQv), P(dKv), P(dVv), P(dS), B, Pp,
                N, C, P(ws), ws.numel() * 4, sync.data_ptr(), slots[0], slots[1], slots[2], _stream())):
            return None
        for t, slot in zip((dQv, dKv, dVv), slots):
            if slot is not None:
                h2_tag(t, slot)
        BP = B * Pp
        new = lambda: torch.empty(N, C, device=dev, dtype=torch.float32)
        dVt = gemm(dS[2], d_vis, new(), N, C, BP, N, C, C, True, False)       # Av^T . d_vis
        dKt = gemm(dS[0], Qv, new(), N, C, BP, N, C, C, True, False)          # dS1^T . Qv
        dQt = gemm(dS[1], Kv, new(), N, C, BP, N, C, C, True, False)          # dS2^T . Kv
        return dQv, dKv, dVv, dQt, dKt, dVt

    @staticmethod
    def backward(ctx, d_vis, d_lan):
        Qv, Kv, Vv, Qt, Kt, Vt, probs = ctx.saved_tensors
        B, Pp, N, C = ctx.dims
        dev = Qv.device
        scale = 1.0 / math.sqrt(C)
        d_vis, d_lan = d_vis.contiguous(), d_lan.contiguous()
        if ctx.px_form and cfg.xattn_bwd_px:
            got = XAttnFn._backward_px(ctx, d_vis, d_lan)
            if got is not None:
                return got
        BP = B * Pp
        Av = probs[:, 0].contiguous().view(BP, N)
        AtT = probs[:, 2].contiguous().view(B, Pp, N)

        def new(*shape):
            return torch.empty(*shape, device=dev, dtype=torch.float32)
        # pixel -> sentence direction:  new_vis = Av . Vt
        dAv = gemm(d_vis, Vt, new(BP, N), BP, N, C, C, C, N, False, True)                      # [BP,N] = d_vis . Vt^T
        dVt = gemm(Av, d_vis, new(N, C), N, C, BP, N, C, C, True, False)                       # Av^T . d_vis
        dS1 = new(BP, N)
        call("tris_softmax_bwd_f32", P(dAv), P(Av), P(dS1), BP, N, scale, _stream())
        dQv = gemm(dS1, Kt, new(B, Pp, C), BP, C, N, N, C, C, False, False)                    # dS1 . Kt
        dKt = gemm(dS1, Qv, new(N, C), N, C, BP, N, C, C, True, False)                         # dS1^T . Qv
        # sentence -> pixel direction:  new_lan[b] = AtT[b]^T . Vv[b]
        dAtT = gemm(Vv, d_lan, new(B, Pp, N), Pp, N, C, C, C, N, False, True, batch=B, sA=Pp * C, sB=N * C, sC=Pp * N)
        dVv = gemm(AtT, d_lan, new(B, Pp, C), Pp, C, N, N, C, C, False, False, batch=B, sA=Pp * N, sB=N * C, sC=Pp * C)
        dS2 = new(B, Pp, N)
        call("tris_softmax_col_bwd_f32", P(dAtT), P(AtT), P(dS2), B, Pp, N, scale, _stream())
        dKv = gemm(dS2, Qt, new(B, Pp, C), BP, C, N, N, C, C, False, False)                    # dS2T . Qt
        dQt = gemm(dS2, Kv, new(N, C), N, C, BP, N, C, C, True, False)                         # dS2T^T . Kv
        return dQv, dKv, dVv, dQt, dKt, dVt


def xattn(Qv, Kv, Vv, Qt, Kt, Vt):
    return XAttnFn.apply(Qv, Kv, Vv, Qt, Kt, Vt)


class AxpyFn(torch.autograd.Function):
    """s * a + b.  grad_box_b: b's gradient (dy itself) is left in that GradBox for another consumer of b to add in its
    data-gradient epilogue instead of being summed by autograd."""

    @staticmethod
    def forward(ctx, a, b, s, grad_box_b=None):
        ctx.s, ctx.box = s, grad_box_b
        return ew("TRIS_EW_AXPY", a.contiguous(), b.contiguous(), s)

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        da = ew("TRIS_EW_SCALE", dy, None, ctx.s) if ctx.needs_input_grad[0] else None
        db = dy if ctx.needs_input_grad[1] else None
        if db is not None and ctx.box is not None and ctx.box.deposit(db):
            db = None
        return da, db, None, None


def axpy(a, b, s, grad_box_b=None):
    return AxpyFn.apply(a, b, s, grad_box_b)


class AxpyBcastFn(torch.autograd.Function):
    """s * a + b with b [n...] broadcast over the leading dimension of a [R, n...]  (model_stage1.py:74: the sentence features of
    the step against every image's attended ones; the expanded copy of b is never made)"""

    @staticmethod
    def forward(ctx, a, b, s, grad_box_b=None):
        _chk(a, b)
        a, b = a.contiguous(), b.contiguous()
        assert a.shape[1:] == b.shape and b.numel() % 4 == 0, (a.shape, b.shape)
        ctx.s, ctx.box = s, grad_box_b
        out = torch.empty_like(a)
        h2_mark_next(out)
        call("tris_elementwise_bcast_f32", EW["TRIS_EW_AXPY"], P(a), P(b), P(out), a.numel(), b.numel(), float(s), _stream())
        return out

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        da = ew("TRIS_EW_SCALE", dy, None, ctx.s) if ctx.needs_input_grad[0] else None
        db = None
        if ctx.needs_input_grad[1]:
            R = dy.shape[0]
            db = colsum(dy, R, dy.numel() // R, torch.empty(dy.shape[1:], device=dy.device, dtype=torch.float32))
            if ctx.box is not None and ctx.box.deposit(db):
                db = None
        return da, db, None, None


def axpy_bcast(a, b, s, grad_box_b=None):
    return AxpyBcastFn.apply(a, b, s, grad_box_b)


class ScaleExpFn(torch.autograd.Function):
    """(x, ls) -> (x * exp(ls), exp(ls)) for a 0-dim device scalar ls  (model_stage1.py:77-78)"""

    @staticmethod
    def forward(ctx, x, ls):
        _chk(x, ls)
        x = x.contiguous()
        out = torch.empty_like(x)
        e = torch.empty((), device=x.device, dtype=torch.float32)
        call("tris_scale_exp_fwd_f32", P(x), P(ls), P(out), P(e), x.numel(), _stream())
        ctx.save_for_backward(out, ls, e)
        ctx.set_materialize_grads(False)
        return out, e

    @staticmethod
    def backward(ctx, dout, de):
        out, ls, e = ctx.saved_tensors
        dx = dls = None
        if dout is not None:
            dout = dout.contiguous()
            dx = torch.empty_like(dout) if ctx.needs_input_grad[0] else None
            dls = torch.empty((), device=out.device, dtype=torch.float32)
            ws = workspace(query("tris_scale_exp_workspace_bytes"))
            call("tris_scale_exp_bwd_f32", P(dout), P(out), P(ls), P(dx), P(dls), P(ws), out.numel(), _stream())
        if de is not None:       # (nobody differentiates through the returned scale on this path; kept correct all the same)
            dls = de * e if dls is None else dls + de * e
        return dx, (dls if ctx.needs_input_grad[1] else None)


def scale_exp(x, ls):
    return ScaleExpFn.apply(x, ls)


def concat_i64(a, b):
    """[a; b] of two int64 row lists (no gradient)"""
    a, b = a.contiguous(), b.contiguous()
    assert a.dtype == b.dtype == torch.int64 and a.shape[1:] == b.shape[1:] and a.is_cuda and b.is_cuda
    out = torch.empty((a.shape[0] + b.shape[0],) + tuple(a.shape[1:]), device=a.device, dtype=torch.int64)
    call("tris_concat_i64", a.data_ptr(), a.numel(), b.data_ptr(), b.numel(), out.data_ptr(), _stream())
    return out


class MulFn(torch.autograd.Function):
    """a * b (same shape)"""

    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        ctx.save_for_backward(a, b)
        return ew("TRIS_EW_MUL", a, b)

    @staticmethod
    def backward(ctx, dy):
        a, b = ctx.saved_tensors
        dy = dy.contiguous()
        return (ew("TRIS_EW_MUL", dy, b) if ctx.needs_input_grad[0] else None,
                ew("TRIS_EW_MUL", dy, a) if ctx.needs_input_grad[1] else None)


def mul(a, b):
    return MulFn.apply(a, b)


class ScoreHeadsFn(torch.autograd.Function):
    """score [B, P, N] -> (cls_out [B,N], cls_fg [B], relu_map [B,1,S,S], sig_map [B,1,S,S]) for training,
    or only relu_map in eval.  model_stage1.py:80-119."""

    @staticmethod
    def forward(ctx, score, h, w, S, train, focal_p, focal_c):
        _chk(score)
        score = score.contiguous()
        B, Pp, N = score.shape
        dev = score.device
        relu_map = torch.empty(B, 1, S, S, device=dev, dtype=torch.float32)
        ctx.cfg = (B, Pp, N, h, w, S, train, focal_p, focal_c)
        ctx.save_for_backward(score)
        if not train:
            call("tris_maps_fwd_f32", P(score), P(relu_map), None, B, h, w, N, S, _stream())
            return relu_map
        cls_out = torch.empty(B, N, device=dev, dtype=torch.float32)
        cls_fg = torch.zeros(B, device=dev, dtype=torch.float32)
        sig_map = torch.empty(B, 1, S, S, device=dev, dtype=torch.float32)
        call("tris_cls_head_fwd_f32", P(score), P(cls_out), P(cls_fg), B, Pp, N, focal_p, focal_c, _stream())
        call("tris_maps_fwd_f32", P(score), P(relu_map), P(sig_map), B, h, w, N, S, _stream())
        ctx.mark_non_differentiable(cls_fg)
        return cls_out, cls_fg, relu_map, sig_map

    @staticmethod
    def backward(ctx, *grads):
        (score,) = ctx.saved_tensors
        B, Pp, N, h, w, S, train, focal_p, focal_c = ctx.cfg
        if train:
            g_cls, _, g_relu, g_sig = grads
        else:
            g_cls, g_relu, g_sig = None, grads[0], None
        dscore = torch.empty_like(score)
        if g_cls is not None:
            call("tris_cls_head_bwd_f32", P(score), P(g_cls.contiguous()), P(dscore), B, Pp, N, focal_p, focal_c,
                 _stream())
        else:
            dscore.zero_()
        if g_relu is not None or g_sig is not None:
            call("tris_maps_bwd_f32", P(score), P(g_relu.contiguous()) if g_relu is not None else None,
                 P(g_sig.contiguous()) if g_sig is not None else None, P(dscore), B, h, w, N, S, _stream())
        return dscore, None, None, None, None, None, None


def score_heads(score, h, w, S, train, focal_p=3.0, focal_c=0.01):
    if score.dim() != 3 or h * w != score.shape[1]:
        raise ValueError(f"score_heads: score {tuple(score.shape)} is not [B, h * w, N] with h * w = {h} * {w}")
    return ScoreHeadsFn.apply(score, h, w, S, train, focal_p, focal_c)


class ResizeFn(torch.autograd.Function):
    """F.interpolate(x [B,C,H,W], size, mode='bilinear', align_corners=align)"""

    @staticmethod
    def forward(ctx, x, Ho, Wo, align):
        _chk(x)
        x = x.contiguous()
        B, C, Hi, Wi = x.shape
        y = torch.empty(B, C, Ho, Wo, device=x.device, dtype=torch.float32)
        call("tris_resize_bilinear_fwd_f32", P(x), P(y), B * C, Hi, Wi, Ho, Wo, int(align), _stream())
        ctx.cfg = (B, C, Hi, Wi, Ho, Wo, int(align))
        return y

    @staticmethod
    def backward(ctx, dy):
        B, C, Hi, Wi, Ho, Wo, align = ctx.cfg
        dx = torch.empty(B, C, Hi, Wi, device=dy.device, dtype=torch.float32)
        call("tris_resize_bilinear_bwd_f32", P(dy.contiguous()), P(dx), B * C, Hi, Wi, Ho, Wo, align, _stream())
        return dx, None, None, None


def resize_bilinear(x, size, align_corners):
    return ResizeFn.apply(x, int(size[0]), int(size[1]), bool(align_corners))


class FgPatchFn(torch.autograd.Function):
    """(cam [B,1,R,R], img [B,C,R,R]) -> fg = cam*img as ViT patch-GEMM rows [B, (R/ps)^2, C*ps*ps]"""

    @staticmethod
    def forward(ctx, cam, img, ps):
        _chk(cam, img)
        cam, img = cam.contiguous(), img.contiguous()
        B, C, R, _ = img.shape
        G = R // ps
        out = torch.empty(B, G * G, C * ps * ps, device=img.device, dtype=torch.float32)
        call("tris_fg_patch_fwd_f32", P(cam), P(img), P(out), B, C, R, ps, _stream())
        ctx.cfg = (B, C, R, ps)
        ctx.save_for_backward(img)
        return out

    @staticmethod
    def backward(ctx, dp):
        (img,) = ctx.saved_tensors
        B, C, R, ps = ctx.cfg
        dcam = torch.empty(B, 1, R, R, device=dp.device, dtype=torch.float32)
        call("tris_fg_patch_bwd_f32", P(dp.contiguous()), P(img), P(dcam), B, C, R, ps, _stream())
        return dcam, None, None


def fg_patches(cam, img, ps):
    if img.dim() != 4 or img.shape[2] != img.shape[3]:
        raise ValueError(f"fg_patches: img {tuple(img.shape)} is not a batch of square images [B,C,R,R]")
    if tuple(cam.shape) != (img.shape[0], 1, img.shape[2], img.shape[3]):
        raise ValueError(f"fg_patches: cam {tuple(cam.shape)} is not {(img.shape[0], 1, img.shape[2], img.shape[3])}")
    if ps < 1 or img.shape[2] % ps:
        raise ValueError(f"fg_patches: patch size {ps} does not divide the image size {img.shape[2]}")
    return FgPatchFn.apply(cam, img, ps)


class VitAssembleFn(torch.autograd.Function):
    """[cls + pos[0]; emb + pos[1:]] -> [B, T, W]; gradients for cls / pos only where they are trained (ViT trunk)"""

    @staticmethod
    def forward(ctx, emb, cls, pos):
        _chk(emb, cls, pos)
        emb = emb.contiguous()
        B, T1, W = emb.shape
        x = torch.empty(B, T1 + 1, W, device=emb.device, dtype=torch.float32)
        call("tris_vit_assemble_fwd_f32", P(emb), P(cls), P(pos), P(x), B, T1 + 1, W, _stream())
        ctx.cfg = (B, T1 + 1, W)
        return x

    @staticmethod
    def backward(ctx, dx):
        B, T, W = ctx.cfg
        dx = dx.contiguous()
        demb = torch.empty(B, T - 1, W, device=dx.device, dtype=torch.float32)
        call("tris_vit_assemble_bwd_f32", P(dx), P(demb), B, T, W, _stream())
        dcls = dpos = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dpos = colsum(dx, B, T * W, torch.empty(T, W, device=dx.device, dtype=torch.float32))   # sum over the batch
            dcls = dpos[0].clone() if ctx.needs_input_grad[1] else None
            dpos = dpos if ctx.needs_input_grad[2] else None
        return demb, dcls, dpos


def vit_assemble(emb, cls, pos):
    return VitAssembleFn.apply(emb, cls, pos)


class Stage1LossFn(torch.autograd.Function):
    """(cls [B,N], f_img [B,E], f_txt [B,E], f_neg [B,K,E]|None) -> losses[4] = (total, l1, l4, l5).
    train_stage1.py:263-284, 340-364.  Text features come from the frozen aux CLIP: no gradient to them."""

    @staticmethod
    def forward(ctx, cls, fi, ft, fneg, w1, w4, w5):
        _chk(cls, fi, ft, fneg)
        cls, fi, ft = cls.contiguous(), fi.contiguous(), ft.contiguous()
        B, N = cls.shape
        E = fi.shape[1]
        K = 0
        if fneg is not None:
            fneg = fneg.contiguous()
            K = fneg.shape[1]
        dev = cls.device
        scratch = torch.empty(B * 4, device=dev, dtype=torch.float32)
        losses = torch.empty(4, device=dev, dtype=torch.float32)
        call("tris_stage1_loss_fwd_f32", P(cls), P(fi), P(ft), P(fneg), B, N, E, K, w1, w4, w5, P(scratch),
             P(scratch, 3 * B), P(losses), _stream())
        ctx.cfg = (B, N, E, K, w1, w4, w5)
        ctx.save_for_backward(cls, fi, ft, fneg)
        return losses

    @staticmethod
    def backward(ctx, g):
        cls, fi, ft, fneg = ctx.saved_tensors
        B, N, E, K, w1, w4, w5 = ctx.cfg
        g = g.contiguous()
        # (the kernels fold the loss weights: dL/dl1 = g[0]*w1 + g[1]; dL/dl5 = g[0]*w5 + g[3]; dL/dl4 = g[0]*w4 + g[2])
        dcls = torch.empty_like(cls)
        dfi = torch.empty_like(fi)
        call("tris_stage1_loss_bwd_f32", P(cls), P(fi), P(ft), P(fneg), P(g), float(w1), float(w4), float(w5), B, N, E, K, P(dcls),
             P(dfi), _stream())
        return dcls, dfi, None, None, None, None, None


def stage1_loss(cls, fi, ft, fneg, w1=1.0, w4=5.0, w5=2.0):
    return Stage1LossFn.apply(cls, fi, ft, fneg, w1, w4, w5)


def eval_post(relu_map, target_u8):
    """validate.py:180-190 for one (image, sentence): returns (iu int64[3] on device = I, U, argmax; cam [oH,oW])."""
    _chk(relu_map, target_u8)
    S = relu_map.shape[-1]
    oH, oW = target_u8.shape[-2:]
    cam = torch.empty(oH, oW, device=relu_map.device, dtype=torch.float32)
    iu = torch.empty(3, device=relu_map.device, dtype=torch.int64)
    ws = workspace(4 * (2 * 1024 + 8))
    call("tris_eval_post_f32", P(relu_map.contiguous()), S, P(target_u8.contiguous()), oH, oW, P(cam), P(iu), P(ws),
         _stream())
    return iu, cam


# ------------------------------------------------------------------------------------------------------ input pipeline
#  uint8 dataset resident in HBM; see tris_amd/dataset/hbm.py
_PIL_TABLES = {}


def _pil_tables(kind, n_in, n_out, device):
    key = (kind, n_in, n_out, str(device))
    t = _PIL_TABLES.get(key)
    if t is None:
        from .dataset import pil_tables
        if kind == "bilinear":
            bounds, kk, ksize = pil_tables.resample_tables(n_in, n_out)
            t = (torch.from_numpy(bounds.copy()).to(device), torch.from_numpy(kk.copy()).to(device), ksize)
        else:
            t = (torch.from_numpy(pil_tables.nearest_index(n_in, n_out).copy()).to(device),)
        _PIL_TABLES[key] = t
    return t


def _chk_u8(*ts):
    for t in ts:
        if not t.is_cuda:
            raise NoGpuError("tris_amd ops run on MI355X only (got a CPU tensor); there is no CPU fallback")
        if t.dtype != torch.uint8:
            raise TypeError(f"expected uint8, got {t.dtype}")


def resample_u8(img, out_h, out_w, out=None):
    """Pillow `resize((out_w, out_h), BILINEAR)` of a uint8 [H,W,C] device image, bit-exact (dataset/transform.py:29)."""
    _chk_u8(img)
    img = img.contiguous()
    H, W, C = img.shape
    if out is None:
        out = torch.empty(out_h, out_w, C, dtype=torch.uint8, device=img.device)
    if (H, W) == (out_h, out_w):
        out.copy_(img)
        return out
    th = _pil_tables("bilinear", W, out_w, img.device) if W != out_w else (None, None, 0)
    tv = _pil_tables("bilinear", H, out_h, img.device) if H != out_h else (None, None, 0)
    tmp = torch.empty(H * out_w * C, dtype=torch.uint8, device=img.device) if (th[0] is not None and tv[0] is not None) \
        else None
    call("tris_resample_u8", P(img), H, W, C, P(th[0]), P(th[1]), th[2], P(tv[0]), P(tv[1]), tv[2], out_h, out_w,
         P(tmp), P(out), _stream())
    return out


def resize_nearest_u8(img, out_h, out_w, out=None):
    """Pillow `resize((out_w, out_h), NEAREST)` of a uint8 [H,W] / [H,W,C] device image (dataset/transform.py:32)."""
    _chk_u8(img)
    img = img.contiguous()
    H, W = img.shape[:2]
    C = img.shape[2] if img.dim() == 3 else 1
    if out is None:
        out = torch.empty((out_h, out_w) + tuple(img.shape[2:]), dtype=torch.uint8, device=img.device)
    if (H, W) == (out_h, out_w):
        out.copy_(img)
        return out
    yi, = _pil_tables("nearest", H, out_h, img.device)
    xi, = _pil_tables("nearest", W, out_w, img.device)
    call("tris_gather2d_u8", P(img), H, W, C, P(yi), P(xi), out_h, out_w, P(out), _stream())
    return out


def mask_sum_nearest_u8(masks, out_h, out_w, out=None):
    """Stage-2 pseudo target of one ref (dataset/ReferDataset.py:178-186): masks uint8 [K,h,w] of 0/1 (a bool stack viewed as
    uint8) -> uint8 [out_h,out_w] = Pillow NEAREST resize of `masks.sum(0)`; K = 0 gives zeros.  K <= 255: the sum is a byte."""
    if masks.dim() != 3:
        raise ValueError(f"expected a [K,h,w] stack, got shape {tuple(masks.shape)}")
    K, H, W = masks.shape
    if K > 255:
        raise ValueError(f"{K} masks in one stack: their sum does not fit the uint8 target (at most 255)")
    _chk_u8(masks)
    if H <= 0 or W <= 0 or out_h <= 0 or out_w <= 0:
        raise ValueError(f"empty image: [{H},{W}] -> [{out_h},{out_w}]")
    masks = masks.contiguous()
    if out is None:
        out = torch.empty(out_h, out_w, dtype=torch.uint8, device=masks.device)
    else:
        _chk_u8(out)
        assert out.shape == (out_h, out_w) and out.is_contiguous()
    yi, = _pil_tables("nearest", H, out_h, masks.device)
    xi, = _pil_tables("nearest", W, out_w, masks.device)
    call("tris_mask_sum_nearest_u8", P(masks) if K else None, K, H, W, P(yi), P(xi), out_h, out_w, P(out), _stream())
    return out


def gather_normalize(cache, index, lut, planar=False):
    """cache uint8 [N,H,W,3], index int64 [B], lut float32 [3,256] -> float32 batch of ToTensor+Normalize'd images:
    planar=False: memory [B,H,W,3], returned as the [B,3,H,W] channels-last view;  planar=True: contiguous [B,3,H,W]."""
    _chk_u8(cache)
    _chk(index, lut)
    N, H, W, C = cache.shape
    assert C == 3 and cache.is_contiguous() and index.dtype == torch.int64
    B = index.numel()
    if planar:
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=cache.device)
    else:
        out = torch.empty(B, H, W, 3, dtype=torch.float32, device=cache.device)
    call("tris_u8_gather_normalize_f32", P(cache), P(index), B, H * W, P(lut.contiguous()), P(out), int(planar), _stream())
    return out if planar else out.permute(0, 3, 1, 2)


def irn_augment_batch(img_arena, lab_arena, packed, desc_bytes, lut, B, crop):
    """IRNet's training augmentation of one batch in one launch (dataset/irn_data.py; IRNet/voc12/dataloader.py:222-285): packed =
    the batch's descriptors (int64 [B, TRIS_IRN_AUG_DESC], desc_bytes of them) followed by its int32 tables, already checked by
    irn_data.validate_batch -> (img float32 [B,3,crop,crop] as the channels-last view of [B,crop,crop,3], label uint8
    [B,crop,crop], label_reduced uint8 [B,crop/4,crop/4])."""
    _chk_u8(img_arena, lab_arena, packed)
    _chk(lut)
    if crop % 4 or desc_bytes != B * CONSTS["TRIS_IRN_AUG_DESC"] * 8 or packed.numel() <= desc_bytes:
        raise ValueError(f"irn_augment_batch: crop {crop}, {desc_bytes} descriptor bytes for a batch of {B}")
    assert img_arena.is_contiguous() and lab_arena.is_contiguous() and packed.is_contiguous() and lut.shape == (3, 256)
    dev = img_arena.device
    img = torch.empty(B, crop, crop, 3, dtype=torch.float32, device=dev)
    label = torch.empty(B, crop, crop, dtype=torch.uint8, device=dev)
    reduced = torch.empty(B, crop // 4, crop // 4, dtype=torch.uint8, device=dev)
    call("tris_irn_augment_batch_u8", P(img_arena), P(lab_arena), P(packed), packed.data_ptr() + desc_bytes, P(lut.contiguous()),
         P(img), P(label), P(reduced), B, crop, _stream())
    return img.permute(0, 3, 1, 2), label, reduced


def gather_rows(table, index):
    """table [N, ...] (any dtype, row size a multiple of 4 bytes), index int64 [R] -> [R, ...]"""
    if not table.is_cuda:
        raise NoGpuError("tris_amd ops run on MI355X only (got a CPU tensor); there is no CPU fallback")
    assert table.is_contiguous() and index.dtype == torch.int64 and index.is_cuda
    row_bytes = table[0].numel() * table.element_size()
    out = torch.empty((index.numel(),) + tuple(table.shape[1:]), dtype=table.dtype, device=table.device)
    if index.numel():
        call("tris_gather_rows", P(table), P(index), index.numel(), row_bytes, P(out), _stream())
    return out


# ------------------------------------------------------------------------------------------------------ Stage-2 decoder
# (csrc/seg.hip; reference model/model_stage2.py, train_stage2.py)  Activations channels-last [B,h,w,C] as everywhere else.
class BnPreluFn(torch.autograd.Function):
    """BatchNorm2d + nn.PReLU() (one slope) on channels-last x [..., C]: ConvBNRelu's tail (model_stage2.py:22-27).  Train mode: batch
    statistics from the producing conv's epilogue (x._bn_part) or a statistics pass, running statistics updated like torch's."""

    @staticmethod
    def forward(ctx, x, gamma, beta, rmean, rvar, slope, training, momentum, eps):
        _chk(x, gamma, beta, rmean, rvar, slope)
        part = getattr(x, "_bn_part", None) if training else None
        x = unplanes(x).contiguous()
        C = x.shape[-1]
        M = x.numel() // C
        if training:
            stats = torch.empty(3 * C, device=x.device, dtype=torch.float32)
            _bn_local_stats(x, part, eps, momentum, stats, rmean, rvar)
            mean, invstd = stats[:C], stats[C:2 * C]
        else:
            mean, invstd = rmean, torch.rsqrt(rvar + eps)
        y = torch.empty_like(x)
        call("tris_bn_prelu_fwd_f32", P(x), P(mean), P(invstd), P(gamma), P(beta), P(slope), P(y), M, C, _stream())
        ctx.cfg = (M, C, bool(training))
        ctx.params = (gamma, beta, slope)
        ctx.save_for_backward(x, gamma, beta, mean, invstd, slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, mean, invstd, slope = ctx.saved_tensors
        M, C, training = ctx.cfg
        dy = unplanes(pl_grad_in(dy.contiguous()))
        sums = torch.empty(2 * C + 1, device=x.device, dtype=torch.float32)
        ws = workspace(query("tris_seg_workspace_bytes", M, C))
        call("tris_bn_prelu_bwd_reduce_f32", P(dy), P(x), P(mean), P(invstd), P(gamma), P(beta), P(slope), M, C, P(sums),
             P(sums, C), P(sums, 2 * C), P(ws), _stream())
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            # eval mode: the statistics are constants, so the mean terms drop out (inv_count 0)
            call("tris_bn_prelu_bwd_apply_f32", P(dy), P(x), P(mean), P(invstd), P(gamma), P(beta), P(slope), P(sums), P(sums, C),
                 1.0 / float(M) if training else 0.0, P(dx), M, C, _stream())
        g, b, a = ctx.params
        dg = _emit(g, lambda o: o.copy_(sums[C:2 * C]), ctx.needs_input_grad[1])
        db = _emit(b, lambda o: o.copy_(sums[:C]), ctx.needs_input_grad[2])
        da = _emit(a, lambda o: o.copy_(sums[2 * C:].view_as(o)), ctx.needs_input_grad[5])
        return dx, dg, db, None, None, da, None, None, None


def bn_prelu(x, gamma, beta, rmean, rvar, slope, training=True, momentum=0.1, eps=1e-5):
    return BnPreluFn.apply(x, gamma, beta, rmean, rvar, slope, bool(training), float(momentum), float(eps))


class UpsampleNhwcFn(torch.autograd.Function):
    """Upsample(x, size) (bilinear, align_corners=False; model_stage2.py:29-35) of channels-last x [B,Hi,Wi,C], with the top-down
    path's skip add (:127-129): -> up [B,Ho,Wo,C] and, when skip is given, up + skip as a second output."""

    @staticmethod
    def forward(ctx, x, skip, Ho, Wo):
        _chk(x, skip)
        x = unplanes(x).contiguous()
        B, Hi, Wi, C = x.shape
        if Ho < Hi or Wo < Wi:
            raise ValueError(f"upsample_nhwc upsamples ({Hi}x{Wi} -> {Ho}x{Wo} would shrink): its backward is the gather form for Ho >= Hi, Wo >= Wi")
        up = torch.empty(B, Ho, Wo, C, device=x.device, dtype=torch.float32)
        s = None
        if skip is not None:
            skip = unplanes(skip).contiguous()
            if tuple(skip.shape) != (B, Ho, Wo, C):
                raise ValueError(f"skip {tuple(skip.shape)} does not match the upsampled map {(B, Ho, Wo, C)}")
            s = torch.empty_like(up)
        call("tris_upsample_nhwc_fwd_f32", P(x), P(skip), P(up), P(s), B, Hi, Wi, Ho, Wo, C, _stream())
        ctx.cfg = (B, Hi, Wi, Ho, Wo, C, skip is not None)
        return (up, s) if s is not None else up

    @staticmethod
    def backward(ctx, d_up, d_sum=None):
        B, Hi, Wi, Ho, Wo, C, has_skip = ctx.cfg
        d_up = None if d_up is None else unplanes(pl_grad_in(d_up.contiguous()))
        d_sum = None if d_sum is None else unplanes(pl_grad_in(d_sum.contiguous()))
        dx = None
        if ctx.needs_input_grad[0] and (d_up is not None or d_sum is not None):
            dx = torch.empty(B, Hi, Wi, C, device=(d_up if d_up is not None else d_sum).device, dtype=torch.float32)
            call("tris_upsample_nhwc_bwd_f32", P(d_up), P(d_sum), P(dx), B, Hi, Wi, Ho, Wo, C, _stream())
        return dx, (d_sum if has_skip else None), None, None


def upsample_nhwc(x, size, skip=None):
    """-> up, or (up, up + skip) with a skip"""
    return UpsampleNhwcFn.apply(x, skip, int(size[0]), int(size[1]))


class Head1Fn(torch.autograd.Function):
    """nn.Conv2d(C, 1, 1, bias=False) on channels-last x [B,h,w,C] (final_seg1..4[1], model_stage2.py:75-86) -> [B,1,h,w]
    (one channel: the NCHW and channels-last layouts coincide)"""

    @staticmethod
    def forward(ctx, x, w):
        _chk(x, w)
        x = unplanes(x).contiguous()
        B, h, wd, C = x.shape
        if w.numel() != C:
            raise ValueError(f"head weight {tuple(w.shape)} does not take {C} channels")
        wf = w.detach().reshape(C).contiguous()
        y = torch.empty(B, 1, h, wd, device=x.device, dtype=torch.float32)
        call("tris_head1_fwd_f32", P(x), P(wf), P(y), B * h * wd, C, _stream())
        ctx.params = (w,)
        ctx.save_for_backward(x, wf)
        return y

    @staticmethod
    def backward(ctx, g):
        x, wf = ctx.saved_tensors
        B, h, wd, C = x.shape
        M = B * h * wd
        g = g.contiguous()
        dx = torch.empty_like(x)
        dw = torch.empty(C, device=x.device, dtype=torch.float32)
        ws = workspace(query("tris_seg_workspace_bytes", M, C))
        call("tris_head1_bwd_f32", P(g), P(x), P(wf), P(dx), P(dw), M, C, P(ws), _stream())
        dW = _emit(ctx.params[0], lambda o: o.copy_(dw.view_as(o)), ctx.needs_input_grad[1])
        return (dx if ctx.needs_input_grad[0] else None), dW


def head1x1(x, w):
    return Head1Fn.apply(x, w)


class Bce4Fn(torch.autograd.Function):
    """criterion (model_stage2.py:139-141) of up to four heads against one target, summed as train_stage2.py:314-319 does:
    -> losses[5] = (l1 + l2 + l3 + l4, l1, l2, l3, l4); x2..x4 may be None (loss 0).  The target is read as int64 (the pseudo masks)
    or fp32; other dtypes are converted to fp32 first, as the reference's target.float()."""

    @staticmethod
    def forward(ctx, target, x1, x2, x3, x4):
        xs = [None if x is None else x.contiguous() for x in (x1, x2, x3, x4)]
        _chk(target, *xs)
        if target.dtype not in (torch.int64, torch.float32):
            target = target.float()
        target = target.contiguous()
        n = target.numel()
        for x in xs:
            if x is not None and x.numel() != n:
                raise ValueError(f"head output {tuple(x.shape)} does not match the target {tuple(target.shape)}")
        kind = int(target.dtype == torch.float32)
        losses = torch.empty(5, device=target.device, dtype=torch.float32)
        ws = workspace(query("tris_bce4_workspace_bytes", n))
        call("tris_bce4_fwd_f32", *[P(x) for x in xs], P(target), kind, n, P(losses), P(ws), _stream())
        ctx.kind = kind
        ctx.save_for_backward(target, *xs)
        return losses

    @staticmethod
    def backward(ctx, g):
        target, *xs = ctx.saved_tensors
        g = g.contiguous()
        ds = [None if x is None or not ctx.needs_input_grad[1 + k] else torch.empty_like(x) for k, x in enumerate(xs)]
        call("tris_bce4_bwd_f32", *[P(x) for x in xs], P(target), ctx.kind, P(g), *[P(d) for d in ds], target.numel(), _stream())
        return (None, *ds)


def bce4(outs, target):
    return Bce4Fn.apply(target, *outs)


def bce(out, target):
    """one head: F.binary_cross_entropy_with_logits(out, target.float(), reduction='mean') as a 0-d tensor"""
    return Bce4Fn.apply(target, out, None, None, None)[1]


class SegLoss5Fn(torch.autograd.Function):
    """The Stage-2 step's loss with EMA consistency (train_stage2.py:302-319): the four BCE terms of Bce4Fn plus l5 = the four
    sigmoid_mse_loss terms (:258-269) against the teacher's maps, in one pass -> losses[6] = (l1 + l2 + l3 + l4 + l5, l1, l2, l3,
    l4, l5).  Heads 2..4 may be None together with their teacher maps.  The teacher maps get no gradient."""

    @staticmethod
    def forward(ctx, target, x1, x2, x3, x4, e1, e2, e3, e4):
        xs = [None if x is None else x.contiguous() for x in (x1, x2, x3, x4)]
        es = [None if e is None else e.detach().contiguous() for e in (e1, e2, e3, e4)]
        _chk(target, *xs, *es)
        if target.dtype not in (torch.int64, torch.float32):
            target = target.float()
        target = target.contiguous()
        n = target.numel()
        for k, (x, e) in enumerate(zip(xs, es)):
            if (x is None) != (e is None):
                raise ValueError(f"head {k + 1}: the student map and the teacher map must both be given or both be absent")
            for t in (x, e):
                if t is not None and (t.numel() != n or t.dtype != torch.float32):
                    raise ValueError(f"head output {tuple(t.shape)} {t.dtype} does not match the target {tuple(target.shape)}")
        kind = int(target.dtype == torch.float32)
        losses = torch.empty(6, device=target.device, dtype=torch.float32)
        ws = workspace(query("tris_seg_loss5_workspace_bytes", n))
        call("tris_seg_loss5_fwd_f32", *[P(x) for x in xs], *[P(e) for e in es], P(target), kind, n, P(losses), P(ws), _stream())
        ctx.kind = kind
        ctx.save_for_backward(target, *xs, *es)
        return losses

    @staticmethod
    def backward(ctx, g):
        target, *rest = ctx.saved_tensors
        xs, es = rest[:4], rest[4:]
        g = g.contiguous()
        ds = [None if x is None or not ctx.needs_input_grad[1 + k] else torch.empty_like(x) for k, x in enumerate(xs)]
        call("tris_seg_loss5_bwd_f32", *[P(x) for x in xs], *[P(e) for e in es], P(target), ctx.kind, P(g), *[P(d) for d in ds],
             target.numel(), _stream())
        return (None, *ds, None, None, None, None)


def seg_loss5(outs, ema_outs, target):
    """outs / ema_outs: the student's and the teacher's four maps (trailing heads may be None in both) -> losses[6]"""
    outs, ema_outs = list(outs), list(ema_outs)
    if len(outs) != len(ema_outs) or not 1 <= len(outs) <= 4:
        raise ValueError(f"{len(outs)} student maps against {len(ema_outs)} teacher maps")
    pad = [None] * (4 - len(outs))
    return SegLoss5Fn.apply(target, *outs, *pad, *ema_outs, *pad)


def _lerp_dense(dst, src):
    """dst and src cover the same elements in the same memory order (a dense tensor and its copy / its arena view)"""
    if dst.dtype != torch.float32 or src.dtype != torch.float32:
        raise TypeError(f"lerp needs fp32 tensors (got {dst.dtype}, {src.dtype})")
    live = [i for i, n in enumerate(dst.shape) if n > 1]        # (the stride of a one-element dimension addresses nothing)
    if dst.shape != src.shape or [dst.stride(i) for i in live] != [src.stride(i) for i in live]:
        raise ValueError(f"lerp: {tuple(dst.shape)} / {dst.stride()} against {tuple(src.shape)} / {src.stride()}")
    if not (dst.is_contiguous() or (dst.dim() == 4 and dst.is_contiguous(memory_format=torch.channels_last))):
        raise ValueError(f"lerp needs dense tensors (shape {tuple(dst.shape)}, strides {dst.stride()})")
    if dst.numel() and dst.data_ptr() == src.data_ptr():
        raise ValueError("lerp: dst and src are the same memory")


class LerpTable:
    """device records {dst, src, n} of many tensor pairs: ema_update walks them in ONE launch, a workgroup per record.  A pair
    longer than CHUNK elements becomes several records cut at multiples of CHUNK (whole 16-byte words: dst and src keep their
    relative alignment), so that no workgroup walks megabytes alone.  Holds the tensors (the records are raw addresses)."""
    CHUNK = 1 << 16

    def __init__(self, pairs):
        pairs = [(d, s) for d, s in pairs if d.numel() > 0]
        for d, s in pairs:
            _chk(d, s)
            _lerp_dense(d, s)
        self.pairs = pairs
        rec = [[d.data_ptr() + 4 * o, s.data_ptr() + 4 * o, min(self.CHUNK, d.numel() - o)]
               for d, s in pairs for o in range(0, d.numel(), self.CHUNK)]
        self.records = torch.tensor(rec, dtype=torch.int64).reshape(len(rec), 3).to(pairs[0][0].device) if rec else None

    def __len__(self):
        return 0 if self.records is None else self.records.shape[0]


def ema_update(what, w):
    """dst <- lerp(dst, src, w) with torch's fp32 definition (w == 1: a copy, w == 0: nothing changes), the teacher update of the
    reference's mean teacher (train_stage2.py:328-332).  what: a LerpTable -- one launch over all its records -- or a list of
    (dst, src) pairs of flat buffers (the teacher's and the optimiser's parameter arenas): one launch each.  In-place without
    telling torch: the caller bumps version counters where it matters (tris_amd.ema)."""
    w = float(w)
    if isinstance(what, LerpTable):
        if len(what):
            call("tris_lerp_table_f32", what.records.data_ptr(), len(what), w, _stream())
        return
    for dst, src in what:
        _chk(dst, src)
        _lerp_dense(dst, src)
        call("tris_lerp_f32", P(dst), P(src), dst.numel(), w, _stream())


def eval_post_signed(seg_map, target_u8):
    """validate.py:179-191 for one (image, sentence) of a SIGNED map (Stage-2 logits): normalised by max + 1e-5 whatever its sign.
    -> (iu int64[3] on device = I, U, first arg-max of the normalised map; cam [oH,oW])"""
    _chk(seg_map, target_u8)
    S = seg_map.shape[-1]
    if seg_map.shape[-2] != S:
        raise ValueError(f"eval_post_signed takes a square map (validate feeds size x size inputs), got {tuple(seg_map.shape)}")
    oH, oW = target_u8.shape[-2:]
    cam = torch.empty(oH, oW, device=seg_map.device, dtype=torch.float32)
    iu = torch.empty(3, device=seg_map.device, dtype=torch.int64)
    ws = workspace(4 * (2049 + 4 * 1024 + 8))
    call("tris_eval_post_signed_f32", P(seg_map.contiguous()), S, P(target_u8.contiguous()), oH, oW, P(cam), P(iu), P(ws),
         _stream())
    return iu, cam


EVAL_BOXES_RECORD = 16   # int32 words of tris_eval_boxes_f32's record (include/tris_hip.h)


def eval_boxes_gt(bbox, device="cuda"):
    """ground-truth boxes (anything array-like, [..., 4] as x1, y1, x2, y2) -> int32 [K, 4] on the device, the operand of eval_boxes"""
    b = torch.as_tensor(bbox).reshape(-1, 4)
    return b.to(device=device, dtype=torch.int32, non_blocking=True).contiguous()


def decode_boxes_record(words):
    """the record's 16 int32 words (a list of Python ints, or 8 int64 words) -> dict of its fields"""
    import numpy as np
    w = np.asarray(words)
    w = w.astype(np.int64).view(np.int32) if len(w) == EVAL_BOXES_RECORD // 2 else w.astype(np.int32)
    return {"hitm": int(w[0]), "n_prop": int(w[1]), "n_nms": int(w[2]), "n_kept": int(w[3]),
            "bbox_hit": tuple(int(v) for v in w[4:8]), "box_acc": int(w[8]), "box_miou": w[9:10].view(np.float32)[0],
            "cmax": float(w[10:12].view(np.float64)[0])}


def eval_boxes(cam, target_u8, gt_box, iu, return_boxes=False):
    """PointM and the box metrics of one (image, sentence) (validate.py:106-117, 191-208; utils/box_eval_utils.py:10-73) behind
    eval_post / eval_post_signed: cam [H,W] and iu int64[3] as they return them, gt_box int32[4] on the device (eval_boxes_gt).
    -> record int32[16] on the device (decode_boxes_record); with return_boxes (a host sync) -> (record, the reference's list
    [(x1, y1, x2, y2, conf)] -- the default list for an all-zero / all-one mask)."""
    _chk(cam, target_u8, iu)
    if cam.dtype != torch.float32 or target_u8.dtype != torch.uint8 or iu.dtype != torch.int64 or iu.numel() != 3:
        raise TypeError("eval_boxes takes (float32 cam, uint8 target, int32 gt_box[4], int64 iu[3])")
    if not torch.is_tensor(gt_box) or not gt_box.is_cuda or gt_box.dtype != torch.int32 or gt_box.numel() != 4:
        raise TypeError("eval_boxes: gt_box is an int32[4] device tensor (ops.eval_boxes_gt)")
    H, W = cam.shape[-2:]
    if tuple(target_u8.shape[-2:]) != (H, W) or cam.numel() != H * W:
        raise ValueError(f"eval_boxes: cam {tuple(cam.shape)} and target {tuple(target_u8.shape)} differ")
    nbytes = query("tris_eval_boxes_workspace_bytes", H, W)
    if nbytes < 0:
        raise ValueError(f"eval_boxes: {H}x{W} is beyond 2^24 pixels")
    rows = 5 * (H * W + 1)
    ws = workspace(nbytes + 256 + 4 * rows)
    base = (ws.data_ptr() + 255) & ~255
    record = torch.empty(EVAL_BOXES_RECORD, device=cam.device, dtype=torch.int32)
    # the kept list is only handed out on request: otherwise it lives behind the workspace
    boxes = torch.empty(H * W + 1, 5, device=cam.device, dtype=torch.int32) if return_boxes else None
    call("tris_eval_boxes_f32", P(cam.contiguous()), P(target_u8.contiguous()), H, W, P(gt_box.contiguous()), P(iu), P(record),
         boxes.data_ptr() if return_boxes else base + ((nbytes + 7) & ~7), base, _stream())
    if not return_boxes:
        return record
    rec = decode_boxes_record(record.tolist())
    if rec["n_prop"] == 0:
        return record, [[0, 0, 1, 1, 0], [0, 0, 1, 1, 0]]
    import numpy as np
    out = []
    for x, y, w, h, cnt in boxes[:rec["n_kept"]].tolist():
        conf = float(np.float64(255 * cnt) / np.float64(w * h) / 255)       # numpy's uint8 slice .mean() / 255
        out.append((float(x), float(y), float(x + w), float(y + h), conf))
    return record, out


# ------------------------------------------------------------------------------------------ ReferIt evaluation (csrc/referit.hip)
def rle_decode_sum_arena(ends, seg_off, ranges, H, W, out=None):
    """targets of the K sentences of one image from a device arena (dataset/rle_arena.py: RleArena.to): ends int32, seg_off int64,
    ranges int32 [K,2] -> uint8 [K,H,W] = cocomask.decode(...).sum(2).astype(uint8) of every sentence, one launch.  The arena's
    builder has checked the run lengths; nothing here reads them back."""
    for t, dt in ((ends, torch.int32), (seg_off, torch.int64), (ranges, torch.int32)):
        if not t.is_cuda:
            raise NoGpuError("tris_amd ops run on MI355X only (got a CPU tensor); there is no CPU fallback")
        if t.dtype != dt:
            raise TypeError(f"expected {dt}, got {t.dtype}")
    if ranges.dim() != 2 or ranges.shape[1] != 2:
        raise ValueError(f"ranges is [K,2], got {tuple(ranges.shape)}")
    if H < 1 or W < 1 or H * W > (1 << 24):
        raise ValueError(f"rle_decode_sum: {H}x{W} is empty or beyond 2^24 pixels")
    K = ranges.shape[0]
    if out is None:
        out = torch.empty(K, H, W, dtype=torch.uint8, device=ranges.device)
    else:
        _chk_u8(out)
        assert tuple(out.shape) == (K, H, W) and out.is_contiguous()
    if K:
        call("tris_rle_decode_sum_u8", P(ends.contiguous()), P(seg_off.contiguous()), P(ranges.contiguous()), K, H, W, P(out),
             _stream())
    return out


def rle_decode_sum(sentences, H, W, names=None, device="cuda"):
    """sentences: per sentence the list of its RLE dicts (counts as a list or a compressed string) -> uint8 [K,H,W] on the device.
    Refused before any launch, naming the sentence (names[k], or its index): a negative count, counts that sum past H*W, more than
    255 segments for one sentence, H*W > 2^24."""
    from .dataset.rle_arena import RleArena
    arena = RleArena()
    ranges = [arena.add_sentence(s, H, W, str(names[k]) if names is not None else f"sentence {k}") for k, s in enumerate(sentences)]
    if not torch.cuda.is_available():
        raise NoGpuError("tris_amd ops run on MI355X only; there is no CPU fallback")
    ends, seg_off = arena.to(device)
    rng = torch.tensor(ranges, dtype=torch.int32).reshape(-1, 2).to(device)
    return rle_decode_sum_arena(ends, seg_off, rng, H, W)


# ------------------------------------------------------------------------------------ REFER polygon targets (csrc/polymask.hip)
def poly_runs(verts, poly_off, hw, host=None):
    """cocomask.frPyObjects of P polygons on the device (dataset/poly_arena.py: PolyArena.build): verts int32 [V,2] upsampled
    vertices, poly_off int64 [P+1], hw int32 [P,2] -> (ends int32 [runs + 1], seg_off int64 [P+1]), the arena rle_decode_sum_arena
    reads.  Count, scan (torch.cumsum), emit: two launches for the whole split.  host = (index int64 [N], lens int64 [N], values
    int32 [sum lens]): segments without vertices whose run ends the host supplies; they take slices of those lengths.  The arena's
    builder has checked coordinates and sizes; nothing here reads them back but the total number of runs."""
    for t, dt in ((verts, torch.int32), (poly_off, torch.int64), (hw, torch.int32)):
        if not t.is_cuda:
            raise NoGpuError("tris_amd ops run on MI355X only (got a CPU tensor); there is no CPU fallback")
        if t.dtype != dt:
            raise TypeError(f"expected {dt}, got {t.dtype}")
    P_ = poly_off.numel() - 1
    if P_ < 0 or hw.numel() != 2 * P_ or verts.dim() != 2 or verts.shape[1] != 2:
        raise ValueError(f"poly_runs: verts {tuple(verts.shape)}, poly_off {tuple(poly_off.shape)}, hw {tuple(hw.shape)}")
    verts, poly_off, hw = verts.contiguous(), poly_off.contiguous(), hw.contiguous()
    dev = poly_off.device
    n_runs = torch.empty(P_, dtype=torch.int32, device=dev)
    if P_:
        call("tris_poly_count_runs", P(verts), P(poly_off), P(hw), P_, P(n_runs), _stream())
    if host is not None:
        index, lens, values = host
        n_runs[index] = lens.to(torch.int32)
    seg_off = torch.zeros(P_ + 1, dtype=torch.int64, device=dev)
    seg_off[1:] = torch.cumsum(n_runs, 0, dtype=torch.int64)
    total = int(seg_off[-1])
    ends = torch.zeros(total + 1, dtype=torch.int32, device=dev)      # (one spare word, as RleArena.to)
    if P_:
        call("tris_poly_emit_runs", P(verts), P(poly_off), P(hw), P(seg_off), P_, P(ends), _stream())
    if host is not None and values.numel():
        first = torch.cumsum(lens, 0) - lens
        pos = torch.arange(values.numel(), device=dev) + torch.repeat_interleave(seg_off[index] - first, lens)
        ends[pos] = values
    return ends, seg_off


def rle_target_nearest(arena, lo, hi, H, W, S, out=None):
    """training target of one ref (ReferDataset.load_mask + transform.py:32): arena = (ends, seg_off) on the device or an object
    with those attributes, segments lo .. hi-1 on an H x W canvas -> uint8 [S,S] = Pillow NEAREST resize of (decoded sum == 1);
    the full-size mask is never formed"""
    ends, seg_off = (arena.ends, arena.seg_off) if hasattr(arena, "ends") else arena
    for t, dt in ((ends, torch.int32), (seg_off, torch.int64)):
        if not t.is_cuda:
            raise NoGpuError("tris_amd ops run on MI355X only (got a CPU tensor); there is no CPU fallback")
        if t.dtype != dt:
            raise TypeError(f"expected {dt}, got {t.dtype}")
    if H < 1 or W < 1 or H * W > (1 << 24) or S < 1:
        raise ValueError(f"rle_target_nearest: {H}x{W} -> {S}x{S} is empty or beyond 2^24 pixels")
    if not 0 <= lo <= hi <= seg_off.numel() - 1 or hi - lo > 255:
        raise ValueError(f"rle_target_nearest: segments {lo}..{hi} of {seg_off.numel() - 1} (at most 255 per ref)")
    if out is None:
        out = torch.empty(S, S, dtype=torch.uint8, device=ends.device)
    else:
        _chk_u8(out)
        assert tuple(out.shape) == (S, S) and out.is_contiguous()
    yi, = _pil_tables("nearest", H, S, ends.device)
    xi, = _pil_tables("nearest", W, S, ends.device)
    call("tris_rle_target_nearest_u8", P(ends), P(seg_off), lo, hi, H, W, P(yi), P(xi), S, S, P(out), _stream())
    return out


# ------------------------------------------------------ scoring artefacts against REFER ground truth (csrc/labelscore.hip)
SCORE_MAX_THRESHOLDS = 64


def _score_arena(arena, who):
    """(ends, seg_off) of an arena argument, contiguous, on the device, of the arena's dtypes"""
    ends, seg_off = (arena.ends, arena.seg_off) if hasattr(arena, "ends") else arena
    for t, dt, name in ((ends, torch.int32, "ends"), (seg_off, torch.int64, "seg_off")):
        if not t.is_cuda:
            raise NoGpuError(f"tris_amd ops run on MI355X only ({who}: {name} is a CPU tensor); there is no CPU fallback")
        if t.dtype != dt:
            raise TypeError(f"{who}: {name} is {t.dtype}, expected {dt}")
    if seg_off.numel() < 1:
        raise ValueError(f"{who}: seg_off is empty (an arena of n segments has n + 1 offsets)")
    return ends.contiguous(), seg_off.contiguous()


def _score_canvas(H, W, who):
    if H < 1 or W < 1 or H * W > (1 << 24):
        raise ValueError(f"{who}: H*W = {H}x{W} is empty or beyond 2^24 pixels")


def _score_rule(gt_rule, who):
    if gt_rule not in (0, 1):
        raise ValueError(f"{who}: gt_rule {gt_rule!r} is neither 0 (covered exactly once) nor 1 (covered at all)")


def _score_range(lo, hi, n_seg, who):
    if not 0 <= lo <= hi <= n_seg:
        raise ValueError(f"{who}: segments {lo}..{hi} lie outside the arena's {n_seg}")
    if hi - lo > 255:
        raise ValueError(f"{who}: segments {lo}..{hi} are {hi - lo}, more than the 255 a ref may have")


class ScoreThresholds:
    """a threshold list checked once: finite, strictly ascending as float32, 1 .. 64 entries.  `.given` the values as they came, `.host` float32
    numpy (what is compared), `.dev(device)` the device copy (made once per device), so that a sweep over many groups neither re-checks nor re-uploads it."""

    def __init__(self, values):
        import numpy as np
        if torch.is_tensor(values):
            values = values.detach().cpu().numpy()
        v = np.asarray(values, np.float64).reshape(-1)
        if not 1 <= v.size <= SCORE_MAX_THRESHOLDS:
            raise ValueError(f"thresholds: T = {v.size} entries, expected 1 .. {SCORE_MAX_THRESHOLDS}")
        with np.errstate(over="ignore"):
            f = v.astype(np.float32)
        bad = np.nonzero(~np.isfinite(f))[0]
        if bad.size:
            raise ValueError(f"thresholds: entry {int(bad[0])} = {float(v[bad[0]])} is not finite")
        bad = np.nonzero(~(f[1:] > f[:-1]))[0]
        if bad.size:
            j = int(bad[0])
            raise ValueError(f"thresholds: not strictly ascending in float32: entry {j} = {float(f[j])!r}, entry {j + 1} = "
                             f"{float(f[j + 1])!r}")
        self.given, self.host, self._dev = [float(x) for x in v], f, {}

    def __len__(self):
        return self.host.size

    def dev(self, device):
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = torch.from_numpy(self.host.copy()).to(device)
        return t


def score_maps(maps, arena, ranges, thresholds, gt_rule=0):
    """validate.py:183-190 for G maps of one size and a whole threshold sweep in one pass, against refs that stay run ends: maps
    float32 [G,H,W]; arena = (ends, seg_off) on the device or an object with those attributes; ranges [G,2] = the segments lo .. hi-1 of
    each map's ref (a host sequence / numpy array, or an int32 device tensor, which is read back to be checked); thresholds a host
    sequence or a ScoreThresholds -> int64 [G, T+1, 2] on the device: [g, b, bit] = the pixels of map g with exactly b thresholds
    strictly below their value (float32) and that ground-truth bit (gt_rule 0: covered by exactly one segment, ReferDataset.load_mask;
    1: covered at all, validate's target != 0).  Two launches whatever G and T are; no host synchronisation with host ranges."""
    import numpy as np
    who = "score_maps"
    if not torch.is_tensor(maps) or not maps.is_cuda:
        raise NoGpuError("tris_amd ops run on MI355X only (score_maps: maps is not a device tensor); there is no CPU fallback")
    if maps.dtype != torch.float32:
        raise TypeError(f"{who}: maps is {maps.dtype}, expected torch.float32")
    if maps.dim() != 3:
        raise ValueError(f"{who}: maps is [G,H,W], got {tuple(maps.shape)}")
    ends, seg_off = _score_arena(arena, who)
    G, H, W = maps.shape
    _score_canvas(H, W, who)
    _score_rule(gt_rule, who)
    if G > 65535:
        raise ValueError(f"{who}: G = {G} maps in one call, at most 65535")
    thr = thresholds if isinstance(thresholds, ScoreThresholds) else ScoreThresholds(thresholds)
    if torch.is_tensor(ranges):
        if not ranges.is_cuda:
            raise NoGpuError("tris_amd ops run on MI355X only (score_maps: ranges is a CPU tensor); there is no CPU fallback")
        if ranges.dtype != torch.int32:
            raise TypeError(f"{who}: ranges is {ranges.dtype}, expected torch.int32")
        host_ranges, dev_ranges = ranges.cpu().numpy(), ranges.contiguous()
    else:
        host_ranges, dev_ranges = np.asarray(ranges, np.int64), None
    if host_ranges.shape != (G, 2):
        raise ValueError(f"{who}: ranges is [G,2] = [{G},2], got {tuple(host_ranges.shape)}")
    n_seg = seg_off.numel() - 1
    for g, (lo, hi) in enumerate(host_ranges.tolist()):
        _score_range(lo, hi, n_seg, f"{who}: map {g}")
    if dev_ranges is None:
        dev_ranges = torch.from_numpy(host_ranges.astype(np.int32)).to(maps.device)
    T = len(thr)
    hist = torch.empty(G, T + 1, 2, dtype=torch.int64, device=maps.device)
    if G:
        ws = workspace(query("tris_score_workspace_bytes", G, H, W, T + 1))
        call("tris_score_maps_f32", P(maps.contiguous()), P(ends), P(seg_off), P(dev_ranges), G, H, W, P(thr.dev(maps.device)), T,
             gt_rule, P(hist), P(ws), _stream())
    return hist


def score_counts(stack_u8, arena, lo, hi, H, W, gt_rule=0):
    """a uint8 stack [K,H,W] (or an [H,W] image: K = 1; K = 0 allowed) against the ref of segments lo .. hi-1 -> int64 [256,2] on the
    device: [s, bit] = the pixels whose byte sum over the K planes is s (mod 256) and that carry that ground-truth bit.  A label image
    of cam_to_ir_label fills rows 1 / 0 / 255; a bool stack viewed as bytes scores instance masks (s > 0 predicted, s > 1 overlapping,
    the pixels Stage 2 gives a target of 2).  Two launches, no host synchronisation."""
    who = "score_counts"
    if not torch.is_tensor(stack_u8) or not stack_u8.is_cuda:
        raise NoGpuError("tris_amd ops run on MI355X only (score_counts: the stack is not a device tensor); there is no CPU fallback")
    if stack_u8.dtype != torch.uint8:
        raise TypeError(f"{who}: the stack is {stack_u8.dtype}, expected torch.uint8 (view a bool stack as bytes)")
    ends, seg_off = _score_arena(arena, who)
    H, W = int(H), int(W)
    _score_canvas(H, W, who)
    _score_rule(gt_rule, who)
    if stack_u8.dim() == 2:
        stack_u8 = stack_u8.unsqueeze(0)
    if stack_u8.dim() != 3 or tuple(stack_u8.shape[1:]) != (H, W):
        raise ValueError(f"{who}: the stack is [K,{H},{W}], got {tuple(stack_u8.shape)}")
    K = stack_u8.shape[0]
    if K > 255:
        raise ValueError(f"{who}: K = {K} planes, their sum does not fit a byte (at most 255)")
    _score_range(int(lo), int(hi), seg_off.numel() - 1, who)
    hist = torch.empty(256, 2, dtype=torch.int64, device=ends.device)
    ws = workspace(query("tris_score_workspace_bytes", 1, H, W, 256))
    call("tris_score_counts_u8", P(stack_u8.contiguous()) if K else None, K, P(ends), P(seg_off), int(lo), int(hi), H, W, gt_rule,
         P(hist), P(ws), _stream())
    return hist


def _score_table(values, n_in, who, axis):
    """one index table of score_planes as int32 numpy: entries < 0 are samples of nothing, the others lie inside 0 .. n_in - 1 and do
    not decrease (the kernel's run walk only goes forward); anything else is a ValueError naming the entry"""
    import numpy as np
    v = np.asarray(values)
    if v.ndim != 1 or v.size < 1 or v.dtype.kind not in "iu":
        raise ValueError(f"{who}: {axis} is a 1-D integer table of at least one entry, got {v.dtype} {tuple(v.shape)}")
    v = v.astype(np.int64)
    bad = np.nonzero(v >= n_in)[0]
    if bad.size:
        raise ValueError(f"{who}: {axis}[{int(bad[0])}] = {int(v[bad[0]])} lies outside the canvas's 0..{n_in - 1}")
    at = np.nonzero(v >= 0)[0]
    back = np.nonzero(np.diff(v[at]) < 0)[0]
    if back.size:
        j = int(at[back[0] + 1])
        raise ValueError(f"{who}: {axis}[{j}] = {int(v[j])} is below an earlier entry {int(v[at[back[0]]])}: the table decreases")
    return np.maximum(v, -1).astype(np.int32)


def _score_out_hw(out_hw, who):
    hw = (out_hw, out_hw) if isinstance(out_hw, int) and not isinstance(out_hw, bool) else out_hw
    if (not isinstance(hw, (tuple, list)) or len(hw) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in hw)
            or hw[0] < 1 or hw[1] < 1 or hw[0] * hw[1] > (1 << 24)):
        raise ValueError(f"{who}: out_hw {out_hw!r} is neither None, a size S >= 1 nor (Hout, Wout) of at most 2^24 samples")
    return int(hw[0]), int(hw[1])


_SCORE_TABLES_OK = set()


def _score_planes_args(stack_u8, arena, lo, hi, H, W, gt_rule, who):
    if not torch.is_tensor(stack_u8) or not stack_u8.is_cuda:
        raise NoGpuError(f"tris_amd ops run on MI355X only ({who}: the stack is not a device tensor); there is no CPU fallback")
    if stack_u8.dtype != torch.uint8:
        raise TypeError(f"{who}: the stack is {stack_u8.dtype}, expected torch.uint8 (view a bool stack as bytes)")
    ends, seg_off = _score_arena(arena, who)
    H, W = int(H), int(W)
    _score_canvas(H, W, who)
    _score_rule(gt_rule, who)
    if stack_u8.dim() != 3 or tuple(stack_u8.shape[1:]) != (H, W):
        raise ValueError(f"{who}: the stack is [K,{H},{W}], got {tuple(stack_u8.shape)}")
    K = stack_u8.shape[0]
    if K > 255:
        raise ValueError(f"{who}: K = {K} planes, their sum does not fit a byte (at most 255)")
    _score_range(int(lo), int(hi), seg_off.numel() - 1, who)
    return stack_u8.contiguous(), ends, seg_off, K, H, W


def _score_planes_launch(stack_u8, K, ends, seg_off, lo, hi, H, W, yi, xi, out_h, out_w, gt_rule):
    table = torch.empty(K + 3, 2, dtype=torch.int64, device=ends.device)
    ws = workspace(query("tris_score_planes_workspace_bytes", K, out_h, out_w))
    call("tris_score_planes_u8", P(stack_u8) if K else None, K, P(ends), P(seg_off), int(lo), int(hi), H, W,
         None if yi is None else P(yi), None if xi is None else P(xi), out_h, out_w, gt_rule, P(table), P(ws), _stream())
    return table


def score_planes(stack_u8, arena, lo, hi, H, W, out_hw=None, gt_rule=0):
    """a uint8 stack [K,H,W] (0 <= K <= 255) against the ref of segments lo .. hi-1, plane by plane -> int64 [K+3, 2] on the device,
    second index the ground-truth bit: rows 0 / 1 / 2 = the samples whose integer sum over the planes (no byte wrap) is 0 / 1 / at
    least 2, row 3+k = the samples where plane k is not 0.  out_hw=None: every pixel once.  out_hw=(Hout, Wout) or a size S: the
    source pixels Pillow's NEAREST resize to that size reads (the tables of mask_sum_nearest_u8 and rle_target_nearest), so rows
    0 .. 2 are the histogram of Stage 2's resized pseudo target against its resized target.  Two launches, no host synchronisation."""
    who = "score_planes"
    stack_u8, ends, seg_off, K, H, W = _score_planes_args(stack_u8, arena, lo, hi, H, W, gt_rule, who)
    if out_hw is None:
        return _score_planes_launch(stack_u8, K, ends, seg_off, lo, hi, H, W, None, None, H, W, gt_rule)
    out_h, out_w = _score_out_hw(out_hw, who)
    for n_in, n_out, axis in ((H, out_h, "yidx"), (W, out_w, "xidx")):
        if (n_in, n_out) not in _SCORE_TABLES_OK:                  # (Pillow's tables pass; checked once per size pair all the same)
            from .dataset import pil_tables
            _score_table(pil_tables.nearest_index(n_in, n_out), n_in, f"{who}: NEAREST {n_in} -> {n_out}", axis)
            _SCORE_TABLES_OK.add((n_in, n_out))
    yi, = _pil_tables("nearest", H, out_h, ends.device)
    xi, = _pil_tables("nearest", W, out_w, ends.device)
    return _score_planes_launch(stack_u8, K, ends, seg_off, lo, hi, H, W, yi, xi, out_h, out_w, gt_rule)


def score_planes_at(stack_u8, arena, lo, hi, H, W, yidx, xidx, gt_rule=0):
    """score_planes on the samples {(yidx[y], xidx[x])} of two host index tables (integer sequences): a repeated index counts as often
    as it appears, an entry < 0 is a sample with every plane 0 and ground-truth bit 0.  The entries >= 0 of a table lie inside the
    canvas and do not decrease, else a ValueError naming the entry.  The tables are uploaded on every call."""
    who = "score_planes_at"
    stack_u8, ends, seg_off, K, H, W = _score_planes_args(stack_u8, arena, lo, hi, H, W, gt_rule, who)
    yi, xi = _score_table(yidx, H, who, "yidx"), _score_table(xidx, W, who, "xidx")
    if yi.size * xi.size > (1 << 24):
        raise ValueError(f"{who}: {yi.size}x{xi.size} samples are beyond 2^24")
    return _score_planes_launch(stack_u8, K, ends, seg_off, lo, hi, H, W, torch.from_numpy(yi).to(ends.device),
                                torch.from_numpy(xi).to(ends.device), int(yi.size), int(xi.size), gt_rule)


def eval_post_group(maps, targets_u8, signed=False, cams=True):
    """validate_referit.py:160-171 for the K sentences of one image in one call: maps [K,S,S] (or [K,1,S,S]), targets_u8 [K,oH,oW]
    counts -> (records int64 [K,4] on the device = I, U, first arg-max of cam, target count at the arg-max; cams [K,oH,oW], None
    with cams=None / False).  records[k,:3] and cams[k] are bit for bit eval_post / eval_post_signed of sentence k on targets != 0."""
    _chk(maps, targets_u8)
    if maps.dtype != torch.float32 or targets_u8.dtype != torch.uint8:
        raise TypeError("eval_post_group takes (float32 maps, uint8 targets)")
    K, S = maps.shape[0], maps.shape[-1]
    if maps.shape[-2] != S or maps.numel() != K * S * S:
        raise ValueError(f"eval_post_group takes K square maps, got {tuple(maps.shape)}")
    if targets_u8.dim() != 3 or targets_u8.shape[0] != K:
        raise ValueError(f"eval_post_group: {K} maps and targets {tuple(targets_u8.shape)}")
    oH, oW = targets_u8.shape[-2:]
    records = torch.empty(K, 4, device=maps.device, dtype=torch.int64)
    cam = torch.empty(K, oH, oW, device=maps.device, dtype=torch.float32) if cams else None
    if K:
        ws = workspace(query("tris_eval_post_group_workspace_bytes", K))
        call("tris_eval_post_group_f32", P(maps.contiguous()), S, P(targets_u8.contiguous()), K, oH, oW, P(cam), P(records),
             1 if signed else 0, P(ws), _stream())
    return records, cam


# ------------------------------------------------------------------------------------- heat-map overlay (csrc/overlay.hip)
_PAINT_LUT = {}


def cam_paint(maps, image_u8=None, lut=None, mode="minmax", want_norm=False, size=None):
    """demo.py:28-48, 94-96 for the K sentences of one image in one call (two launches): maps float32 [K,Sh,Sw] (or [K,1,Sh,Sw]),
    image_u8 uint8 [H,W,3] RGB or None (then `size` = (H, W), default the maps' own), lut uint8 [256,3] (default
    tris_amd.predict.JET), mode "minmax" (get_norm_cam on the resized, clamped map) or "unit" (maps already in [0, 1]).
    -> (heat uint8 [K,H,W,3], norm float32 [K,H,W] | None, range float32 [K,2] = min, max after the clamp, argmax int64 [K] = raster
    index of the first maximum), all on the device; nothing is synchronised.  Arguments must be contiguous: a strided view is
    refused by name, not copied."""
    if mode not in ("minmax", "unit"):
        raise ValueError(f"cam_paint: mode is 'minmax' or 'unit', got {mode!r}")
    if not torch.is_tensor(maps):
        raise TypeError("cam_paint: maps is a float32 device tensor")
    if lut is None and maps.is_cuda:
        lut = _PAINT_LUT.get(maps.device)
        if lut is None:
            from .predict import JET
            lut = _PAINT_LUT[maps.device] = torch.from_numpy(JET.copy()).to(maps.device)
    for name, t, dt in (("maps", maps, torch.float32), ("image_u8", image_u8, torch.uint8), ("lut", lut, torch.uint8)):
        if t is None:
            continue
        if not torch.is_tensor(t) or not t.is_cuda:
            raise NoGpuError(f"tris_amd ops run on MI355X only (cam_paint: {name} is not a device tensor); there is no CPU fallback")
        if t.dtype != dt:
            raise TypeError(f"cam_paint: {name} must be {dt}, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"cam_paint: {name} must be contiguous")
    if maps.dim() == 4 and maps.shape[1] == 1:
        maps = maps.reshape(maps.shape[0], maps.shape[2], maps.shape[3])
    if maps.dim() != 3 or maps.shape[1] < 1 or maps.shape[2] < 1:
        raise ValueError(f"cam_paint: maps is [K,Sh,Sw], got {tuple(maps.shape)}")
    K, Sh, Sw = maps.shape
    if tuple(lut.shape) != (256, 3):
        raise ValueError(f"cam_paint: lut is [256,3], got {tuple(lut.shape)}")
    if image_u8 is not None:
        if image_u8.dim() != 3 or image_u8.shape[2] != 3:
            raise ValueError(f"cam_paint: image_u8 is [H,W,3], got {tuple(image_u8.shape)}")
        H, W = image_u8.shape[:2]
        if size is not None and tuple(size) != (H, W):
            raise ValueError(f"cam_paint: size {tuple(size)} and image_u8 {tuple(image_u8.shape)} differ")
    else:
        H, W = (Sh, Sw) if size is None else (int(size[0]), int(size[1]))
    if H < 1 or W < 1 or K > 65535:
        raise ValueError(f"cam_paint: {K} maps to {H}x{W}")
    dev = maps.device
    heat = torch.empty(K, H, W, 3, dtype=torch.uint8, device=dev)
    norm = torch.empty(K, H, W, dtype=torch.float32, device=dev) if want_norm else None
    rng = torch.empty(K, 2, dtype=torch.float32, device=dev)
    arg = torch.empty(K, dtype=torch.int64, device=dev)
    if K:
        ws = workspace(query("tris_cam_paint_workspace_bytes", K, H, W) + 256)
        base = (ws.data_ptr() + 255) & ~255
        call("tris_cam_paint_f32", P(maps), K, Sh, Sw, P(image_u8), H, W, P(lut), CONSTS["TRIS_PAINT_UNIT" if mode == "unit" else
             "TRIS_PAINT_MINMAX"], P(heat), P(norm), P(rng), P(arg), base, _stream())
    return heat, norm, rng, arg


# ------------------------------------------------------------------------------------- instance-mask synthesis (IRNet tail)
# csrc/insseg.hip; the public functions with the reference's names are in tris_amd/irn.py
def _chk_t(t, dtype):
    if not t.is_cuda:
        raise NoGpuError("tris_amd ops run on MI355X only (got a CPU tensor); there is no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    return t.contiguous()


def irn_centroids(dp, iterations=300):
    """find_centroids_with_refinement: dp float32 [2,h,w] -> int32 [2,h,w] (y, x), bit-identical to the reference's numpy"""
    dp = _chk_t(dp, torch.float32)
    _, h, w = dp.shape
    out = torch.empty(2, h, w, dtype=torch.int32, device=dp.device)
    call("tris_irn_centroids_f32", P(dp), h, w, int(iterations), P(out), _stream())
    return out


def irn_weak_mask(dp, thres=2.5):
    """sqrt(dp[1]^2 + dp[0]^2) < thres as uint8 [h,w]"""
    dp = _chk_t(dp, torch.float32)
    _, h, w = dp.shape
    out = torch.empty(h, w, dtype=torch.uint8, device=dp.device)
    call("tris_irn_weak_mask_f32", P(dp), h, w, float(thres), P(out), _stream())
    return out


def cc_label(img):
    """skimage.measure.label(connectivity=1, background=0) of uint8 [H,W] or [B,H,W] -> (labels int32 of the same shape, counts
    int32 [B] on device)"""
    img = _chk_t(img, torch.uint8)
    H, W = img.shape[-2:]
    B = img.numel() // max(H * W, 1) if img.dim() == 3 else 1
    labels = torch.empty(img.shape, dtype=torch.int32, device=img.device)
    counts = torch.zeros(B, dtype=torch.int32, device=img.device)
    if B * H * W:
        ws = workspace(query("tris_cc_workspace_bytes", B, H, W))
        call("tris_cc_label_u8", P(img), B, H, W, P(labels), P(counts), P(ws), _stream())
    return labels, counts


def irn_cluster(centroids, dp_label, n_label):
    """cluster_centroids' gather + compress_range: -> (instance map int32 [h,w] in 0..K-1, K int32 [1] on device)"""
    centroids = _chk_t(centroids, torch.int32)
    dp_label = _chk_t(dp_label, torch.int32)
    _, h, w = centroids.shape
    inst = torch.empty(h, w, dtype=torch.int32, device=centroids.device)
    k = torch.empty(1, dtype=torch.int32, device=centroids.device)
    ws = workspace(4 * (int(n_label) + 1))
    call("tris_irn_cluster_i32", P(centroids), P(dp_label), int(n_label), h, w, P(inst), P(k), P(ws), _stream())
    return inst, k


def irn_instance_cam(cam, inst_map, K):
    """separte_score_by_mask: cam [h,w], instance map int32 [h,w] -> [K,h,w]"""
    cam = _chk_t(cam, torch.float32)
    inst_map = _chk_t(inst_map, torch.int32)
    h, w = cam.shape
    out = torch.empty(K, h, w, dtype=torch.float32, device=cam.device)
    call("tris_irn_instance_cam_f32", P(cam), P(inst_map), K, h * w, P(out), _stream())
    return out


def irn_affinity(edge, dirs, path_off, path_cells, beta=10):
    """edge [h,w] -> (Wt [n_dirs, h, w] = a^beta towards each search direction, colsum [h,w]); tables: irn.device_tables"""
    edge = _chk_t(edge, torch.float32)
    dirs, path_off, path_cells = (_chk_t(t, torch.int32) for t in (dirs, path_off, path_cells))
    h, w = edge.shape
    nd = dirs.shape[0]
    Wt = torch.empty(nd, h, w, dtype=torch.float32, device=edge.device)
    colsum = torch.empty(h, w, dtype=torch.float32, device=edge.device)
    call("tris_irn_affinity_f32", P(edge), h, w, P(dirs), P(path_off), P(path_cells), nd, float(beta), P(Wt), P(colsum), _stream())
    return Wt, colsum


def irn_walk(x, edge, Wt, colsum, dirs, steps):
    """`steps` products v <- v T from v0 = x (1 - edge): x [K,h,w] -> [K,h,w]; one launch per step, any map size"""
    x, edge, Wt, colsum = (_chk_t(t, torch.float32) for t in (x, edge, Wt, colsum))
    dirs = _chk_t(dirs, torch.int32)
    K, h, w = x.shape
    out = torch.empty(K, h, w, dtype=torch.float32, device=x.device)
    tmp = torch.empty_like(out)
    call("tris_irn_walk_f32", P(x), P(edge), P(Wt), P(colsum), P(dirs), dirs.shape[0], K, h, w, int(steps), P(out), P(tmp),
         _stream())
    return out


def irn_finish(rw, size, bg_thres=0.25):
    """x4 bilinear upsample (align_corners=False) cropped to size, / global max, arg-max against the background:
    rw [K,h,w] -> (rw_up [K,H,W], labels int32 [H,W] in 0..K)"""
    rw = _chk_t(rw, torch.float32)
    K, h, w = rw.shape
    H, W = int(size[0]), int(size[1])
    if K < 1 or not (0 < H <= 4 * h and 0 < W <= 4 * w):
        raise ValueError(f"irn_finish: K={K}, map {h}x{w}, size {H}x{W}")
    up = torch.empty(K, H, W, dtype=torch.float32, device=rw.device)
    labels = torch.empty(H, W, dtype=torch.int32, device=rw.device)
    ws = workspace(4 * 1032)
    call("tris_irn_finish_f32", P(rw), K, h, w, H, W, float(bg_thres), P(up), P(labels), P(ws), _stream())
    return up, labels


def irn_label_masks(labels, K, base=1):
    """to_one_hot: int32 [H,W] -> uint8 [K,H,W], plane k = (labels == k + base); base 1 is to_one_hot(labels)[1:]"""
    labels = _chk_t(labels, torch.int32)
    H, W = labels.shape
    masks = torch.empty(K, H, W, dtype=torch.uint8, device=labels.device)
    call("tris_irn_label_masks_u8", P(labels), K, H * W, int(base), P(masks), _stream())
    return masks


def irn_fragments(frag_labels, counts, rw_up, min_area):
    """detect_instance's fragments from the labelled masks: frag_labels int32 [K,H,W], counts: K Python ints ->
    (score float32 [F], area int32 [F], masks uint8 [F,H,W]), fragments in (row, label) order"""
    frag_labels = _chk_t(frag_labels, torch.int32)
    rw_up = _chk_t(rw_up, torch.float32)
    K, H, W = frag_labels.shape
    offs, F = [], 0
    for c in counts:
        offs.append(F)
        F += int(c)
    dev = rw_up.device
    score = torch.empty(F, dtype=torch.float32, device=dev)
    area = torch.empty(F, dtype=torch.int32, device=dev)
    masks = torch.empty(F, H, W, dtype=torch.uint8, device=dev)
    if F:
        offsets = torch.tensor(offs, dtype=torch.int32).to(dev)
        ws = workspace(4 * F)
        call("tris_irn_fragments_f32", P(frag_labels), P(rw_up), P(offsets), K, H * W, int(min_area), F, P(score), P(area),
             P(masks), P(ws), _stream())
    return score, area, masks


# --------------------------------------------------------------------------------- IRNet edge / displacement network (inference)
# csrc/irnnet.hip; the module that strings them together is tris_amd/irn_net.py.  Inference only: no autograd Functions.
class autotune_off:
    """inside: dense products take the cost model's (tile, split-K) choice -- no first-encounter timing runs and no entry in the
    per-process cache of tuned shapes (a network whose input size changes from call to call would add ~60 shapes per size)"""

    def __enter__(self):
        self.prev = int(_lib.load().tris_get_autotune())
        set_autotune(False)
        return self

    def __exit__(self, *exc):
        set_autotune(bool(self.prev))
        return False


def irn_stem(img_u8, lut, wk, mean, invstd, gamma, beta):
    """img uint8 [H,W,3], lut [3,256], wk [7,7,3,64] -> relu(bn(conv7x7 s2 p3)) of [img, flip_w(img)]: [2,Ho,Wo,64]"""
    img_u8 = _chk_t(img_u8, torch.uint8)
    _chk(lut, wk, mean, invstd, gamma, beta)
    H, W, C = img_u8.shape
    if C != 3 or tuple(wk.shape) != (7, 7, 3, 64) or not wk.is_contiguous():
        raise ValueError(f"irn_stem: image {tuple(img_u8.shape)}, weight {tuple(wk.shape)}")
    y = torch.empty(2, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64, dtype=torch.float32, device=img_u8.device)
    call("tris_irn_stem_f32", P(img_u8), P(lut.contiguous()), P(wk), P(mean), P(invstd), P(gamma), P(beta), P(y), H, W, _stream())
    return y


def maxpool3s2(x):
    """nn.MaxPool2d(3, 2, 1) on channels-last [B,H,W,C]"""
    x = _chk_t(x, torch.float32)
    B, H, W, C = x.shape
    y = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, dtype=torch.float32, device=x.device)
    call("tris_maxpool3s2_f32", P(x), P(y), B, H, W, C, _stream())
    return y


def subsample2(x):
    """x[:, ::2, ::2, :] as a contiguous tensor (the gather of a stride-2 1x1 convolution)"""
    x = _chk_t(x, torch.float32)
    B, H, W, C = x.shape
    y = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, dtype=torch.float32, device=x.device)
    call("tris_subsample2_f32", P(x), P(y), B, H, W, C, _stream())
    return y


def group_norm_stats(x, G, eps=1e-5):
    """x [B,H,W,C] -> stats float32 [B,G,2] = (mean, 1/sqrt(var + eps)) per image and group; fixed-order fp64 sums"""
    x = _chk_t(x, torch.float32)
    B, H, W, C = x.shape
    stats = torch.empty(B, G, 2, dtype=torch.float32, device=x.device)
    ws = workspace(query("tris_gn_workspace_bytes", B, H * W, G))
    call("tris_gn_stats_f32", P(x), B, H * W, C, G, float(eps), P(stats), P(ws), _stream())
    return stats


def gn_apply_up(x, stats, gamma, beta, G, scale=1, size=None, relu=False, out=None, c_off=0):
    """relu?(crop(upsample_bilinear(groupnorm(x), x scale), size)) for x [B,Hi,Wi,C].  out [B,Ho,Wo,Ct] with c_off: the result
    is written into channels [c_off, c_off + C) of `out` (a concatenation buffer).  stats None: no normalisation."""
    x = _chk_t(x, torch.float32)
    _chk(stats, gamma, beta)
    B, Hi, Wi, C = x.shape
    Ho, Wo = (Hi * scale, Wi * scale) if size is None else (int(size[0]), int(size[1]))
    if out is None:
        out = torch.empty(B, Ho, Wo, C, dtype=torch.float32, device=x.device)
    if tuple(out.shape[:3]) != (B, Ho, Wo) or not out.is_contiguous() or c_off % 4 or c_off + C > out.shape[3]:
        raise ValueError(f"gn_apply_up: out {tuple(out.shape)} does not take [{B},{Ho},{Wo},{C}] at channel {c_off}")
    call("tris_gn_apply_up_f32", P(x), P(stats), P(gamma), P(beta), P(out, c_off), B, Hi, Wi, C, int(G), int(scale), Ho, Wo,
         out.shape[3], int(relu), _stream())
    return out


def irn_head(x, w, bias=None):
    """x [B,h,w,C] (C % 32 == 0), w [N,C] with N = 1 | 2 -> [B,h,w,N] = x . w^T + bias"""
    x = _chk_t(x, torch.float32)
    _chk(w, bias)
    C = x.shape[-1]
    N = w.numel() // C
    M = x.numel() // C
    y = torch.empty(*x.shape[:-1], N, dtype=torch.float32, device=x.device)
    call("tris_irn_head_f32", P(x), C, P(w.contiguous()), P(bias), P(y), M, C, N, _stream())
    return y


def irn_net_finish(edge_out, dp_out):
    """edge_out [2,h,w] (or [2,h,w,1]), dp_out [2,h,w,2] -> (edge [h,w] = sigmoid(row 0 / 2 + flip_w(row 1) / 2), dp [2,h,w] of row 0)"""
    edge_out = _chk_t(edge_out, torch.float32)
    dp_out = _chk_t(dp_out, torch.float32)
    h, w = dp_out.shape[1:3]
    edge = torch.empty(h, w, dtype=torch.float32, device=dp_out.device)
    dp = torch.empty(2, h, w, dtype=torch.float32, device=dp_out.device)
    call("tris_irn_net_finish_f32", P(edge_out), P(dp_out), P(edge), P(dp), h, w, _stream())
    return edge, dp


def bn_frozen(x, mean, invstd, gamma, beta, resid=None, relu=False):
    """FixedBatchNorm (IRNet/net/resnet50.py:10-13): tris_bn_apply_f32 with running statistics and an invstd formed once at load
    time; optional residual add and ReLU.  The pass leaves the amax of what it writes for the h2 product that reads it."""
    _chk(x, mean, invstd, gamma, beta, resid)
    x = x.contiguous()
    C = x.shape[-1]
    y = torch.empty_like(x)
    h2_mark_next(y)
    call("tris_bn_apply_f32", P(x), P(mean), P(invstd), P(gamma), P(beta), P(None if resid is None else resid.contiguous()), P(y),
         x.numel() // C, C, int(relu), _stream())
    return y


# ------------------------------------------------------------------------- IRNet affinity / displacement losses (training)
# csrc/irnloss.hip; the public functions are in tris_amd/irn_loss.py
_IRN_TABLE_RADIUS = {}


def _irn_table_radius(dirs, path_off, path_cells):
    """radius the tables were built for (max |offset| + 1), after one host check per table set that they are what the kernels index
    by: dy >= 0, path_off an ascending [D+1] into path_cells, every cell inside its direction's bounding box"""
    key = (dirs.data_ptr(), path_off.data_ptr(), path_cells.data_ptr(), dirs.shape[0], path_cells.shape[0])
    r = _IRN_TABLE_RADIUS.get(key)
    if r is None:
        d, o, c = dirs.cpu().numpy(), path_off.cpu().numpy(), path_cells.cpu().numpy()
        D = d.shape[0]
        ok = d.ndim == 2 and d.shape[1] == 2 and D >= 1 and o.shape == (D + 1,) and c.ndim == 2 and c.shape[1] == 2
        ok = ok and o[0] == 0 and o[-1] == c.shape[0] and (o[1:] > o[:-1]).all() and (d[:, 0] >= 0).all()
        if ok:
            own = d.repeat(o[1:] - o[:-1], axis=0)                 # the direction of every cell
            ok = ((c[:, 0] >= 0) & (c[:, 0] <= own[:, 0]) & (c[:, 1] >= own[:, 1].clip(max=0)) & (c[:, 1] <= own[:, 1].clip(min=0))).all()
        if not ok:
            raise ValueError(f"irn_aff_losses: dirs {tuple(dirs.shape)}, path_off {tuple(path_off.shape)}, path_cells "
                             f"{tuple(path_cells.shape)} are not the tables of irn.device_tables")
        r = _IRN_TABLE_RADIUS[key] = int(abs(d).max()) + 1
    return r


def irn_loss_check(edge_out, dp_out, label, radius):
    """-> (B, h, w); ValueError naming the shapes for what the op does not take"""
    what = (f"edge_out {tuple(edge_out.shape)} {edge_out.dtype}, dp_out {tuple(dp_out.shape)} {dp_out.dtype}, "
            f"label {tuple(label.shape)} {label.dtype}")
    if edge_out.dim() != 4 or dp_out.dim() != 4 or label.dim() != 3:
        raise ValueError(f"irn_aff_losses takes edge_out [B,1,h,w], dp_out [B,2,h,w], label [B,h,w]; got {what}")
    B, _, h, w = edge_out.shape
    if tuple(edge_out.shape) != (B, 1, h, w) or tuple(dp_out.shape) != (B, 2, h, w) or tuple(label.shape) != (B, h, w) or B < 1:
        raise ValueError(f"irn_aff_losses takes edge_out [B,1,h,w], dp_out [B,2,h,w], label [B,h,w]; got {what}")
    if edge_out.dtype != torch.float32 or dp_out.dtype != torch.float32 or label.dtype != torch.uint8:
        raise ValueError(f"irn_aff_losses takes float32 maps and a uint8 label; got {what}")
    r = int(radius) - 1
    if r < 1 or r > 15:
        raise ValueError(f"irn_aff_losses: radius {radius} (2 .. 16)")
    if h < r + 1 or w < 2 * r + 1:
        raise ValueError(f"irn_aff_losses: a [{h},{w}] map has no source pixel at radius {radius} (needs h >= {r + 1}, w >= {2 * r + 1}); "
                         f"got {what}")
    return B, h, w


class IrnAffLossFn(torch.autograd.Function):
    """AffinityDisplacementLoss.forward's four loss maps (IRNet/net/resnet50_irn.py:211-222) reduced as train_irn.py:57-63 does,
    with the pair labels of voc12/dataloader.py:90-109 taken from `label` in the kernel: -> (losses[4], counts int64 [3])"""

    @staticmethod
    def forward(ctx, edge_out, dp_out, label, dirs, path_off, path_cells, radius):
        B, h, w = irn_loss_check(edge_out, dp_out, label, radius)
        edge_out, dp_out = _chk_t(edge_out, torch.float32), _chk_t(dp_out, torch.float32)
        label = _chk_t(label, torch.uint8)
        dirs, path_off, path_cells = (_chk_t(t, torch.int32) for t in (dirs, path_off, path_cells))
        if _irn_table_radius(dirs, path_off, path_cells) != radius:
            raise ValueError(f"irn_aff_losses: the tables are not those of radius {radius}")
        dev = edge_out.device
        losses = torch.empty(4, dtype=torch.float32, device=dev)
        counts = torch.empty(3, dtype=torch.int64, device=dev)
        norm = torch.empty(5, dtype=torch.float64, device=dev)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        arg_count = torch.empty(B, 3, h, w, dtype=torch.int32, device=dev) if need else None   # (the launch zeroes it)
        ws = workspace(query("tris_irn_loss_workspace_bytes", B, h, w, radius))
        call("tris_irn_loss_fwd_f32", P(edge_out), P(dp_out), P(label), B, h, w, radius, P(dirs), P(path_off), P(path_cells),
             dirs.shape[0], path_cells.shape[0], P(losses), P(counts), P(norm), P(arg_count), P(ws), _stream())
        ctx.radius = radius
        if need:
            ctx.save_for_backward(edge_out, dp_out, label, dirs, arg_count, norm)
        ctx.mark_non_differentiable(counts)
        return losses, counts

    @staticmethod
    def backward(ctx, g, _g_counts):
        edge_out, dp_out, label, dirs, arg_count, norm = ctx.saved_tensors
        B, _, h, w = edge_out.shape
        g = g.to(torch.float32).contiguous()
        d_edge = torch.empty_like(edge_out) if ctx.needs_input_grad[0] else None
        d_dp = torch.empty_like(dp_out) if ctx.needs_input_grad[1] else None
        call("tris_irn_loss_bwd_f32", P(edge_out), P(dp_out), P(label), B, h, w, ctx.radius, P(dirs), dirs.shape[0], P(arg_count),
             P(norm), P(g), P(d_edge), P(d_dp), _stream())
        return d_edge, d_dp, None, None, None, None, None


def irn_aff_losses(edge_out, dp_out, label, dirs, path_off, path_cells, radius=None):
    """edge_out [B,1,h,w] logits, dp_out [B,2,h,w], label uint8 [B,h,w] at the maps' size, tables of irn.device_tables(device, radius)
    -> (losses[4] = (pos_aff, neg_aff, dp_fg, dp_bg), counts int64 [3] = (N_bg, N_fg, N_neg)), differentiable in the two maps.
    radius: what the tables were built for; None reads it from the tables (one device-to-host copy per table set)."""
    for t in (edge_out, dp_out, label, dirs, path_off, path_cells):
        if not t.is_cuda:
            irn_loss_check(edge_out, dp_out, label, 2 if radius is None else radius)
            raise NoGpuError("tris_amd ops run on MI355X only (got a CPU tensor); there is no CPU fallback")
    if radius is None:
        radius = _irn_table_radius(*(_chk_t(t, torch.int32) for t in (dirs, path_off, path_cells)))
    return IrnAffLossFn.apply(edge_out, dp_out, label, dirs, path_off, path_cells, int(radius))


# ------------------------------------------------------------------------ IRNet edge / displacement heads (training)
# csrc/irntrain.hip (+ the float stem of csrc/irnnet.hip); the trainer and the heads' autograd Function are tris_amd/irn_train.py
def irn_stem_batch(img, wk, mean, invstd, gamma, beta):
    """img float32 [B,H,W,3], already normalised (zeros where the loader padded), wk [7,7,3,64] -> relu(bn(conv7x7 s2 p3)):
    [B,Ho,Wo,64]; no flip row"""
    img = _chk_t(img, torch.float32)
    _chk(wk, mean, invstd, gamma, beta)
    if img.dim() != 4 or img.shape[3] != 3 or tuple(wk.shape) != (7, 7, 3, 64) or not wk.is_contiguous():
        raise ValueError(f"irn_stem_batch: image {tuple(img.shape)}, weight {tuple(wk.shape)}")
    B, H, W, _ = img.shape
    y = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64, dtype=torch.float32, device=img.device)
    call("tris_irn_stem_batch_f32", P(img), P(wk), P(mean), P(invstd), P(gamma), P(beta), P(y), B, H, W, _stream())
    return y


def gn_up_bwd(d_out, out, c_off, t, stats, gamma, G, scale=1, want_du=False, dgamma=None, dbeta=None):
    """backward of gn_apply_up(t, stats, gamma, beta, G, scale, size, relu=True, out, c_off): d_out / out [B,Ho,Wo,Ct] the gradient
    of the concatenation buffer and the buffer itself (only channels [c_off, c_off + C) are read; the ReLU mask is out > 0)
    -> (dt [B,Hi,Wi,C], dgamma [C], dbeta [C]) (+ du, the gradient of the GroupNorm output, when want_du).  dgamma / dbeta: where to
    write them (a gradient arena's views) instead of fresh tensors"""
    t = _chk_t(t, torch.float32)
    _chk(d_out, out, stats, gamma)
    B, Hi, Wi, C = t.shape
    if (d_out.shape != out.shape or out.dim() != 4 or out.shape[0] != B or not out.is_contiguous() or not d_out.is_contiguous()
            or c_off % 4 or c_off + C > out.shape[3] or tuple(stats.shape) != (B, G, 2) or gamma.numel() != C):
        raise ValueError(f"gn_up_bwd: gradient {tuple(d_out.shape)}, output {tuple(out.shape)}, input {tuple(t.shape)}, channel {c_off}")
    Ho, Wo, Ct = out.shape[1:]
    dt = torch.empty_like(t)
    du = torch.empty_like(t) if want_du else None
    dgamma = torch.empty(C, dtype=torch.float32, device=t.device) if dgamma is None else dgamma
    dbeta = torch.empty(C, dtype=torch.float32, device=t.device) if dbeta is None else dbeta
    ws = workspace(query("tris_gn_up_bwd_workspace_bytes", B, Hi * Wi, C, int(G)))
    call("tris_gn_up_bwd_f32", P(d_out, c_off), P(out, c_off), Ct, P(t), P(stats.contiguous()), P(gamma.contiguous()), P(dt), P(du),
         P(dgamma), P(dbeta), B, Hi, Wi, C, int(G), int(scale), Ho, Wo, P(ws), _stream())
    return (dt, dgamma, dbeta, du) if want_du else (dt, dgamma, dbeta)


def irn_head_bwd(g, x, w, want_db=False, dw=None, db=None):
    """backward of irn_head: g [...,N] the gradient of its result, x [...,C], w [N,C] -> (dx [...,C], dw [N,C], db [N] | None).
    dw / db: where to write them (a gradient arena's views, N C and N contiguous floats) instead of fresh tensors"""
    x = _chk_t(x, torch.float32)
    g = _chk_t(g, torch.float32)
    _chk(w)
    C = x.shape[-1]
    N = w.numel() // C
    M = x.numel() // C
    if g.numel() != M * N:
        raise ValueError(f"irn_head_bwd: gradient {tuple(g.shape)} for {M} rows of {N}")
    dx = torch.empty_like(x)
    dw = torch.empty(N, C, dtype=torch.float32, device=x.device) if dw is None else dw
    if db is None and want_db:
        db = torch.empty(N, dtype=torch.float32, device=x.device)
    ws = workspace(query("tris_irn_head_bwd_workspace_bytes", M, C, N))
    call("tris_irn_head_bwd_f32", P(g), P(x), C, P(w.contiguous()), P(dx), P(dw), P(db), M, C, N, P(ws), _stream())
    return dx, dw, db


# ------------------------------------------------------------------------------------------ dense-CRF label pass (IRNet)
# csrc/crf.hip; the lattices, the mean field and the functions with the reference's names are in tris_amd/crf.py
def crf_lattice_points(img, tx, ty, tc, scale, H, W):
    """per pixel the d+1 lattice vertices and barycentric weights: -> (keys int64 [N,d+1] packed, bary float32 [N,d+1]).
    d = len(scale) = 2 (features tx[x], ty[y]; img, tc None) | 5 (and tc[r], tc[g], tc[b] of img uint8 [H,W,3])"""
    tx, ty, scale = (_chk_t(t, torch.float32) for t in (tx, ty, scale))
    d = scale.numel()
    if d not in (2, 5) or tx.numel() != W or ty.numel() != H:
        raise ValueError(f"crf_lattice_points: d={d}, tables {tx.numel()} x {ty.numel()} for an image of {H}x{W}")
    if d == 5:
        img, tc = _chk_t(img, torch.uint8), _chk_t(tc, torch.float32)
        if tuple(img.shape) != (H, W, 3) or tc.numel() != 256:
            raise ValueError(f"crf_lattice_points: image {tuple(img.shape)}, colour table {tc.numel()}")
    else:
        img = tc = None
    keys = torch.empty(H * W, d + 1, dtype=torch.int64, device=tx.device)
    bary = torch.empty(H * W, d + 1, dtype=torch.float32, device=tx.device)
    call("tris_crf_lattice_points_f32", P(img), P(tx), P(ty), P(tc), P(scale), H, W, d, P(keys), P(bary), _stream())
    return keys, bary


def crf_neighbours(uniq, d):
    """sorted distinct packed keys int64 [M] -> int32 [d+1, 2, M], -1 for an absent neighbour"""
    uniq = _chk_t(uniq, torch.int64)
    M = uniq.numel()
    nbr = torch.empty(d + 1, 2, M, dtype=torch.int32, device=uniq.device)
    call("tris_crf_neighbours_i64", P(uniq), M, int(d), P(nbr), _stream())
    return nbr


def crf_filter(x, d, bary, inv, order, off, nbr, norm=None):
    """one permutohedral filter pass: x [N,C] (C = 1 | 2 | 4) -> [N,C] = norm * K(norm * x) (plain K without norm)"""
    x, bary = _chk_t(x, torch.float32), _chk_t(bary, torch.float32)
    inv, order, off, nbr = (_chk_t(t, torch.int32) for t in (inv, order, off, nbr))
    N, C = x.shape
    M = off.numel() - 1
    if tuple(bary.shape) != (N, d + 1) or tuple(inv.shape) != (N, d + 1) or order.numel() != N * (d + 1) \
            or tuple(nbr.shape) != (d + 1, 2, M) or C not in (1, 2, 4):
        raise ValueError(f"crf_filter: x {tuple(x.shape)}, d={d}, M={M}, bary {tuple(bary.shape)}, nbr {tuple(nbr.shape)}")
    if norm is not None:
        norm = _chk_t(norm, torch.float32)
        if norm.numel() != N:
            raise ValueError(f"crf_filter: norm of {norm.numel()} for {N} points")
    out = torch.empty_like(x)
    ws = workspace(query("tris_crf_filter_workspace_bytes", M, C))
    call("tris_crf_filter_f32", P(x), P(out), N, C, int(d), M, P(bary), P(inv), P(order), P(off), P(nbr), P(norm), P(ws), _stream())
    return out


def crf_norm(k1):
    """1 / sqrt(K 1 + 1e-20)"""
    k1 = _chk_t(k1, torch.float32)
    out = torch.empty_like(k1)
    call("tris_crf_norm_f32", P(k1), k1.numel(), P(out), _stream())
    return out


def crf_unary_cam(cam, thr_fg, thr_bg, e_same, e_diff):
    """cam [H,W] -> (U, Q) [N, 2 CRFs, 2 labels]: negative values are 0, label = cam > thr (strict), Q = softmax(-U)"""
    cam = _chk_t(cam, torch.float32)
    N = cam.numel()
    U = torch.empty(N, 2, 2, dtype=torch.float32, device=cam.device)
    Q = torch.empty_like(U)
    call("tris_crf_unary_cam_f32", P(cam), N, float(thr_fg), float(thr_bg), float(e_same), float(e_diff), P(U), P(Q), _stream())
    return U, Q


def crf_unary_labels(labels, e_same, e_diff):
    """labels uint8 [R,N] of 0 / 1, R = 1 | 2 -> (U, Q) [N, R, 2]"""
    labels = _chk_t(labels, torch.uint8)
    R, N = labels.shape
    if R not in (1, 2):
        raise ValueError(f"crf_unary_labels: {R} label maps")
    U = torch.empty(N, R, 2, dtype=torch.float32, device=labels.device)
    Q = torch.empty_like(U)
    call("tris_crf_unary_labels_u8", P(labels), R, N, float(e_same), float(e_diff), P(U), P(Q), _stream())
    return U, Q


def crf_update(U, g, b, wg, wb, out=None):
    """Q = softmax over the labels of -U + wg g + wb b; all [N,R,2]"""
    U, g, b = (_chk_t(t, torch.float32) for t in (U, g, b))
    N, R, _ = U.shape
    Q = torch.empty_like(U) if out is None else out
    call("tris_crf_update_f32", P(U), P(g), P(b), float(wg), float(wb), N, R, P(Q), _stream())
    return Q


def crf_combine(Q):
    """Q [N,2,2] -> uint8 [N]: fg_pred, 255 where fg_pred == 0, 0 where bg_pred + fg_pred == 0"""
    Q = _chk_t(Q, torch.float32)
    out = torch.empty(Q.shape[0], dtype=torch.uint8, device=Q.device)
    call("tris_crf_combine_u8", P(Q), Q.shape[0], P(out), _stream())
    return out
