"""Stage-2 EMA consistency training on the MI355X: the lerp kernels and the six-loss kernel of csrc/seg.hip against fp64 torch, the
teacher's forward (trunk on running statistics, decoder on batch statistics) and one trainer step against tests/oracle_ema.py, the
update schedule on the device in both layouts (bound to the optimiser's arenas / unbound), reproducibility, and that a step
without a teacher is the step it was."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-3
U = 2.0 ** -24


@pytest.fixture(params=["x3", "h2"])
def arith(request):
    """both arithmetics of the dense products, as tests/test_gpu_stage2.py (the model tests only: the kernels below have no products)"""
    from tris_amd import ops
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(request.param)
    yield request.param
    ops.set_gemm_mode(prev)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


# ---------------------------------------------------------------------------------------------------------------- lerp
SIZES = (1, 3, 64, 2053)
WEIGHTS = (0.0, 1.0, 0.25, 0.5, 1 - 0.7846)


def _lerp_operands(n, seed):
    """randn operands with planted +-1e30, zeros of both signs and denormals.  A special value is always paired with an ordinary
    one (or with +-1e30): the bound under test is relative to |a| + |b|, and fp32 cannot resolve a result below 2^-149 whatever
    the kernel does, so a pair of two denormals has no fp32 answer inside it."""
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    plant_a = [1e30, -1e30, 0.0, 1e-40, -0.0, 3.0]
    plant_b = [-1e30, 0.7, -1.3, 0.9, 2.0, -1e-41]
    if n >= 16:
        plant_a += [0.3, -1e30, 0.0]
        plant_b += [-0.0, -1e30, 0.0]
    for i, (x, y) in enumerate(zip(plant_a, plant_b)):
        if i < n:
            a[i], b[i] = x, y
    return a, b


def _view_at(t, off):
    """a copy of t on the device that starts `off` floats into its buffer (off = 1: 4-byte but not 16-byte aligned)"""
    buf = torch.full((t.numel() + off + 4,), 7.0, device="cuda")
    v = buf[off:off + t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * off) % 16
    return buf, v


@pytest.mark.parametrize("offs", [(0, 0), (1, 1), (1, 0)])
@pytest.mark.parametrize("n", SIZES)
def test_lerp_against_fp64_and_the_exact_weights(n, offs):
    from tris_amd import ops
    a, b = _lerp_operands(n, 10 + n)
    for w in WEIGHTS:
        abuf, ad = _view_at(a, offs[0])
        _, bd = _view_at(b, offs[1])
        ops.ema_update([(ad, bd)], w)
        got = ad.cpu()
        assert torch.equal(bd.cpu().view(torch.int32), b.view(torch.int32))                       # src is only read
        assert bool((abuf[:offs[0]] == 7.0).all()) and bool((abuf[offs[0] + n:] == 7.0).all())      # nothing outside [0, n)
        if w == 1.0:
            assert torch.equal(got.view(torch.int32), b.view(torch.int32))       # bit for bit: signed zeros and denormals too
        elif w == 0.0:
            assert torch.equal(got.view(torch.int32), a.view(torch.int32))
        else:
            w32 = float(torch.tensor(w, dtype=torch.float64).float())            # the weight the kernel receives
            want = a.double() + w32 * (b.double() - a.double())
            # three fp32 roundings, each at most 2^-24 of an intermediate no larger than |a| + |b|, and a factor 4/3 over that
            bound = 4 * U * (a.double().abs() + b.double().abs())
            assert bool(((got.double() - want).abs() <= bound).all()), (n, w, float(((got.double() - want).abs() - bound).max()))


def test_lerp_table_equals_the_single_launches():
    from tris_amd import ops
    total = sum(SIZES) + 64
    for w in (0.25, 1 - 0.7846, 1.0):
        # one int64 allocation: float views of its head hold the teacher tensors (dst / src on or one float off a 16-byte line in
        # all four combinations), its last 8 words stand next to them and must not change
        raw = torch.arange(1000, 1000 + total // 2 + 40, dtype=torch.int64, device="cuda")
        guard = raw[-8:]
        fl = raw[:-8].view(torch.float32)
        fl.fill_(7.0)
        keep = raw.clone()
        dsts, srcs, singles, pos = [], [], [], 0
        for j, n in enumerate(SIZES):
            a, b = _lerp_operands(n, 20 + n)
            pos = (pos + 3) // 4 * 4 + (j % 2)
            d = fl[pos:pos + n]
            d.copy_(a)
            pos += n + 2
            _, s = _view_at(b, (j // 2) % 2)
            _, d1 = _view_at(a, j % 2)
            ops.ema_update([(d1, s)], w)
            dsts.append(d), srcs.append(s), singles.append(d1)
        table = ops.LerpTable(list(zip(dsts, srcs)))
        assert len(table) == len(SIZES)
        ops.ema_update(table, w)
        covered = torch.zeros_like(fl, dtype=torch.bool)
        for d, d1 in zip(dsts, singles):
            assert torch.equal(d.view(torch.int32), d1.view(torch.int32))
            covered[(d.data_ptr() - fl.data_ptr()) // 4:][:d.numel()] = True
        assert bool((fl[~covered] == 7.0).all()) and int(covered.sum()) == sum(SIZES)
        assert torch.equal(guard, keep[-8:])


@pytest.mark.parametrize("offs", [(1, 1), (1, 0)])
def test_lerp_table_cuts_long_records(offs):
    """a tensor longer than LerpTable.CHUNK becomes several records (cut at whole 16-byte words): the same bits as one launch"""
    from tris_amd import ops
    n = 2 * ops.LerpTable.CHUNK + 5
    a, b = _lerp_operands(n, 3)
    abuf, ad = _view_at(a, offs[0])
    _, bd = _view_at(b, offs[1])
    _, a1 = _view_at(a, 0)
    table = ops.LerpTable([(ad, bd)])
    assert len(table) == 3 and table.records[:, 2].tolist() == [ops.LerpTable.CHUNK, ops.LerpTable.CHUNK, 5]
    ops.ema_update(table, 0.2154)
    ops.ema_update([(a1, bd)], 0.2154)
    assert torch.equal(ad.view(torch.int32), a1.view(torch.int32))
    assert bool((abuf[:offs[0]] == 7.0).all()) and bool((abuf[offs[0] + n:] == 7.0).all())


def test_lerp_refuses_what_it_cannot_address():
    from tris_amd import ops
    a = torch.zeros(4, 6, device="cuda")
    with pytest.raises(ValueError):
        ops.ema_update([(a.t(), torch.zeros(6, 4, device="cuda"))], 0.5)       # not dense
    with pytest.raises(ValueError):
        ops.ema_update([(a, a)], 0.5)
    with pytest.raises(TypeError):
        ops.ema_update([(a.double(), a.double().clone())], 0.5)


# ---------------------------------------------------------------------------------------------------------------- seg_loss5
def _maps(shape, seed):
    g = torch.Generator().manual_seed(seed)
    n = int(torch.tensor(shape).prod())
    outs, emas = [], []
    for k in range(4):
        x, e = 3 * torch.randn(shape, generator=g), 3 * torch.randn(shape, generator=g)
        for i, v in enumerate((0.0, 20.0, -20.0, 100.0, -100.0)):         # planted in the student and, elsewhere, in the teacher
            x.view(-1)[(3 * k + i) % n] = v
            e.view(-1)[(3 * k + i + 7) % n] = v
        outs.append(x), emas.append(e)
    return outs, emas


def _dev(t, misaligned):
    return _view_at(t.reshape(-1), 1)[1].view(t.shape) if misaligned else t.cuda()


CASES = [((1, 1, 5, 7), "i64", 4, False),      # tail only, under one block
         ((2, 1, 32, 32), "f32", 4, False),
         ((3, 1, 67, 61), "i64", 4, False),    # odd, several blocks
         ((2, 1, 32, 32), "i64", 1, False),    # heads 2..4 absent
         ((3, 1, 67, 61), "i64", 4, True),     # every map one float off a 16-byte line
         ((3, 1, 67, 61), "f32", 4, True)]
WTS = torch.tensor([1.0, 0.5, -0.3, 2.0, 0.7, 1.5])      # d(objective) / d(losses[6]): every g_k of the backward is exercised


@pytest.mark.parametrize("shape,kind,heads,misaligned", CASES)
def test_seg_loss5_against_fp64(shape, kind, heads, misaligned):
    import oracle_ema as E
    from tris_amd import ops
    outs, emas = _maps(shape, 31 + shape[-1])
    t = torch.randint(0, 3, shape, generator=torch.Generator().manual_seed(5))
    assert int(t.max()) == 2
    if kind == "f32":
        t = t.float() * 0.5
    outs, emas = outs[:heads], emas[:heads]
    rs = [o.double().requires_grad_() for o in outs]
    want = torch.stack(E.losses6(rs, [e.double() for e in emas], t.double()))
    (want * WTS.double()).sum().backward()
    assert float(want[5].detach()) > 0.01

    def run(mis):
        ds = [_dev(o, mis).requires_grad_() for o in outs]
        es = [_dev(e, mis) for e in emas]
        got = ops.seg_loss5(ds, es, _dev(t, mis and kind == "f32"))
        (got * WTS.cuda()).sum().backward()
        assert all(e.grad is None for e in es)
        return got.detach(), [d.grad for d in ds]
    got, grads = run(misaligned)
    assert got.shape == (6,)
    print("seg_loss5", shape, kind, heads, misaligned, "loss rel", _rel(got, want), "grad rel", [_rel(d, r.grad) for d, r in zip(grads, rs)])
    assert _rel(got, want) < 1e-6
    for d, r in zip(grads, rs):
        assert _rel(d, r.grad) < 1e-5
    # two launches are bit-identical; 4-byte aligned bases give the bits of 16-byte aligned ones
    got2, grads2 = run(misaligned)
    assert torch.equal(got, got2) and all(torch.equal(p, q) for p, q in zip(grads, grads2))
    if misaligned:
        got3, grads3 = run(False)
        assert torch.equal(got, got3) and all(torch.equal(p, q) for p, q in zip(grads, grads3))


@pytest.mark.parametrize("shape,kind,heads,misaligned", CASES)
def test_seg_loss5_with_the_student_as_teacher_is_bce4(shape, kind, heads, misaligned):
    from tris_amd import ops
    outs, _ = _maps(shape, 77)
    t = torch.randint(0, 3, shape, generator=torch.Generator().manual_seed(6))
    t = (t.float() * 0.5 if kind == "f32" else t).cuda()
    outs = outs[:heads]
    ds = [_dev(o, misaligned).requires_grad_() for o in outs]
    got = ops.seg_loss5(ds, [d.detach() for d in ds], t)
    (got * WTS.cuda()).sum().backward()
    bs = [o.cuda().requires_grad_() for o in outs]
    ref = ops.bce4(bs + [None] * (4 - heads), t)
    (ref * WTS[:5].cuda()).sum().backward()
    assert float(got[5]) == 0.0
    assert torch.equal(got[:5].detach(), ref.detach())
    for d, b in zip(ds, bs):
        assert torch.equal(d.grad, b.grad)


def test_seg_loss5_contracts():
    from tris_amd import ops
    x = [torch.randn(1, 1, 4, 4, device="cuda") for _ in range(4)]
    t = torch.zeros(1, 1, 4, 4, dtype=torch.long, device="cuda")
    with pytest.raises(ValueError):
        ops.seg_loss5(x, x[:3], t)
    with pytest.raises(ValueError):
        ops.seg_loss5(x, x[:3] + [torch.randn(1, 1, 4, 5, device="cuda")], t)
    with pytest.raises(ValueError):
        ops.seg_loss5([x[0], None, x[2]], [x[0], x[1], x[2]], t)
    got = ops.seg_loss5(x, x, t.to(torch.uint8))              # any target dtype, as bce4
    assert torch.equal(got[:5], ops.bce4(x, t))


# ---------------------------------------------------------------------------------------------------------------- the model
SIZE, B, T = 64, 2, 20


def _args():
    from tris_amd.args import get_parser
    return get_parser().parse_args(["--backbone", "clip-RN50", "--size", str(SIZE), "--max_query_len", str(T), "--batch_size", str(B)])


def _student_and_teacher(sd=None, **ema_kw):
    """as train_stage2.main: the EMA is built right after TRIS(args).cuda() (root in train mode, backbone in eval mode), then
    model.train().  Weights: the seed-fill of tests/test_gpu_stage2.py (sd: a state to start from instead)"""
    import warnings
    from oracle_stage2 import reset_slopes
    from tris_amd.ema import EMA
    from tris_amd.model.model_stage2 import TRIS
    from tris_amd.utils.synth import seed_fill
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = TRIS(_args()).cuda()
    if sd is None:
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        seed_fill(sd, 1234)
        reset_slopes(sd)
    m.load_state_dict(sd)
    ema = EMA(m, **ema_kw)
    m.train()
    return m, ema, sd


def _optimizer(m):
    from tris_amd.optim import FusedAdamW
    bb, hd = m.trainable_parameters()
    return FusedAdamW([{"params": bb, "lr": 5e-6, "weight_decay": 0.01}, {"params": hd, "lr": 5e-5, "weight_decay": 0.01}], lr=5e-5,
                      weight_decay=0.01)


def _state(module):
    return {k: v.detach().clone() for k, v in module.state_dict().items()}


@pytest.fixture(scope="module")
def oracle_64():
    """fp64 restatement at 64 px, B = 2, T = 20: the student's four maps (everything in train mode), the teacher's four maps (trunk
    on running statistics, decoder on batch statistics) with the decoder statistics its forward leaves, and the six losses"""
    import oracle_ema as E
    import oracle_stage2 as S
    from tris_amd.utils.synth import synthetic_batch
    m, ema, sd = _student_and_teacher()
    del m, ema
    b = synthetic_batch(B, SIZE, T, 0, seed=7)
    tgt = torch.randint(0, 3, (B, 1, SIZE, SIZE), generator=torch.Generator().manual_seed(9))

    def sd64():
        return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    with torch.no_grad():
        outs = S.forward(sd64(), b["img"].double(), b["word_ids"], True)
        tsd = sd64()
        eouts = E.teacher_forward(tsd, b["img"].double(), b["word_ids"])
        losses = torch.stack(E.losses6(outs, eouts, tgt))
    return dict(sd=sd, b=b, tgt=tgt, outs=outs, ema_outs=eouts, losses=losses, teacher_sd=tsd)


def test_teacher_forward_against_fp64(oracle_64, arith):
    from tris_amd import ops
    o = oracle_64
    m, ema, _ = _student_and_teacher(o["sd"])
    before, tbefore = _state(m), _state(ema.ema_model)
    ops.h2_begin_step()
    with torch.no_grad():
        outs = ema(o["b"]["img"].cuda(), o["b"]["word_ids"].cuda())
    ops.h2_end_step()
    assert len(outs) == 4 and all(tuple(x.shape) == (B, 1, SIZE, SIZE) and not x.requires_grad for x in outs)
    for a, r in zip(outs, o["ema_outs"]):
        assert float((a.double().cpu() - r).abs().max()) < TOL * max(1.0, float(r.abs().max()))
    # it is not the all-train forward: the two differ by far more than the bound
    assert float((o["ema_outs"][0] - o["outs"][0]).abs().max()) > 20 * TOL * max(1.0, float(o["outs"][0].abs().max()))
    after, tafter = _state(m), _state(ema.ema_model)
    for k in before:
        assert torch.equal(before[k], after[k]), k                       # the student is bit-unchanged
    # side effect: the decoder's running statistics move (batch statistics), the trunk's do not (running statistics)
    for k in ("reduced_c1.bn.running_mean", "output1.bn.running_var", "final_seg4.0.bn.running_mean"):
        assert _rel(tafter[k], o["teacher_sd"][k]) < TOL and not torch.equal(tafter[k], tbefore[k]), k
    for k in tafter:
        if k.startswith("backbone.") or not ("running_" in k or "num_batches" in k):
            assert torch.equal(tafter[k], tbefore[k]), k
    assert int(tafter["reduced_c1.bn.num_batches_tracked"]) == 1 and int(tafter["backbone.visual.bn1.num_batches_tracked"]) == 0


@pytest.mark.parametrize("bound", [True, False])
def test_one_trainer_step_with_ema_against_the_oracle(oracle_64, arith, bound):
    from tris_amd import ops
    from tris_amd.train_stage2 import train_step
    o = oracle_64
    m, ema, _ = _student_and_teacher(o["sd"])
    opt = _optimizer(m)
    if bound:
        ema.bind(opt)
    first_id = ops._H2_STEP_IDS[0]
    losses = train_step(m, opt, o["b"]["img"].cuda(), o["b"]["word_ids"].cuda(), o["tgt"].cuda(), ema, True)
    if arith == "h2":
        assert ops._H2_STEP_IDS[0] == first_id + 1       # student and teacher fit ONE amax pool: it was not restarted mid-step
    assert losses.shape == (6,) and not losses.requires_grad
    got = losses.double().cpu()
    print("ema step", arith, bound, got.tolist(), o["losses"].tolist())
    assert float((got - o["losses"]).abs().max()) < TOL
    assert float(got[5]) > TOL                           # l5 is there (1.8e-3 at these weights)
    # update() at step 0 is the copy: every floating tensor of the teacher is the student's UPDATED one, bit for bit ...
    s, t = _state(m), _state(ema.ema_model)
    assert ema.step == 1
    for k in s:
        if s[k].is_floating_point():
            assert torch.equal(s[k].view(torch.int32), t[k].view(torch.int32)), k
    assert not torch.equal(s["output1.conv.weight"].cpu(), o["sd"]["output1.conv.weight"])
    # ... and num_batches_tracked is the teacher's own: 1 where ITS forward ran on batch statistics, 0 in its eval-mode trunk
    assert int(s["backbone.visual.bn1.num_batches_tracked"]) == 1 and int(t["backbone.visual.bn1.num_batches_tracked"]) == 0
    assert int(t["reduced_c1.bn.num_batches_tracked"]) == 1
    ema.update()                                          # step 1: skipped (update_every = 10)
    t2 = _state(ema.ema_model)
    assert all(torch.equal(t[k], t2[k]) for k in t)


PROBES = ["output1.conv.weight", "backbone.visual.layer1.0.conv1.weight", "backbone.logit_scale", "backbone.visual.bn1.running_mean"]


def test_schedule_on_the_device_in_both_layouts(oracle_64, arith):
    """EMA(update_after_step=2, update_every=1): updates 0..2 copy, update 3 copies and averages, update 4 averages.  Three
    parameters -- one of each arena and one outside them -- and one BatchNorm buffer of the trunk (which the teacher's own forward
    does not move) follow the oracle's recurrence fed the student's tensors of every step."""
    import oracle_ema as E
    from tris_amd.train_stage2 import train_step
    o = oracle_64
    img, ids, tgt = o["b"]["img"].cuda(), o["b"]["word_ids"].cuda(), o["tgt"].cuda()
    final = {}
    for bound in (True, False):
        m, ema, _ = _student_and_teacher(o["sd"], update_after_step=2, update_every=1)
        opt = _optimizer(m)
        if bound:
            ema.bind(opt)
        sched = E.Schedule(update_after_step=2, update_every=1)
        teacher = {k: o["sd"][k].double().clone() for k in PROBES}
        err = {k: torch.zeros_like(teacher[k]) for k in PROBES}
        lerps = 0
        for step in range(5):
            train_step(m, opt, img, ids, tgt, ema, True)
            sd = m.state_dict()
            student = {k: sd[k].detach().double().cpu() for k in PROBES}
            acts = sched()
            for a in acts:
                if a[0] == "copy":
                    for k in PROBES:
                        err[k].zero_()
                else:
                    lerps += 1
                    for k in PROBES:      # the lerp bound of test_lerp_against_fp64, accumulated (an earlier error shrinks by 1 - w)
                        err[k] += 4 * U * (teacher[k].abs() + student[k].abs())
                E.apply(teacher, student, [a])
        assert lerps == 2 and ema.step == 5 and ema.initted
        got = _state(ema.ema_model)
        sd = m.state_dict()
        for k in PROBES:
            assert bool(((got[k].double().cpu() - teacher[k]).abs() <= err[k]).all()), (bound, k)
        assert not torch.equal(got["output1.conv.weight"], sd["output1.conv.weight"])     # it lags the student now
        final[bound] = (got, _state(m))
        del m, ema, opt
    for part in (0, 1):
        for k in final[True][part]:
            assert torch.equal(final[True][part][k], final[False][part][k]), (part, k)


def test_two_ema_runs_from_one_state_are_bitwise_identical(oracle_64, arith):
    from tris_amd.train_stage2 import train_step
    o = oracle_64
    res = []
    for _ in range(2):
        m, ema, _ = _student_and_teacher(o["sd"], update_after_step=0, update_every=1)
        opt = _optimizer(m)
        ema.bind(opt)
        ls = [train_step(m, opt, o["b"]["img"].cuda(), o["b"]["word_ids"].cuda(), o["tgt"].cuda(), ema, True).clone() for _ in range(2)]
        res.append((torch.stack(ls), _state(m), _state(ema.ema_model)))
        del m, ema, opt
    assert torch.isfinite(res[0][0]).all() and float(res[0][0][1, 5]) > 0
    assert torch.equal(res[0][0], res[1][0])
    for part in (1, 2):
        for k in res[0][part]:
            assert torch.equal(res[0][part][k], res[1][part][k]), (part, k)


def test_without_a_teacher_the_step_is_the_step_it_was(oracle_64, arith):
    """model_ema=None: the five losses and the updated model, bit for bit those of the step as it stood before EMA existed
    (forward -> ops.bce4 -> backward -> AdamW in one h2 bracket)"""
    from tris_amd import ops
    from tris_amd.train_stage2 import train_step
    o = oracle_64
    img, ids, tgt = o["b"]["img"].cuda(), o["b"]["word_ids"].cuda(), o["tgt"].cuda()
    m, _, _ = _student_and_teacher(o["sd"])
    opt = _optimizer(m)
    got = train_step(m, opt, img, ids, tgt)
    after = _state(m)
    del m, opt
    m, _, _ = _student_and_teacher(o["sd"])
    opt = _optimizer(m)
    ops.h2_begin_step()
    ref = ops.bce4(m(img, ids), tgt)
    opt.zero_grad()
    ref[0].backward()
    opt.step()
    ops.h2_end_step()
    assert got.shape == (5,) and torch.equal(got, ref.detach())
    want = _state(m)
    for k in want:
        assert torch.equal(after[k], want[k]), k
    assert float((got.double().cpu() - o["losses"][:5]).abs()[1:].max()) < TOL
    with pytest.raises(ValueError):
        train_step(m, opt, img, ids, tgt, None, True)
