"""Stage-2 (pseudo-mask decoder) on the MI355X: the kernels of csrc/seg.hip against fp64 torch on CPU, every decoder convolution
shape, the whole model against the fp64 restatement (tests/oracle_stage2.py), one optimiser step, reproducibility, the signed
evaluation and the script-level trainer."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 1e-3


@pytest.fixture(autouse=True, params=["x3", "h2"])
def arith(request):
    """both arithmetics of the dense products, as tests/test_gpu_parity.py"""
    from tris_amd import ops
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(request.param)
    yield request.param
    ops.set_gemm_mode(prev)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _args(size=320, extra=()):
    from tris_amd.args import get_parser
    return get_parser().parse_args(["--backbone", "clip-RN50", "--size", str(size), "--max_query_len", "20", "--batch_size", "2"]
                                   + list(extra))


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,H,W,C", [(2, 10, 12, 64), (2, 10, 10, 512), (2, 80, 80, 32)])
def test_bn_prelu_forward_backward(training, B, H, W, C):
    from tris_amd import ops
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, H, W, C, generator=g) * 2 + 0.3
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    rm, rv = 0.1 * torch.randn(C, generator=g), 1 + 0.1 * torch.rand(C, generator=g)
    a = torch.tensor([0.23])
    dy = torch.randn(B, H, W, C, generator=g)
    # reference: fp64 torch on the NCHW view
    xs = [t.double().requires_grad_() for t in (x, gamma, beta, a)]
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    z = F.batch_norm(xs[0].permute(0, 3, 1, 2), rm64, rv64, xs[1], xs[2], training, 0.1, 1e-5)
    y_ref = F.prelu(z, xs[3]).permute(0, 2, 3, 1)
    y_ref.backward(dy.double())
    dev = [t.cuda().requires_grad_() for t in (x, gamma, beta, a)]
    rmd, rvd = rm.cuda(), rv.cuda()
    y = ops.bn_prelu(dev[0], dev[1], dev[2], rmd, rvd, dev[3], training)
    y.backward(dy.cuda())
    assert _rel(y, y_ref) < 1e-6
    for d, r in zip(dev, xs):
        assert _rel(d.grad, r.grad) < 1e-5, (d.shape, _rel(d.grad, r.grad))
    assert _rel(rmd, rm64) < 1e-6 and _rel(rvd, rv64) < 1e-6
    # launched twice on the same inputs: bitwise identical
    y2 = ops.bn_prelu(dev[0].detach(), dev[1].detach(), dev[2].detach(), rm.cuda(), rv.cuda(), dev[3].detach(), training)
    y3 = ops.bn_prelu(dev[0].detach(), dev[1].detach(), dev[2].detach(), rm.cuda(), rv.cuda(), dev[3].detach(), training)
    assert torch.equal(y2, y3)
    grads = []
    for _ in range(2):
        ts = [t.detach().clone().requires_grad_() for t in dev]
        ops.bn_prelu(ts[0], ts[1], ts[2], rm.cuda(), rv.cuda(), ts[3], training).backward(dy.cuda())
        grads.append([t.grad.clone() for t in ts])
    assert all(torch.equal(p, q) for p, q in zip(*grads))


@pytest.mark.parametrize("hw", [((10, 10), (20, 20)), ((7, 9), (20, 17))])
def test_upsample_add_nhwc(hw):
    from tris_amd import ops
    (Hi, Wi), (Ho, Wo) = hw
    g = torch.Generator().manual_seed(2)
    B, C = 2, 32
    x, skip = torch.randn(B, Hi, Wi, C, generator=g), torch.randn(B, Ho, Wo, C, generator=g)
    d_up, d_sum = torch.randn(B, Ho, Wo, C, generator=g), torch.randn(B, Ho, Wo, C, generator=g)
    xr, sr = x.double().requires_grad_(), skip.double().requires_grad_()
    up_r = F.interpolate(xr.permute(0, 3, 1, 2), (Ho, Wo), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    sum_r = up_r + sr
    torch.autograd.backward([up_r, sum_r], [d_up.double(), d_sum.double()])
    xd, sd_ = x.cuda().requires_grad_(), skip.cuda().requires_grad_()
    up, s = ops.upsample_nhwc(xd, (Ho, Wo), skip=sd_)
    torch.autograd.backward([up, s], [d_up.cuda(), d_sum.cuda()])
    assert _rel(up, up_r) < 1e-6 and _rel(s, sum_r) < 1e-6
    assert _rel(xd.grad, xr.grad) < 1e-6 and torch.equal(sd_.grad.cpu(), d_sum)
    # the NCHW resize of the library gives the same bits
    nchw = ops.resize_bilinear(x.cuda().permute(0, 3, 1, 2).contiguous(), (Ho, Wo), False)
    assert torch.equal(nchw.permute(0, 2, 3, 1).contiguous(), up.detach())
    # the NCHW backward as well, for one incoming gradient
    xn = x.cuda().permute(0, 3, 1, 2).contiguous().requires_grad_()
    ops.resize_bilinear(xn, (Ho, Wo), False).backward(d_up.cuda().permute(0, 3, 1, 2).contiguous())
    xc = x.cuda().requires_grad_()
    ops.upsample_nhwc(xc, (Ho, Wo)).backward(d_up.cuda())
    assert torch.equal(xn.grad.permute(0, 2, 3, 1).contiguous(), xc.grad)
    again = ops.upsample_nhwc(x.cuda(), (Ho, Wo), skip=skip.cuda())
    assert torch.equal(again[0], up.detach()) and torch.equal(again[1], s.detach())


@pytest.mark.parametrize("C", [32, 64])
def test_head1x1(C):
    from tris_amd import ops
    g = torch.Generator().manual_seed(3)
    x, w, gy = torch.randn(2, 20, 20, C, generator=g), 0.1 * torch.randn(1, C, 1, 1, generator=g), torch.randn(2, 1, 20, 20, generator=g)
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    yr = F.conv2d(xr.permute(0, 3, 1, 2), wr)
    yr.backward(gy.double())
    xd, wd = x.cuda().requires_grad_(), w.cuda().requires_grad_()
    y = ops.head1x1(xd, wd)
    y.backward(gy.cuda())
    assert y.shape == (2, 1, 20, 20)
    assert _rel(y, yr) < 1e-6 and _rel(xd.grad, xr.grad) < 1e-6 and _rel(wd.grad, wr.grad) < 1e-6
    assert torch.equal(ops.head1x1(x.cuda(), w.cuda()), y.detach())


def test_bce_four_heads():
    from tris_amd import ops
    g = torch.Generator().manual_seed(4)
    outs = [3 * torch.randn(2, 1, 32, 32, generator=g) for _ in range(4)]
    t = torch.randint(0, 3, (2, 1, 32, 32), generator=g)          # pseudo targets may exceed 1 (summed instances)
    assert int(t.max()) == 2
    rs = [o.double().requires_grad_() for o in outs]
    ls = [F.binary_cross_entropy_with_logits(r, t.double(), reduction="mean") for r in rs]
    (ls[0] + ls[1] + ls[2] + ls[3]).backward()
    ds = [o.cuda().requires_grad_() for o in outs]
    got = ops.bce4(ds, t.cuda())
    got[0].backward()
    want = torch.stack([sum(ls)] + ls).detach()
    assert _rel(got, want) < 1e-6
    for d, r in zip(ds, rs):
        assert _rel(d.grad, r.grad) < 1e-5
    assert torch.equal(ops.bce4([o.cuda() for o in outs], t.cuda()), got.detach())


def _np_signed_eval(m, tgt):
    """validate.py:179-191 on numpy / torch CPU (fp32): I, U, np.argmax of the normalised map"""
    oH, oW = tgt.shape
    pred = F.interpolate(m, (oH, oW), align_corners=True, mode="bilinear").squeeze(0)
    pred /= F.adaptive_max_pool2d(pred, (1, 1)) + 1e-5
    pred = pred.squeeze(0)
    cam = pred.clone()
    p = pred.gt(1e-9)
    t = torch.from_numpy(tgt).bool()
    return int((p & t).sum()), int((p | t).sum()), int(np.argmax(cam.numpy(), axis=None))


@pytest.mark.parametrize("kind", ["mixed", "negative", "positive"])
def test_signed_eval(kind):
    from tris_amd import ops
    g = torch.Generator().manual_seed(5)
    m = torch.randn(1, 1, 40, 40, generator=g)
    if kind == "negative":
        m = -m.abs() - 0.5
    elif kind == "positive":
        m = m.abs() + 0.1
    tgt = (torch.rand(57, 71, generator=g) > 0.6).numpy().astype(np.uint8)
    I, U, am = _np_signed_eval(m.clone(), tgt)
    iu, cam = ops.eval_post_signed(m.cuda(), torch.from_numpy(tgt).cuda())
    assert iu.tolist() == [I, U, am]
    iu2, cam2 = ops.eval_post_signed(m.cuda(), torch.from_numpy(tgt).cuda())
    assert torch.equal(iu, iu2) and torch.equal(cam, cam2)
    if kind == "negative":   # the sign flips: the prediction is the negative pixels, the hit point the arg-min
        assert am == int(np.argmin(F.interpolate(m, (57, 71), align_corners=True, mode="bilinear").numpy()))


# ---------------------------------------------------------------------------------------------------------------- decoder convolutions
SHAPES = [(256, 64, 80), (512, 128, 40), (1024, 256, 20), (2048, 512, 10), (512, 256, 10), (256, 128, 20), (128, 64, 40),
          (64, 32, 80), (32, 32, 80), (64, 32, 80), (128, 64, 40), (256, 64, 20)]


@pytest.mark.parametrize("cin,cout,hw", SHAPES)
def test_decoder_conv_shapes(cin, cout, hw):
    from tris_amd import ops
    g = torch.Generator().manual_seed(cin + cout + hw)
    x = torch.randn(2, hw, hw, cin, generator=g)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(2, hw, hw, cout, generator=g)
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    yr = F.conv2d(xr.permute(0, 3, 1, 2), wr, padding=1).permute(0, 2, 3, 1)
    yr.backward(dy.double())
    xd, wd = x.cuda().requires_grad_(), torch.nn.Parameter(w.cuda())
    y = ops.conv3x3(xd, wd, 1, stats=True)
    y.backward(dy.cuda())
    assert _rel(y, yr) < 1e-4 and _rel(xd.grad, xr.grad) < 1e-4 and _rel(wd.grad, wr.grad) < 1e-4


# ---------------------------------------------------------------------------------------------------------------- the model
def _model(size=320):
    import warnings
    from oracle_stage2 import reset_slopes
    from tris_amd.model.model_stage2 import TRIS
    from tris_amd.utils.synth import seed_fill
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = TRIS(_args(size)).cuda()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    seed_fill(sd, 1234)
    reset_slopes(sd)
    m.load_state_dict(sd)
    return m, sd


# (reduced_c4.relu.weight is not a probe here: its gradient -- 2.8e-5 -- is a sum over 512 channels that cancels ~20x, so the ~1 %
#  round-off of each channel's term, the floor every other probe shows, becomes 30-60 % of the sum.  The kernel's slope gradient at
#  exactly that shape is checked against fp64 in test_bn_prelu_forward_backward.)
PROBES = ["final_seg1.1.weight", "final_seg3.0.relu.weight", "output1.relu.weight", "output2.conv.weight",
          "reduced_c1.bn.weight", "reduced_c4.bn.weight", "reduced_c4.bn.bias", "attention3.Wq.weight", "attention2.Wk.weight", "backbone.visual.layer4.2.conv3.weight",
          "backbone.visual.layer1.0.conv1.weight", "backbone.transformer.resblocks.11.mlp.c_fc.weight"]


@pytest.fixture(scope="module")
def oracle_320():
    """fp64 restatement at B = 2, 320 px: outputs, losses, gradients of the probes, running statistics after the forward"""
    import oracle_stage2 as S
    from tris_amd.utils.synth import synthetic_batch
    m, sd = _model()
    del m
    b = synthetic_batch(2, 320, 20, 0, seed=7)
    tgt = torch.randint(0, 3, (2, 1, 320, 320), generator=torch.Generator().manual_seed(9))
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for k in PROBES:
        sd64[k].requires_grad_()
    outs = S.forward(sd64, b["img"].double(), b["word_ids"], True)
    ls = S.losses(outs, tgt)
    ls[0].backward()
    # the same in fp32 on the CPU: how far ONE correct fp32 implementation lands from fp64 calibrates the gradient bound
    sd32 = {k: v.clone() for k, v in sd.items()}
    for k in PROBES:
        sd32[k].requires_grad_()
    S.losses(S.forward(sd32, b["img"], b["word_ids"], True), tgt)[0].backward()
    ev_sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    with torch.no_grad():
        ev = S.forward(ev_sd, b["img"].double(), b["word_ids"], False)
    return dict(sd=sd, b=b, tgt=tgt, outs=[o.detach() for o in outs], losses=torch.stack([l.detach() for l in ls]),
                grads={k: sd64[k].grad for k in PROBES}, dev32={k: float((sd32[k].grad.double() - sd64[k].grad).norm()) for k in PROBES},
                eval=ev, rm={k: sd64[k].detach() for k in sd64 if k.endswith("running_mean")})


def test_model_forward_backward_against_fp64(oracle_320, arith):
    from tris_amd import ops
    o = oracle_320
    m, _ = _model()
    m.train()
    img, ids, tgt = o["b"]["img"].cuda(), o["b"]["word_ids"].cuda(), o["tgt"].cuda()
    ops.h2_begin_step()
    outs = m(img, ids)
    losses = ops.bce4(outs, tgt)
    losses[0].backward()
    ops.wgrad_join()
    ops.h2_end_step()
    for a, r in zip(outs, o["outs"]):
        assert (a.detach().double().cpu() - r).abs().max() < TOL * max(1.0, float(r.abs().max()))
    assert (losses.detach().double().cpu() - o["losses"]).abs().max() < TOL
    params = dict(m.named_parameters())
    bad = []
    for k in PROBES:
        # noise-calibrated (tests/test_gpu_parity.py): within 8x the fp32 CPU run's distance from fp64, never tighter than 1e-3 of the norm
        n64 = float(o["grads"][k].norm())
        dev = float((params[k].grad.double().cpu() - o["grads"][k]).norm())
        if dev > max(8.0 * o["dev32"][k], 1e-3 * n64):
            bad.append((k, dev / n64, o["dev32"][k] / n64))
    assert not bad, bad
    sd = m.state_dict()
    for k in ("reduced_c1.bn.running_mean", "output1.bn.running_mean", "final_seg4.0.bn.running_mean"):
        assert _rel(sd[k], o["rm"][k]) < TOL
    m.load_state_dict(o["sd"])     # (the eval reference runs on the running statistics BEFORE the train forward above)
    m.eval()
    with torch.no_grad():
        ev = m(img, ids)
    assert ev.shape == (2, 1, 320, 320)
    assert (ev.double().cpu() - o["eval"]).abs().max() < TOL * max(1.0, float(o["eval"].abs().max()))


def test_optimizer_step_against_adamw_oracle(oracle_320):
    """one FusedAdamW step over the two Stage-2 groups (lr * lr_multi for the backbone, lr for the head; weight decay, bias
    correction) against oracle.tris_oracle.adamw_step fed the same gradients; parameters without a gradient stay bit-unchanged"""
    from oracle import tris_oracle as O
    from tris_amd import ops
    from tris_amd.optim import FusedAdamW
    o = oracle_320
    m, _ = _model()
    m.train()
    bb, hd = m.trainable_parameters()
    lr, mult, wd = 5e-5, 0.1, 0.01
    opt = FusedAdamW([{"params": bb, "lr": lr * mult, "weight_decay": wd}, {"params": hd, "lr": lr, "weight_decay": wd}], lr=lr,
                     weight_decay=wd)
    named = dict(m.named_parameters())
    before = {k: v.detach().cpu().clone() for k, v in named.items()}
    ops.h2_begin_step()
    opt.zero_grad()
    losses = ops.bce4(m(o["b"]["img"].cuda(), o["b"]["word_ids"].cuda()), o["tgt"].cuda())
    losses[0].backward()
    ops.wgrad_join()
    torch.cuda.synchronize()
    grads = {k: v.grad.detach().cpu().clone() for k, v in named.items() if v.grad is not None and not getattr(v, "_tris_no_grad_path", False)}
    opt.step()
    ops.h2_end_step()
    frozen = ["backbone.text_projection", "backbone.logit_scale"] + [k for k in named if ".attnpool." in k]
    assert not any(k in grads for k in frozen)
    ids_bb = {id(p) for p in bb}
    for group_lr, keys in ((lr * mult, [k for k in grads if id(named[k]) in ids_bb]), (lr, [k for k in grads if id(named[k]) not in ids_bb])):
        want = {k: before[k].clone() for k in keys}
        O.adamw_step(want, {k: grads[k] for k in keys}, {}, group_lr, wd=wd)
        for k in keys:
            got = named[k].detach().cpu()
            # (two fp32 evaluations of the same update: a rounding step of the parameter apart at most)
            assert bool(((got - want[k]).abs() <= 1e-3 * group_lr + 2.4e-7 * want[k].abs()).all()), k
    for k in frozen:
        assert torch.equal(named[k].detach().cpu(), before[k]), k


def test_two_steps_from_one_state_are_bitwise_identical():
    from tris_amd.optim import FusedAdamW
    from tris_amd.train_stage2 import train_step
    from tris_amd.utils.synth import synthetic_batch
    b = synthetic_batch(48, 320, 20, 0, seed=11)
    tgt = torch.randint(0, 3, (48, 1, 320, 320), generator=torch.Generator().manual_seed(3)).cuda()
    res = []
    for _ in range(2):
        m, _sd = _model()
        m.train()
        bb, hd = m.trainable_parameters()
        opt = FusedAdamW([{"params": bb, "lr": 5e-6}, {"params": hd, "lr": 5e-5}], lr=5e-5, weight_decay=0.01)
        losses = train_step(m, opt, b["img"].cuda(), b["word_ids"].cuda(), tgt)
        res.append((losses.clone(), {k: v.detach().clone() for k, v in m.state_dict().items()}))
        del m, opt
    assert torch.isfinite(res[0][0]).all()
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k


# ---------------------------------------------------------------------------------------------------------------- evaluation + trainer
def _pseudo_dir(root, size_hint=None):
    """synthetic pseudo masks for every train item of the mini dataset: two overlapping instances per ref"""
    from tris_amd.dataset.ReferDataset import ReferDataset
    from tris_amd.utils.synth import word_hash_tokenize
    ds = ReferDataset(root, "refcocog", "umd", split="train", eval_mode=False, size=64, tokenizer=word_hash_tokenize)
    d = os.path.join(root, "pseudo")
    os.makedirs(d, exist_ok=True)
    rng = np.random.RandomState(0)
    for i in range(len(ds)):
        _, img_id, rec = ds.image_record(i)
        h, w = rec["height"], rec["width"]
        mk = np.zeros((2, h, w), dtype=bool)
        y0, x0 = rng.randint(0, h // 2), rng.randint(0, w // 2)
        mk[0, y0:y0 + h // 2, x0:x0 + w // 2] = True
        mk[1, h // 4:, w // 4:] = True
        np.save(os.path.join(d, f"{i}_{img_id}.npy"), {"mask": mk}, allow_pickle=True)
    return d


def test_validate_groups_agree_and_match_the_restatement(tmp_path):
    """validate on a mini REFER set: TRIS_EVAL_GROUP 1 and 16 give the same (oIoU, mIoU, hit); the numbers agree with the fp32 CPU
    restatement of the model followed by validate.py:179-191 / isCorrectHit; save_cam writes the reference's names"""
    import json
    import oracle_stage2 as S
    from tris_amd.config import cfg
    from tris_amd.dataset.ReferDataset import ReferDataset
    from tris_amd.dataset.transform import get_transform
    from tris_amd.train_stage1 import build_loader
    from tris_amd.utils.synth import make_mini_refer, word_hash_tokenize
    from tris_amd.validate import validate
    root = make_mini_refer(str(tmp_path / "data"), n_images=6, seed=3)
    m, sd = _model(64)
    args = _args(64, ["--cam_save_dir", str(tmp_path / "cams"), "--name_save_dir", str(tmp_path / "names")])
    ds = ReferDataset(root, "refcocog", "umd", image_transforms=get_transform(64, False), split="val", eval_mode=True, size=64,
                      max_tokens=20, tokenizer=word_hash_tokenize)
    res = {}
    for grp in (1, 16):
        with cfg.override(eval_group=grp):
            res[grp] = validate(args, build_loader(args, ds, 1, False, False), m, 0, save_cam=(grp == 1))
    assert float(res[1][0]) == float(res[16][0]) and float(res[1][1]) == float(res[16][1]) and res[1][2] == res[16][2]
    # the restatement, sentence by sentence (the reference's loop)
    I_t = U_t = hits = n = 0
    ious, names = [], []
    for idx in range(len(ds)):
        smp, tg = ds[idx]
        tgt = (tg["target"].reshape(tg["target"].shape[-2:]) != 0).numpy().astype(np.uint8)
        for j in range(smp["word_ids"].shape[-1]):
            with torch.no_grad():
                out = S.forward({k: v.clone() for k, v in sd.items()}, smp["img"][None], smp["word_ids"][:, :, j], False)
            I, U, am = _np_signed_eval(out, tgt)
            y, x = divmod(am, tgt.shape[1])
            hits += int(any(b[0] <= x <= b[2] and b[1] <= y <= b[3] for b in np.asarray(tg["boxes"]).reshape(-1, 4)))
            I_t, U_t, n = I_t + I, U_t + U, n + 1
            ious.append(I / U if U else 0.0)
            names.append(f"{idx}_{j}_{tg['img_path']}")
    assert abs(float(res[1][0]) - 100 * I_t / U_t) < 0.5 and abs(float(res[1][1]) - 100 * np.mean(ious)) < 0.5
    assert abs(res[1][2] - 100 * hits / n) <= 100.0 / n + 1e-9
    assert sorted(os.listdir(str(tmp_path / "cams"))) == sorted(nm + ".npy" for nm in names)
    assert json.load(open(str(tmp_path / "names" / f"{args.dataset}_train_cam_name.json"))) == names


def test_script_level_main_trains_checkpoints_and_resumes(tmp_path):
    """python -m tris_amd.train_stage2 for one epoch on mini REFER with synthetic pseudo masks writes the checkpoints; --resume
    --pretrain <ckpt> --eval reloads it and reports the same mIoU.  Subprocesses under a time limit."""
    import ast
    import subprocess
    import sys
    from tris_amd.utils.synth import make_mini_refer, make_pseudo_masks
    root = make_mini_refer(str(tmp_path / "data"), n_images=8, seed=6)
    pseudo = make_pseudo_masks(root, str(tmp_path / "pseudo"))
    out = str(tmp_path / "out")
    argv = ["--refer_data_root", root, "--dataset", "refcocog", "--splitBy", "umd", "--size", "64", "--batch_size", "4",
            "--epoch", "1", "--test_split", "val", "--output", out, "--print-freq", "1", "--backbone", "clip-RN50",
            "--max_query_len", "20", "--pseudo_path", pseudo]
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TRIS_RANDOM_INIT="1")
    r = subprocess.run([sys.executable, "-m", "tris_amd.train_stage2"] + argv, cwd=repo, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    best = ast.literal_eval([ln for ln in r.stdout.splitlines() if ln.startswith("{'val_acc'")][-1])
    assert best["epoch"] == 0 and os.path.exists(best["path"]) and os.path.exists(best["hit_path"])
    assert os.path.basename(best["path"]) == "ckpt_320_epoch_0.pth" and os.path.basename(best["hit_path"]) == "ckpt_320_epoch_0_hit.pth"
    assert "Validat on the train split" in r.stdout
    ck = torch.load(best["path"], map_location="cpu")
    assert len(ck["model"]) == 625
    r2 = subprocess.run([sys.executable, "-m", "tris_amd.train_stage2"] + argv + ["--resume", "--eval", "--pretrain",
                        os.path.basename(best["path"])], cwd=repo, env=env, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr[-3000:]
    val = float([ln for ln in r2.stdout.splitlines() if ln.startswith("val: ")][-1].split(",")[0].split(":")[1])
    assert abs(val - best["val_acc"]) < 1e-3


def test_scheduler_steps_per_epoch_and_no_aux_clip(tmp_path, monkeypatch):
    """quirk 1: the poly LambdaLR counts iterations but is stepped once per EPOCH (train_stage2.py:133,192) -- epoch e trains at
    lr * (1 - e / (iters_per_epoch * epochs)) ** 0.9, the backbone group at lr * lr_multi times the same factor; quirk 7: the aux
    ViT-B/32 of train_stage2.py:170 is not loaded"""
    from tris_amd import train_stage2
    from tris_amd.CLIP import clip
    from tris_amd.args import get_parser
    from tris_amd.utils.synth import make_mini_refer, make_pseudo_masks, word_hash_tokenize
    root = make_mini_refer(str(tmp_path / "data"), n_images=8, seed=6)
    pseudo = make_pseudo_masks(root, str(tmp_path / "pseudo"))
    seen, loaded = [], []
    real_load = clip.load

    def load(name, *a, **k):
        loaded.append(name)
        return real_load(name, *a, **k)

    def fake_epoch(train_loader, model, optimizer, epoch, local_rank, args, iteration=0, clip_model=None, model_ema=None):
        seen.append((epoch, len(train_loader), [g["lr"] for g in optimizer.param_groups]))
        return iteration + len(train_loader)
    monkeypatch.setattr(clip, "load", load)
    monkeypatch.setattr(train_stage2, "train_one_epoch", fake_epoch)
    args = get_parser().parse_args(["--refer_data_root", root, "--dataset", "refcocog", "--splitBy", "umd", "--size", "64",
                                    "--batch_size", "2", "--epoch", "3", "--test_split", "val", "--output", str(tmp_path / "out"),
                                    "--backbone", "clip-RN50", "--max_query_len", "20", "--pseudo_path", pseudo, "--lr", "1e-3",
                                    "--lr_multi", "0.1"])
    train_stage2.main(args, tokenizer=word_hash_tokenize)
    assert [e for e, _, _ in seen] == [0, 1, 2]
    n_it = seen[0][1]
    assert n_it > 1
    for e, _, lrs in seen:
        f = (1 - e / (n_it * 3)) ** 0.9
        assert abs(lrs[0] - 1e-3 * 0.1 * f) < 1e-12 and abs(lrs[1] - 1e-3 * f) < 1e-12, (e, lrs)
    assert seen[1][2][1] > 1e-3 * (1 - 1 / 3) ** 0.9        # per iteration it would have decayed this far in one epoch
    assert loaded and all("ViT" not in str(nm) for nm in loaded), loaded


def test_criterion_and_shape_contracts():
    """criterion takes any target dtype (the reference's target.float()); the upsample refuses to shrink; non-square maps are
    refused by the signed evaluation"""
    from tris_amd import ops
    from tris_amd.model.model_stage2 import criterion
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 1, 16, 24, generator=g)
    t = torch.randint(0, 3, (2, 1, 16, 24), generator=g)
    want = F.binary_cross_entropy_with_logits(x.double(), t.double())
    for tt in (t, t.float(), t.to(torch.uint8), t.float() * 0.5):
        w = F.binary_cross_entropy_with_logits(x.double(), tt.double())
        xd = x.cuda().requires_grad_()
        got = criterion(xd, tt.cuda())
        got.backward()
        xr = x.double().requires_grad_()
        F.binary_cross_entropy_with_logits(xr, tt.double()).backward()
        assert got.dim() == 0 and abs(float(got) - float(w)) < 1e-6 and _rel(xd.grad, xr.grad) < 1e-5
    assert abs(float(criterion(x.cuda(), t.cuda())) - float(want)) < 1e-6
    with pytest.raises(ValueError):
        ops.upsample_nhwc(torch.randn(1, 8, 8, 32, device="cuda"), (4, 8))
    with pytest.raises(ValueError):
        ops.eval_post_signed(torch.randn(1, 1, 8, 12, device="cuda"), torch.zeros(8, 12, dtype=torch.uint8, device="cuda"))


def test_non_square_input_gives_image_sized_maps():
    """img_size = x.shape[2:] (model_stage2.py:106): a 64 x 96 input gives 64 x 96 maps"""
    m, _ = _model(64)
    from tris_amd.utils.synth import synthetic_batch
    b = synthetic_batch(2, 64, 20, 0, seed=3)
    img = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(1)).cuda()
    m.train()
    outs = m(img, b["word_ids"].cuda())
    assert all(tuple(o.shape) == (2, 1, 64, 96) for o in outs)
    m.eval()
    with torch.no_grad():
        assert tuple(m(img, b["word_ids"].cuda()).shape) == (2, 1, 64, 96)


def test_conv_epilogue_statistics_into_bn_prelu_at_reduced_c4():
    """reduced_c4's shape (2048 -> 512 at 10 x 10, B = 2): conv3x3 with the BatchNorm statistics in its epilogue (_bn_part ->
    tris_bn_finalize_f32) feeding bn_prelu, forward and backward -- the slope gradient included -- against fp64 torch"""
    from tris_amd import ops
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 10, 10, 2048, generator=g)
    w = (torch.randn(512, 2048, 3, 3, generator=g) / (3 * 2048 ** 0.5)).contiguous(memory_format=torch.channels_last)
    gamma, beta = 1 + 0.1 * torch.randn(512, generator=g), 0.1 * torch.randn(512, generator=g)
    a = torch.tensor([0.27])
    dy = torch.randn(2, 10, 10, 512, generator=g)
    ref = [t.double().requires_grad_() for t in (x, w, gamma, beta, a)]
    rm, rv = torch.zeros(512, dtype=torch.float64), torch.ones(512, dtype=torch.float64)
    z = F.batch_norm(F.conv2d(ref[0].permute(0, 3, 1, 2), ref[1], padding=1), rm, rv, ref[2], ref[3], True, 0.1, 1e-5)
    F.prelu(z, ref[4]).permute(0, 2, 3, 1).backward(dy.double())
    xd = x.cuda().requires_grad_()
    wd, gd, bd, ad = (torch.nn.Parameter(t.cuda()) for t in (w, gamma, beta, a))
    y = ops.conv3x3(xd, wd, 1, stats=True)
    assert getattr(y, "_bn_part", None) is not None          # the epilogue statistics path is the one under test
    rmd, rvd = torch.zeros(512, device="cuda"), torch.ones(512, device="cuda")
    out = ops.bn_prelu(y, gd, bd, rmd, rvd, ad, True)
    out.backward(dy.cuda())
    # (the running mean is 0.1 x the channel means of the product, small against its values: the product's own 1e-4 bound)
    assert _rel(rmd, rm) < 1e-4 and _rel(rvd, rv) < 1e-4
    for d, r in zip((xd, wd, gd, bd, ad), ref):
        assert _rel(d.grad, r.grad) < 1e-4, (tuple(r.shape), _rel(d.grad, r.grad))
