"""The IRNet edge / displacement network on the MI355X (csrc/irnnet.hip, tris_amd/irn_net.py): every new kernel against fp64 torch
and for bitwise repeatability, the existing product paths on the odd shapes the network brings, the whole network on the recorded
images against the fp64 restatement (tests/oracle_irn.py) within 8x the reference's own fp32 error, determinism across image
sizes, and the command line from images to instance-mask files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

import oracle_irn as O

pytestmark = pytest.mark.gpu
U = 2.0 ** -24          # unit roundoff of fp32


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
    return float((a - b).abs().max() / b.abs().max())


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _twice(fn):
    """run a launch twice: the results are bitwise equal; returns the first"""
    a, b = fn(), fn()
    assert torch.equal(a, b)
    return a


# ------------------------------------------------------------------------------------------------------------- new kernels
@pytest.mark.parametrize("H,W", [(65, 97), (72, 50), (64, 96), (33, 35)])
def test_stem(H, W):
    """uint8 -> table -> [img, flip] -> 7x7 s2 p3 -> frozen BatchNorm -> ReLU.  Bound: an fp32 FMA chain of K = 147 terms plus the
    eight roundings of the epilogue is within (K + 8) u of sum |x||w| scaled by the BatchNorm (standard forward bound, u = 2^-24)."""
    from tris_amd import ops
    from tris_amd.irn_net import normalize_table
    from tris_amd.utils.synth import irn_image
    g = torch.Generator().manual_seed(H * W)
    img = irn_image(H, W, seed=H + W)
    w = torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5
    mean, var = 0.1 * torch.randn(64, generator=g), 1 + 0.1 * torch.rand(64, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(64, generator=g), 0.1 * torch.randn(64, generator=g)
    invstd = (1.0 / torch.sqrt(var.double() + 1e-5)).float()
    x = O.batch_of(img).double()
    sc = (invstd.double() * gamma.double()).view(1, -1, 1, 1)
    pre = F.conv2d(x, w.double(), stride=2, padding=3)
    ref = F.relu((pre - mean.double().view(1, -1, 1, 1)) * sc + beta.double().view(1, -1, 1, 1))
    amp = (F.conv2d(x.abs(), w.double().abs(), stride=2, padding=3) + mean.double().abs().view(1, -1, 1, 1)) * sc.abs() \
        + beta.double().abs().view(1, -1, 1, 1)
    d = lambda t: t.cuda()
    args = (d(torch.from_numpy(img)), d(normalize_table()), d(w.permute(2, 3, 1, 0).contiguous()), d(mean), d(invstd), d(gamma), d(beta))
    y = _twice(lambda: ops.irn_stem(*args))
    assert tuple(y.shape) == (2, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64)
    err = (_nchw(y).double().cpu() - ref).abs()
    print(f"stem {H}x{W}: max err / bound = {float((err / ((147 + 8) * U * amp)).max()):.3f}, rel {_rel(_nchw(y), ref):.2e}")
    assert bool((err <= (147 + 8) * U * amp).all())


@pytest.mark.parametrize("B,H,W,C", [(2, 33, 49, 64), (2, 36, 25, 64), (2, 32, 48, 64), (1, 5, 7, 8)])
def test_maxpool_and_subsample(B, H, W, C):
    """exact operations: bitwise against torch (a padded tap never wins: the inputs are all negative)"""
    from tris_amd import ops
    g = torch.Generator().manual_seed(B * H * W)
    x = -torch.rand(B, H, W, C, generator=g) - 0.5
    y = _twice(lambda: ops.maxpool3s2(x.cuda()))
    assert torch.equal(_nchw(y).cpu(), F.max_pool2d(_nchw(x), 3, 2, 1))
    s = _twice(lambda: ops.subsample2(x.cuda()))
    assert torch.equal(s.cpu(), x[:, ::2, ::2, :])


GN_SHAPES = [(32, 4), (64, 8), (128, 16), (256, 16)]


@pytest.mark.parametrize("C,G", GN_SHAPES)
@pytest.mark.parametrize("h,w", [(17, 25), (18, 13), (5, 7), (120, 160)])
def test_group_norm(C, G, h, w):
    """statistics (fixed-order fp64 sums, stored as fp32: one rounding, 2 u relative for invstd through the division) and the apply with
    and without ReLU.  Apply bound: four fp32 roundings on magnitudes up to |x - mean| invstd |gamma| + |beta|, plus the roundings of the
    stored fp32 mean and invstd, which act on |mean| invstd |gamma| too: 8 u of (|x - mean| + |mean|) invstd |gamma| + |beta|."""
    from tris_amd import ops
    g = torch.Generator().manual_seed(C + h * w)
    x = torch.randn(2, h, w, C, generator=g) * (1 + torch.rand(1, 1, 1, C, generator=g)) + torch.randn(1, 1, 1, C, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    xd = _nchw(x).double()
    xg = xd.reshape(2, G, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    st = _twice(lambda: ops.group_norm_stats(x.cuda(), G))
    assert _rel(st[..., 0], mean) <= 2 * U + 1e-12 and float(((st[..., 1].double().cpu() * torch.sqrt(var + 1e-5)) - 1).abs().max()) <= 2 * U
    for relu in (False, True):
        ref = F.group_norm(xd, G, gamma.double(), beta.double(), 1e-5)
        ref = F.relu(ref) if relu else ref
        y = _twice(lambda: ops.gn_apply_up(x.cuda(), st, gamma.cuda(), beta.cuda(), G, relu=relu))
        mu_c = mean.repeat_interleave(C // G, 1).view(2, C, 1, 1)
        is_c = (1 / torch.sqrt(var + 1e-5)).repeat_interleave(C // G, 1).view(2, C, 1, 1)
        amp = ((xd - mu_c).abs() + mu_c.abs()) * is_c * gamma.double().abs().view(1, C, 1, 1) + beta.double().abs().view(1, C, 1, 1)
        err = (_nchw(y).double().cpu() - ref).abs()
        print(f"gn C{C} G{G} {h}x{w} relu={relu}: max err / bound {float((err / (8 * U * amp)).max()):.3f}")
        assert bool((err <= 8 * U * amp).all())


@pytest.mark.parametrize("C,G,scale,hi,wi,ho,wo", [(32, 4, 2, 9, 13, 17, 25), (32, 4, 4, 5, 7, 17, 25), (256, 16, 2, 5, 7, 9, 13),
                                                   (256, 16, 2, 9, 7, 18, 13), (32, 4, 4, 4, 6, 16, 24), (256, 16, 2, 30, 40, 60, 80)])
def test_gn_upsample_crop_relu_slice(C, G, scale, hi, wi, ho, wo):
    """GroupNorm -> bilinear x scale -> crop -> ReLU -> channel slice of a wider buffer, against the unfused fp64 composition; the
    rest of the buffer is untouched.  Bound: the apply's 8 u plus the six roundings of the two-level blend, 14 u of the largest
    normalised magnitude among the four corners (bounded here by the map's maximum, plus |mean| invstd |gamma| for the rounding of
    the stored mean)."""
    from tris_amd import ops
    g = torch.Generator().manual_seed(C * scale + hi * wi)
    x = torch.randn(2, hi, wi, C, generator=g) * 2 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    n = F.group_norm(_nchw(x).double(), G, gamma.double(), beta.double(), 1e-5)
    ref = F.relu(F.interpolate(n, scale_factor=scale, mode="bilinear", align_corners=False)[..., :ho, :wo])
    Ct, off = C + 64, 32
    st = ops.group_norm_stats(x.cuda(), G)

    def run():
        out = torch.full((2, ho, wo, Ct), -7.0, device="cuda")
        ops.gn_apply_up(x.cuda(), st, gamma.cuda(), beta.cuda(), G, scale, (ho, wo), True, out, off)
        return out
    out = _twice(run).cpu()
    assert bool((out[..., :off] == -7).all()) and bool((out[..., off + C:] == -7).all())
    err = float((_nchw(out[..., off:off + C]).double() - ref).abs().max())
    xg = _nchw(x).double().reshape(2, G, -1)
    mag = float(n.abs().max()) + float((xg.mean(-1).abs() / torch.sqrt(xg.var(-1, unbiased=False) + 1e-5)).max() * gamma.abs().max())
    print(f"gn+up C{C} x{scale} {hi}x{wi}->{ho}x{wo}: err {err:.3e}, bound {14 * U * mag:.3e}")
    assert err <= 14 * U * mag
    # without a norm the blend is the library's: bit for bit the existing NHWC upsample, cropped
    up = ops.upsample_nhwc(x.cuda(), (hi * scale, wi * scale))
    plain = ops.gn_apply_up(x.cuda(), None, None, None, G, scale, (ho, wo), False)
    assert torch.equal(plain, up[:, :ho, :wo, :].contiguous())


@pytest.mark.parametrize("C,N", [(160, 1), (256, 2)])
@pytest.mark.parametrize("h,w", [(17, 25), (120, 160)])
def test_narrow_heads(C, N, h, w):
    """bound: (C + 1) u sum |x||w| + |b| for an fp32 sum of C products and the bias add"""
    from tris_amd import ops
    g = torch.Generator().manual_seed(C + h)
    x = torch.randn(2, h, w, C, generator=g)
    wt, b = torch.randn(N, C, generator=g) / C ** 0.5, torch.randn(N, generator=g)
    ref = x.double() @ wt.double().t() + b.double()
    amp = x.double().abs() @ wt.double().abs().t() + b.double().abs()
    y = _twice(lambda: ops.irn_head(x.cuda(), wt.cuda(), b.cuda()))
    err = (y.double().cpu() - ref).abs()
    print(f"head C{C} N{N}: max err / bound {float((err / ((C + 1) * U * amp)).max()):.3f}")
    assert tuple(y.shape) == (2, h, w, N) and bool((err <= (C + 1) * U * amp).all())


@pytest.mark.parametrize("h,w", [(17, 25), (18, 13), (120, 160)])
def test_flip_average_sigmoid(h, w):
    """dp is a copy (exact).  edge: z has two roundings (|z| u each), the sigmoid's slope is at most 1/4, expf and the division are
    within a few u of a value below 1: 1e-6 absolute for |z| <= 10."""
    from tris_amd import ops
    g = torch.Generator().manual_seed(h * w)
    e, dpo = torch.randn(2, h, w, generator=g) * 3, torch.randn(2, h, w, 2, generator=g)
    r = _twice(lambda: torch.cat([t.reshape(-1) for t in ops.irn_net_finish(e.cuda(), dpo.cuda())]))
    edge, dp = ops.irn_net_finish(e.cuda(), dpo.cuda())
    assert r.numel() == 3 * h * w and torch.equal(dp.cpu(), dpo[0].permute(2, 0, 1))
    ref = torch.sigmoid(e[0].double() / 2 + e[1].double().flip(-1) / 2)
    assert float((edge.double().cpu() - ref).abs().max()) <= 1e-6


# ------------------------------------------------------------------------------------------ existing product paths, new shapes
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C,H,W", [(64, 17, 25), (128, 17, 25), (128, 9, 13), (256, 9, 13), (256, 9, 7), (512, 5, 7), (128, 18, 13)])
def test_conv3x3_forward_on_odd_maps(stride, C, H, W):
    """ops.conv3x3 forward at the trunk's channel counts, B = 2, odd H and W, stride 1 and 2, against fp64: the 1e-4 of the largest
    magnitude that tests/test_gpu_stage2.py::test_decoder_conv_shapes holds the same kernels to"""
    from tris_amd import ops
    g = torch.Generator().manual_seed(C + H * W + stride)
    x = torch.randn(2, H, W, C, generator=g)
    w = (torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5)).contiguous(memory_format=torch.channels_last)
    ref = F.conv2d(_nchw(x).double(), w.double(), stride=stride, padding=1)
    wp = torch.nn.Parameter(w.cuda(), requires_grad=False)
    with torch.no_grad(), ops.autotune_off():
        y = _twice(lambda: ops.conv3x3(x.cuda(), wp, stride))
    r = _rel(_nchw(y), ref)
    print(f"conv3x3 C{C} {H}x{W} s{stride}: {r:.2e}")
    assert tuple(_nchw(y).shape) == tuple(ref.shape) and r < 1e-4


@pytest.mark.parametrize("cin,cout,H,W", [(256, 512, 17, 25), (512, 1024, 9, 13), (256, 512, 18, 13), (64, 256, 17, 25)])
def test_strided_1x1_downsample(cin, cout, H, W):
    """the downsample convolution: row subsample + the existing product, against fp64 conv2d(stride=2) (stride 1 for layer1)"""
    from tris_amd import ops
    stride = 1 if cin == 64 else 2
    g = torch.Generator().manual_seed(cin + H)
    x = torch.randn(2, H, W, cin, generator=g)
    w = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    ref = F.conv2d(_nchw(x).double(), w.double(), stride=stride)
    wp = torch.nn.Parameter(w.cuda(), requires_grad=False)
    with torch.no_grad(), ops.autotune_off():
        y = _twice(lambda: ops.linear(ops.subsample2(x.cuda()) if stride == 2 else x.cuda(), wp))
    r = _rel(_nchw(y), ref)
    print(f"1x1 s{stride} {cin}->{cout} {H}x{W}: {r:.2e}")
    assert r < 1e-4


# ------------------------------------------------------------------------------------------------------------ the network
@pytest.fixture(scope="module")
def g15(golden):
    return golden("g15_irn_net.npz")


@pytest.fixture(scope="module")
def net(g15):
    from tris_amd.irn_net import EdgeDisplacement
    m = EdgeDisplacement()
    O.filled_state_dict(int(g15["seed"]), float(g15["gain"]), m)
    return m.cuda()


@pytest.fixture(scope="module")
def oracle64(g15):
    """the fp64 restatement on the recorded images"""
    sd = O.filled_state_dict(int(g15["seed"]), float(g15["gain"]))
    torch.set_num_threads(16)
    return [O.forward(sd, O.batch_of(img), torch.float64) for img in O.images()]


def test_network_against_fp64(net, g15, oracle64, arith):
    """edge_out, dp_out, edge and dp of the three recorded images: the GPU result lies within 8 e_ref of the fp64 restatement, where
    e_ref = max |recorded fp32 - fp64| / max |fp64| is the reference's own fp32 error on that tensor (the margin of
    tests/test_gpu_stage2.py for a GPU fp32-class run against an fp32 CPU run).  The taps are printed for diagnosis."""
    worst = 0.0
    for i, img in enumerate(O.images()):
        out = net.forward_raw(img, taps=True)
        ref = oracle64[i]
        got = {"edge_out": out["edge_out"][:, None], "dp_out": _nchw(out["dp_out"]), "edge": out["edge"][None], "dp": out["dp"]}
        for k in range(5):
            print(f"[{arith}] image {i} x{k + 1}: gpu {_rel(_nchw(out['taps'][k]), ref['taps'][k]):.3e}")
        for name in ("edge_out", "dp_out", "edge", "dp"):
            r64 = ref[name].numpy()
            e_ref = float(np.abs(g15[f"i{i}_{name}"].astype(np.float64) - r64).max() / np.abs(r64).max())
            e_gpu = _rel(got[name], ref[name])
            worst = max(worst, e_gpu / e_ref)
            print(f"[{arith}] image {i} {name}: e_ref {e_ref:.3e}, gpu {e_gpu:.3e}, ratio {e_gpu / e_ref:.2f}")
            assert tuple(got[name].shape) == r64.shape
            assert e_gpu <= 8 * e_ref, (arith, i, name, e_gpu, e_ref)
    print(f"[{arith}] worst ratio {worst:.2f}")


def test_network_is_deterministic(net):
    imgs = O.images()
    e0, d0 = net(imgs[0])
    e1, d1 = net(imgs[0])
    assert torch.equal(e0, e1) and torch.equal(d0, d1)
    net(imgs[1])                     # another size, grey
    net(torch.from_numpy(imgs[2]).cuda())
    e2, d2 = net(imgs[0])
    assert torch.equal(e0, e2) and torch.equal(d0, d2)
    assert e0.dtype == d0.dtype == torch.float32 and e0.is_cuda and tuple(d0.shape) == (2,) + tuple(e0.shape)
    h, w = e0.shape
    assert (h, w) == ((imgs[0].shape[0] - 1) // 4 + 1, (imgs[0].shape[1] - 1) // 4 + 1)


def test_command_line_from_images(net, g15, tmp_path, arith):
    """python -m tris_amd.make_ins_seg --irn_weights_name ... --voc12_root ...: two Pillow-written images, three names of which two
    share the first image.  One file per name with the reference's keys, each equal array for array to irn.make_ins_seg on that
    image's (edge, dp) from EdgeDisplacement.forward in this process; the two names that share an image cost one network pass."""
    from PIL import Image
    from tris_amd import irn
    from tris_amd.make_ins_seg import image_file, load_image
    from tris_amd.utils.synth import irn_image
    root, D, Odir = tmp_path / "train2014", tmp_path / "cam", tmp_path / "out"
    root.mkdir(), D.mkdir()
    ids = {"0_17": 17, "1_17": 17, "2_40": 40}
    pix = {17: irn_image(70, 93, seed=1), 40: irn_image(64, 80, seed=2, grey=True)}
    for k, a in pix.items():
        Image.fromarray(a).save(root / ("COCO_train2014_%012d.jpg" % k), format="JPEG", quality=95)
    rng = np.random.RandomState(3)
    cams = {}
    for name, k in ids.items():
        H, W = pix[k].shape[:2]
        low = rng.rand((H - 1) // 4 + 1, (W - 1) // 4 + 1).astype(np.float32)
        cams[name] = np.repeat(np.repeat(low, 4, 0), 4, 1)[:H, :W].copy()
        np.save(D / (name + ".npy"), cams[name])
    with open(tmp_path / "names.json", "w") as f:
        json.dump(list(ids), f)
    torch.save({k: v.cpu() for k, v in net.state_dict().items()}, tmp_path / "irn.pth")
    env = dict(os.environ, TRIS_GEMM_MODE=arith, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "tris_amd.make_ins_seg", "--cam_out_dir", str(D), "--irn_weights_name",
                        str(tmp_path / "irn.pth"), "--voc12_root", str(root), "--ins_seg_out_dir", str(Odir), "--train_list",
                        str(tmp_path / "names.json")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr[-2000:])
    assert p.returncode == 0
    assert "edge / displacement network: 2 passes for 3 names" in p.stdout
    calls = net.calls
    for name, k in ids.items():
        got = np.load(Odir / (name + ".npy"), allow_pickle=True).item()
        assert sorted(got) == ["cam", "class", "mask", "score"]
        img = load_image(image_file(name, str(root)))
        assert img.shape == pix[k].shape[:2] + (3,)
        edge, dp = net(img)
        want = irn.make_ins_seg(cams[name], edge, dp, img.shape[:2])
        for key in want:
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (name, key)
        assert got["mask"].dtype == bool and got["mask"].shape[1:] == img.shape[:2]
    assert net.calls == calls + 3
