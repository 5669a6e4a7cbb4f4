"""Stage-2 fed from the HBM loader: tris_mask_sum_nearest_u8 against Pillow bit for bit, the `pseudo_gt` batch key against
ReferDataset.load_pseudo, the absent / evaluation / broken-file cases, one Stage-2 step from either loader, image sharing between
two caches of one split, and the script-level trainer under both values of TRIS_HBM_LOADER."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

KW = dict(dataset="refcocog", splitBy="umd", max_tokens=20)


def _dataset(root, size, split="train", eval_mode=False, pseudo_path=None):
    from tris_amd.dataset.ReferDataset import ReferDataset
    from tris_amd.dataset.transform import get_transform
    from tris_amd.utils.synth import word_hash_tokenize
    return ReferDataset(refer_data_root=root, image_transforms=get_transform(size, not eval_mode), split=split, eval_mode=eval_mode,
                        size=size, pseudo_path=pseudo_path, tokenizer=word_hash_tokenize, **KW)


def _mini(tmp_path, size):
    """the two datasets of the loader tests: 9 small images at 32 px, 6 images of up to 500 px at the network's 320 px"""
    from tris_amd.utils.synth import make_mini_refer, make_pseudo_masks
    if size == 32:
        root = make_mini_refer(str(tmp_path / "data"), n_images=9, seed=4, max_side=72)
    else:
        root = make_mini_refer(str(tmp_path / "data"), n_images=6, seed=4, max_side=500)
    return root, make_pseudo_masks(root, str(tmp_path / "pseudo"))


def _same(a, b, path=""):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape, (path, a.dtype, b.dtype, a.shape, b.shape)
        assert torch.equal(a.cpu(), b.cpu()), path
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), (path, a.keys(), b.keys())
        for k in a:
            _same(a[k], b[k], path + "/" + str(k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    else:
        assert a == b, (path, a, b)


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
def _pillow(m, out_h, out_w):
    """the reference's own expression (dataset/ReferDataset.py:184-186)"""
    return np.asarray(Image.fromarray((m * 1.0).sum(0)).resize((out_w, out_h), Image.NEAREST))


@pytest.mark.parametrize("K,h,w,S", [(1, 37, 53, 16), (2, 53, 37, 16), (3, 20, 31, 64), (0, 9, 12, 8), (2, 64, 64, 64), (3, 1, 9, 8),
                                     (2, 427, 640, 320), (255, 3, 5, 4)])
def test_mask_sum_nearest_u8_equals_pillow(K, h, w, S):
    from tris_amd import ops
    rng = np.random.default_rng(1000 * K + h)
    m = np.ones((K, h, w), bool) if K == 255 else rng.random((K, h, w)) < 0.4
    dev = torch.from_numpy(m.view(np.uint8)).cuda()
    for out_h, out_w in ((S, S), (16, 24)):
        want = _pillow(m, out_h, out_w)
        got = ops.mask_sum_nearest_u8(dev, out_h, out_w)
        again = ops.mask_sum_nearest_u8(dev, out_h, out_w)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (out_h, out_w)
        assert np.array_equal(got.cpu().numpy(), want), (K, h, w, out_h, out_w)
        assert torch.equal(got, again)
    if K == 255:
        assert int(got.min()) == 255        # every pixel the full count: no wrap
    if K == 3 and S == 64:
        assert int(_pillow(m, S, S).max()) == 3
    # into a row of a larger buffer (what the cache does), neighbours untouched
    buf = torch.full((3, S, S), 7, dtype=torch.uint8, device="cuda")
    ops.mask_sum_nearest_u8(dev, S, S, out=buf[1])
    assert np.array_equal(buf[1].cpu().numpy(), _pillow(m, S, S)) and bool((buf[0] == 7).all()) and bool((buf[2] == 7).all())


# ---------------------------------------------------------------------------------------------------------------- 2. the loader
@pytest.mark.parametrize("size", [32, 320])
def test_pseudo_gt_equals_load_pseudo_and_other_keys_are_unchanged(tmp_path, size):
    from tris_amd.dataset.hbm import HbmLoader, HbmReferCache
    root, pseudo = _mini(tmp_path, size)
    ds = _dataset(root, size, pseudo_path=pseudo)
    plain = _dataset(root, size)
    cache, pcache = HbmReferCache(ds, size), HbmReferCache(plain, size)
    assert cache.pseudo.dtype == torch.uint8 and tuple(cache.pseudo.shape) == (len(ds), size, size)
    assert cache.nbytes() == pcache.nbytes() + len(ds) * size * size
    np.random.seed(5)
    got = list(HbmLoader(cache, batch_size=4))
    np.random.seed(5)
    base = list(HbmLoader(pcache, batch_size=4))
    assert len(got) == len(base) == (len(ds) + 3) // 4 and len(ds) % 4 != 0     # (a ragged last batch is part of the case)
    seen = set()
    for b, ((gs, gt), (bs, bt)) in enumerate(zip(got, base)):
        idx = list(range(4 * b, min(4 * b + 4, len(ds))))
        pg = gt.pop("pseudo_gt")
        assert pg.dtype == torch.int64 and tuple(pg.shape) == (len(idx), 1, size, size) and pg.is_cuda
        assert torch.equal(pg.cpu(), torch.stack([ds.load_pseudo(i) for i in idx]))
        seen |= set(torch.unique(pg).tolist())
        _same(gs, bs, "samples")
        _same(gt, bt, "targets")
    assert seen == {0, 1, 2}


# ---------------------------------------------------------------------------------------------------------------- 3. absent, eval, broken
def test_no_pseudo_path_eval_mode_and_broken_files(tmp_path):
    from tris_amd.dataset.hbm import HbmLoader, HbmReferCache
    root, pseudo = _mini(tmp_path, 32)
    S = 32
    plain = _dataset(root, S)
    c = HbmReferCache(plain, S)
    assert c.pseudo is None
    assert c.nbytes() == c.images.numel() + c.tokens.numel() * c.tokens.element_size() + c.targets.numel()
    assert all("pseudo_gt" not in t for _, t in HbmLoader(c, batch_size=4))
    # an evaluation dataset handed the train-only directory (validate.py:64) reads no file
    ev = _dataset(root, S, split="val", eval_mode=True, pseudo_path=pseudo)
    ec = HbmReferCache(ev, S)
    assert ec.pseudo is None and len(ev) > 0
    assert all("pseudo_gt" not in t for _, t in HbmLoader(ec, batch_size=1))
    # a missing file is found when the cache is built, not mid-epoch
    ds = _dataset(root, S, pseudo_path=pseudo)
    name = f"3_{ds.image_record(3)[1]}.npy"
    keep = open(os.path.join(pseudo, name), "rb").read()
    os.remove(os.path.join(pseudo, name))
    with pytest.raises(FileNotFoundError, match=name.replace(".", r"\.")):
        HbmReferCache(ds, S)
    # a stack that is not bool (a writer that summed or cast it) is refused by name
    m = np.load(__import__("io").BytesIO(keep), allow_pickle=True).item()["mask"]
    np.save(os.path.join(pseudo, name), {"mask": m.astype(np.uint8)}, allow_pickle=True)
    with pytest.raises(TypeError, match=name.replace(".", r"\.")):
        HbmReferCache(ds, S)
    np.save(os.path.join(pseudo, name), {"mask": m}, allow_pickle=True)
    assert HbmReferCache(ds, S).pseudo is not None


# ---------------------------------------------------------------------------------------------------------------- 4. one step
@pytest.mark.parametrize("mode", ["h2", "x3"])
def test_stage2_step_from_hbm_batch_equals_dataloader_batch(tmp_path, mode):
    """train_stage2.train_step on the loader's channels-last batch and on the DataLoader-collated NCHW batch of the same two refs,
    each from a freshly seed-filled model: the five losses are bitwise equal (the bar of
    test_gpu_data.py::test_train_step_from_hbm_batch_equals_planar_batch)"""
    import warnings
    from torch.utils.data import default_collate
    from tris_amd import ops
    from tris_amd.args import get_parser
    from tris_amd.dataset.hbm import HbmLoader, HbmReferCache
    from tris_amd.model.model_stage2 import TRIS
    from tris_amd.optim import FusedAdamW
    from tris_amd.train_stage2 import train_step
    from tris_amd.utils.synth import make_mini_refer, make_pseudo_masks, seed_fill
    root = make_mini_refer(str(tmp_path / "data"), n_images=6, seed=2)
    pseudo = make_pseudo_masks(root, str(tmp_path / "pseudo"))
    ds = _dataset(root, 64, pseudo_path=pseudo)
    np.random.seed(0)
    hs, ht = next(iter(HbmLoader(HbmReferCache(ds, 64), batch_size=2)))
    np.random.seed(0)
    ds_s, ds_t = default_collate([ds[0], ds[1]])
    assert torch.equal(hs["img"].cpu(), ds_s["img"]) and torch.equal(ht["pseudo_gt"].cpu(), ds_t["pseudo_gt"])
    assert torch.equal(hs["word_ids"].cpu(), ds_s["word_ids"])
    args = get_parser().parse_args(["--backbone", "clip-RN50", "--size", "64", "--max_query_len", "20", "--batch_size", "2"])
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(mode)
    try:
        losses = []
        for samples, targets in ((hs, ht), (ds_s, ds_t)):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                model = TRIS(args).cuda()
            seed_fill(model.state_dict(), 1234)
            model.train()
            bb, hd = model.trainable_parameters()
            opt = FusedAdamW([{"params": bb, "lr": 5e-6}, {"params": hd, "lr": 5e-5}], lr=5e-5, weight_decay=0.01)
            losses.append(train_step(model, opt, samples["img"].cuda(), samples["word_ids"].squeeze(1).cuda(),
                                     targets["pseudo_gt"].cuda()).clone())
            del model, opt
    finally:
        ops.set_gemm_mode(prev)
    assert losses[0].shape == (5,) and bool(torch.isfinite(losses[0]).all())
    assert torch.equal(losses[0], losses[1]), (losses[0].tolist(), losses[1].tolist())


# ---------------------------------------------------------------------------------------------------------------- 5. image sharing
def test_images_from_shares_the_decoded_split(tmp_path):
    from tris_amd.dataset.hbm import HbmLoader, HbmReferCache
    root, pseudo = _mini(tmp_path, 320)
    S = 320
    train = HbmReferCache(_dataset(root, S, pseudo_path=pseudo), S)
    ev = _dataset(root, S, split="train", eval_mode=True)
    calls = []
    real = ev.load_image
    ev.load_image = lambda i: (calls.append(i), real(i))[1]
    shared = HbmReferCache(ev, S, images_from=train)
    assert calls == [] and shared.images.data_ptr() == train.images.data_ptr()
    assert shared.nbytes() == shared.tokens.numel() * shared.tokens.element_size() + sum(m.numel() for m in shared.eval_targets)
    own = HbmReferCache(ev, S)
    assert len(calls) == train.images.shape[0] and own.images.data_ptr() != train.images.data_ptr()
    a, b = HbmLoader(shared, batch_size=1), HbmLoader(own, batch_size=1)
    for i in range(len(ev)):
        (gs, gt), (rs, rt) = a.eval_batch(i), b.eval_batch(i)
        assert torch.equal(gs["img"], rs["img"])
        _same(gs, rs, "samples")
        _same(gt, rt, "targets")
    # the val split holds one image no train ref has: decoded once, into a private tensor behind the donor's rows
    val = _dataset(root, S, split="val", eval_mode=True)
    held = set(train.slot_by_img)
    lacking = [i for i in range(len(val)) if val.image_record(i)[1] not in held]
    assert 0 < len(lacking) < len(val)
    vcalls = []
    vreal = val.load_image
    val.load_image = lambda i: (vcalls.append(i), vreal(i))[1]
    mixed = HbmReferCache(val, S, images_from=train)
    first = {}
    for i in lacking:
        first.setdefault(val.image_record(i)[1], i)
    assert sorted(vcalls) == sorted(first.values())         # one decode per image the donor lacks, none for the others
    assert mixed.images.data_ptr() != train.images.data_ptr() and mixed.images.shape[0] == train.images.shape[0] + len(vcalls)
    vown = HbmReferCache(val, S)
    for i in range(len(val)):
        (gs, gt), (rs, rt) = HbmLoader(mixed, batch_size=1).eval_batch(i), HbmLoader(vown, batch_size=1).eval_batch(i)
        _same(gs, rs, "samples")
        _same(gt, rt, "targets")
    # the donor is left as it was
    assert train.images.shape[0] == len(held) and set(train.slot_by_img) == held
    with pytest.raises(ValueError):
        HbmReferCache(val, 64, images_from=train)


# ---------------------------------------------------------------------------------------------------------------- 6. the script
def test_script_level_trains_from_either_loader(tmp_path):
    """python -m tris_amd.train_stage2 for one epoch at 64 px: from the HBM loader by default, from the DataLoader under
    TRIS_HBM_LOADER=0.  Two subprocesses, each under its own time limit, the second only after the first has passed."""
    import ast
    import math
    import re
    import subprocess
    import sys
    from tris_amd.utils.synth import make_mini_refer, make_pseudo_masks
    root = make_mini_refer(str(tmp_path / "data"), n_images=8, seed=6)
    pseudo = make_pseudo_masks(root, str(tmp_path / "pseudo"))
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for hbm, loader in (("1", "HbmLoader"), ("0", "DataLoader")):
        out = str(tmp_path / f"out{hbm}")
        argv = ["--refer_data_root", root, "--dataset", "refcocog", "--splitBy", "umd", "--size", "64", "--batch_size", "4",
                "--epoch", "1", "--test_split", "val", "--output", out, "--print-freq", "1", "--backbone", "clip-RN50",
                "--max_query_len", "20", "--pseudo_path", pseudo]
        env = dict(os.environ, TRIS_RANDOM_INIT="1")
        env.pop("TRIS_HBM_LOADER", None)
        if hbm == "0":
            env["TRIS_HBM_LOADER"] = "0"
        r = subprocess.run([sys.executable, "-m", "tris_amd.train_stage2"] + argv, cwd=repo, env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        assert f"training batches from {loader}" in r.stderr, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Train:[")]
        assert lines
        for ln in lines:
            vals = [float(v) for v in re.findall(r"(?:loss|l[1-4]): (\S+)", ln)]
            assert len(vals) == 5 and all(math.isfinite(v) for v in vals), ln
        best = ast.literal_eval([ln for ln in r.stdout.splitlines() if ln.startswith("{'val_acc'")][-1])
        assert best["epoch"] == 0 and os.path.exists(best["path"])
        assert "Validat on the train split" in r.stdout
