"""IRNet's training input pipeline on the MI355X (csrc/irndata.hip, tris_amd.dataset.irn_data, tris_amd.train_irn).

Every comparison is for equal bytes: the kernel against tests/oracle_irn_data.py (Pillow and numpy; pinned to the reference by
tests/test_irn_data_host.py and tests/golden/g18_irn_data.npz), the loader against the oracle under the same random numbers, a
training step fed by the loader against the same step on the oracle's arrays, and the command line against a hand-driven loop."""
import json
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import oracle_irn_data as O
from conftest import ROOT

pytestmark = pytest.mark.gpu
N_IMAGES = len(O.SIZES) + 1            # the four sizes and the grey image


def _write(tmp, names, images, labels):
    root, lab = tmp / "train2014", tmp / "ir_label"
    root.mkdir()
    lab.mkdir()
    for name, img, label in zip(names, images, labels):
        i = name.split("_")[-1]
        Image.fromarray(img).save(root / f"COCO_train2014_{i.zfill(12)}.jpg", format="PNG")     # lossless, under the rule's name
        Image.fromarray(label).save(lab / f"{name}.png")
    (tmp / "names.json").write_text(json.dumps(names))
    return str(tmp / "names.json"), str(lab), str(root)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """the four sizes and the grey image, as files; -> (paths, images, labels)"""
    images = [O.synthetic_image(i) for i in range(N_IMAGES)]
    labels = [O.synthetic_label(i) for i in range(N_IMAGES)]
    names = [f"s_{i}_{i + 1}" for i in range(N_IMAGES)]
    return _write(tmp_path_factory.mktemp("irn_small"), names, images, labels), images, labels


def _cache(paths, crop):
    from tris_amd.dataset import irn_data as D
    return D.HbmIrnCache(D.ReferAffinityData(*paths, crop_size=crop), "cuda")


def _explicit(images, crop, scales, flips, where):
    """one IrnAugParams per image; where: 0 = offsets 0, 1 = at their maximum, 2 = in between"""
    from tris_amd.dataset.irn_data import IrnAugParams
    out = []
    for img, s, f in zip(images, scales, flips):
        H, W = img.shape[:2]
        h, w = IrnAugParams.target_size(H, W, s)
        top, left = abs(h - crop), abs(w - crop)
        top, left = ((0, 0), (top, left), (top // 2, left // 3))[where]
        out.append(IrnAugParams.explicit(H, W, crop, s, f, top, left))
    return out


def _expect(images, labels, params, crop):
    got = [O.apply(img, lab, O.from_params(p), crop) for img, lab, p in zip(images, labels, params)]
    return tuple(np.stack([g[k] for g in got]) for k in range(3))


def _check(out, want, what):
    img, label, reduced = out
    a = img.permute(0, 2, 3, 1)
    assert a.is_contiguous() and a.dtype == torch.float32          # channels-last memory: what the stem kernel reads
    assert np.array_equal(a.cpu().numpy().view(np.uint32), want[0].view(np.uint32)), what
    assert np.array_equal(label.cpu().numpy(), want[1]), what
    assert np.array_equal(reduced.cpu().numpy(), want[2]), what


BATCHES = [   # (scales, flips, where): 0.5 / 1.5 / 1.004 and 1.0 (neither axis changes), both flips, offsets 0 / max / between
    ([0.5, 1.5, 1.5, 1.004, 0.61], [False, True, False, True, True], 0),
    ([0.5, 1.5, 1.5, 0.5, 1.27], [True, False, True, False, False], 1),
    ([1.004, 0.93, 1.0, 1.5, 1.5], [False, True, True, False, True], 2),
    # exactly one axis changes (1.004 changes none at these sizes): 37x54, 65x48 (63x48 at 0.99), 51x81, 20x92, 45x61 -- a column table only
    # (flag 1) or a row table only (flag 2), each flipped and not
    ([1.01, 1.01, 1.008, 1.02, 1.009], [False, True, False, True, False], 2),
    ([1.01, 1.01, 1.008, 1.02, 1.009], [True, False, True, False, True], 1),
    ([1.01, 0.99, 1.008, 1.02, 1.009], [True, True, False, False, True], 0),
]
ONE_AXIS_FLAGS = [1, 2, 1, 1, 1]         # of the last three batches, without the flip's bit


@pytest.mark.parametrize("crop", [40, 72])       # below and above one 32-wide tile, neither a multiple of it
def test_kernel_equals_the_oracle(small, crop):
    from tris_amd import irn_loss
    from tris_amd.dataset.irn_data import D_FLAGS, IrnAugParams, IrnLoader, build_batch
    paths, images, labels = small
    cache = _cache(paths, crop)
    assert cache.nbytes >= sum(a.size for a in images) and all(o % 16 == 0 for o in cache.image_offsets + cache.label_offsets)
    loader = IrnLoader(cache, N_IMAGES, seed=0)
    idx = list(range(N_IMAGES))
    kinds = set()
    for scales, flips, where in BATCHES:
        params = _explicit(images, crop, scales, flips, where)
        for p in params:
            kinds.add(("pad" if p.target[0] <= crop else "crop") + "_" + ("pad" if p.target[1] <= crop else "crop"))
        if scales[0] == 1.01:
            desc, _ = build_batch([cache.sample(i) for i in idx], params, crop)
            assert [int(f) & 3 for f in desc[:, D_FLAGS]] == ONE_AXIS_FLAGS
            assert [bool(int(f) & 4) for f in desc[:, D_FLAGS]] == flips
        out = loader.augment(idx, params)
        _check(out, _expect(images, labels, params, crop), (crop, scales, where))
        assert torch.equal(out[2], irn_loss.reduce_label(out[1]))
        again = loader.augment(idx, params)                         # two runs: equal bytes
        assert all(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)) for a, b in zip(out, again))
    assert {"pad_pad", "crop_crop"} <= kinds, kinds
    # the top-left mode on the same batch
    params = [IrnAugParams.top_left(a.shape[0], a.shape[1], crop) for a in images]
    _check(loader.augment(idx, params), _expect(images, labels, params, crop), (crop, "top left"))
    tl = list(IrnLoader.top_left(cache, N_IMAGES))
    assert len(tl) == 1 and torch.equal(tl[0], loader.augment(idx, params)[0])


def test_a_box_outside_the_crop_is_refused_before_the_launch(small):
    from tris_amd.dataset.irn_data import IrnAugParams, IrnLoader
    paths, images, _ = small
    loader = IrnLoader(_cache(paths, 40), 1)
    good = IrnAugParams.explicit(37, 53, 40, 1.5, False, 0, 0)
    bad = IrnAugParams(good.scale, good.flip, good.target, (8,) + (48,) + good.box[2:4] + (0, 40) + good.box[6:])
    with pytest.raises(ValueError, match="outside the crop of 40"):
        loader.augment([0], [bad])


def test_loader_epoch_equals_the_oracle_under_the_same_random_numbers(small):
    from tris_amd.dataset.irn_data import IrnLoader
    paths, images, labels = small
    crop, B, seed = 40, 2, 11
    loader = IrnLoader(_cache(paths, crop), B, seed=seed)
    assert len(loader) == 2
    rng = random.Random(seed)
    gen = torch.Generator().manual_seed(seed)
    for epoch in range(2):                                          # the second epoch goes on with both streams
        order = torch.randperm(N_IMAGES, generator=gen).tolist()
        batches = list(loader)
        assert len(batches) == 2
        for k, out in enumerate(batches):
            idx = order[k * B:(k + 1) * B]
            draws = [O.draw(rng, images[i].shape[0], images[i].shape[1], crop) for i in idx]
            want = [O.apply(images[i], labels[i], d, crop) for i, d in zip(idx, draws)]
            _check(out, tuple(np.stack([w[j] for w in want]) for j in range(3)), (epoch, k))


# --------------------------------------------------------------------------------------------------- training from the loader
def _train_images(n=6):
    """images and labels between 100 and 200 pixels a side: every label holds background, an object and ignored pixels"""
    rng = np.random.default_rng(5)
    images, labels = [], []
    for i in range(n):
        H, W = int(rng.integers(100, 200)), int(rng.integers(100, 200))
        yy, xx = np.mgrid[0:H, 0:W]
        a = np.stack([128 + 100 * np.sin(yy / (9.0 + c) + i) * np.cos(xx / (11.0 + i)) for c in range(3)], 2)
        images.append(np.clip(a + rng.normal(0, 10, a.shape), 0, 255).astype(np.uint8))
        lab = np.zeros((H, W), np.uint8)
        lab[H // 4:H // 4 + H // 2, W // 3:W // 3 + W // 3] = 1
        lab[rng.integers(0, H, 40), rng.integers(0, W, 40)] = 255
        labels.append(lab)
    return images, labels


@pytest.fixture(scope="module")
def train_set(tmp_path_factory):
    images, labels = _train_images()
    names = [f"t_{i}_{i + 1}" for i in range(len(images))]
    return _write(tmp_path_factory.mktemp("irn_train"), names, images, labels), images, labels


def _filled_net():
    from tris_amd.irn_net import EdgeDisplacement
    from tris_amd.utils.synth import irn_fill
    net = EdgeDisplacement()
    irn_fill(net.state_dict(), 0, 1.0)
    return net


def _heads(sd):
    return {k: v for k, v in sd.items() if k.startswith("fc_")}


def test_train_step_from_the_loader_equals_the_step_on_the_oracles_arrays(train_set):
    from tris_amd.dataset.irn_data import IrnLoader
    from tris_amd.irn_train import IrnTrainer
    paths, images, labels = train_set
    crop, B, seed = 128, 2, 3
    loader = IrnLoader(_cache(paths, crop), B, seed=seed, shuffle=False)
    img, label, reduced = next(iter(loader))
    rng = random.Random(seed)
    draws = [O.draw(rng, images[i].shape[0], images[i].shape[1], crop) for i in range(B)]
    want = [O.apply(images[i], labels[i], d, crop) for i, d in enumerate(draws)]
    results = []
    for feed in ((img, reduced), (torch.from_numpy(np.stack([w[0] for w in want])).cuda(),
                                  torch.from_numpy(np.stack([w[2] for w in want])).cuda())):
        tr = IrnTrainer(_filled_net().cuda(), lr=0.1, weight_decay=1e-4, max_step=10)
        out = tr.train_step(*feed)
        results.append((out["losses"].cpu(), out["counts"].cpu(), _heads(tr.state_dict())))
    (l0, c0, h0), (l1, c1, h1) = results
    assert int(c0.min()) > 0, c0                                    # every class of pairs is there
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)) and torch.equal(c0, c1)
    assert all(torch.equal(h0[k], h1[k]) for k in h0)
    # the full-size label gives the same step (IrnTrainer reduces it itself)
    tr = IrnTrainer(_filled_net().cuda(), lr=0.1, weight_decay=1e-4, max_step=10)
    assert torch.equal(tr.train_step(img, label)["losses"].cpu().view(torch.int32), l0.view(torch.int32))


def test_command_line_end_to_end(train_set, tmp_path):
    from tris_amd import train_irn
    from tris_amd.dataset.irn_data import HbmIrnCache, IrnLoader, ReferAffinityData
    from tris_amd.irn_net import EdgeDisplacement
    from tris_amd.irn_train import IrnTrainer
    paths, images, labels = train_set
    crop, B, seed = 128, 2, 4
    backbone = {k[len("resnet50."):]: v.clone() for k, v in _filled_net().state_dict().items() if k.startswith("resnet50.")}
    torch.save(backbone, tmp_path / "r50.pth")
    out_file = tmp_path / "irn.pth"
    cmd = [sys.executable, "-m", "tris_amd.train_irn", "--train_list", paths[0], "--ir_label_out_dir", paths[1], "--voc12_root",
           paths[2], "--irn_crop_size", str(crop), "--irn_batch_size", str(B), "--irn_num_epoches", "1", "--irn_weights_name",
           str(out_file), "--irn_backbone_weights", str(tmp_path / "r50.pth"), "--seed", str(seed), "--num_workers", "8"]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)      # a fresh process with its own limit
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "step:    0/    3" in run.stdout and "Analyzing displacements mean ... done." in run.stdout
    saved = torch.load(out_file, map_location="cpu")
    EdgeDisplacement().load_state_dict(saved)                        # what make_ins_seg --irn_weights_name does
    # the same by hand
    net = train_irn.initial_network(str(tmp_path / "r50.pth"), seed)
    initial = {k: v.clone() for k, v in _heads(net.state_dict()).items()}
    trainer = IrnTrainer(net.cuda(), lr=0.1, weight_decay=1e-4, max_step=3, radius=10)
    cache = HbmIrnCache(ReferAffinityData(*paths, crop_size=crop), "cuda")
    steps = 0
    for img, _, reduced in IrnLoader(cache, B, seed=seed):
        trainer.train_step(img, reduced)
        steps += 1
    assert steps == 3
    mean = trainer.fit_mean_shift(IrnLoader.top_left(cache, B)).cpu()
    mine = trainer.state_dict()
    assert set(mine) == set(saved)
    assert all(torch.equal(mine[k], saved[k]) for k in mine), [k for k in mine if not torch.equal(mine[k], saved[k])][:5]
    assert torch.equal(saved["mean_shift.running_mean"], mean) and bool((mean != 0).all())
    same = [k for k in initial if initial[k].dim() > 1 and torch.equal(initial[k], saved[k])]     # every head matrix has moved
    assert not same, same
