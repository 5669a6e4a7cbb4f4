"""REFER polygon targets built on the MI355X (csrc/polymask.hip, dataset/poly_arena.py, cfg.poly_targets): device run ends against
runs_numpy, decoded masks against the unchanged dataset/cocomask.py, the training-target kernel against the resize of the decoded
mask, and the HBM cache with the knob on against the cache with the knob off.  All comparisons exact."""
import json
import os

import numpy as np
import pytest
import torch

import poly_cases

pytestmark = pytest.mark.gpu


def _build(cases):
    """cases: (name, xy, h, w), one ref each -> (DeviceArena, ends numpy, seg_off numpy)"""
    from tris_amd.dataset.poly_arena import PolyArena
    arena = PolyArena()
    for name, xy, h, w in cases:
        arena.add_ref([xy], h, w, name)
    built = arena.build("cuda")
    return built, built.ends.cpu().numpy(), built.seg_off.cpu().numpy()


def _decode(built, k, h, w):
    from tris_amd import ops
    return ops.rle_decode_sum_arena(built.ends, built.seg_off, built.ranges[k:k + 1], h, w)[0].cpu().numpy()


def _check_ends(cases, ends, seg_off):
    from tris_amd.dataset.poly_arena import runs_numpy, upsample
    assert seg_off[0] == 0 and seg_off.size == len(cases) + 1 and ends.size == seg_off[-1] + 1
    for k, (name, xy, h, w) in enumerate(cases):
        assert np.array_equal(ends[seg_off[k]:seg_off[k + 1]], runs_numpy(upsample(xy), h, w)), name


def test_slope_sweep_every_edge_up_to_40_steps():
    """every 2-vertex polygon whose edge spans (dx, dy) upsampled steps, 0..40 each, in the four sign combinations (there and back:
    each polygon walks its edge once flipped and once not), on a 10x10 canvas; one arena, one count and one emit launch"""
    from tris_amd import ops
    from tris_amd.dataset.poly_arena import upsample
    X0, Y0 = 23, 26
    cases = []
    for sx in (1, -1):
        for sy in (1, -1):
            for dx in range(41):
                for dy in range(41):
                    xy = [X0 / 5, Y0 / 5, (X0 + sx * dx) / 5, (Y0 + sy * dy) / 5]
                    cases.append((f"edge {sx * dx:+d},{sy * dy:+d}", xy, 10, 10))
    v = np.stack([upsample(c[1]) for c in cases])
    assert (v[:, 0] == [X0, Y0]).all() and (np.abs(v[:, 1] - [X0, Y0]).max(0) == [40, 40]).all()     # the edges meant are the edges built
    built, ends, seg_off = _build(cases)
    _check_ends(cases, ends, seg_off)
    masks = ops.rle_decode_sum_arena(built.ends, built.seg_off, built.ranges, 10, 10).cpu().numpy()
    for k, (name, xy, h, w) in enumerate(cases):
        assert np.array_equal(masks[k], poly_cases.oracle_mask(xy, h, w)), name


def test_random_polygons_and_named_cases_in_one_arena():
    cases = poly_cases.all_cases(300, seed=20240612)
    built, ends, seg_off = _build(cases)
    _check_ends(cases, ends, seg_off)
    for k, (name, xy, h, w) in enumerate(cases):
        assert np.array_equal(_decode(built, k, h, w), poly_cases.oracle_mask(xy, h, w)), name
    again = _build(cases)[1]
    assert np.array_equal(ends, again)            # (the order in which crossings take their slots does not show)


def _zigzag(sweeps, short=0, w=256, h=64):
    """`sweeps` horizontal sweeps over a w x h canvas, rising from y = 1 to y = h - 1; the first turn stops `short` pixels early"""
    ys = np.linspace(1.0, h - 1.0, sweeps + 1)
    xy = []
    for i in range(sweeps + 1):
        xy += [0.0 if i % 2 == 0 else float(w), float(ys[i])]
    xy[2] -= short
    return xy


def test_slices_at_and_beyond_the_lds_sort_capacity():
    """The emit kernel sorts up to tris_poly_sort_capacity() (4096) run ends in LDS and longer slices in place in global memory.  A
    zig-zag of 50 sweeps over a 256 x 64 canvas leaves about 12.8k crossings (the global path).  A slice has an odd length (a closed
    boundary crosses the centre line of a column an even number of times, and H*W closes it), so the last LDS size is capacity - 1
    and the first global one capacity + 1: 16 sweeps, the first turn one pixel short for the former.  Small polygons sit between
    them: their slices must come out untouched."""
    from tris_amd import _lib
    cap = _lib.query("tris_poly_sort_capacity")
    assert cap == 4096
    small = ("small", [3.0, 3.0, 20.5, 4.0, 11.0, 30.0], 64, 256)
    cases = [small, ("zig-zag 50", _zigzag(50), 64, 256), small, ("capacity - 1", _zigzag(16, short=1), 64, 256),
             ("capacity + 1", _zigzag(16), 64, 256), small]
    built, ends, seg_off = _build(cases)
    lens = np.diff(seg_off)
    assert lens[1] > 3 * cap and lens[3] == cap - 1 and lens[4] == cap + 1 and lens[0] == lens[2] == lens[5] < 200, lens
    _check_ends(cases, ends, seg_off)
    for k, (name, xy, h, w) in enumerate(cases):
        assert np.array_equal(_decode(built, k, h, w), poly_cases.oracle_mask(xy, h, w)), name


def test_host_route_segments_share_the_arena():
    """an RLE dict and a polygon beyond the device's coordinate bound take slices the host fills, between device polygons"""
    from tris_amd.dataset import cocomask
    from tris_amd.dataset.poly_arena import COORD_MAX, PolyArena
    h, w = 20, 33
    tri, sq = [1.0, 1.0, 30.0, 4.5, 9.0, 18.0], [5, 5, 25, 5, 25, 15, 5, 15]
    far = [2.0, 2.0, float(COORD_MAX // 5 + 10), 10.0, 4.0, 19.0]          # upsampled: just beyond the device's bound
    rle = cocomask.frPyObjects([sq], h, w)[0]
    refs = [[tri], [rle], [tri, far, sq], rle, [sq]]
    arena = PolyArena()
    for k, seg in enumerate(refs):
        arena.add_ref(seg, h, w, f"ref {k}")
    assert arena.n_host_segments == 3
    built = arena.build("cuda")
    from tris_amd import ops
    got = ops.rle_decode_sum_arena(built.ends, built.seg_off, built.ranges, h, w).cpu().numpy()
    for k, polys in enumerate([[tri], [sq], [tri, far, sq], [sq], [sq]]):          # (the RLE dict is the square)
        want = sum(poly_cases.oracle_mask(p, h, w).astype(np.int64) for p in polys)
        assert np.array_equal(got[k], want), k
    assert got[2].max() == 3


@pytest.mark.parametrize("H,W,S", [(7, 5, 4), (33, 20, 32), (72, 50, 32), (20, 33, 64)])
def test_training_target_equals_resize_of_the_decoded_mask(H, W, S):
    from tris_amd import ops
    from tris_amd.dataset import cocomask
    from tris_amd.dataset.poly_arena import PolyArena

    def blob(cx, cy, r, n, phase):
        a = phase + 2 * np.pi * np.arange(n) / n
        return np.stack([cx * W + r * min(H, W) * np.cos(a), cy * H + r * min(H, W) * np.sin(a)], 1).round(2).reshape(-1).tolist()
    one = [blob(0.5, 0.5, 0.35, 7, 0.3)]
    two = [blob(0.4, 0.45, 0.3, 6, 0.1), blob(0.6, 0.55, 0.3, 5, 0.7)]                     # overlapping: the overlap is not target
    three = [blob(0.3, 0.3, 0.22, 5, 0.2), blob(0.7, 0.6, 0.25, 8, 0.0), blob(0.5, 0.5, 0.2, 4, 0.5)]
    arena = PolyArena()
    ranges = [arena.add_ref(seg, H, W, f"ref {k}") for k, seg in enumerate((one, two, three))]
    built = arena.build("cuda")
    buf = torch.full((5, S, S), 7, dtype=torch.uint8, device="cuda")
    seen = set()
    for k, (seg, (lo, hi)) in enumerate(zip((one, two, three), ranges)):
        summed = cocomask.decode(cocomask.frPyObjects(seg, H, W)).sum(2)
        seen |= set(np.unique(summed).tolist())
        full = torch.from_numpy((summed == 1).astype(np.uint8)).cuda()
        want = ops.resize_nearest_u8(full, S, S)
        got = ops.rle_target_nearest(built, lo, hi, H, W, S)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (S, S)
        assert torch.equal(got, want), k
        ops.rle_target_nearest(built, lo, hi, H, W, S, out=buf[k + 1])       # into a row of the cache, neighbours untouched
        assert torch.equal(buf[k + 1], want)
    assert bool((buf[0] == 7).all()) and bool((buf[4] == 7).all())
    if min(H, W) >= 20:
        assert {0, 1, 2} <= seen            # the two-polygon ref really overlaps


# ------------------------------------------------------------------------------------------------------------------ the loader
KW = dict(dataset="refcocog", splitBy="umd", max_tokens=20)


def _dataset(root, size, split="train", eval_mode=False):
    from tris_amd.dataset.ReferDataset import ReferDataset
    from tris_amd.dataset.transform import get_transform
    from tris_amd.utils.synth import word_hash_tokenize
    return ReferDataset(refer_data_root=root, image_transforms=get_transform(size, not eval_mode), split=split, eval_mode=eval_mode,
                        size=size, tokenizer=word_hash_tokenize, **KW)


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


def _rewrite_annotations(root):
    """every third annotation gets a second polygon that overlaps the first; one holds an uncompressed RLE dict instead"""
    from tris_amd.dataset import cocomask
    path = os.path.join(root, "refer", "refcocog", "instances.json")
    inst = json.load(open(path))
    size = {i["id"]: (i["height"], i["width"]) for i in inst["images"]}
    for k, a in enumerate(inst["annotations"]):
        h, w = size[a["image_id"]]
        p = np.asarray(a["segmentation"][0]).reshape(-1, 2)
        if k in (4, 7):                      # (ref 4 is a training ref, ref 7 an evaluation ref)
            a["segmentation"] = [cocomask.frPyObjects(a["segmentation"], h, w)[0]]
        elif k % 3 == 0:
            a["segmentation"].append((p + [0.31 * (p[:, 0].max() - p[:, 0].min()), 1.5]).round(2).reshape(-1).tolist())
    json.dump(inst, open(path, "w"))
    return sum(len(a["segmentation"]) == 2 for a in inst["annotations"])


def test_cache_with_the_knob_on_equals_the_cache_with_the_knob_off(tmp_path, monkeypatch):
    from tris_amd.config import cfg
    from tris_amd.dataset.ReferDataset import ReferDataset
    from tris_amd.dataset.hbm import HbmLoader, HbmReferCache
    from tris_amd.utils.synth import make_mini_refer
    S = 32
    root = make_mini_refer(str(tmp_path / "data"), n_images=9, seed=4, max_side=72)
    assert _rewrite_annotations(root) >= 3
    tr, ev = _dataset(root, S), _dataset(root, S, split="val", eval_mode=True)
    assert len(tr) > 4 and len(ev) > 1
    assert cfg.poly_targets is False
    off_tr, off_ev = HbmReferCache(tr, S), HbmReferCache(ev, S)

    def refuse(self, index):
        raise AssertionError("ReferDataset.load_mask called with cfg.poly_targets on")
    with cfg.override(poly_targets=True):
        monkeypatch.setattr(ReferDataset, "load_mask", refuse)
        on_tr, on_ev = HbmReferCache(tr, S), HbmReferCache(ev, S)
        monkeypatch.undo()
    # training
    assert torch.equal(on_tr.targets, off_tr.targets) and on_tr.arena is None and on_tr.nbytes() == off_tr.nbytes()
    assert {0, 1} == set(torch.unique(on_tr.targets).tolist())
    for c in (on_tr, on_ev):
        for k in ("boxes", "orig_size", "img_path"):
            assert torch.equal(getattr(c, k), getattr(off_tr if c is on_tr else off_ev, k)), k
        assert c.files == (off_tr if c is on_tr else off_ev).files
    np.random.seed(5)
    a = next(iter(HbmLoader(on_tr, batch_size=4)))
    np.random.seed(5)
    b = next(iter(HbmLoader(off_tr, batch_size=4)))
    _same(a, b, "train")
    # evaluation: no masks kept, every batch equal
    assert on_ev.eval_targets == [] and on_ev.targets is None and len(off_ev.eval_targets) == len(ev)
    assert on_ev.nbytes() == on_ev.images.numel() + on_ev.tokens.numel() * on_ev.tokens.element_size() + on_ev.arena.nbytes()
    assert on_ev.arena.nbytes() == sum(t.numel() * t.element_size() for t in (on_ev.arena.ends, on_ev.arena.seg_off, on_ev.arena.ranges))
    got, want = list(HbmLoader(on_ev, batch_size=1)), list(HbmLoader(off_ev, batch_size=1))
    assert len(got) == len(want) == len(ev)
    for i, (x, y) in enumerate(zip(got, want)):
        _same(x, y, f"eval {i}")
