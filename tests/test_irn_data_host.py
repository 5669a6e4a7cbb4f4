"""Host side of IRNet's training input pipeline (tris_amd.dataset.irn_data, tris_amd.train_irn): no GPU.

  * tests/oracle_irn_data.py equals every case the reference produced (tests/golden/g18_irn_data.npz), bit for bit
  * the product's draw equals the oracle's and the recorded one
  * the table builder's tables, run through a numpy statement of the kernel's integer arithmetic, equal Pillow bit for bit
  * pil_tables.resample_tables' default output is what it was before the filter argument
  * descriptor validation and the command line's parser
"""
import json
import random

import numpy as np
import pytest
from PIL import Image

import oracle_irn_data as O
from tris_amd.dataset import irn_data as D
from tris_amd.dataset import pil_tables

SIZES = [(37, 53), (64, 48), (51, 80), (20, 90)]
FACTORS = [0.5, 0.61, 0.93, 1.0, 1.004, 1.27, 1.5]


@pytest.fixture(scope="module")
def g18(golden):
    return golden("g18_irn_data.npz")


def case_inputs(g, n):
    j = int(g[f"c{n}_index"])
    return g[f"image{_image_of(j)}"], g[f"label{j}"]


def _image_of(j):
    return [0, 1, 1, 2, 3, 4][j]          # the list of the fixture: names 1 and 2 share an image


# ------------------------------------------------------------------------------------------------ the oracle and the reference
def test_fixture_took_every_branch(g18):
    counts = dict(zip(g18["branch_names"].tolist(), g18["branch_counts"].tolist()))
    assert set(counts) == {"pad_x", "crop_x", "pad_y", "crop_y", "flip", "no_flip", "axis_unchanged", "offset_zero", "offset_max"}
    assert min(counts.values()) >= 1, counts
    assert g18["image4"].ndim == 2                         # the grey image
    assert (g18["image1"] == 255).any() and (g18["image1"] == 0).any()


def test_oracle_equals_every_recorded_item(g18):
    crop, radius = int(g18["crop"]), int(g18["radius"])
    for n in range(int(g18["n_cases"])):
        img, label = case_inputs(g18, n)
        d = O.draw(random.Random(int(g18[f"c{n}_seed"])), img.shape[0], img.shape[1], crop)
        u, bit, rx, ry = g18[f"c{n}_draw"]
        assert d["scale"] == 0.5 + u * (1.5 - 0.5) and d["flip"] == bool(bit), n
        assert (max(d["cont"][1], d["src"][1]), max(d["cont"][0], d["src"][0])) == (int(rx), int(ry)), n
        a, lab, red = O.apply(img, label, d, crop)
        want = g18[f"c{n}_img"]
        assert np.array_equal(a.transpose(2, 0, 1).view(np.uint32), want.view(np.uint32)), n
        assert np.array_equal(lab, g18[f"c{n}_label"]), n
        for got, key in zip(O.pair_labels(red, radius), ("aff_bg_pos_label", "aff_fg_pos_label", "aff_neg_label")):
            assert np.array_equal(got, g18[f"c{n}_{key}"].astype(np.float32)), (n, key)


def test_oracle_top_left_equals_the_recorded_items(g18):
    crop = int(g18["crop"])
    for j in range(6):
        img = g18[f"image{_image_of(j)}"]
        a, _, _ = O.apply(img, None, O.top_left(img.shape[0], img.shape[1], crop), crop)
        assert np.array_equal(a.transpose(2, 0, 1).view(np.uint32), g18[f"t{j}_img"].view(np.uint32)), j


def test_product_draw_equals_the_oracle(g18):
    crop = int(g18["crop"])
    for n in range(int(g18["n_cases"])):
        img, _ = case_inputs(g18, n)
        seed = int(g18[f"c{n}_seed"])
        p = D.IrnAugParams.draw(random.Random(seed), img.shape[0], img.shape[1], crop)
        d = O.draw(random.Random(seed), img.shape[0], img.shape[1], crop)
        assert O.from_params(p) == d and p.box == O.box8(d), n
    p = D.IrnAugParams.top_left(20, 90, 40)
    assert O.from_params(p) == O.top_left(20, 90, 40)
    # one stream for a whole batch: the second sample continues where the first stopped
    a, b = random.Random(3), random.Random(3)
    assert [D.IrnAugParams.draw(a, 64, 48, 40).box for _ in range(3)] == [O.box8(O.draw(b, 64, 48, 40)) for _ in range(3)]


def test_normalisation_table_is_the_reference_arithmetic():
    lut = D.normalisation_table()
    assert lut.dtype == np.float32 and lut.shape == (3, 256)
    a = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    assert np.array_equal(O.normalise(a).reshape(256, 3).T.view(np.uint32), lut.view(np.uint32))


# ------------------------------------------------------------------------------------------------ tables against Pillow
def emulate(img, label, p, crop):
    """the kernel's arithmetic in numpy, driven by build_batch's descriptor and tables -> (img f32 [crop,crop,3], label, reduced)"""
    img3 = np.stack([img, img, img], axis=2) if img.ndim == 2 else img
    H, W = img3.shape[:2]
    desc, tables = D.build_batch([(0, 0, H, W)], [p], crop)
    D.validate_batch(desc, tables, crop, img3.size, label.size)
    d = desc[0]
    ct, cb, cl, cr, it, ib, il, ir = (int(v) for v in d[D.D_CT:D.D_IR + 1])
    n_c, n_r, flags = cr - cl, cb - ct, int(d[D.D_FLAGS])
    a = img3.astype(np.int64)

    def taps(o_b, o_k, ks, n):
        b = tables[int(d[o_b]):int(d[o_b]) + 2 * n].reshape(n, 2)
        return b, tables[int(d[o_k]):int(d[o_k]) + ks * n].reshape(n, ks).astype(np.int64)

    if flags & 1:
        b, k = taps(D.D_COLB, D.D_COLK, int(d[D.D_KH]), n_c)
        a = np.stack([np.clip(((a[:, f:f + c] * k[e, :c, None]).sum(1) + (1 << 21)) >> 22, 0, 255) for e, (f, c) in enumerate(b)], 1)
    else:
        cols = np.arange(il, ir)
        a = a[:, (int(d[D.D_WT]) - 1 - cols) if flags & 4 else cols]
    if flags & 2:
        b, k = taps(D.D_ROWB, D.D_ROWK, int(d[D.D_KV]), n_r)
        a = np.stack([np.clip(((a[f:f + c] * k[e, :c, None, None]).sum(0) + (1 << 21)) >> 22, 0, 255) for e, (f, c) in enumerate(b)])
    else:
        a = a[it:ib]
    lut = D.normalisation_table()
    out = np.zeros((crop, crop, 3), np.float32)
    for c in range(3):
        out[ct:cb, cl:cr, c] = lut[c][a[..., c]]
    xnn = tables[int(d[D.D_XNN]):int(d[D.D_XNN]) + n_c]
    ynn = tables[int(d[D.D_YNN]):int(d[D.D_YNN]) + n_r]
    lab = np.full((crop, crop), 255, np.uint8)
    lab[ct:cb, cl:cr] = label[ynn][:, xnn]
    return out, lab, lab[2::4, 2::4]


def _image(H, W, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    a[2:12, 3:11] = 255
    a[2:12, 11:19] = 0
    return a


@pytest.mark.parametrize("size", SIZES)
def test_bicubic_tables_equal_pillow_full_window(size):
    H, W = size
    img = _image(H, W, H * W)
    for s in FACTORS:
        Ht, Wt = D.IrnAugParams.target_size(H, W, s)
        want = O.resize(img, (Ht, Wt), Image.BICUBIC)
        a = img.astype(np.int64)
        if Wt != W:
            b, k, ks = pil_tables.resample_tables(W, Wt, "bicubic")
            assert ks <= D.KMAX
            a = np.stack([np.clip(((a[:, f:f + c] * k[x, :c, None].astype(np.int64)).sum(1) + (1 << 21)) >> 22, 0, 255)
                          for x, (f, c) in enumerate(b)], 1)
        if Ht != H:
            b, k, ks = pil_tables.resample_tables(H, Ht, "bicubic")
            a = np.stack([np.clip(((a[f:f + c] * k[y, :c, None, None].astype(np.int64)).sum(0) + (1 << 21)) >> 22, 0, 255)
                          for y, (f, c) in enumerate(b)])
        assert np.array_equal(a.astype(np.uint8), want), (size, s)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_cropped_window_tables_equal_the_window_of_pillows_result(size, flip):
    H, W = size
    img = _image(H, W, H + W)
    label = np.random.default_rng(H).choice(np.asarray([0, 1, 255], np.uint8), size=(H, W))
    for s in FACTORS:
        for crop in (24, 40, 72):
            Ht, Wt = D.IrnAugParams.target_size(H, W, s)
            for top, left in ((0, 0), (abs(Ht - crop), abs(Wt - crop)), (abs(Ht - crop) // 2, abs(Wt - crop) // 3)):
                p = D.IrnAugParams.explicit(H, W, crop, s, flip, top, left)
                got = emulate(img, label, p, crop)
                want = O.apply(img, label, O.from_params(p), crop)
                assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (size, s, crop, top, left)
                assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (size, s, crop, top, left)
    # the flip alone: the full window's flipped column order is np.fliplr of the resized image
    if flip:
        Ht, Wt = D.IrnAugParams.target_size(H, W, 1.27)
        p = D.IrnAugParams(1.27, True, (Ht, Wt), (0, Ht, 0, Wt, 0, Ht, 0, Wt))
        got = emulate(img, label, p, 120)[0][:Ht, :Wt]
        want = O.normalise(np.fliplr(O.resize(img, (Ht, Wt), Image.BICUBIC)))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# exactly one axis changes size: (size, scale, the one table's flag -- 1 columns, 2 rows).  None of FACTORS does this at SIZES
# (1.004 and 1.0 change neither axis of any of them, every other factor changes both).
ONE_AXIS = [((20, 90), 1.02, 1), ((37, 53), 1.01, 1), ((51, 80), 1.008, 1), ((64, 48), 1.01, 2), ((64, 48), 0.99, 2)]


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("size,scale,flag", ONE_AXIS)
def test_one_axis_changed_has_one_table_and_equals_pillow(size, scale, flag, flip):
    H, W = size
    Ht, Wt = D.IrnAugParams.target_size(H, W, scale)
    assert (Wt != W, Ht != H) == (flag == 1, flag == 2)
    img = _image(H, W, H * 3 + W)
    label = np.random.default_rng(W).choice(np.asarray([0, 1, 255], np.uint8), size=(H, W))
    for crop in (24, 40, 72):
        for top, left in ((0, 0), (abs(Ht - crop), abs(Wt - crop)), (abs(Ht - crop) // 2, abs(Wt - crop) // 3)):
            p = D.IrnAugParams.explicit(H, W, crop, scale, flip, top, left)
            desc, tables = D.build_batch([(0, 0, H, W)], [p], crop)
            assert int(desc[0, D.D_FLAGS]) == flag | (4 if flip else 0)
            n_c, n_r = p.box[3] - p.box[2], p.box[1] - p.box[0]
            ks = int(desc[0, D.D_KH if flag == 1 else D.D_KV])
            assert int(desc[0, D.D_KV if flag == 1 else D.D_KH]) == 0 and ks > 0
            assert tables.size == (n_c if flag == 1 else n_r) * (2 + ks) + n_c + n_r          # one table, two label index rows
            got = emulate(img, label, p, crop)
            want = O.apply(img, label, O.from_params(p), crop)
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (size, scale, crop, top, left)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (size, scale, crop, top, left)


def test_factors_change_both_axes_or_neither():
    """what the cases above are for: the issue's factors never give a table on one axis only at its sizes"""
    for H, W in SIZES:
        for s in FACTORS:
            Ht, Wt = D.IrnAugParams.target_size(H, W, s)
            assert (Ht != H) == (Wt != W), (H, W, s)


def test_only_the_window_entries_are_built():
    p = D.IrnAugParams.explicit(64, 48, 24, 1.5, True, 10, 7)
    desc, tables = D.build_batch([(0, 0, 64, 48)], [p], 24)
    ks_h, ks_v = int(desc[0, D.D_KH]), int(desc[0, D.D_KV])
    assert tables.size == 24 * (2 + ks_h) + 24 * (2 + ks_v) + 2 * 24
    p = D.IrnAugParams.explicit(20, 90, 40, 1.02, False, 3, 5)          # 20 x 92: the height does not change, no row table
    desc, tables = D.build_batch([(0, 0, 20, 90)], [p], 40)
    assert p.target == (20, 92) and int(desc[0, D.D_FLAGS]) == 1 and int(desc[0, D.D_KV]) == 0
    assert tables.size == 40 * (2 + int(desc[0, D.D_KH])) + 40 + 20
    p = D.IrnAugParams.explicit(20, 90, 40, 1.004, False, 3, 5)         # 20 x 90: neither axis changes, no table at all
    desc, tables = D.build_batch([(0, 0, 20, 90)], [p], 40)
    assert p.target == (20, 90) and int(desc[0, D.D_FLAGS]) == 0 and tables.size == 40 + 20


# ------------------------------------------------------------------------------------------------ resample_tables' default
PARENT_TABLES = {      # recorded from the commit before the filter argument
    (5, 3): ([[0, 3], [1, 3], [3, 2]], [[2396745, 1797559, 0, 0, 0], [932068, 2330169, 932068, 0, 0], [1797559, 2396745, 0, 0, 0]], 5),
    (4, 7): ([[0, 1], [0, 2], [0, 2], [1, 2], [2, 2], [2, 2], [3, 1]],
             [[4194304, 0, 0], [2696338, 1497966, 0], [299593, 3894711, 0], [2097152, 2097152, 0], [3894711, 299593, 0],
              [1497966, 2696338, 0], [4194304, 0, 0]], 3),
    (9, 4): ([[0, 3], [1, 5], [3, 5], [6, 3]],
             [[1557884, 1797559, 838861, 0, 0, 0, 0], [306900, 1125301, 1739102, 920701, 102300, 0, 0],
              [102300, 920701, 1739102, 1125301, 306900, 0, 0], [838861, 1797559, 1557884, 0, 0, 0, 0]], 7),
    (6, 6): ([[0, 2], [1, 2], [2, 2], [3, 2], [4, 2], [5, 1]],
             [[4194304, 0, 0], [4194304, 0, 0], [4194304, 0, 0], [4194304, 0, 0], [4194304, 0, 0], [4194304, 0, 0]], 3),
    (7, 2): ([[0, 5], [2, 5]], [[877878, 1268045, 1072961, 682794, 292626, 0, 0, 0, 0],
                                [292626, 682794, 1072961, 1268045, 877878, 0, 0, 0, 0]], 9),
}


def test_resample_tables_default_is_unchanged():
    for (n_in, n_out), (bounds, kk, ksize) in PARENT_TABLES.items():
        b, k, ks = pil_tables.resample_tables(n_in, n_out)
        assert ks == ksize and b.dtype == np.int32 and k.dtype == np.int32
        assert b.tobytes() == np.asarray(bounds, np.int32).tobytes() and k.tobytes() == np.asarray(kk, np.int32).tobytes()
        b2, k2, ks2 = pil_tables.resample_taps(n_in, n_out, np.arange(n_out), "bilinear")      # the vectorised form agrees
        assert ks2 == ks and np.array_equal(b2, b) and np.array_equal(k2, k)
        assert np.array_equal(pil_tables.nearest_taps(n_in, n_out, np.arange(n_out)), pil_tables.nearest_index(n_in, n_out))


# ------------------------------------------------------------------------------------------------------------- validation
def _valid():
    p = D.IrnAugParams.explicit(64, 48, 40, 1.27, False, 5, 3)
    desc, tables = D.build_batch([(0, 0, 64, 48)], [p], 40)
    return desc, tables


def test_validation_accepts_a_built_batch_and_names_what_it_refuses():
    desc, tables = _valid()
    D.validate_batch(desc, tables, 40, 64 * 48 * 3, 64 * 48)
    bad = tables.copy()
    off = int(desc[0, D.D_COLB])
    bad[off + 2 * 39] = 47                                   # the last column's first tap at the image's last column, 4+ taps long
    with pytest.raises(ValueError, match="column tap reads outside its image"):
        D.validate_batch(desc, bad, 40, 64 * 48 * 3, 64 * 48)
    bad = tables.copy()
    bad[int(desc[0, D.D_YNN])] = 64
    with pytest.raises(ValueError, match="label row index reads outside its image"):
        D.validate_batch(desc, bad, 40, 64 * 48 * 3, 64 * 48)
    d2 = desc.copy()
    d2[0, D.D_CB] += 8
    d2[0, D.D_IB] += 8
    with pytest.raises(ValueError, match="outside the crop of 40"):
        D.validate_batch(d2, tables, 40, 64 * 48 * 3, 64 * 48)
    with pytest.raises(ValueError, match="outside the image arena"):
        D.validate_batch(desc, tables, 40, 64 * 48 * 3 - 1, 64 * 48)
    with pytest.raises(ValueError, match="not a positive multiple of 4"):
        D.validate_batch(desc, tables, 42, 64 * 48 * 3, 64 * 48)
    with pytest.raises(ValueError, match="not a positive multiple of 4"):
        D.build_batch([(0, 0, 64, 48)], [D.IrnAugParams.top_left(64, 48, 42)], 42)
    # a scale below the kernel's reach is refused, not run
    p = D.IrnAugParams.explicit(400, 400, 40, 0.2, False, 0, 0)
    desc, tables = D.build_batch([(0, 0, 400, 400)], [p], 40)
    with pytest.raises(ValueError, match="scale too small"):
        D.validate_batch(desc, tables, 40, 400 * 400 * 3, 400 * 400)


def _write_list(tmp_path, names, images, labels):
    root, lab = tmp_path / "train2014", tmp_path / "ir_label"
    root.mkdir()
    lab.mkdir()
    for name, img, label in zip(names, images, labels):
        i = name.split("_")[-1]
        Image.fromarray(img).save(root / f"COCO_train2014_{i.zfill(12)}.jpg", format="PNG")       # lossless, under the name the rule wants
        if label is not None:
            Image.fromarray(label).save(lab / f"{name}.png")
    (tmp_path / "names.json").write_text(json.dumps(names))
    return str(tmp_path / "names.json"), str(lab), str(root)


def test_index_refuses_by_name(tmp_path):
    names = ["x_0_7", "x_1_8", "x_2_9"]
    images = [O.synthetic_image(0), O.synthetic_image(4), O.synthetic_image(1)]
    labels = [O.synthetic_label(0), None, O.synthetic_label(2)]           # the second is missing, the third has another image's size
    lst, lab, root = _write_list(tmp_path, names, images, labels)
    with pytest.raises(ValueError, match="not a positive multiple of 4"):
        D.ReferAffinityData(lst, lab, root, crop_size=42)
    data = D.ReferAffinityData(lst, lab, root, crop_size=40)
    assert len(data) == 3 and data.image_path(0).endswith("COCO_train2014_000000000007.jpg")
    assert np.array_equal(data.load_image(0), images[0]) and np.array_equal(data.load_label(0, (37, 53)), labels[0])
    grey = data.load_image(1)
    assert grey.shape == (45, 60, 3) and np.array_equal(grey[..., 0], images[1]) and np.array_equal(grey[..., 2], images[1])
    with pytest.raises(FileNotFoundError, match="x_1_8.png"):
        data.load_label(1, (45, 60))
    with pytest.raises(ValueError, match="x_2_9.png is 51x80"):
        data.load_label(2, (64, 48))
    assert D.ReferAffinityData(lst, lab, str(tmp_path / "referit"), 40).image_path(0).endswith("referit/7.jpg")


def test_pack_arena_aligns_every_offset():
    arrays = [np.full(n, i + 1, np.uint8) for i, n in enumerate((5, 16, 33))]
    arena, offs = D.pack_arena(arrays, 16, 16)
    assert offs == [0, 16, 32] and arena.size == 32 + 48 + 16
    assert all(np.array_equal(arena[o:o + a.size], a) for a, o in zip(arrays, offs))


# ------------------------------------------------------------------------------------------------------------ command line
def test_train_irn_parser_has_the_reference_flags_and_defaults(capsys):
    from tris_amd import train_irn
    a = train_irn.get_parser().parse_args(["--train_list", "n.json", "--ir_label_out_dir", "L", "--voc12_root", "I",
                                           "--irn_weights_name", "w.pth"])
    assert (a.irn_crop_size, a.irn_batch_size, a.irn_num_epoches, a.irn_learning_rate, a.irn_weight_decay) == (512, 32, 3, 0.1, 1e-4)
    assert a.work_space is None and a.num_workers == 0 and a.seed == 0 and a.irn_backbone_weights is None
    a = train_irn.get_parser().parse_args(["--train_list", "n.json", "--ir_label_out_dir", "L", "--voc12_root", "I",
                                           "--irn_weights_name", "w.pth", "--work_space", "ws", "--num_workers", "12",
                                           "--irn_crop_size", "128", "--irn_batch_size", "2", "--irn_num_epoches", "1",
                                           "--irn_learning_rate", "0.05", "--irn_weight_decay", "0", "--seed", "5",
                                           "--irn_backbone_weights", "r50.pth"])
    assert (a.num_workers, a.irn_crop_size, a.seed, a.irn_backbone_weights) == (12, 128, 5, "r50.pth")
    with pytest.raises(SystemExit) as e:
        train_irn.main(["--train_list", "n.json", "--ir_label_out_dir", "L", "--voc12_root", "I", "--irn_weights_name", "w.pth"])
    assert "--irn_backbone_weights FILE is required" in str(e.value) and "never downloads" in str(e.value)
