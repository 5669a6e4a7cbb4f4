"""Instance-mask synthesis on the MI355X (csrc/insseg.hip, tris_amd/irn.py): every stage fed the input the reference recorded for
that stage (tests/golden/g14_insseg.npz), so the stages are judged independently, then end to end against the numpy oracle
(tests/oracle_insseg.py)."""
import json
import os

import numpy as np
import pytest
import torch

import oracle_insseg as O
from oracle_insseg import scenes

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def g14(golden):
    return golden("g14_insseg.npz")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.cpu().numpy()


def tables():
    from tris_amd import irn
    return irn.device_tables(torch.device("cuda"))


# --------------------------------------------------------------------------------------------------------- centroids
def test_centroids_equal_the_reference_everywhere(g14):
    from tris_amd import irn, ops
    for i, s in scenes(g14):
        got = host(ops.irn_centroids(dev(s["dp"])))
        assert got.dtype == np.int32 and np.array_equal(got, s["centroids"]), i
        assert np.array_equal(irn.find_centroids_with_refinement(s["dp"]), s["centroids"])
    # fewer iterations and a field that pushes against the border: still the oracle's, bit for bit
    rng = np.random.default_rng(5)
    dp = (rng.standard_normal((2, 13, 17)) * 3).astype(np.float32)
    for it in (1, 7, 50):
        assert np.array_equal(host(ops.irn_centroids(dev(dp), it)), O.find_centroids(dp, it)), it


# ------------------------------------------------------------------------------------------------ connected components
def spiral(n):
    m = np.zeros((n, n), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    for _ in range(n * n):
        ny, nx = y + dy, x + dx
        ahead = (ny + dy, nx + dx)
        blocked = not (0 <= ny < n and 0 <= nx < n) or m[ny, nx] or \
            (0 <= ahead[0] < n and 0 <= ahead[1] < n and m[ahead])
        if blocked:
            dy, dx = dx, -dy
            ny, nx = y + dy, x + dx
            ahead = (ny + dy, nx + dx)
            if not (0 <= ny < n and 0 <= nx < n) or m[ny, nx] or (0 <= ahead[0] < n and 0 <= ahead[1] < n and m[ahead]):
                break
        y, x = ny, nx
        m[y, x] = 1
    return m


def adversarial_masks():
    out = {"spiral": spiral(41), "spiral_inverse": 1 - spiral(30), "single": np.zeros((9, 11), np.uint8),
           "ones": np.ones((33, 70), np.uint8), "zeros": np.zeros((12, 5), np.uint8),
           "checker": (np.indices((37, 53)).sum(0) % 2).astype(np.uint8),
           "width1": (np.arange(67) % 5 != 0).astype(np.uint8)[:, None], "height1": (np.arange(300) % 7 != 3).astype(np.uint8)[None]}
    out["single"][4, 6] = 1
    u = np.zeros((40, 31), np.uint8)         # a U: two long arms that meet only in the last row
    u[:, 2] = u[:, 28] = u[39, 2:29] = 1
    out["u_late_merge"] = u
    comb = np.zeros((50, 64), np.uint8)      # a comb whose teeth join at the bottom, next to a detached tooth
    comb[:, ::2] = 1
    comb[49, :40] = 1
    out["comb"] = comb
    rng = np.random.default_rng(3)
    out["noise"] = (rng.random((120, 159)) < 0.58).astype(np.uint8)
    return out


def test_cc_label_equals_the_oracle_on_adversarial_shapes():
    from tris_amd import ops
    for name, m in adversarial_masks().items():
        want, n = O.cc_label(m)
        lab, cnt = ops.cc_label(dev(m))
        assert lab.dtype == torch.int32 and int(cnt.item()) == n, name
        assert np.array_equal(host(lab), want), name


def test_cc_label_batch_of_differing_images(g14):
    from tris_amd import ops
    rng = np.random.default_rng(11)
    batch = np.stack([(rng.random((45, 38)) < p).astype(np.uint8) for p in (0.0, 0.2, 0.5, 0.62, 0.9, 1.0)] + [spiral(45)[:, :38]])
    lab, cnt = ops.cc_label(dev(batch))
    for b in range(len(batch)):
        want, n = O.cc_label(batch[b])
        assert int(cnt[b]) == n and np.array_equal(host(lab[b]), want), b
    for i, s in scenes(g14):                                  # the golden's own masks: the instance planes of the label map
        K = len(s["rw"])
        masks = (s["labels"][None] == np.arange(1, K + 1)[:, None, None]).astype(np.uint8)
        lab, cnt = ops.cc_label(dev(masks))
        for k in range(K):
            want, n = O.cc_label(masks[k])
            assert int(cnt[k]) == n and np.array_equal(host(lab[k]), want), (i, k)


def test_instance_map_equals_the_reference(g14):
    from tris_amd import irn, ops
    for i, s in scenes(g14):
        dp = dev(s["dp"])
        weak = ops.irn_weak_mask(dp)
        assert np.array_equal(host(weak).astype(bool), O.weak_mask(s["dp"]))
        lab, cnt = ops.cc_label(weak)
        inst, k = ops.irn_cluster(dev(s["centroids"], torch.int32), lab, int(cnt.item()))
        K = int(s["instance_map"].max()) + 1
        assert int(k.item()) == K and np.array_equal(host(inst), s["instance_map"]), i
        onehot = irn.cluster_centroids(s["centroids"].astype(np.int32), s["dp"])
        assert onehot.dtype == bool and np.array_equal(onehot, s["instance_map"][None] == np.arange(K)[:, None, None])
        icam = ops.irn_instance_cam(dev(s["instance_cam"].sum(0)), inst, K)
        assert np.array_equal(host(icam), s["instance_cam"])
        # the resize of the response map on its recorded input.  Both sides are f32 with a source coordinate scale * index whose
        # f32 scale is half an ulp off, so a blend weight is up to index * eps off: (max(H, W) + 4) eps of the map's maximum
        # (4 for the roundings of the blend itself)
        H, W = s["size"]
        cams = ops.resize_bilinear(dev(s["cam"])[None, None], s["edge"].shape, True)[0, 0]
        got = host(ops.irn_instance_cam(cams, dev(s["instance_map"], torch.int32), K))
        err = np.abs(got - s["instance_cam"]).max()
        print(f"scene {i}: resized response map error {err / (EPS * s['cam'].max()):.2f} eps of the maximum")
        assert err <= (max(H, W) + 4) * EPS * s["cam"].max(), i


# --------------------------------------------------------------------------------------------------------- affinity
def test_affinity_and_column_sums_at_f32_rounding(g14):
    """a = 1 - max(edge) carries half an ulp, which a^beta multiplies by beta = 10 -> 5 ulp, plus the power function's own error
    (at most 2 ulp; the device library documents 1) and the final rounding: 8 ulp of the weight.  The column sum adds 68 such
    weights to 1 in float64 and rounds once: their 8 ulp and half an ulp of the sum, 8.5 ulp."""
    from tris_amd import ops
    for i, s in scenes(g14):
        Wt, colsum = ops.irn_affinity(dev(s["edge"]), *tables(), int(g14["beta"]))
        want_w, want_c = O.affinity(s["edge"], int(g14["beta"]))
        err_w = np.abs(host(Wt) - want_w)
        err_c = np.abs(host(colsum) - want_c)
        print(f"scene {i}: weights {np.max(err_w / np.maximum(want_w, 1e-30)) / EPS:.2f} ulp, column sums {np.max(err_c / want_c) / EPS:.2f} ulp")
        assert (err_w <= 8 * EPS * want_w).all(), i
        assert (host(Wt)[want_w == 0] == 0).all()
        assert (err_c <= 8.5 * EPS * want_c).all(), i


# ------------------------------------------------------------------------------------------------------------- walk
def test_walk_within_twice_the_reference_noise(g14):
    """e_ref = max |golden rw - oracle rw| / max |oracle rw| is the reference's own f32 noise; the kernel's same quantity must be
    <= 2 e_ref (two f32 evaluations with different summation orders are each that far from the f64 value).  One form of the
    walk exists: the LDS-resident one was measured slower and removed ("Instance-mask synthesis")."""
    from tris_amd import ops
    for i, s in scenes(g14):
        want = O.propagate_to_edge(s["instance_cam"].astype(np.float64), s["edge"], int(g14["beta"]), int(g14["exp_times"]))
        top = np.abs(want).max()
        e_ref = np.abs(s["rw"] - want).max() / top
        edge = dev(s["edge"])
        Wt, colsum = ops.irn_affinity(edge, *tables(), int(g14["beta"]))
        got = host(ops.irn_walk(dev(s["instance_cam"]), edge, Wt, colsum, tables()[0], 2 ** int(g14["exp_times"])))
        e = np.abs(got - want).max() / top
        print(f"scene {i}: e_ref {e_ref:.3e}  kernel {e:.3e}")
        assert e <= 2 * e_ref, i


def test_walk_large_map_against_the_sparse_oracle(g14):
    """160 x 160, K = 3: beyond any dense reference; bound: twice the largest e_ref of the recorded scenes"""
    from tris_amd import ops
    from tris_amd.utils.synth import make_ins_seg_scene
    e_ref = 0.0
    for _, s in scenes(g14):
        want = O.propagate_to_edge(s["instance_cam"].astype(np.float64), s["edge"], int(g14["beta"]), int(g14["exp_times"]))
        e_ref = max(e_ref, np.abs(s["rw"] - want).max() / np.abs(want).max())
    cam, edge, dp = make_ins_seg_scene(640, 640, n_blobs=4, seed=2)
    rng = np.random.default_rng(4)
    x = (cam[::4, ::4][None] * (rng.random((3, 160, 160)) < 0.5)).astype(np.float32)
    Wt, colsum = ops.irn_affinity(dev(edge), *tables(), 10)
    got = host(ops.irn_walk(dev(x), dev(edge), Wt, colsum, tables()[0], 256))
    want = O.propagate_to_edge(x.astype(np.float64), edge, 10, 8)
    e = np.abs(got - want).max() / np.abs(want).max()
    print(f"160x160 K=3: e {e:.3e} (bound {2 * e_ref:.3e})")
    assert e <= 2 * e_ref


@pytest.mark.parametrize("exp_times", [0, 3, 8])
def test_propagate_to_edge(g14, exp_times):
    from tris_amd import irn
    for i, s in scenes(g14):
        x = s["instance_cam"][:, None]
        want = O.propagate_to_edge(s["instance_cam"].astype(np.float64), s["edge"], int(g14["beta"]), exp_times)
        ref8 = O.propagate_to_edge(s["instance_cam"].astype(np.float64), s["edge"], int(g14["beta"]), int(g14["exp_times"]))
        e_ref = np.abs(s["rw"] - ref8).max() / np.abs(ref8).max()
        got = irn.propagate_to_edge(x, s["edge"], radius=5, beta=int(g14["beta"]), exp_times=exp_times)
        assert got.shape == (len(x), 1) + s["edge"].shape and got.dtype == np.float32
        assert np.abs(got[:, 0] - want).max() / np.abs(want).max() <= 2 * e_ref, i
        t = irn.propagate_to_edge(dev(x), dev(s["edge"]), exp_times=exp_times)
        assert t.is_cuda and np.abs(host(t)[:, 0] - want).max() / np.abs(want).max() <= 2 * e_ref


# ----------------------------------------------------------------------------------------------------------- finish
def test_finish_on_the_recorded_walk(g14):
    """rw_up: three interpolations (a difference, a product and a sum each) and the division by the maximum, every operation
    half an ulp of a value <= the maximum, which the division maps to 1: 8 ulp of 1.  Labels: equal wherever the oracle's top-1 /
    top-2 gap is >= 1e-3, and those pixels are all but 0.5 %."""
    from tris_amd import ops
    for i, s in scenes(g14):
        up, labels = ops.irn_finish(dev(s["rw"]), s["size"], float(g14["bg_thres"]))
        want_up, want_labels, gap = O.finish(s["rw"].astype(np.float64), s["size"], float(g14["bg_thres"]))
        assert tuple(up.shape) == (len(s["rw"]),) + s["size"] and labels.dtype == torch.int32
        err = np.abs(host(up) - want_up).max()
        print(f"scene {i}: rw_up error {err / EPS:.2f} ulp of 1, undecided share {(gap < 1e-3).mean():.5f}")
        assert err <= 8 * EPS and np.abs(host(up) - s["rw_up"]).max() <= 8 * EPS
        decided = gap >= 1e-3
        assert (~decided).mean() <= 0.005
        assert np.array_equal(host(labels)[decided], s["labels"][decided]) and np.array_equal(want_labels[decided], s["labels"][decided])


# -------------------------------------------------------------------------------------------------------- fragments
def test_fragments_on_the_recorded_label_map(g14):
    from tris_amd import irn
    zeros = 0
    for i, s in scenes(g14):
        K = len(s["rw"])
        H, W = s["size"]
        masks = s["labels"][None] == np.arange(1, K + 1)[:, None, None]
        det = irn.detect_instance(s["rw_up"], masks, np.zeros(K, np.int64), max_fragment_size=H * W * 0.01)
        assert det["mask"].dtype == bool and np.array_equal(det["mask"], s["det_mask"]), i           # masks and their order
        assert det["class"].dtype == s["det_class"].dtype and np.array_equal(det["class"], s["det_class"])
        assert det["score"].dtype == s["det_score"].dtype
        assert np.abs(det["score"] - s["det_score"]).max() <= EPS                                    # a max of recorded values
        small = s["det_mask"].reshape(len(s["det_mask"]), -1).sum(1) < H * W * 0.01
        assert (det["score"][small] == 0).all() and (det["score"][~small] > 0).all()
        zeros += int(small.sum())
        det0 = irn.detect_instance(s["rw_up"], masks, np.zeros(K, np.int64))                         # no size limit
        assert (det0["score"] > 0).all() and det0["score"].dtype == np.float32
    assert zeros >= 1


def test_fragments_with_several_components_per_row():
    """what detect_instance exists for: rows whose masks fall into many fragments.  Rows with hundreds of fragments that share
    64-pixel waves (checkerboard, noise: the per-lane atomics), a comb, and an empty row between them (a zero count inside the
    offsets); masks, their (row, raster) order, classes, areas and scores against the oracle, with and without the size limit."""
    from tris_amd import irn, ops
    H, W = 50, 64
    shapes = adversarial_masks()
    rng = np.random.default_rng(8)
    rows = [shapes["comb"], (np.indices((H, W)).sum(0) % 2).astype(np.uint8), np.zeros((H, W), np.uint8),
            shapes["noise"][:H, :W], (rng.random((H, W)) < 0.3).astype(np.uint8)]
    masks = np.stack(rows).astype(bool)
    score_map = rng.random((len(rows), H, W)).astype(np.float32)
    score_map[4] = 0                                   # a row whose scores are all 0
    class_id = np.array([3, 1, 4, 1, 5], np.int64)
    counts = [O.cc_label(m)[1] for m in masks]
    assert counts[2] == 0 and min(counts[0], counts[1], counts[3], counts[4]) > 10
    for limit in (0, 3.5, 40.0):
        want = O.detect_instance(score_map, masks, class_id, limit)
        got = irn.detect_instance(score_map, masks, class_id, max_fragment_size=limit)
        assert got["mask"].shape == (sum(counts), H, W) and np.array_equal(got["mask"], want["mask"]), limit
        assert got["class"].dtype == np.int64 and np.array_equal(got["class"], want["class"])
        assert got["score"].dtype == want["score"].dtype and np.array_equal(got["score"], want["score"]), limit
    # the op itself: areas and the fragment order through the offsets
    fl, cnt = ops.cc_label(dev(masks.astype(np.uint8)))
    assert cnt.cpu().tolist() == counts
    score, area, fm = ops.irn_fragments(fl, counts, dev(score_map), 4)
    want = O.detect_instance(score_map, masks, class_id, 4)
    assert np.array_equal(host(area), want["mask"].reshape(len(want["mask"]), -1).sum(1))
    assert np.array_equal(host(fm).astype(bool), want["mask"]) and np.array_equal(host(score), want["score"].astype(np.float32))


# ------------------------------------------------------------------------------------------------------- end to end
def labels_of(cam, bg):
    return np.argmax(np.concatenate([np.full((1,) + cam.shape[1:], bg, cam.dtype), cam]), 0)


def check_end_to_end(out, cam, edge, dp, size, bg, golden_labels=None):
    ora = O.make_ins_seg(cam, edge, dp, size, ins_seg_bg_thres=bg)
    K = ora["K"]
    assert out["cam"].dtype == np.float32 and out["cam"].shape == (K,) + tuple(size)
    # raw inputs: the walk may be 2 e_ref (2.5e-5 on the recorded scenes) off, in the numerator and in the maximum it is divided by
    assert np.abs(out["cam"] - ora["rw_up"]).max() <= 1e-4
    labels = labels_of(out["cam"], np.float32(bg))
    decided = ora["gap"] >= 1e-3
    assert (~decided).mean() <= 0.005
    assert np.array_equal(labels[decided], ora["labels"][decided])
    if golden_labels is not None:
        assert np.array_equal(labels[decided], golden_labels[decided])
    # the fragments are the oracle's detect_instance of the kernel's own label map and maps
    masks = labels[None] == np.arange(1, K + 1)[:, None, None]
    want = O.detect_instance(out["cam"], masks, np.zeros(K, np.int64), size[0] * size[1] * 0.01)
    assert out["mask"].dtype == bool and np.array_equal(out["mask"], want["mask"])
    assert np.array_equal(out["class"], want["class"]) and out["class"].dtype == np.int64
    assert out["score"].dtype == want["score"].dtype and np.array_equal(out["score"], want["score"])
    return want


def test_make_ins_seg_end_to_end(g14):
    from tris_amd import irn
    for i, s in scenes(g14):
        out = irn.make_ins_seg(s["cam"], s["edge"], s["dp"], s["size"], beta=int(g14["beta"]), exp_times=int(g14["exp_times"]),
                               ins_seg_bg_thres=float(g14["bg_thres"]))
        assert set(out) == {"score", "mask", "class", "cam"}
        check_end_to_end(out, s["cam"], s["edge"], s["dp"], s["size"], float(g14["bg_thres"]), s["labels"])
        assert out["mask"].shape == s["det_mask"].shape and out["score"].dtype == s["det_score"].dtype


def test_saved_file_round_trips_into_the_stage2_target(g14, tmp_path):
    """what ReferDataset.load_pseudo does with the file: sum of the masks, NEAREST to size x size"""
    from PIL import Image
    from tris_amd import irn
    _, s = next(scenes(g14))
    out = irn.make_ins_seg(s["cam"], s["edge"], s["dp"], s["size"])
    np.save(tmp_path / "3_17.npy", out, allow_pickle=True)
    info = np.load(tmp_path / "3_17.npy", allow_pickle=True).item()
    got = np.asarray(Image.fromarray((info["mask"] * 1.0).sum(0)).resize((64, 64), Image.NEAREST))
    want = np.asarray(Image.fromarray((s["det_mask"] * 1.0).sum(0)).resize((64, 64), Image.NEAREST))
    gap = O.finish(s["rw"].astype(np.float64), s["size"], 0.25)[2]
    decided = np.asarray(Image.fromarray((gap >= 1e-3).astype(np.uint8)).resize((64, 64), Image.NEAREST)) > 0
    assert got.shape == (64, 64) and got.max() == 1 and np.array_equal(got[decided], want[decided])


def test_all_background_gives_empty_arrays(g14):
    """no pixel beats the background (threshold above the normalised maximum of 1): the reference fails in np.stack([]); here the
    arrays have a leading dimension of 0"""
    from tris_amd import irn
    _, s = next(scenes(g14))
    out = irn.make_ins_seg(s["cam"], s["edge"], s["dp"], s["size"], ins_seg_bg_thres=1.5)
    assert out["mask"].shape == (0,) + s["size"] and out["mask"].dtype == bool
    assert out["score"].shape == (0,) and out["class"].shape == (0,) and out["class"].dtype == np.int64
    assert out["cam"].shape == (len(s["rw"]),) + s["size"] and float(out["cam"].max()) == 1.0


def test_cli_output_is_a_pseudo_path(tmp_path):
    """python -m tris_amd.make_ins_seg on a two-name list; the output directory then serves ReferDataset(pseudo_path=...), which is
    what tris_amd.train_stage2 --pseudo_path builds"""
    from tris_amd import make_ins_seg
    from tris_amd.dataset.ReferDataset import ReferDataset
    from tris_amd.dataset.transform import get_transform
    from tris_amd.utils.synth import make_ins_seg_scene, make_mini_refer, word_hash_tokenize
    root = make_mini_refer(str(tmp_path / "data"), n_images=6, seed=1)
    plain = ReferDataset(root, "refcocog", "umd", image_transforms=get_transform(64, True), split="train", eval_mode=False,
                         size=64, tokenizer=word_hash_tokenize)
    D, E, Odir = (str(tmp_path / n) for n in ("cam", "irn", "ins_seg"))
    os.makedirs(D)
    os.makedirs(E)
    names, inputs = [], []
    for i in range(2):
        _, img_id, rec = plain.image_record(i)
        H, W = rec["height"], rec["width"]
        cam, edge, dp = make_ins_seg_scene(H, W, n_blobs=2, seed=i)
        names.append(f"{i}_{img_id}")
        np.save(os.path.join(D, names[-1] + ".npy"), cam)
        np.savez(os.path.join(E, names[-1] + ".npz"), edge=edge, dp=dp)
        inputs.append((cam, edge, dp, (H, W)))
    with open(tmp_path / "names.json", "w") as f:
        json.dump(names, f)
    make_ins_seg.main(["--cam_out_dir", D, "--irn_out_dir", E, "--ins_seg_out_dir", Odir, "--train_list", str(tmp_path / "names.json")])
    assert sorted(os.listdir(Odir)) == sorted(n + ".npy" for n in names)
    ds = ReferDataset(root, "refcocog", "umd", image_transforms=get_transform(64, True), split="train", eval_mode=False, size=64,
                      pseudo_path=Odir, tokenizer=word_hash_tokenize)
    for i, (cam, edge, dp, size) in enumerate(inputs):
        out = np.load(os.path.join(Odir, names[i] + ".npy"), allow_pickle=True).item()
        check_end_to_end(out, cam, edge, dp, size, 0.25)
        t = ds.load_pseudo(i)
        assert t.dtype == torch.int64 and tuple(t.shape) == (1, 64, 64) and int(t.max()) >= 1
