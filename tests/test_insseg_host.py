"""Instance-mask synthesis without a GPU: the numpy oracle (tests/oracle_insseg.py) against every stage the reference recorded
(tests/golden/g14_insseg.npz, tools/gen_golden_insseg.py), the host direction / path tables against PathIndex.search_paths, the
C ABI of csrc/insseg.hip, the no-CPU-fallback rule and the command line."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

import oracle_insseg as O
from oracle_insseg import golden_paths, scenes

ENTRY_POINTS = ["tris_irn_centroids_f32", "tris_irn_weak_mask_f32", "tris_cc_workspace_bytes", "tris_cc_label_u8",
                "tris_irn_cluster_i32", "tris_irn_instance_cam_f32", "tris_irn_affinity_f32", "tris_irn_walk_f32", "tris_irn_finish_f32", "tris_irn_label_masks_u8",
                "tris_irn_fragments_f32"]


@pytest.fixture(scope="module")
def g14(golden):
    return golden("g14_insseg.npz")


# ------------------------------------------------------------------------------------------------------ the goldens
def test_golden_is_what_the_tests_rely_on(g14):
    """>= 2 scenes with >= 3 instances, a fragment below 1 % somewhere (score exactly 0), an instance that splits into several
    fragments (so the recorded fragment order is more than the row order), map sizes that are not multiples of 4"""
    n3 = small = split = 0
    for _, s in scenes(g14):
        n3 += int(s["instance_map"].max()) + 1 >= 3
        H, W = s["size"]
        area = s["det_mask"].reshape(len(s["det_mask"]), -1).sum(1)
        assert ((s["det_score"] == 0) == (area < H * W * 0.01)).all()
        small += bool((area < H * W * 0.01).any())
        split += len(s["det_mask"]) > int(s["instance_map"].max()) + 1
        assert H % 4 and W % 4 and s["edge"].shape == ((H - 1) // 4 + 1, (W - 1) // 4 + 1)
    assert n3 >= 2 and small >= 1 and split >= 1
    assert any(s["edge"].shape[0] != s["edge"].shape[1] for _, s in scenes(g14))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g14_insseg.npz")) < 1 << 20


# ------------------------------------------------------------------------------------------- oracle against the reference
def test_oracle_integer_stages_are_exact(g14):
    for i, s in scenes(g14):
        cen = O.find_centroids(s["dp"])
        assert np.array_equal(cen, s["centroids"]), i
        inst, K = O.instance_map(s["centroids"].astype(np.int32), s["dp"])
        assert K == int(s["instance_map"].max()) + 1 and np.array_equal(inst, s["instance_map"]), i


def test_oracle_walk_within_reference_noise(g14):
    """the reference's own f32 noise against the float64 sparse walk.  The reference's dense f32 result was measured against a
    float64 sparse walk on random maps of this size at 4.3e-5 and 3.5e-5 of the map's maximum; the bound is twice the larger,
    8.6e-5.  The resized response map, the walk's input, is compared as well: torch forms the source coordinate as an f32 scale
    times the index, so a blend weight is up to index * eps off: (max(H, W) + 4) eps of the map's maximum."""
    for i, s in scenes(g14):
        rw = O.propagate_to_edge(s["instance_cam"].astype(np.float64), s["edge"], int(g14["beta"]), int(g14["exp_times"]))
        e_ref = np.abs(s["rw"] - rw).max() / np.abs(rw).max()
        print(f"scene {i}: e_ref = {e_ref:.3e}")
        assert e_ref < 2 * 4.3e-5, (i, e_ref)
        K = len(s["rw"])
        icam = O.resize_align_corners(s["cam"], *s["edge"].shape)[None] * (s["instance_map"][None] == np.arange(K)[:, None, None])
        e_cam = np.abs(icam - s["instance_cam"]).max()
        print(f"scene {i}: resized response map {e_cam:.3e}")
        assert e_cam <= (max(s["size"]) + 4) * np.finfo(np.float32).eps * s["cam"].max(), i


def test_oracle_finish_and_fragments(g14):
    for i, s in scenes(g14):
        up, labels, gap = O.finish(s["rw"], s["size"], float(g14["bg_thres"]))
        assert up.dtype == np.float32
        assert np.abs(up - s["rw_up"]).max() <= 4 * np.finfo(np.float32).eps     # rw_up <= 1; blend order differs by ulps
        decided = gap >= 1e-3
        assert (~decided).mean() <= 0.005 and np.array_equal(labels[decided], s["labels"][decided]), i
        K = len(s["rw"])
        H, W = s["size"]
        masks = s["labels"][None] == np.arange(1, K + 1)[:, None, None]
        det = O.detect_instance(s["rw_up"], masks, np.zeros(K, np.int64), H * W * 0.01)
        assert np.array_equal(det["mask"], s["det_mask"]) and np.array_equal(det["class"], s["det_class"])
        assert det["score"].dtype == s["det_score"].dtype and np.array_equal(det["score"], s["det_score"])


def test_oracle_cc_label_numbering():
    m = np.array([[0, 1, 0, 1], [1, 1, 0, 1], [0, 0, 0, 0], [1, 0, 1, 1]])
    lab, n = O.cc_label(m)
    assert n == 4 and np.array_equal(lab, [[0, 1, 0, 2], [1, 1, 0, 2], [0, 0, 0, 0], [3, 0, 4, 4]])
    try:                                  # where scipy is installed: its 4-neighbour labelling numbers components the same way
        import scipy.ndimage as scipy_ndimage
    except ImportError:
        return
    rng = np.random.default_rng(0)
    for p in (0.3, 0.55, 0.8):
        m = rng.random((23, 31)) < p
        want = scipy_ndimage.label(m, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
        lab, n = O.cc_label(m)
        assert n == want[1] and np.array_equal(lab, want[0])


def test_oracle_sparse_walk_equals_dense_matrix_power():
    """the algebra the kernels rest on: x T^(2^t) = 2^t gathers, against the dense float64 matrix at a toy size"""
    rng = np.random.default_rng(1)
    h, w, t = 7, 9, 3
    edge = rng.random((h, w))
    x = rng.random((2, h, w))
    Wt, colsum = O.affinity(edge, beta=4)
    n = h * w
    A = np.eye(n)
    for d, ((dy, dx), _) in enumerate(O.search_paths()):
        for y in range(h):
            for xx in range(w):
                if y + dy < h and 0 <= xx + dx < w:
                    i, j = y * w + xx, (y + dy) * w + xx + dx
                    A[i, j] = A[j, i] = Wt[d, y, xx]
    assert np.allclose(A.sum(0), colsum.reshape(-1), rtol=1e-13)
    T = np.linalg.matrix_power(A / A.sum(0, keepdims=True), 2 ** t)
    want = ((x * (1 - edge)).reshape(2, n) @ T).reshape(2, h, w)
    assert np.allclose(O.walk(x, edge, Wt, colsum, 2 ** t), want, rtol=1e-11, atol=1e-14)


# ----------------------------------------------------------------------------------------------------- host tables
def test_host_tables_equal_path_index(g14):
    from tris_amd import irn
    want = golden_paths(g14)
    assert len(want) == 34 and {len(c) for _, c in want} <= set(range(2, 12))
    for paths in (irn.search_paths(5), O.search_paths(5)):
        got = {(d, frozenset(cells)) for d, cells in paths}
        assert len(paths) == 34 and got == want
        assert all(d in cells and (0, 0) in cells for d, cells in paths)
    assert irn.search_dirs(5) == [d for d, _ in irn.search_paths(5)]


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_and_library_exports_the_entry_points():
    from tris_amd import _lib
    decls, _ = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIBPATH)
    for name in ENTRY_POINTS:
        assert name in decls, f"{name} is not declared in include/tris_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert _lib.query("tris_cc_workspace_bytes", 3, 10, 7) == 2 * 3 * 10 * 7 * 4
    src = open(os.path.join(ROOT, "include", "tris_hip.h")).read()
    assert src.count("labels.py:") >= 8 and src.count("indexing.py:") >= 3      # each declaration cites what it replaces


def test_new_ops_have_no_cpu_fallback():
    from tris_amd import irn, ops
    dp, edge, cam = torch.zeros(2, 5, 6), torch.zeros(5, 6), torch.zeros(18, 21)
    i32 = torch.zeros(2, 5, 6, dtype=torch.int32)
    tables = [torch.zeros(34, 2, dtype=torch.int32), torch.zeros(35, dtype=torch.int32), torch.zeros(200, 2, dtype=torch.int32)]
    calls = [lambda: ops.irn_centroids(dp), lambda: ops.irn_weak_mask(dp), lambda: ops.cc_label(torch.zeros(5, 6, dtype=torch.uint8)),
             lambda: ops.irn_cluster(i32, i32[0], 3), lambda: ops.irn_instance_cam(edge, i32[0], 2),
             lambda: ops.irn_affinity(edge, *tables), lambda: ops.irn_walk(dp, edge, torch.zeros(34, 5, 6), edge, tables[0], 4),
             lambda: ops.irn_finish(dp, (18, 21)), lambda: ops.irn_label_masks(i32[0], 2),
             lambda: ops.irn_fragments(i32, [1, 1], dp, 3),
             lambda: irn.propagate_to_edge(dp[:, None], edge), lambda: irn.find_centroids_with_refinement(dp),
             lambda: irn.cluster_centroids(i32, dp), lambda: irn.detect_instance(dp, dp > 0, [0, 0]),
             lambda: irn.make_ins_seg(cam, edge, dp, (18, 21))]
    for c in calls:
        with pytest.raises(ops.NoGpuError):
            c()
    if not torch.cuda.is_available():
        with pytest.raises(ops.NoGpuError):
            irn.make_ins_seg(cam.numpy(), edge.numpy(), dp.numpy(), (18, 21))


def test_radius_other_than_5_is_refused():
    from tris_amd import irn
    with pytest.raises(NotImplementedError):
        irn.propagate_to_edge(torch.zeros(1, 1, 4, 4), torch.zeros(4, 4), radius=3)


def test_cli_argument_names():
    from tris_amd.make_ins_seg import get_parser
    a = get_parser().parse_args(["--cam_out_dir", "D", "--irn_out_dir", "E", "--ins_seg_out_dir", "O", "--train_list", "n.json"])
    assert (a.cam_out_dir, a.irn_out_dir, a.ins_seg_out_dir, a.train_list) == ("D", "E", "O", "n.json")
    assert (a.beta, a.exp_times, a.ins_seg_bg_thres) == (10, 8, 0.25)
    a = get_parser().parse_args(["--cam_out_dir", "D", "--irn_out_dir", "E", "--ins_seg_out_dir", "O", "--train_list", "n.json",
                                 "--beta", "8", "--exp_times", "6", "--ins_seg_bg_thres", "0.3"])
    assert (a.beta, a.exp_times, a.ins_seg_bg_thres) == (8, 6, 0.3)
    with pytest.raises(SystemExit):
        get_parser().parse_args(["--cam_out_dir", "D"])


def test_empty_result_loads_as_an_all_zero_target(tmp_path):
    """the stated difference from the reference: no pixel beats the background -> arrays with a leading dimension of 0, which
    ReferDataset.load_pseudo's expression turns into an all-zero target"""
    from PIL import Image
    det = O.detect_instance(np.zeros((2, 9, 11), np.float32), np.zeros((2, 9, 11), bool), [0, 0], 1.0)
    assert det["mask"].shape == (0, 9, 11) and det["score"].shape == (0,) and det["class"].shape == (0,)
    np.save(tmp_path / "0_1.npy", det, allow_pickle=True)
    info = np.load(tmp_path / "0_1.npy", allow_pickle=True).item()
    gt = np.asarray(Image.fromarray((info["mask"] * 1.0).sum(0)).resize((8, 8), Image.NEAREST))
    assert gt.shape == (8, 8) and not gt.any()
