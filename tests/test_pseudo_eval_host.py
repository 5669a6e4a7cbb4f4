"""Host side of the artefact scoring (tris_amd/pseudo_eval.py, tris_amd/eval_pseudo.py): names, thresholds, aggregation, the
command line.  No GPU."""
import json
import math

import numpy as np
import pytest

import oracle_pseudo_eval as O


@pytest.fixture(scope="module")
def mini(tmp_path_factory):
    from tris_amd.dataset.ReferDataset import ReferDataset
    from tris_amd.utils.synth import make_mini_refer, word_hash_tokenize
    root = make_mini_refer(str(tmp_path_factory.mktemp("pe") / "data"), n_images=5, seed=3, max_side=40)
    ds = ReferDataset(refer_data_root=root, dataset="refcocog", splitBy="umd", split="train", eval_mode=True,
                      tokenizer=word_hash_tokenize)
    return root, ds


# ------------------------------------------------------------------------------------------------------------------ names
def test_both_name_forms_parse(mini):
    from tris_amd import pseudo_eval as pe
    _, ds = mini
    assert pe.parse_name("12_581857") == (12, "581857")
    assert pe.parse_name("12_3_581857") == (12, "581857")
    for bad in ("12", "a_5", "1_2_3_4", "1__5", "-1_5"):
        with pytest.raises(ValueError, match="neither"):
            pe.parse_name(bad)
    plain = [f"{i}_{ds.image_record(i)[1]}" for i in range(len(ds))]
    sent = [f"{i}_{j}_{ds.image_record(i)[1]}" for i in range(len(ds)) for j in range(len(ds.all_sentences[i]))]
    assert pe.resolve_names(plain, ds) == list(range(len(ds)))
    assert pe.resolve_names(sent, ds) == [i for i in range(len(ds)) for _ in ds.all_sentences[i]]


def test_mismatched_image_id_and_out_of_range_index_are_refused(mini):
    from tris_amd import pseudo_eval as pe
    _, ds = mini
    img = ds.image_record(1)[1]
    wrong = f"1_{img + 1}"
    with pytest.raises(ValueError) as e:
        pe.resolve_names([f"0_{ds.image_record(0)[1]}", wrong], ds)
    assert repr(wrong) in str(e.value) and "image id" in str(e.value)
    beyond = f"{len(ds)}_0_{img}"
    with pytest.raises(ValueError) as e:
        pe.resolve_names([beyond], ds)
    assert repr(beyond) in str(e.value) and "outside" in str(e.value)


# ------------------------------------------------------------------------------------------------------------------ thresholds
def test_threshold_list_is_validated():
    from tris_amd import ops
    from tris_amd.pseudo_eval import default_thresholds
    d = default_thresholds()
    assert len(d) == 20 and d[0] == 1e-9 and d[1] == 0.05 and d[-1] == 0.95 and d[10] == 0.5
    t = ops.ScoreThresholds(d)
    assert t.host.dtype == np.float32 and len(t) == 20
    assert len(ops.ScoreThresholds(np.linspace(0, 1, 64))) == 64
    with pytest.raises(ValueError, match="strictly ascending.*entry 1"):
        ops.ScoreThresholds([0.1, 0.3, 0.2])
    with pytest.raises(ValueError, match="strictly ascending.*entry 0"):
        ops.ScoreThresholds([0.25, 0.25])
    with pytest.raises(ValueError, match="strictly ascending"):
        ops.ScoreThresholds([1.0, 1.0 + 1e-12])                  # (equal once they are float32)
    with pytest.raises(ValueError, match="entry 1 = nan is not finite"):
        ops.ScoreThresholds([0.1, float("nan")])
    with pytest.raises(ValueError, match="not finite"):
        ops.ScoreThresholds([0.1, float("inf")])
    with pytest.raises(ValueError, match="not finite"):
        ops.ScoreThresholds([0.1, 1e39])                         # (infinite as float32)
    with pytest.raises(ValueError, match="T = 65"):
        ops.ScoreThresholds(np.linspace(0, 1, 65))
    with pytest.raises(ValueError, match="T = 0"):
        ops.ScoreThresholds([])


def test_command_line_threshold_list():
    from tris_amd.eval_pseudo import parse_thresholds
    assert parse_thresholds("0.1,0.25").host.tolist() == [np.float32(0.1), np.float32(0.25)]
    assert len(parse_thresholds(None)) == 20
    with pytest.raises(ValueError, match="comma-separated"):
        parse_thresholds("0.1;0.2")
    with pytest.raises(ValueError, match="strictly ascending"):
        parse_thresholds("0.2,0.1")


# ------------------------------------------------------------------------------------------------------------------ numbers
def _close(got, want):
    assert got.keys() == want.keys(), (got.keys(), want.keys())
    for k in want:
        g, w = got[k], want[k]
        if isinstance(w, list):
            assert len(g) == len(w), k
            for a, b in zip(g, w):
                assert (a is None and b is None) or math.isclose(a, b, rel_tol=1e-12, abs_tol=1e-12), (k, g, w)
        elif w is None or isinstance(w, int):
            assert g == w and type(g) is type(w), (k, g, w)
        else:
            assert math.isclose(g, w, rel_tol=1e-12, abs_tol=1e-12), (k, g, w)
    json.dumps(got)                          # (plain Python numbers and None: it serialises, None as null)


def _scene(rng, n, h=9, w=7):
    gts = [rng.rand(h, w) < 0.4 for _ in range(n)]
    gts[0][:] = False                        # an empty ground truth: with an empty prediction U = 0
    return gts


def test_summarise_cams_against_the_oracle():
    from tris_amd import pseudo_eval as pe
    rng = np.random.RandomState(0)
    thr = [1e-9, 0.2, 0.3, 0.4, 0.9]
    gts = _scene(rng, 6)
    maps = [rng.rand(9, 7).astype(np.float32) for _ in gts]
    maps[0][:] = 0                                                  # U = 0 at every threshold
    maps[1][3, 3] = np.nan
    maps[2][2, 2] = np.float32(0.3)                                 # equal to a threshold: not above it
    hist = O.maps_hist(np.stack(maps), np.stack(gts), thr)
    I, U = pe.sweep_iu(hist)
    for n, (m, g) in enumerate(zip(maps, gts)):
        for j, t in enumerate(np.asarray(thr, np.float32)):
            with np.errstate(invalid="ignore"):
                assert (int(I[n, j]), int(U[n, j])) == O.iu(m > t, g), (n, j)
    assert U[0].tolist() == [0] * 5
    _close(pe.summarise_cams(hist, thr), O.cams_summary(maps, gts, thr))
    none = pe.summarise_cams(np.zeros((0, 6, 2), np.int64), thr)
    assert none["names"] == 0 and none["mIoU"] == [None] * 5 and none["best_threshold"] is None
    _close(none, O.cams_summary([], [], thr))


def test_best_threshold_is_the_first_on_ties():
    from tris_amd import pseudo_eval as pe
    rng = np.random.RandomState(1)
    gts = _scene(rng, 4)
    maps = [np.where(g, 0.7, 0.1).astype(np.float32) * (rng.rand(*g.shape) < 0.8) for g in gts]    # values 0, 0.1, 0.7 only
    thr = [0.05, 0.2, 0.3, 0.6, 0.8]                               # 0.2, 0.3 and 0.6 cut the same pixels: one mIoU, the best
    got = pe.summarise_cams(O.maps_hist(np.stack(maps), np.stack(gts), thr), thr)
    assert got["mIoU"][1] == got["mIoU"][2] == got["mIoU"][3] > max(got["mIoU"][0], got["mIoU"][4])
    assert got["best_threshold"] == 0.2 and got["best_mIoU"] == got["mIoU"][1]
    _close(got, O.cams_summary(maps, gts, thr))


def test_summarise_labels_and_masks_against_the_oracle():
    from tris_amd import pseudo_eval as pe
    rng = np.random.RandomState(2)
    gts = _scene(rng, 5)
    labels = [rng.choice(np.array([0, 1, 255], np.uint8), size=g.shape, p=[0.5, 0.3, 0.2]) for g in gts]
    labels[0][:] = 0                                                # U = 0: nothing labelled, nothing to find
    _close(pe.summarise_labels(O.hist_of_labels(labels, gts)), O.labels_summary(labels, gts))
    # zero denominators: no pixel labelled 1 or 0 anywhere, no ground truth anywhere
    blank = [np.full((4, 4), 255, np.uint8)] * 2
    nogt = [np.zeros((4, 4), bool)] * 2
    got = pe.summarise_labels(O.hist_of_labels(blank, nogt))
    assert got["fg_precision"] is None and got["bg_precision"] is None and got["fg_recall"] is None and got["ignored_share"] == 1.0
    assert got["mIoU"] == 0.0 and got["oIoU"] == 0.0
    _close(got, O.labels_summary(blank, nogt))
    assert "null" in json.dumps(got)

    stacks = [rng.rand(k, *g.shape) < 0.3 for k, g in zip((0, 1, 2, 3, 0), gts)]
    hist, K = O.hist_of_masks(stacks, gts), [s.shape[0] for s in stacks]
    got = pe.summarise_masks(hist, K)
    _close(got, O.masks_summary(stacks, gts))
    assert got["mean_K"] == 6 / 5 and got["empty_share"] == 2 / 5 and 0 < got["overlap_share"] < 1
    empty = pe.summarise_masks(O.hist_of_masks(stacks[:1], gts[:1]), [0])
    assert empty["overlap_share"] is None and empty["mIoU"] == 0.0          # (K = 0 on an empty ground truth: U = 0)
    I, U = pe.masks_iu(hist)
    for n, (s, g) in enumerate(zip(stacks, gts)):
        assert (int(I[n]), int(U[n])) == O.iu(s.sum(0) > 0 if s.shape[0] else np.zeros(g.shape, bool), g)
    I, U = pe.labels_iu(O.hist_of_labels(labels, gts))
    for n, (l, g) in enumerate(zip(labels, gts)):
        assert (int(I[n]), int(U[n])) == O.iu(l == 1, g)


# ------------------------------------------------------------------------------------------------------------------ command line
def test_parser_carries_the_reference_names_and_defaults():
    from tris_amd.eval_pseudo import get_parser
    a = get_parser().parse_args([])
    assert (a.refer_data_root, a.dataset, a.splitBy, a.split) == ("../../data/", "refcoco", "unc", "train")
    assert a.train_list == "voc12/train_aug.txt"
    assert a.cam_out_dir is None and a.ir_label_out_dir is None and a.ins_seg_out_dir is None       # (a default would be scored)
    assert a.cam_eval_thres is None and a.out is None and a.per_name is None
    b = get_parser().parse_args("--refer_data_root R --dataset refcocog --splitBy umd --split val --train_list n.json --cam_out_dir D "
                                "--ir_label_out_dir L --ins_seg_out_dir O --cam_eval_thres 0.1,0.2 --out s.json --per_name r.npz".split())
    assert (b.cam_out_dir, b.ir_label_out_dir, b.ins_seg_out_dir, b.cam_eval_thres) == ("D", "L", "O", "0.1,0.2")


def test_command_refuses_to_run_with_none_of_the_three_directories(mini, tmp_path):
    from tris_amd import eval_pseudo
    root, ds = mini
    names = tmp_path / "names.json"
    names.write_text(json.dumps([f"0_{ds.image_record(0)[1]}"]))
    argv = ["--refer_data_root", root, "--dataset", "refcocog", "--splitBy", "umd", "--train_list", str(names)]
    with pytest.raises(SystemExit) as e:
        eval_pseudo.main(argv)
    assert "at least one of --cam_out_dir, --ir_label_out_dir, --ins_seg_out_dir" in str(e.value)
    with pytest.raises(SystemExit, match="strictly ascending"):
        eval_pseudo.main(argv + ["--cam_out_dir", str(tmp_path), "--cam_eval_thres", "0.5,0.5"])


def test_command_needs_the_gpu(mini, tmp_path, monkeypatch):
    import torch
    from tris_amd import eval_pseudo, ops
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)      # (so the refusal also shows where a GPU is present)
    root, _ = mini
    with pytest.raises(ops.NoGpuError):
        eval_pseudo.main(["--refer_data_root", root, "--dataset", "refcocog", "--splitBy", "umd", "--train_list", "absent.json",
                          "--cam_out_dir", str(tmp_path)])
