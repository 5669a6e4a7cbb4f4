"""Host side of the instance-level scoring (tris_amd/pseudo_eval.py summarise_instances and its reader, the two flags of
tris_amd/eval_pseudo.py, the index-table checks of ops.score_planes).  No GPU."""
import json
import math
from fractions import Fraction

import numpy as np
import pytest

import oracle_instances as OI


def _rec(a, i, g, score):
    """a record of score_instances from per-instance areas and intersections (rows 0 .. 2 carry only what g needs)"""
    K = len(a)
    t = np.zeros((K + 3, 2), np.int64)
    t[0, 1] = g
    for k in range(K):
        t[3 + k] = (a[k] - i[k], i[k])
    return {"table": t, "scored": t[:3].copy(), "K": K, "score": np.asarray(score, np.float64)}


def _hand_case():
    return [_rec([60, 80], [60, 80], 100, [.9, .2]), _rec([30], [30], 100, [.8]), _rec([40, 55], [40, 55], 100, [.7, .7])]


def _same(got, want, path=""):
    assert type(got) is type(want) or {type(got), type(want)} == {int, float}, (path, got, want)
    if isinstance(want, dict):
        assert got.keys() == want.keys(), (path, got.keys(), want.keys())
        for k in want:
            _same(got[k], want[k], f"{path}/{k}")
    elif isinstance(want, float):
        assert math.isclose(got, want, rel_tol=1e-12, abs_tol=1e-12), (path, got, want)
    else:
        assert got == want, (path, got, want)


# ------------------------------------------------------------------------------------------------------------------ AP
def test_ap_hand_case_at_every_threshold():
    from tris_amd import pseudo_eval as pe
    recs = _hand_case()
    want = {10: Fraction(1, 2), 11: Fraction(1, 2), 12: Fraction(1, 3), 15: Fraction(1, 15), 16: Fraction(1, 15), 17: Fraction(0)}
    ranked = OI.ranked(recs)
    assert [d[0] for d in ranked] == [0, 1, 2, 2, 0]
    for q, ap in want.items():
        assert OI.ap_at(ranked, 3, q) == ap, q                                    # the oracle, in fractions
        assert math.isclose(pe._voc_ap(ranked, 3, q), float(ap), rel_tol=0, abs_tol=1e-15), q
    got = pe.summarise_instances(recs)
    assert math.isclose(got["ap50"], 0.5, abs_tol=1e-15) and math.isclose(got["ap75"], 1 / 15, abs_tol=1e-15) and got["n_pos"] == 3
    # tau: .5 .55 .6 .65 .7 .75 .8 .85 .9 .95  (.65 and .7: only the .8 instance of name 0 passes, at rank 5, as at .75)
    assert math.isclose(got["ap"], (0.5 + 0.5 + 1 / 3 + 4 / 15) / 10, abs_tol=1e-15)
    _same(got, OI.instances_summary(recs))
    json.dumps(got)


def test_ap_score_ties_go_by_name_position_then_plane():
    from tris_amd import pseudo_eval as pe
    # every score equal: the order is name 0 plane 0, name 0 plane 1, name 1 plane 0.  Name 0's first plane misses and its second
    # hits; with the planes swapped the hit comes first and the precision envelope differs
    miss_first = [_rec([50, 100], [10, 100], 100, [.5, .5]), _rec([100], [100], 100, [.5])]
    hit_first = [_rec([100, 50], [100, 10], 100, [.5, .5]), _rec([100], [100], 100, [.5])]
    a, b = pe.summarise_instances(miss_first), pe.summarise_instances(hit_first)
    # miss, hit, hit: precision 0, 1/2, 2/3 -> the envelope is 2/3 at both recall steps; hit, miss, hit: 1, 1/2, 2/3 -> 1 then 2/3
    assert math.isclose(a["ap50"], 2 / 3, abs_tol=1e-15) and math.isclose(b["ap50"], 5 / 6, abs_tol=1e-15)
    # across names: the earlier name's detection ranks first although the list gives the later one first by plane
    across = [_rec([100], [20], 100, [.5]), _rec([100], [100], 100, [.5])]
    swapped = across[::-1]
    assert pe.summarise_instances(across)["ap50"] == 0.25 and pe.summarise_instances(swapped)["ap50"] == 0.5
    for recs in (miss_first, hit_first, across, swapped):
        _same(pe.summarise_instances(recs), OI.instances_summary(recs))
    # scores are compared as float64: 0.1 + 0.2 ranks above 0.3
    f64 = [_rec([100], [100], 100, [0.3]), _rec([100], [0], 100, [0.1 + 0.2])]
    assert pe.summarise_instances(f64)["ap50"] == 0.25


def test_ap_a_name_without_ground_truth_only_adds_false_positives():
    from tris_amd import pseudo_eval as pe
    recs = [_rec([10], [0], 0, [.9]), _rec([100], [100], 100, [.8]), _rec([], [], 0, [])]
    got = pe.summarise_instances(recs)
    assert got["n_pos"] == 1 and got["ap50"] == 0.5 and got["ap"] == 0.5          # one FP ranks above the only TP
    _same(got, OI.instances_summary(recs))
    none = pe.summarise_instances([_rec([10], [0], 0, [.9]), _rec([], [], 0, [])])
    assert none["n_pos"] == 0 and none["ap50"] is None and none["ap75"] is None and none["ap"] is None
    _same(none, OI.instances_summary([_rec([10], [0], 0, [.9]), _rec([], [], 0, [])]))
    assert "null" in json.dumps(none)


# ------------------------------------------------------------------------------------------------------------------ policies
def test_policies_against_the_oracle_on_real_stacks_with_K_0_names():
    from tris_amd import pseudo_eval as pe
    rng = np.random.RandomState(4)
    recs = []
    for K in (0, 1, 3, 0, 4, 2):
        gt = rng.rand(9, 7) < 0.4
        if len(recs) == 3:
            gt[:] = False                                                          # K = 0 on an empty ground truth: U = 0
        stack = rng.rand(K, 9, 7) < 0.3
        score = rng.choice([0.0, 0.0, 0.3, 0.7, 0.7], K)
        recs.append(OI.record(stack, score, gt))
    got = pe.summarise_instances(recs)
    _same(got, OI.instances_summary(recs))
    assert got["names"] == 6 and got["instances"] == 10 and 0 < got["zero_score_share"] < 1
    # union is today's masks numbers
    masks = pe.summarise_masks(np.stack([r["table"][:3] for r in recs]), [r["K"] for r in recs])
    assert got["union"] == {"mIoU": masks["mIoU"], "oIoU": masks["oIoU"]}
    only_empty = pe.summarise_instances([recs[0], recs[3]])
    g0 = int(recs[0]["table"][:3, 1].sum())
    assert g0 > 0 and only_empty["top1"] == only_empty["best"] == {"mIoU": 0.0, "oIoU": 0.0}
    assert only_empty["zero_score_share"] is None and only_empty["zero_score_fp_share"] is None and only_empty["instances"] == 0
    _same(only_empty, OI.instances_summary([recs[0], recs[3]]))
    assert pe.summarise_instances([])["top1"] == {"mIoU": None, "oIoU": None}
    _same(pe.summarise_instances([]), OI.instances_summary([]))


def test_best_is_decided_by_exact_fractions_and_ties_go_to_the_first():
    from tris_amd import pseudo_eval as pe
    # a = i, so u = g for both: IoUs 2^60 / g and (2^60 + 1) / g differ by 3e-19, far below float64's resolution at 1/3
    g, i1, i2 = 3 * (1 << 60) + 2, 1 << 60, (1 << 60) + 1
    assert float(Fraction(i1, g)) == float(Fraction(i2, g)) and i1 / g == i2 / g          # (floats cannot tell them apart)
    assert pe.pick_best([i1, i2], [i1, i2], g) == 1 and pe.pick_best([i2, i1], [i2, i1], g) == 0
    assert pe.pick_best([i1, i1, i2, i2], [i1, i1, i2, i2], g) == 2
    got = pe.summarise_instances([_rec([i1, i2], [i1, i2], g, [.5, .4])])                  # (int64 holds them)
    _same(got, OI.instances_summary([_rec([i1, i2], [i1, i2], g, [.5, .4])]))
    # equal fractions in different terms: 20/40 and 30/60 -> the first; top1 takes the other
    tie = _rec([30, 60], [20, 30], 30, [.1, .9])
    assert pe.pick_best([30, 60], [20, 30], 30) == 0 and pe.pick_best([60, 30], [30, 20], 30) == 0
    assert pe.pick_top1([.1, .9]) == 1 and pe.pick_top1([.7, .7]) == 0 and pe.pick_top1([]) is None and pe.pick_best([], [], 5) is None
    got = pe.summarise_instances([tie, _rec([10], [0], 10, [.3])])
    assert got["best"]["oIoU"] == 100.0 * 20 / (40 + 20) and got["top1"]["oIoU"] == 100.0 * 30 / (60 + 20)
    _same(got, OI.instances_summary([tie, _rec([10], [0], 10, [.3])]))
    # no ground truth and an empty instance: every IoU is 0 by definition -> the first
    assert pe.pick_best([0, 5], [0, 0], 0) == 0


def test_zero_score_shares_and_their_zero_denominators():
    from tris_amd import pseudo_eval as pe
    recs = [_rec([50, 10, 4], [40, 2, 0], 60, [.9, 0, -1.0]), _rec([20], [5], 30, [0])]
    got = pe.summarise_instances(recs)
    assert got["zero_score_share"] == 3 / 4 and got["zero_score_fp_share"] == (8 + 4 + 15) / (10 + 8 + 4 + 15)
    _same(got, OI.instances_summary(recs))
    exact = pe.summarise_instances([_rec([50], [50], 60, [0.0])])     # no false-positive area at all
    assert exact["zero_score_share"] == 1.0 and exact["zero_score_fp_share"] is None
    empty = pe.summarise_instances([_rec([], [], 60, [])])
    assert empty["zero_score_share"] is None and empty["zero_score_fp_share"] is None


# ------------------------------------------------------------------------------------------------------------------ reader
def test_reader_returns_scores_of_either_dtype_and_refuses_by_message(tmp_path):
    from tris_amd import pseudo_eval as pe
    mask = np.zeros((2, 5, 4), bool)
    mask[0, 1:3] = True

    def save(name, rec):
        np.save(tmp_path / f"{name}.npy", rec, allow_pickle=True)
        return str(tmp_path / f"{name}.npy")
    stack, score = pe._read_instances(save("f", {"mask": mask, "score": np.array([0.5, 0.0], np.float32)}), 5, 4)
    assert stack.dtype == np.uint8 and stack.shape == (2, 5, 4) and score.dtype == np.float64 and score.tolist() == [0.5, 0.0]
    stack, score = pe._read_instances(save("i", {"mask": np.zeros((0, 5, 4), bool), "score": np.zeros(0, np.int64)}), 5, 4)
    assert stack.shape == (0, 5, 4) and score.shape == (0,)
    _, score = pe._read_instances(save("i2", {"mask": mask, "score": np.array([3, 0])}), 5, 4)
    assert score.tolist() == [3.0, 0.0]
    assert np.array_equal(pe._read_masks(save("m", {"mask": mask}), 5, 4), mask.view(np.uint8))       # (the old reader asks for no score)
    for name, rec, words in (("missing", {"mask": mask}, "has no 'score'"),
                             ("short", {"mask": mask, "score": np.array([0.5])}, "expected one number for each of the 2 masks"),
                             ("twod", {"mask": mask, "score": np.zeros((2, 1))}, "expected one number for each of the 2 masks"),
                             ("nan", {"mask": mask, "score": np.array([0.5, np.nan])}, "non-finite value (nan) at instance 1"),
                             ("inf", {"mask": mask, "score": np.array([np.inf, 1.0])}, "non-finite value (inf) at instance 0")):
        with pytest.raises(ValueError) as e:
            pe._read_instances(save(name, rec), 5, 4)
        assert f"{name}.npy" in str(e.value) and words in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------------------------------ tables
def test_pillows_nearest_tables_never_decrease_and_stay_inside():
    """what the kernel's forward-only run walk relies on, for every size pair the tests and Stage 2 use"""
    from tris_amd import ops
    from tris_amd.dataset import pil_tables
    sizes = list(range(1, 70)) + [320, 384, 448, 480, 640]
    for n_in in sizes:
        for n_out in sizes:
            t = pil_tables.nearest_index(n_in, n_out)
            got = ops._score_table(t, n_in, "t", "yidx")
            assert got.dtype == np.int32 and np.array_equal(got, t), (n_in, n_out)
            v = t[t >= 0]
            assert v.size and (np.diff(v) >= 0).all() and v.max() < n_in, (n_in, n_out)


def test_index_tables_are_refused_by_name():
    from tris_amd import ops
    assert ops._score_table([0, 0, -1, 2, 2, -5, 3], 4, "w", "xidx").tolist() == [0, 0, -1, 2, 2, -1, 3]
    with pytest.raises(ValueError, match=r"w: yidx\[2\] = 1 is below an earlier entry 3: the table decreases"):
        ops._score_table([0, 3, 1], 4, "w", "yidx")
    with pytest.raises(ValueError, match=r"w: yidx\[3\] = 1 is below an earlier entry 2"):
        ops._score_table([0, 2, -1, 1], 4, "w", "yidx")                    # (a hole between them does not hide it)
    with pytest.raises(ValueError, match=r"w: xidx\[1\] = 4 lies outside the canvas's 0\.\.3"):
        ops._score_table([0, 4], 4, "w", "xidx")
    with pytest.raises(ValueError, match="1-D integer table"):
        ops._score_table([0.5, 1.0], 4, "w", "xidx")
    with pytest.raises(ValueError, match="1-D integer table"):
        ops._score_table([], 4, "w", "xidx")
    for bad in (0, -3, (0, 5), (5,), (4, 5, 6), 2.5, True, (4097, 4096), "7"):
        with pytest.raises(ValueError, match="out_hw .* is neither None, a size S >= 1 nor"):
            ops._score_out_hw(bad, "score_planes")
    assert ops._score_out_hw(7, "w") == (7, 7) and ops._score_out_hw((3, 9), "w") == (3, 9) and ops._score_out_hw([4096, 4096], "w")


# ------------------------------------------------------------------------------------------------------------------ command line
@pytest.fixture(scope="module")
def mini(tmp_path_factory):
    from tris_amd.dataset.ReferDataset import ReferDataset
    from tris_amd.utils.synth import make_mini_refer, word_hash_tokenize
    root = make_mini_refer(str(tmp_path_factory.mktemp("pi") / "data"), n_images=3, seed=3, max_side=40)
    ds = ReferDataset(refer_data_root=root, dataset="refcocog", splitBy="umd", split="train", eval_mode=True,
                      tokenizer=word_hash_tokenize)
    return root, ds


def test_parser_takes_the_two_flags_in_the_references_form():
    from tris_amd.eval_pseudo import get_parser
    a = get_parser().parse_args([])
    assert a.eval_ins_seg_pass is False and a.size is None                        # (a default size would be scored)
    for text, want in (("True", True), ("true", True), ("False", False), ("0", False), ("1", True)):
        assert get_parser().parse_args(["--eval_ins_seg_pass", text]).eval_ins_seg_pass is want
    assert get_parser().parse_args(["--size", "320"]).size == 320
    with pytest.raises(SystemExit):
        get_parser().parse_args(["--eval_ins_seg_pass", "perhaps"])
    with pytest.raises(SystemExit):
        get_parser().parse_args(["--size", "big"])


def test_command_refuses_the_flags_without_the_masks_and_a_size_of_zero(mini, tmp_path):
    from tris_amd import eval_pseudo
    root, ds = mini
    names = tmp_path / "names.json"
    names.write_text(json.dumps([f"0_{ds.image_record(0)[1]}"]))
    argv = ["--refer_data_root", root, "--dataset", "refcocog", "--splitBy", "umd", "--train_list", str(names)]
    with pytest.raises(SystemExit, match="--eval_ins_seg_pass True scores instance masks and needs --ins_seg_out_dir"):
        eval_pseudo.main(argv + ["--cam_out_dir", str(tmp_path), "--eval_ins_seg_pass", "True"])
    with pytest.raises(SystemExit, match="--size scores instance masks and needs --ins_seg_out_dir"):
        eval_pseudo.main(argv + ["--ir_label_out_dir", str(tmp_path), "--size", "320"])
    with pytest.raises(SystemExit, match="--size 0 is not a training resolution"):
        eval_pseudo.main(argv + ["--ins_seg_out_dir", str(tmp_path), "--size", "0"])
    with pytest.raises(SystemExit, match="--size -5 is not a training resolution"):
        eval_pseudo.main(argv + ["--ins_seg_out_dir", str(tmp_path), "--size", "-5"])


class _Arena:
    pass


def test_without_the_flags_the_command_asks_for_and_writes_what_it_did(mini, tmp_path, monkeypatch):
    """run() with the device work replaced by recorders: without the flags neither new pass is called and the summary's keys, the
    printed lines and the .npz keys are the ones the command had; with them only the new keys and lines are added and 'masks' is the
    same object of numbers"""
    import torch
    from tris_amd import eval_pseudo, pseudo_eval as pe
    root, ds = mini
    names = [f"{i}_{ds.image_record(i)[1]}" for i in range(len(ds))]
    lst = tmp_path / "names.json"
    lst.write_text(json.dumps(names))
    N, called = len(names), []
    hist = np.tile(np.array([[[5, 1], [2, 3], [1, 1]]], np.int64), (N, 1, 1))
    rec = _rec([4, 2], [3, 1], 5, [.5, 0])
    rec["table"][:3], rec["scored"] = hist[0], hist[0]

    class FakeGT:
        def __init__(self, dataset, indices):
            self.arena, self.device = _Arena(), "cpu"
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(pe, "GroundTruth", FakeGT)
    monkeypatch.setattr(pe, "score_masks", lambda n, d, gt: (called.append("masks"), (hist, np.full(N, 2, np.int64)))[1])
    monkeypatch.setattr(pe, "score_masks_train", lambda n, d, gt, s: (called.append(f"train {s}"), (hist // 2, np.full(N, 2, np.int64)))[1])
    monkeypatch.setattr(pe, "score_instances", lambda n, d, gt, **kw: (called.append("instances"), [rec] * N)[1])
    base = ["--refer_data_root", root, "--dataset", "refcocog", "--splitBy", "umd", "--train_list", str(lst), "--ins_seg_out_dir", "O"]

    def go(*more):
        lines, npz = [], tmp_path / "rec.npz"
        args = eval_pseudo.get_parser().parse_args(base + ["--per_name", str(npz)] + list(more))
        return eval_pseudo.run(args, log=lines.append), lines, sorted(np.load(str(npz)).files)
    plain, lines, keys = go()
    assert called == ["masks"]
    assert set(plain) == {"dataset", "splitBy", "split", "names", "masks"}
    assert keys == ["mask_I", "mask_K", "mask_U", "mask_hist", "names"]
    assert len(lines) == 2 and lines[0].startswith("instance masks (O)")
    del called[:]
    both, more_lines, more_keys = go("--eval_ins_seg_pass", "True", "--size", "320")
    assert called == ["masks", "train 320", "instances"]
    assert set(both) == set(plain) | {"instances", "masks_train"} and both["masks"] == plain["masks"]
    assert more_lines[:2] == lines and len(more_lines) > 2
    assert set(more_keys) == set(keys) | {"mask_train_hist", "inst_offsets", "inst_score", "inst_area", "inst_inter", "inst_gt_area"}
    assert both["masks_train"] == pe.summarise_masks(hist // 2, np.full(N, 2)) and both["instances"] == pe.summarise_instances([rec] * N)
    r = np.load(str(tmp_path / "rec.npz"))
    assert r["inst_offsets"].tolist() == list(range(0, 2 * N + 1, 2)) and r["inst_gt_area"].tolist() == [5] * N
    assert r["inst_area"].tolist() == [4, 2] * N and r["inst_inter"].tolist() == [3, 1] * N and r["inst_score"].tolist() == [.5, 0] * N
    json.dumps(both)
    del called[:]
    off, _, off_keys = go("--eval_ins_seg_pass", "False")
    assert called == ["masks"] and off == plain and off_keys == keys
