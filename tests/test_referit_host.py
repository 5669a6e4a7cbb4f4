"""ReferIt on the host: the dataset classes against the recording of the reference's (tests/golden/g19_referit.npz, written by
tools/gen_golden_referit.py; its masks are pinned to tris_amd.dataset.cocomask, not to pycocotools), the run-boundary arena against
cocomask.decode, the refusals of ops.rle_decode_sum, the command line's --distributed rule, the drop-in names, the C declarations
and the restated loop of tests/oracle_referit.py on hand-made cams."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle_referit as O

SIZE = 64


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return O.synthetic_root(tmp_path_factory.mktemp("referit"))


@pytest.fixture(scope="module")
def datasets(tree):
    from tris_amd.dataset.Dataset_referit import get_refit_dataset
    return get_refit_dataset(SimpleNamespace(size=SIZE, refer_data_root=tree, max_query_len=20, negative_samples=0))


def test_image_loader_equals_the_recorded_reference(datasets, golden):
    g = golden("g19_referit.npz")
    ds = datasets[1]
    assert [str(f) for f in ds.files] == list(g["files"]) == list(O.SIZES)
    kept = []
    for n in range(len(ds)):
        img, out, sizes, path = ds[n]
        assert path.endswith(f"images/{ds.files[n]}.jpg")
        assert tuple(sizes) == tuple(g[f"t{n}_size"]) == O.SIZES[str(ds.files[n])]
        assert img.dtype == torch.float32 and np.array_equal(img.numpy(), g[f"t{n}_img"])          # bit for bit
        assert list(out.keys()) == list(g[f"t{n}_keys"])
        kept.append(list(out.keys()))
        for k, it in out.items():
            assert it["word_id"].dtype == torch.int32 and np.array_equal(it["word_id"].numpy(), g[f"t{n}_{k}_word_id"])
            assert it["bbox"].shape == g[f"t{n}_{k}_bbox"].shape and it["bbox"].ndim == 2 and np.array_equal(it["bbox"], g[f"t{n}_{k}_bbox"])
            assert it["mask"].dtype == np.uint8 and np.array_equal(it["mask"], g[f"t{n}_{k}_mask"])
    # the gap of the filtered annotation, the image without survivors, the annotation exactly at 5 %
    assert kept == [["0", "2", "3"], ["0", "1", "2"], [], ["0", "2"]]
    assert ds[0][1]["2"]["mask"].max() == 2                                                         # a count, not a boolean
    assert ds[3][1]["0"]["bbox"].shape == (2, 4)


def test_train_loader_equals_the_recorded_reference(datasets, golden):
    g = golden("g19_referit.npz")
    ds = datasets[0]
    assert len(ds) == int(g["n_train"]) == 7
    for n in range(len(ds)):
        img, word_id, neg = ds[n]
        assert neg == -1 and isinstance(word_id, np.ndarray) and word_id.dtype == g[f"r{n}_word_id"].dtype
        assert np.array_equal(word_id, g[f"r{n}_word_id"]) and np.array_equal(img.numpy(), g[f"r{n}_img"])


def test_scipy_is_imported_lazily():
    import tris_amd.dataset.Dataset_referit as D
    assert "sio" not in vars(D) and callable(D.load_referit_gt_mask) and callable(D.pil_loader)


def test_string_form_round_trips():
    from tris_amd.dataset import cocomask
    for counts in ([0, 5, 3, 2], [7, 1, 900, 40, 3, 3, 1000, 2], [12]):
        assert cocomask._counts_from_string(O.counts_to_string(counts)) == counts


def _segments():
    """every segment of the fixture, with its image size and a name"""
    for key, rec in O.annotations().items():
        H, W = O.SIZES[key]
        for i, a in enumerate(rec["annotations"]):
            for j, r in enumerate(a["segmentation"]):
                yield f"{key}/{i}/{j}", r, H, W


def test_arena_round_trips_every_fixture_segment():
    from tris_amd.dataset import cocomask
    from tris_amd.dataset.rle_arena import RleArena, decode_sum_numpy
    forms = set()
    for name, r, H, W in _segments():
        arena = RleArena()
        rng = arena.add_sentence([r], H, W, name)
        ends, seg_off = arena.arrays()
        assert ends.dtype == np.int32 and seg_off.dtype == np.int64 and rng == (0, 1)
        got = decode_sum_numpy(ends, seg_off, [rng], H, W)[0]
        assert np.array_equal(got, cocomask.decode(r)), name
        c = r["counts"]
        forms.add("string" if isinstance(c, str) else "first0" if c[0] == 0 else "zero_run" if 0 in c else "plain")
    assert forms == {"string", "first0", "zero_run", "plain"}
    # whole sentences in one arena: sums over segments, an empty sentence between two others, a short sum
    arena, want, ranges = RleArena(), [], []
    H, W = O.SIZES["1001"]
    a = O.annotations()["1001"]["annotations"]
    for s in (a[2]["segmentation"], [], a[0]["segmentation"], [{"size": [H, W], "counts": [3, 5]}]):
        ranges.append(arena.add_sentence(s, H, W))
        want.append(cocomask.decode(s).sum(2).astype(np.uint8) if s else np.zeros((H, W), np.uint8))
    got = decode_sum_numpy(*arena.arrays(), ranges, H, W)
    assert np.array_equal(got, np.stack(want)) and got[0].max() == 2 and got[3].sum() == 5


def test_refusals_name_the_offender():
    from tris_amd import ops
    ok = {"size": [4, 5], "counts": [3, 4, 13]}
    cases = [([[ok], [{"size": [4, 5], "counts": [3, 4, 14]}]], 4, 5, "past H\\*W"),
             ([[ok], [{"size": [4, 5], "counts": [3, -1, 5]}]], 4, 5, "negative count"),
             ([[ok], [ok] * 256], 4, 5, "256 segments")]
    for sents, H, W, what in cases:
        with pytest.raises(ValueError, match=f"img7/1.*{what}"):
            ops.rle_decode_sum(sents, H, W, names=["img7/0", "img7/1"])
    with pytest.raises(ValueError, match="big.*2\\^24"):
        ops.rle_decode_sum([[{"size": [4097, 4096], "counts": [5]}]], 4097, 4096, names=["big"])
    # and the cache's builder names the key and the annotation (the same builder, the name the cache gives it)
    from tris_amd.dataset.rle_arena import RleArena
    with pytest.raises(ValueError, match="1001 annotation 2 segment 0.*past"):
        RleArena().add_sentence([{"size": [4, 5], "counts": [21]}], 4, 5, "1001 annotation 2")
    with pytest.raises(ValueError, match="size"):
        RleArena().add_sentence([{"size": [5, 4], "counts": [20]}], 4, 5, "x")
    if not torch.cuda.is_available():                       # well-formed input reaches the GPU check: no CPU fallback
        with pytest.raises(ops.NoGpuError):
            ops.rle_decode_sum([[ok]], 4, 5)


def test_distributed_is_refused():
    from tris_amd import validate_referit as VR
    from tris_amd.args import get_parser
    args = get_parser().parse_args(["--size", "64", "--dataset", "referit", "--test_split", "test", "--backbone", "clip-RN50",
                                    "--max_query_len", "20", "--refer_data_root", "/nonexistent", "--output", "/nonexistent", "--resume",
                                    "--pretrain", "x.pth", "--eval", "--distributed"])
    with pytest.raises(NotImplementedError, match="per rank"):
        VR.main(args)


def test_dropin_aliases_resolve():
    import tris_amd.dropin as d
    assert d.ALIASES["validate_referit"] == "tris_amd.validate_referit"
    assert d.ALIASES["dataset.Dataset_referit"] == "tris_amd.dataset.Dataset_referit"
    tops = {n.split(".")[0] for n in d.ALIASES}
    parked = {n: sys.modules.pop(n) for n in list(sys.modules) if n.split(".")[0] in tops and not n.startswith("tris_amd")}
    d.install()
    try:
        from validate_referit import isCorrectHit, main, validate          # noqa: F401
        from dataset.Dataset_referit import ImageLoader, ImageLoader_train, get_flicker_transform, get_refit_dataset  # noqa: F401
        assert validate.__module__ == "tris_amd.validate_referit" and ImageLoader.__module__ == "tris_amd.dataset.Dataset_referit"
    finally:
        d.uninstall()
        sys.modules.update(parked)


def test_c_symbols_are_declared():
    from tris_amd import _lib
    from conftest import ROOT
    decls, _ = _lib.parse_header()
    for name in ("tris_rle_decode_sum_u8", "tris_eval_post_group_f32", "tris_eval_post_group_workspace_bytes"):
        assert name in decls
    assert len(decls["tris_eval_post_group_f32"][1]) == 11 and len(decls["tris_rle_decode_sum_u8"][1]) == 8
    src = open(os.path.join(ROOT, "include", "tris_hip.h")).read()
    assert "validate_referit.py:160-171" in src and "Dataset_referit.py:141-144" in src
    assert "referit" in open(os.path.join(ROOT, "tris_amd", "csrc", "build.sh")).read().split("for f in ")[1].split(";")[0].split()


# ------------------------------------------------------------------------------------------------ the restated loop
def _cam(H, W, y, x, on=None):
    c = np.zeros((H, W), np.float32)
    if on is not None:
        c[on] = 0.5
    c[y, x] = 1.0
    return c


def test_restated_loop_on_hand_made_cams():
    H, W = 9, 11
    mask = np.zeros((H, W), np.uint8)
    mask[2:6, 2:8] = 1
    mask[3:5, 3:5] += 1                                        # counts 2 inside
    near, far = [2, 2, 7, 5], [8, 6, 10, 8]
    s = {"bbox": np.array([near]), "mask": mask}
    two = O.restate([[s]], [[_cam(H, W, 3, 3)]])               # arg-max on a count-2 pixel
    one = O.restate([[s]], [[_cam(H, W, 2, 6)]])               # on a count-1 pixel
    assert two["pairs"] == [(1, 0)] and one["pairs"] == [(1, 1)] and two["hitm"] == 0.0 and one["hitm"] == 100.0
    # bounds are inclusive; a second box scores the hit
    assert O.restate([[{"bbox": np.array([far, near]), "mask": mask}]], [[_cam(H, W, 5, 7)]])["pairs"] == [(1, 1)]
    assert O.restate([[{"bbox": np.array([far]), "mask": mask}]], [[_cam(H, W, 5, 7)]])["pairs"] == [(0, 1)]
    # I / U on (mask != 0)
    cam = _cam(H, W, 2, 2, on=(slice(2, 6), slice(0, 4)))
    r = O.restate([[s]], [[cam]])
    assert r["oiou"] == 100 * 8 / 32 and r["miou"] == 100 * (8 / 32)
    # U == 0: IoU 0, nothing divides
    empty = {"bbox": np.array([near]), "mask": np.zeros((H, W), np.uint8)}
    z = O.restate([[empty]], [[np.zeros((H, W), np.float32)]])
    assert z["miou"] == 0.0 and z["oiou"] == 0.0 and z["n_sent"] == 1
    # an image with no sentences changes nothing
    a = O.restate([[s], [], [s]], [[cam], [], [_cam(H, W, 3, 3)]])
    b = O.restate([[s], [s]], [[cam], [_cam(H, W, 3, 3)]])
    assert a == b and a["n_sent"] == 2
    # the package's isCorrectHit is the same rule
    from tris_amd.validate_referit import isCorrectHit
    for y, x in ((3, 3), (2, 6), (8, 10)):
        c = _cam(H, W, y, x).astype(np.float64)
        assert isCorrectHit(s["bbox"], c, mask)[::2] == O.is_correct_hit(s["bbox"], c, mask)[::2]


def test_the_checkpoint_decides_the_stage(tmp_path):
    """the reference switches stages by editing an import; main() reads it off the checkpoint's keys"""
    from tris_amd import validate_referit as VR
    from tris_amd.model import model_stage1, model_stage2
    args = SimpleNamespace(output=str(tmp_path), pretrain="s2.pth", resume=True)
    torch.save({"model": {"reduced_c1.conv.weight": torch.zeros(1)}}, tmp_path / "s2.pth")
    torch.save({"model": {"vis_project.weight": torch.zeros(1)}}, tmp_path / "s1.pth")
    assert VR._model_class(args) is model_stage2.TRIS
    args.pretrain = "s1.pth"
    assert VR._model_class(args) is model_stage1.TRIS
    args.pretrain = None
    assert VR._model_class(args) is model_stage1.TRIS
