"""Scoring response maps, CRF labels and instance masks against ground truth that stays run ends (csrc/labelscore.hip,
ops.score_maps / ops.score_counts, tris_amd/pseudo_eval.py, python -m tris_amd.eval_pseudo) on the MI355X.  Every comparison is of
integers and exact: histograms against tests/oracle_pseudo_eval.py (rle_arena.decode_sum_numpy and boolean counting), the I and U of
validate's threshold against ops.eval_post, the command's numbers against ReferDataset.load_mask, the host rasteriser."""
import json
import math
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle_pseudo_eval as O
import poly_cases
from conftest import ROOT

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 67), (67, 1), (37, 53), (64, 64), (130, 257)]
THRESHOLDS = {
    1: [1e-9],
    2: [0.25, 0.5],
    20: [1e-9] + [round(0.05 * k, 2) for k in range(1, 20)],
    64: np.linspace(-0.5, 1.5, 64).astype(np.float32).tolist(),
}


# ------------------------------------------------------------------------------------------------------------------ ground truth
def _counts(rng, n, short=False, zero_first=False):
    """random run lengths over n positions, background first"""
    cuts = np.unique(rng.randint(1, n + 1, int(rng.randint(1, 13)))).tolist()
    if short and cuts[-1] == n:
        cuts = cuts[:-1] or ([n - 1] if n > 1 else [0])
    if not short and cuts[-1] != n:
        cuts.append(n)
    counts = np.diff([0] + cuts).tolist()
    return [0] + counts if zero_first else counts


def _hand_made(H, W, seed):
    """-> (RleArena, [(kind, (lo, hi))]): the refs every size is scored against"""
    from tris_amd import _lib
    from tris_amd.dataset.rle_arena import RleArena
    rng, n, arena, refs = np.random.RandomState(seed), H * W, RleArena(), []
    cap = _lib.query("tris_score_stage_capacity")
    assert cap == 4096

    def add(kind, segs):
        refs.append((kind, arena.add_sentence([{"counts": c} for c in segs], H, W, kind)))
    add("an empty range", [])
    add("one segment", [_counts(rng, n)])
    add("counts that stop short of H*W", [_counts(rng, n, short=True)])
    add("a zero-length first run", [_counts(rng, n, zero_first=True)])
    a = _counts(rng, n, zero_first=True)
    add("two overlapping segments", [a, [0, n]])                     # the second covers everything: the first's pixels count 2
    add("a segment without runs", [[]])
    add("three segments", [_counts(rng, n), _counts(rng, n, short=True), _counts(rng, n, zero_first=True)])
    if n >= cap:
        add("as many runs as the staging holds", [[1] * cap])
        add("one run more than the staging holds", [[0] + [1] * cap] if n == cap else [[1] * (cap + 1)])
    if n > 3 * cap:
        add("many times the staging, in two segments", [[1] * (2 * cap + 3), [2] * (cap + 1)])
    return arena, refs


_SCENES = {}


def _scene(H, W):
    """per size: the device arena, the refs and their ground-truth bits under both rules, computed once and left unchanged"""
    if (H, W) not in _SCENES:
        arena, refs = _hand_made(H, W, seed=1000 * H + W)
        ends, seg_off = arena.arrays()
        ranges = [r for _, r in refs]
        bits = {rule: O.gt_bits(ends, seg_off, ranges, H, W, rule) for rule in (0, 1)}
        for b in bits.values():
            b.setflags(write=False)
        _SCENES[(H, W)] = (arena.to("cuda"), refs, bits)
    return _SCENES[(H, W)]


def _maps(rng, G, H, W, thr):
    """values in [0, 1) with thresholds themselves, NaN, +inf and -inf planted; map 1 all zero"""
    m = rng.rand(G, H, W).astype(np.float32)
    flat = m.reshape(G, -1)
    n = flat.shape[1]
    t32 = np.asarray(thr, np.float32)
    for g in range(G):
        k = min(n, 3 * len(t32))
        flat[g, rng.choice(n, k, replace=False)] = t32[rng.randint(0, len(t32), k)]
        if n >= 8:
            flat[g, rng.choice(n, 3, replace=False)] = [np.nan, np.inf, -np.inf]
    if G > 1:
        m[1] = 0
    if n < 8:
        flat[0, 0] = [np.nan, np.inf, -np.inf, t32[0]][(G + len(t32)) % 4]
    return m


def _check_maps(H, W, combos, seed):
    from tris_amd import ops
    (ends, seg_off), refs, bits = _scene(H, W)
    rng = np.random.RandomState(seed)
    for shift, (G, T) in enumerate(combos):
        thr = THRESHOLDS[T]
        pick = [(g + shift) % len(refs) for g in range(G)]
        ranges = [refs[k][1] for k in pick]
        maps = _maps(rng, G, H, W, thr)
        dev = torch.from_numpy(maps).cuda()
        for rule in (0, 1):
            # (the ranges as a host list, and as a device tensor that the op reads back)
            rg = ranges if rule == 0 else torch.tensor(ranges, dtype=torch.int32, device="cuda")
            got = ops.score_maps(dev, (ends, seg_off), rg, thr, gt_rule=rule)
            assert got.dtype == torch.int64 and tuple(got.shape) == (G, T + 1, 2)
            want = O.maps_hist(maps, bits[rule][pick], thr)
            assert int(want.sum()) == G * H * W
            got = got.cpu().numpy()
            for g in range(G):
                assert np.array_equal(got[g], want[g]), (H, W, G, T, rule, g, refs[pick[g]][0])


@pytest.mark.parametrize("H,W", SIZES)
def test_score_maps_equals_the_oracle(H, W):
    _check_maps(H, W, [(G, T) for G in (1, 3, 17) for T in (1, 2, 20, 64)], seed=H * 7 + W)
    kinds = [k for k, _ in _scene(H, W)[1]]
    if H * W >= 4096:
        assert "one run more than the staging holds" in kinds           # the global-memory path ran (G = 17 takes every ref)


def test_score_maps_sums_several_partial_rows_at_480x640():
    from tris_amd import _lib
    H, W = 480, 640
    per_map = _lib.query("tris_score_workspace_bytes", 1, H, W, 21) // (2 * 21 * 4)
    assert per_map > 1                                                   # more than one partial row per map
    assert _lib.query("tris_score_workspace_bytes", 3, H, W, 21) == 3 * per_map * 2 * 21 * 4
    assert _lib.query("tris_score_workspace_bytes", 1, 4097, 4096, 21) == -1
    _check_maps(H, W, [(3, 20)], seed=5)
    assert len(_scene(H, W)[1]) == 10                                    # (the long refs included; shift 0 takes refs 0, 1, 2 ...)
    _check_maps(H, W, [(1, 1)] * 7 + [(3, 2)], seed=6)                   # ... and shift 7 the three that reach the staging limit


def test_score_maps_on_the_named_polygons():
    """tests/poly_cases.named_cases() through PolyArena (the degenerate and out-of-frame polygons included), one ref each, grouped
    by canvas; a second ref per canvas holds all its polygons, so that overlaps separate the two rules"""
    from tris_amd import ops
    from tris_amd.dataset.poly_arena import PolyArena
    cases = poly_cases.named_cases()
    arena, ranges, by_size = PolyArena(), [], {}
    for name, xy, h, w in cases:
        ranges.append(arena.add_ref([xy], h, w, name))
        by_size.setdefault((h, w), []).append(len(ranges) - 1)
    for (h, w), ks in list(by_size.items()):
        ranges.append(arena.add_ref([cases[k][1] for k in ks], h, w, f"all of {h}x{w}"))
        by_size[(h, w)] = ks + [len(ranges) - 1]
    built = arena.build("cuda")
    ends, seg_off = built.ends.cpu().numpy(), built.seg_off.cpu().numpy()
    rng = np.random.RandomState(11)
    thr = THRESHOLDS[20]
    differ = 0
    for (h, w), ks in by_size.items():
        maps = _maps(rng, len(ks), h, w, thr)
        rg = [ranges[k] for k in ks]
        masks = [sum(poly_cases.oracle_mask(cases[j][1], h, w).astype(np.int64) for j in (ks[:-1] if k == ks[-1] else [k])) for k in ks]
        for rule in (0, 1):
            bits = O.gt_bits(ends, seg_off, rg, h, w, rule)
            assert np.array_equal(bits, np.stack([(m == 1) if rule == 0 else (m != 0) for m in masks])), (h, w)   # (the host rasteriser)
            got = ops.score_maps(torch.from_numpy(maps).cuda(), built, rg, thr, gt_rule=rule).cpu().numpy()
            assert np.array_equal(got, O.maps_hist(maps, bits, thr)), (h, w, rule)
        differ += int((masks[-1] > 1).sum())
    assert differ > 0


# ------------------------------------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize("H,W", [(37, 53), (130, 257)])
def test_score_counts_equals_the_oracle(H, W):
    from tris_amd import ops
    arena, refs, bits = _scene(H, W)
    rng = np.random.RandomState(H + W)
    label = rng.choice(np.array([0, 1, 255], np.uint8), size=(1, H, W), p=[0.5, 0.3, 0.2])
    label[0, H // 2, W // 3] = 7                                         # one stray value: counted where it falls
    ones = (rng.rand(255, H, W) < 0.02).astype(np.uint8)
    ones[:, 3, 5] = 1                                                    # a pixel where all 255 masks meet: sum 255
    stacks = {
        "K = 0": np.zeros((0, H, W), np.uint8),
        "a label image": label,
        "two masks": (rng.rand(2, H, W) < 0.4).astype(np.uint8),
        "two planes that wrap": np.stack([np.full((H, W), 200, np.uint8), rng.choice(np.array([0, 55, 100], np.uint8), size=(H, W))]),
        "K = 255": ones,
    }
    for what, stack in stacks.items():
        dev = torch.from_numpy(stack).cuda()
        for k, (kind, (lo, hi)) in enumerate(refs):
            for rule in (0, 1):
                got = ops.score_counts(dev, arena, lo, hi, H, W, gt_rule=rule)
                assert got.dtype == torch.int64 and tuple(got.shape) == (256, 2)
                want = O.counts_hist(stack, bits[rule][k])
                assert np.array_equal(got.cpu().numpy(), want), (what, kind, rule)
    assert O.counts_hist(ones, bits[0][1])[255].sum() >= 1 and O.counts_hist(label, bits[0][1])[7].sum() == 1
    assert O.counts_hist(stacks["two planes that wrap"], bits[0][1])[44].sum() > 0          # 200 + 100 = 44 in a byte
    # an [H,W] image is a stack of one; a bool stack goes in as its bytes
    img = torch.from_numpy(label[0]).cuda()
    lo, hi = refs[4][1]
    assert torch.equal(ops.score_counts(img, arena, lo, hi, H, W), ops.score_counts(img[None], arena, lo, hi, H, W))
    two = torch.from_numpy(stacks["two masks"].astype(bool)).cuda()
    assert np.array_equal(ops.score_counts(two.view(torch.uint8), arena, lo, hi, H, W).cpu().numpy(),
                          O.counts_hist(stacks["two masks"], bits[0][4]))


def test_two_launches_give_equal_bytes():
    from tris_amd import ops
    H, W = 130, 257
    arena, refs, _ = _scene(H, W)
    rng = np.random.RandomState(3)
    maps = torch.from_numpy(_maps(rng, 17, H, W, THRESHOLDS[20])).cuda()
    ranges = [refs[g % len(refs)][1] for g in range(17)]
    a = ops.score_maps(maps, arena, ranges, THRESHOLDS[20])
    b = ops.score_maps(maps, arena, ranges, THRESHOLDS[20])
    assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()
    stack = torch.from_numpy((rng.rand(5, H, W) < 0.3).astype(np.uint8)).cuda()
    lo, hi = refs[-1][1]
    a = ops.score_counts(stack, arena, lo, hi, H, W, gt_rule=1)
    b = ops.score_counts(stack, arena, lo, hi, H, W, gt_rule=1)
    assert torch.equal(a, b) and int(a.sum()) == H * W


def test_validates_threshold_gives_eval_posts_I_and_U():
    """ops.eval_post scores one map against a decoded target at validate's threshold; score_maps on the cam it returns, against the
    same ref as run ends under gt_rule 1 (target != 0), counts the same I and U"""
    from tris_amd import ops
    H, W = 37, 53
    (ends, seg_off), refs, _ = _scene(H, W)
    rng = np.random.RandomState(9)
    for k in (1, 4, 6):
        lo, hi = refs[k][1]
        tgt = ops.rle_decode_sum_arena(ends, seg_off, torch.tensor([[lo, hi]], dtype=torch.int32, device="cuda"), H, W)[0]
        relu_map = torch.from_numpy(np.maximum(rng.randn(20, 20), 0).astype(np.float32)).cuda()      # (about half the map is 0)
        iu, cam = ops.eval_post(relu_map, tgt)
        hist = ops.score_maps(cam[None], (ends, seg_off), [(lo, hi)], [1e-9], gt_rule=1).cpu().numpy()[0]
        I, U = int(hist[1, 1]), int(hist[1, 0] + hist[:, 1].sum())
        assert [I, U] == iu[:2].tolist() and 0 < I < U, refs[k][0]


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_arguments_the_kernels_would_have_to_trust_are_refused():
    from tris_amd import ops
    from tris_amd.dataset.rle_arena import RleArena
    H, W = 4, 5
    big = RleArena()
    for _ in range(3):
        big.add_sentence([{"counts": [3, 2]}] * 100, H, W)
    arena = big.to("cuda")                                               # 300 segments
    maps = torch.zeros(2, H, W, device="cuda")
    ok = [(0, 1), (1, 3)]
    assert int(ops.score_maps(maps, arena, ok, [0.5]).sum()) == 2 * H * W
    with pytest.raises(ValueError, match=r"score_maps: H\*W = 4097x4096 .* beyond 2\^24"):
        ops.score_maps(torch.empty(1, 4097, 4096, device="cuda"), arena, [(0, 1)], [0.5])
    with pytest.raises(ValueError, match=r"score_counts: H\*W = 4097x4096 .* beyond 2\^24"):
        ops.score_counts(torch.zeros(1, H, W, dtype=torch.uint8, device="cuda"), arena, 0, 1, 4097, 4096)
    with pytest.raises(ValueError, match="T = 0 entries"):
        ops.score_maps(maps, arena, ok, [])
    with pytest.raises(ValueError, match="T = 65 entries"):
        ops.score_maps(maps, arena, ok, np.linspace(0, 1, 65))
    with pytest.raises(ValueError, match="not strictly ascending.*entry 0 = 0.5"):
        ops.score_maps(maps, arena, ok, [0.5, 0.5])
    with pytest.raises(ValueError, match="entry 1 = nan is not finite"):
        ops.score_maps(maps, arena, ok, [0.5, float("nan")])
    with pytest.raises(ValueError, match="K = 256 planes"):
        ops.score_counts(torch.zeros(256, H, W, dtype=torch.uint8, device="cuda"), arena, 0, 1, H, W)
    with pytest.raises(ValueError, match=r"map 1: segments 299\.\.301 lie outside the arena's 300"):
        ops.score_maps(maps, arena, [(0, 1), (299, 301)], [0.5])
    with pytest.raises(ValueError, match=r"map 0: segments 2\.\.1 lie outside"):
        ops.score_maps(maps, arena, torch.tensor([[2, 1], [0, 1]], dtype=torch.int32, device="cuda"), [0.5])
    with pytest.raises(ValueError, match=r"map 1: segments 10\.\.266 are 256, more than the 255"):
        ops.score_maps(maps, arena, [(0, 255), (10, 266)], [0.5])
    with pytest.raises(ValueError, match=r"score_counts: segments -1\.\.2 lie outside"):
        ops.score_counts(torch.zeros(1, H, W, dtype=torch.uint8, device="cuda"), arena, -1, 2, H, W)
    with pytest.raises(ValueError, match=r"score_counts: segments 0\.\.256 are 256"):
        ops.score_counts(torch.zeros(1, H, W, dtype=torch.uint8, device="cuda"), arena, 0, 256, H, W)
    with pytest.raises(ValueError, match=r"ranges is \[G,2\] = \[2,2\], got \(1, 2\)"):
        ops.score_maps(maps, arena, [(0, 1)], [0.5])
    with pytest.raises(ValueError, match=r"the stack is \[K,4,5\], got \(1, 5, 4\)"):
        ops.score_counts(torch.zeros(1, W, H, dtype=torch.uint8, device="cuda"), arena, 0, 1, H, W)
    with pytest.raises(ValueError, match="gt_rule 2"):
        ops.score_maps(maps, arena, ok, [0.5], gt_rule=2)
    # dtypes
    with pytest.raises(TypeError, match="maps is torch.float64"):
        ops.score_maps(maps.double(), arena, ok, [0.5])
    with pytest.raises(TypeError, match="the stack is torch.bool"):
        ops.score_counts(torch.zeros(1, H, W, dtype=torch.bool, device="cuda"), arena, 0, 1, H, W)
    with pytest.raises(TypeError, match="ends is torch.int64"):
        ops.score_maps(maps, (arena[0].long(), arena[1]), ok, [0.5])
    with pytest.raises(TypeError, match="seg_off is torch.int32"):
        ops.score_counts(torch.zeros(1, H, W, dtype=torch.uint8, device="cuda"), (arena[0], arena[1].int()), 0, 1, H, W)
    with pytest.raises(TypeError, match="ranges is torch.int64"):
        ops.score_maps(maps, arena, torch.tensor(ok, device="cuda"), [0.5])
    # CPU tensors
    with pytest.raises(ops.NoGpuError, match="maps"):
        ops.score_maps(maps.cpu(), arena, ok, [0.5])
    with pytest.raises(ops.NoGpuError, match="seg_off is a CPU tensor"):
        ops.score_maps(maps, (arena[0], arena[1].cpu()), ok, [0.5])
    with pytest.raises(ops.NoGpuError, match="ranges is a CPU tensor"):
        ops.score_maps(maps, arena, torch.tensor(ok, dtype=torch.int32), [0.5])
    with pytest.raises(ops.NoGpuError, match="the stack"):
        ops.score_counts(torch.zeros(1, H, W, dtype=torch.uint8), arena, 0, 1, H, W)


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def artefacts(tmp_path_factory):
    """a mini REFER data set with response maps, label images and instance masks for its train refs, names in both forms, and the
    ground truth of every ref from ReferDataset.load_mask"""
    from PIL import Image
    from tris_amd.dataset.ReferDataset import ReferDataset
    from tris_amd.utils.synth import make_mini_refer, make_pseudo_masks, word_hash_tokenize
    tmp = tmp_path_factory.mktemp("pseudo_eval")
    root = make_mini_refer(str(tmp / "data"), n_images=5, seed=8, max_side=60)
    ds = ReferDataset(refer_data_root=root, dataset="refcocog", splitBy="umd", split="train", eval_mode=True, tokenizer=word_hash_tokenize)
    D, L, Om = tmp / "cam", tmp / "lab", tmp / "ins"
    D.mkdir()
    L.mkdir()
    make_pseudo_masks(root, str(Om), seed=2)
    rng = np.random.RandomState(21)
    a = {"tmp": tmp, "root": root, "D": D, "L": L, "O": Om, "gt": {}, "cam": {}, "lab": {}, "stack": {}, "plain": [], "sent": []}
    for i in range(len(ds)):
        img = ds.image_record(i)[1]
        gt = np.asarray(ds.load_mask(i)[0]) == 1
        plain = f"{i}_{img}"
        a["plain"].append(plain)
        if i == 2:                                                       # one name without instances
            np.save(Om / f"{plain}.npy", {"mask": np.zeros((0,) + gt.shape, bool)}, allow_pickle=True)
        a["stack"][plain] = np.load(Om / f"{plain}.npy", allow_pickle=True).item()["mask"]
        for name in [plain] + [f"{i}_{j}_{img}" for j in range(len(ds.all_sentences[i]))]:
            cam = (rng.rand(*gt.shape) * (0.3 + 0.7 * gt)).astype(np.float32)
            cam[rng.rand(*gt.shape) < 0.2] = 0
            lab = rng.choice(np.array([0, 1, 255], np.uint8), size=gt.shape, p=[0.5, 0.3, 0.2])
            lab[gt & (rng.rand(*gt.shape) < 0.6)] = 1
            np.save(D / f"{name}.npy", cam)
            Image.fromarray(lab).save(L / f"{name}.png")
            a["gt"][name], a["cam"][name], a["lab"][name] = gt, cam, lab
            if name != plain:
                a["sent"].append(name)
    assert len(a["plain"]) > 4 and len(a["sent"]) > len(a["plain"]) and any(g.any() for g in a["gt"].values())
    return a


def _command(a, names, *more):
    lst, out = a["tmp"] / "names.json", a["tmp"] / "summary.json"
    lst.write_text(json.dumps(names))
    if out.exists():
        out.unlink()
    cmd = [sys.executable, "-m", "tris_amd.eval_pseudo", "--refer_data_root", a["root"], "--dataset", "refcocog", "--splitBy", "umd",
           "--train_list", str(lst), "--out", str(out)] + [str(m) for m in more]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)     # a fresh process with its own limit
    return run, (json.loads(out.read_text()) if out.exists() else None)


def _same_numbers(got, want, path=""):
    """integers and None equal; floats equal up to the order of a float64 sum (the oracle adds name by name)"""
    assert type(got) is type(want) or {type(got), type(want)} == {int, float}, (path, got, want)
    if isinstance(want, dict):
        assert got.keys() == want.keys(), (path, got.keys(), want.keys())
        for k in want:
            _same_numbers(got[k], want[k], f"{path}/{k}")
    elif isinstance(want, list):
        assert len(got) == len(want), path
        for j, (g, w) in enumerate(zip(got, want)):
            _same_numbers(g, w, f"{path}[{j}]")
    elif isinstance(want, float):
        assert math.isclose(got, want, rel_tol=1e-12, abs_tol=1e-12), (path, got, want)
    else:
        assert got == want, (path, got, want)


def test_command_on_names_of_the_plain_form_scores_all_three_artefacts(artefacts):
    from tris_amd import pseudo_eval as pe
    a, names = artefacts, artefacts["plain"]
    npz = a["tmp"] / "records.npz"
    run, got = _command(a, names, "--cam_out_dir", a["D"], "--ir_label_out_dir", a["L"], "--ins_seg_out_dir", a["O"], "--per_name", npz)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "response maps" in run.stdout and "CRF labels" in run.stdout and "instance masks" in run.stdout and "<- best mIoU" in run.stdout
    thr = pe.default_thresholds()
    gts, cams, labs = [a["gt"][n] for n in names], [a["cam"][n] for n in names], [a["lab"][n] for n in names]
    stacks = [a["stack"][n] for n in names]
    assert (got["dataset"], got["splitBy"], got["split"], got["names"]) == ("refcocog", "umd", "train", len(names))
    _same_numbers(got["cams"], O.cams_summary(cams, gts, thr))
    _same_numbers(got["labels"], O.labels_summary(labs, gts))
    _same_numbers(got["masks"], O.masks_summary(stacks, gts))
    assert got["masks"]["empty_share"] == 1 / len(names) and got["masks"]["mean_K"] == 2 * (len(names) - 1) / len(names)
    assert got["masks"]["overlap_share"] > 0 and got["cams"]["best_mIoU"] > got["cams"]["mIoU"][0] > 0
    # bit for bit: the per-name integers, and the summary formed from the oracle's histograms
    rec = np.load(str(npz))
    assert rec["names"].tolist() == names
    for j, t in enumerate(np.asarray(thr, np.float32)):
        want = [O.iu(c > t, g) for c, g in zip(cams, gts)]
        assert rec["cam_I"][:, j].tolist() == [w[0] for w in want] and rec["cam_U"][:, j].tolist() == [w[1] for w in want], j
    assert np.array_equal(rec["label_hist"], O.hist_of_labels(labs, gts)) and np.array_equal(rec["mask_hist"], O.hist_of_masks(stacks, gts))
    assert rec["mask_K"].tolist() == [s.shape[0] for s in stacks]
    assert got["labels"] == pe.summarise_labels(O.hist_of_labels(labs, gts))
    assert got["masks"] == pe.summarise_masks(O.hist_of_masks(stacks, gts), [s.shape[0] for s in stacks])


def test_command_on_names_of_the_sentence_form(artefacts):
    a, names = artefacts, artefacts["sent"]
    run, got = _command(a, names, "--cam_out_dir", a["D"], "--ir_label_out_dir", a["L"], "--cam_eval_thres", "1e-9,0.3,0.5")
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    gts = [a["gt"][n] for n in names]
    assert set(got) == {"dataset", "splitBy", "split", "names", "cams", "labels"} and got["names"] == len(names)
    _same_numbers(got["cams"], O.cams_summary([a["cam"][n] for n in names], gts, [1e-9, 0.3, 0.5]))
    _same_numbers(got["labels"], O.labels_summary([a["lab"][n] for n in names], gts))


@pytest.mark.parametrize("fault", ["a missing map", "a wrongly sized label", "a non-bool mask"])
def test_command_ends_with_a_message_naming_the_file(artefacts, fault, tmp_path):
    from PIL import Image
    a, names = artefacts, artefacts["plain"]
    victim = names[3]
    if fault == "a missing map":
        D = tmp_path / "cam"
        D.mkdir()
        for n in names:
            if n != victim:
                np.save(D / f"{n}.npy", a["cam"][n])
        run, _ = _command(a, names, "--cam_out_dir", D)
        file, words = f"{victim}.npy", "does not exist"
    elif fault == "a wrongly sized label":
        L = tmp_path / "lab"
        L.mkdir()
        for n in names:
            Image.fromarray(a["lab"][n][:-1] if n == victim else a["lab"][n]).save(L / f"{n}.png")
        run, _ = _command(a, names, "--ir_label_out_dir", L)
        file, words = f"{victim}.png", "does not go with an image of"
    else:
        Om = tmp_path / "ins"
        Om.mkdir()
        for n in names:
            s = a["stack"][n]
            np.save(Om / f"{n}.npy", {"mask": s.astype(np.uint8) if n == victim else s}, allow_pickle=True)
        run, _ = _command(a, names, "--ins_seg_out_dir", Om)
        file, words = f"{victim}.npy", "'mask' is uint8, expected bool"
    assert run.returncode != 0 and file in run.stderr and words in run.stderr, run.stdout[-1000:] + run.stderr[-2000:]
    assert "Traceback" not in run.stderr


def test_a_stray_label_value_is_refused_naming_file_and_value(artefacts, tmp_path):
    """in process: the readers run before anything is launched"""
    from PIL import Image
    from tris_amd import pseudo_eval as pe
    a = artefacts
    name = a["plain"][0]
    lab = a["lab"][name].copy()
    lab[1, 2] = 9
    Image.fromarray(lab).save(tmp_path / f"{name}.png")
    with pytest.raises(ValueError) as e:
        pe._read_label(str(tmp_path / f"{name}.png"), *lab.shape)
    assert f"{name}.png" in str(e.value) and "label value 9" in str(e.value)
