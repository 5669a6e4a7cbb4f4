"""Plane-by-plane scoring of instance masks, optionally at the Stage-2 training resolution (csrc/labelscore.hip
tris_score_planes_u8, ops.score_planes / ops.score_planes_at, pseudo_eval.score_instances, the two flags of python -m
tris_amd.eval_pseudo) on the MI355X.  Every comparison is of integers and exact: tables against tests/oracle_instances.py (boolean
counting over the sampled grid), against ops.score_counts, and against the histogram of ops.mask_sum_nearest_u8 over
ops.rle_target_nearest; the command's numbers against ReferDataset.load_mask and Pillow's own NEAREST resize."""
import ctypes

import numpy as np
import pytest
import torch

import oracle_instances as OI
import oracle_pseudo_eval as O
import poly_cases
from test_gpu_pseudo_eval import _command, _same_numbers, _scene, artefacts  # noqa: F401  (artefacts: the fixture)

pytestmark = pytest.mark.gpu

CANVASES = [(1, 1), (1, 65), (65, 1), (63, 64), (64, 65), (130, 67), (480, 640), (1025, 1025)]
INVALID = 1                                      # hipErrorInvalidValue


def _stack(rng, K, H, W):
    s = (rng.rand(K, H, W) < 0.35).astype(np.uint8)
    if K > 1:
        s[1] = 0                                 # an instance that found nothing
    return s


@pytest.mark.parametrize("H,W", CANVASES)
def test_score_planes_equals_the_oracle_on_the_full_grid(H, W):
    """every hand-made ref of the size (empty range, short counts, zero-length first run, overlaps, the staging limit where the
    canvas holds it), both rules, K cycling through 0, 1, 2, 5; 1025 x 1025 has 289 tiles for 256 workgroups and takes K = 1"""
    from tris_amd import _lib, ops
    arena, refs, bits = _scene(H, W)
    rng = np.random.RandomState(H * 3 + W)
    Ks = [1] if (H, W) == (1025, 1025) else [0, 1, 2, 5]
    stacks = {K: _stack(rng, K, H, W) for K in Ks}
    devs = {K: torch.from_numpy(s).cuda() for K, s in stacks.items()}
    for k, (kind, (lo, hi)) in enumerate(refs):
        K = Ks[k % len(Ks)]
        for rule in (0, 1):
            got = ops.score_planes(devs[K], arena, lo, hi, H, W, gt_rule=rule)
            assert got.dtype == torch.int64 and tuple(got.shape) == (K + 3, 2) and got.is_cuda
            want = OI.planes_table(stacks[K], bits[rule][k])
            assert int(want[:3].sum()) == H * W
            assert np.array_equal(got.cpu().numpy(), want), (kind, K, rule)
    kinds = [kind for kind, _ in refs]
    if H * W >= 4096:
        assert "one run more than the staging holds" in kinds
    if (H, W) in ((480, 640), (1025, 1025)):
        assert "many times the staging, in two segments" in kinds
        tiles = ((H + 63) // 64) * ((W + 63) // 64)
        rows = _lib.query("tris_score_planes_workspace_bytes", 1, H, W) // (2 * 4 * 4)
        assert rows == min(tiles, 256) and (tiles > 256) == ((H, W) == (1025, 1025))      # 289 tiles: workgroups stride


def test_score_planes_with_255_planes_and_with_bytes_above_one():
    from tris_amd import _lib, ops
    H, W = 9, 7
    arena, refs, bits = _scene(H, W)
    rng = np.random.RandomState(8)
    many = (rng.rand(255, H, W) < 0.1).astype(np.uint8)
    many[:, 3, 5] = 1                                                      # all 255 planes meet here
    assert _lib.query("tris_score_planes_workspace_bytes", 255, H, W) == 2 * 258 * 4      # more bins than score_counts has
    for k in (1, 4, 6):
        lo, hi = refs[k][1]
        got = ops.score_planes(torch.from_numpy(many).cuda(), arena, lo, hi, H, W).cpu().numpy()
        assert got.shape == (258, 2) and np.array_equal(got, OI.planes_table(many, bits[0][k])), refs[k][0]
    # bytes above 1: 200 + 56 is 0 in a byte and 256 as an integer (row 2); a lone 2 is a sum of 2, not of 1; 255 * 5 does not wrap
    H, W = 130, 67
    arena, refs, bits = _scene(H, W)
    wide = rng.choice(np.array([0, 0, 1, 2, 56, 200, 255], np.uint8), size=(5, H, W))
    wide[:, 0, 0] = (200, 56, 0, 0, 0)
    wide[:, 0, 1] = (0, 0, 2, 0, 0)
    wide[:, 0, 2] = 255
    s = wide.astype(np.int64).sum(0)
    assert ((s >= 256) & (s % 256 < 2)).any()                              # pixels a byte sum would put in rows 0 or 1
    for k in (1, 4):
        lo, hi = refs[k][1]
        for rule in (0, 1):
            got = ops.score_planes(torch.from_numpy(wide).cuda(), arena, lo, hi, H, W, gt_rule=rule).cpu().numpy()
            assert np.array_equal(got, OI.planes_table(wide, bits[rule][k])), (refs[k][0], rule)


def test_score_planes_on_the_named_polygons():
    """tests/poly_cases.named_cases() through PolyArena, one ref per polygon and one per canvas holding all of its polygons (overlaps
    separate the rules), full grid and a sampled one, against the host rasteriser's mask"""
    from tris_amd import ops
    from tris_amd.dataset import pil_tables
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
    rng = np.random.RandomState(12)
    for (h, w), ks in by_size.items():
        stack = _stack(rng, 3, h, w)
        dev = torch.from_numpy(stack).cuda()
        oh, ow = max(1, (2 * h) // 3), w + 3
        yi, xi = pil_tables.nearest_index(h, oh), pil_tables.nearest_index(w, ow)
        for k in ks:
            members = ks[:-1] if k == ks[-1] else [k]
            mask = sum(poly_cases.oracle_mask(cases[j][1], h, w).astype(np.int64) for j in members)
            for rule in (0, 1):
                gt = (mask == 1) if rule == 0 else (mask != 0)
                got = ops.score_planes(dev, built, *ranges[k], h, w, gt_rule=rule).cpu().numpy()
                assert np.array_equal(got, OI.planes_table(stack, gt)), (h, w, k, rule)
                got = ops.score_planes(dev, built, *ranges[k], h, w, out_hw=(oh, ow), gt_rule=rule).cpu().numpy()
                assert np.array_equal(got, OI.planes_table(stack, gt, yi, xi)), (h, w, k, rule, "sampled")


# ------------------------------------------------------------------------------------------------------------------ sampled grids
@pytest.mark.parametrize("H,W,out_hw", [(13, 11, (7, 5)), (5, 4, (12, 9)), (130, 67, (70, 140)), (480, 640, 320)])
def test_score_planes_on_pillows_nearest_grid(H, W, out_hw):
    """down-sampling, up-sampling (repeated indices count as often as they appear), and the histogram Stage 2 trains on: rows 0 .. 2
    equal the histogram of ops.mask_sum_nearest_u8 against ops.rle_target_nearest, ops that were here before"""
    from tris_amd import ops
    from tris_amd.dataset import pil_tables
    arena, refs, bits = _scene(H, W)
    oh, ow = (out_hw, out_hw) if isinstance(out_hw, int) else out_hw
    yi, xi = pil_tables.nearest_index(H, oh), pil_tables.nearest_index(W, ow)
    if oh > H:
        assert (np.diff(yi) == 0).any()
    rng = np.random.RandomState(H + W)
    for k, (kind, (lo, hi)) in enumerate(refs):
        K = (0, 1, 2, 5)[k % 4]
        stack = _stack(rng, K, H, W)
        dev = torch.from_numpy(stack).cuda()
        for rule in (0, 1):
            got = ops.score_planes(dev, arena, lo, hi, H, W, out_hw=out_hw, gt_rule=rule)
            want = OI.planes_table(stack, bits[rule][k], yi, xi)
            assert int(want[:3].sum()) == oh * ow
            assert np.array_equal(got.cpu().numpy(), want), (kind, K, rule)
        if oh == ow:                                                         # (rle_target_nearest makes square targets)
            s = ops.mask_sum_nearest_u8(dev, oh, ow).long().clamp(max=2)
            t = ops.rle_target_nearest(arena, lo, hi, H, W, oh).long()
            hist = torch.bincount((2 * s + t).reshape(-1), minlength=6).reshape(3, 2)
            assert torch.equal(ops.score_planes(dev, arena, lo, hi, H, W, out_hw=oh)[:3], hist), kind


def test_identity_tables_give_the_bytes_of_no_tables_and_holes_count_as_nothing():
    from tris_amd import ops
    H, W = 130, 67
    arena, refs, bits = _scene(H, W)
    rng = np.random.RandomState(2)
    stack = _stack(rng, 5, H, W)
    dev = torch.from_numpy(stack).cuda()
    for k in (1, 4, 6, len(refs) - 1):
        lo, hi = refs[k][1]
        plain = ops.score_planes(dev, arena, lo, hi, H, W)
        assert torch.equal(ops.score_planes(dev, arena, lo, hi, H, W, out_hw=(H, W)), plain)           # Pillow's H -> H table
        assert torch.equal(ops.score_planes_at(dev, arena, lo, hi, H, W, np.arange(H), np.arange(W)), plain)
        # hand-made tables: holes at the start, in the middle and at the end, repeats, a jump over most of the canvas
        yi = [-1, 0, 0, 3, -1, -1, 4, 64, 64, 65, 129, -1] + [129] * 60
        xi = [5, -1, 5, 6, 66, 66, -7]
        for rule in (0, 1):
            got = ops.score_planes_at(dev, arena, lo, hi, H, W, yi, xi, gt_rule=rule).cpu().numpy()
            want = OI.planes_table(stack, bits[rule][k], yi, xi)
            assert int(want[:3].sum()) == len(yi) * len(xi) and np.array_equal(got, want), (refs[k][0], rule)
        none = ops.score_planes_at(dev, arena, lo, hi, H, W, [-1, -1], [-1]).cpu().numpy()
        assert none[0].tolist() == [2, 0] and int(none[1:].sum()) == 0


# ------------------------------------------------------------------------------------------------------------------ other witnesses
@pytest.mark.parametrize("H,W", [(64, 65), (130, 67)])
def test_rows_equal_score_counts_folded(H, W):
    from tris_amd import ops
    arena, refs, _ = _scene(H, W)
    rng = np.random.RandomState(W)
    stack = torch.from_numpy(_stack(rng, 5, H, W)).cuda()
    for kind, (lo, hi) in refs:
        for rule in (0, 1):
            table = ops.score_planes(stack, arena, lo, hi, H, W, gt_rule=rule)
            hist = ops.score_counts(stack, arena, lo, hi, H, W, gt_rule=rule)
            assert torch.equal(table[:3], torch.stack([hist[0], hist[1], hist[2:].sum(0)])), (kind, rule)
            for k in range(5):
                one = ops.score_counts(stack[k:k + 1], arena, lo, hi, H, W, gt_rule=rule)
                assert torch.equal(table[3 + k], one[1:].sum(0)), (kind, rule, k)


def test_two_launches_give_equal_bytes():
    from tris_amd import ops
    H, W = 130, 67
    arena, refs, _ = _scene(H, W)
    stack = torch.from_numpy(_stack(np.random.RandomState(3), 5, H, W)).cuda()
    lo, hi = refs[-1][1]
    for out_hw in (None, 50):
        a = ops.score_planes(stack, arena, lo, hi, H, W, out_hw=out_hw, gt_rule=1)
        b = ops.score_planes(stack, arena, lo, hi, H, W, out_hw=out_hw, gt_rule=1)
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr() and int(a[:3].sum()) == (H * W if out_hw is None else 2500)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_the_entry_point_refuses_without_writing_the_table():
    """the C ABI's own refusals: the return value is hipErrorInvalidValue and a table filled with a sentinel keeps every byte"""
    from tris_amd import _lib
    from tris_amd.dataset.rle_arena import RleArena
    H, W = 4, 5
    host = RleArena()
    host.add_sentence([{"counts": [3, 2]}], H, W)
    ends, seg_off = host.to("cuda")
    stack = torch.ones(2, H, W, dtype=torch.uint8, device="cuda")
    idx = torch.arange(8, dtype=torch.int32, device="cuda") // 2           # 0 0 1 1 2 2 3 3: inside both axes, never decreasing
    table = torch.full((600, 2), -12345, dtype=torch.int64, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    fn = _lib.load().tris_score_planes_u8
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def go(K=2, lo=0, hi=1, h=H, w=W, yi=None, xi=None, oh=H, ow=W, rule=0, tbl=table):
        return fn(P(stack), K, P(ends), P(seg_off), lo, hi, h, w, yi, xi, oh, ow, rule, None if tbl is None else P(tbl), P(ws), None)
    assert go() == 0 and int(table[:5].sum()) == 3 * H * W and bool((table[5:] == -12345).all())      # (the accepted call: K + 3 rows)
    table.fill_(-12345)
    bad = {"no tables and another size": go(oh=H, ow=W + 1), "no tables and another height": go(oh=H - 1),
           "yidx alone": go(yi=P(idx), oh=4, ow=W), "xidx alone": go(xi=P(idx), oh=H, ow=4),
           "K = 256": go(K=256), "K = -1": go(K=-1), "a canvas beyond 2^24": go(h=4097, w=4096, oh=4097, ow=4096),
           "an output grid beyond 2^24": go(yi=P(idx), xi=P(idx), oh=4097, ow=4096), "an empty output grid": go(yi=P(idx), xi=P(idx), oh=0, ow=4),
           "256 segments": go(hi=256), "gt_rule 2": go(rule=2), "no table": go(tbl=None)}
    torch.cuda.synchronize()
    assert all(v == INVALID for v in bad.values()), bad
    assert bool((table == -12345).all())
    assert go(yi=P(idx), xi=P(idx), oh=8, ow=8) == 0 and int(table[:3].sum()) == 64
    q = lambda *a: _lib.query("tris_score_planes_workspace_bytes", *a)
    assert q(256, 4, 4) == -1 and q(-1, 4, 4) == -1 and q(1, 0, 4) == -1 and q(1, 4097, 4096) == -1 and q(0, 1, 1) == 2 * 3 * 4


def test_arguments_the_kernel_would_have_to_trust_are_refused_by_name():
    from tris_amd import ops
    from tris_amd.dataset.rle_arena import RleArena
    H, W = 4, 5
    big = RleArena()
    for _ in range(3):
        big.add_sentence([{"counts": [3, 2]}] * 100, H, W)
    arena = big.to("cuda")
    stack = torch.zeros(2, H, W, dtype=torch.uint8, device="cuda")
    assert int(ops.score_planes(stack, arena, 0, 1, H, W)[:3].sum()) == H * W
    with pytest.raises(ValueError, match=r"score_planes_at: yidx\[2\] = 1 is below an earlier entry 3: the table decreases"):
        ops.score_planes_at(stack, arena, 0, 1, H, W, [0, 3, 1], [0, 1])
    with pytest.raises(ValueError, match=r"score_planes_at: xidx\[1\] = 5 lies outside the canvas's 0\.\.4"):
        ops.score_planes_at(stack, arena, 0, 1, H, W, [0, 3], [0, 5])
    with pytest.raises(ValueError, match="K = 256 planes"):
        ops.score_planes(torch.zeros(256, H, W, dtype=torch.uint8, device="cuda"), arena, 0, 1, H, W)
    with pytest.raises(ValueError, match=r"score_planes: H\*W = 4097x4096 .* beyond 2\^24"):
        ops.score_planes(stack, arena, 0, 1, 4097, 4096)
    with pytest.raises(ValueError, match=r"out_hw \(4097, 4096\) is neither"):
        ops.score_planes(stack, arena, 0, 1, H, W, out_hw=(4097, 4096))
    with pytest.raises(ValueError, match="out_hw 0 is neither"):
        ops.score_planes(stack, arena, 0, 1, H, W, out_hw=0)
    with pytest.raises(ValueError, match=r"the stack is \[K,4,5\], got \(2, 5, 4\)"):
        ops.score_planes(stack.reshape(2, W, H), arena, 0, 1, H, W)
    with pytest.raises(ValueError, match=r"score_planes: segments 299\.\.301 lie outside the arena's 300"):
        ops.score_planes(stack, arena, 299, 301, H, W)
    with pytest.raises(ValueError, match=r"score_planes: segments 0\.\.256 are 256"):
        ops.score_planes(stack, arena, 0, 256, H, W)
    with pytest.raises(ValueError, match="gt_rule 2"):
        ops.score_planes(stack, arena, 0, 1, H, W, gt_rule=2)
    with pytest.raises(TypeError, match="the stack is torch.bool"):
        ops.score_planes(stack.bool(), arena, 0, 1, H, W)
    with pytest.raises(TypeError, match="ends is torch.int64"):
        ops.score_planes(stack, (arena[0].long(), arena[1]), 0, 1, H, W)
    with pytest.raises(ops.NoGpuError, match="the stack"):
        ops.score_planes(stack.cpu(), arena, 0, 1, H, W)
    with pytest.raises(ops.NoGpuError, match="seg_off is a CPU tensor"):
        ops.score_planes(stack, (arena[0], arena[1].cpu()), 0, 1, H, W)
    with pytest.raises(ops.NoGpuError, match="the stack"):
        ops.score_planes_at(stack.cpu(), arena, 0, 1, H, W, [0], [0])


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_command_scores_the_instances_and_the_training_grid(artefacts, tmp_path):
    """a fresh process on the synthetic artefacts, with a 'score' written beside every 'mask': instances and masks_train equal the
    oracle's (ground truth from ReferDataset.load_mask; the training grid from Pillow's own NEAREST resize of the mask sum and of the
    target), instances.union equals masks, and masks is the same with and without the flags"""
    from PIL import Image
    from tris_amd import pseudo_eval as pe
    a, names, S = artefacts, artefacts["plain"], 37
    Om = tmp_path / "ins"
    Om.mkdir()
    rng = np.random.RandomState(5)
    scores = {}
    for j, n in enumerate(names):
        K = a["stack"][n].shape[0]
        scores[n] = np.zeros(K, np.int64) if j % 4 == 1 else rng.choice([0.0, 0.4, 0.4, 0.9], K)       # (irn.py writes int64 zeros)
        np.save(Om / f"{n}.npy", {"mask": a["stack"][n], "score": scores[n]}, allow_pickle=True)
    assert any((s <= 0).any() and (s > 0).any() for s in scores.values())
    npz = tmp_path / "records.npz"
    run, plain = _command(a, names, "--ins_seg_out_dir", Om)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    plain_out = run.stdout
    assert set(plain) == {"dataset", "splitBy", "split", "names", "masks"}
    run, got = _command(a, names, "--ins_seg_out_dir", Om, "--eval_ins_seg_pass", "True", "--size", S, "--per_name", npz)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stdout.startswith(plain_out) and "instances one by one" in run.stdout and f"at {S} x {S}" in run.stdout
    assert set(got) == set(plain) | {"instances", "masks_train"} and got["masks"] == plain["masks"]
    gts, stacks = [a["gt"][n] for n in names], [a["stack"][n] for n in names]
    _same_numbers(got["masks"], O.masks_summary(stacks, gts))
    recs = [OI.record(s, scores[n], g) for n, s, g in zip(names, stacks, gts)]
    _same_numbers(got["instances"], OI.instances_summary(recs))
    assert got["instances"] == pe.summarise_instances(recs)
    assert got["instances"]["union"] == {"mIoU": got["masks"]["mIoU"], "oIoU": got["masks"]["oIoU"]}
    assert got["instances"]["ap50"] is not None and 0 < got["instances"]["zero_score_share"] < 1

    def nearest(img):
        return np.asarray(Image.fromarray(img).resize((S, S), Image.NEAREST))
    small = [np.stack([nearest(p.astype(np.uint8)) for p in s]).astype(bool) if s.shape[0] else np.zeros((0, S, S), bool) for s in stacks]
    small_gt = [nearest(g.astype(np.uint8)).astype(bool) for g in gts]
    _same_numbers(got["masks_train"], O.masks_summary(small, small_gt))
    rec = np.load(str(npz))
    assert np.array_equal(rec["mask_train_hist"], O.hist_of_masks(small, small_gt))
    for n, (s, g) in enumerate(zip(stacks, gts)):                                  # Pillow resizes the sum as it resizes the planes
        total = s.sum(0).astype(np.uint8) if s.shape[0] else np.zeros(g.shape, np.uint8)
        assert np.array_equal(nearest(total), small[n].sum(0).astype(np.uint8) if s.shape[0] else np.zeros((S, S), np.uint8))
    off = rec["inst_offsets"].tolist()
    assert off == np.concatenate([[0], np.cumsum([s.shape[0] for s in stacks])]).tolist()
    assert rec["inst_gt_area"].tolist() == [int(g.sum()) for g in gts]
    assert rec["inst_area"].tolist() == [int(p.sum()) for s in stacks for p in s]
    assert rec["inst_inter"].tolist() == [int((p & g).sum()) for s, g in zip(stacks, gts) for p in s]
    assert rec["inst_score"].tolist() == [float(v) for n in names for v in scores[n]]


def test_command_names_the_file_without_a_score(artefacts):
    a, names = artefacts, artefacts["plain"]
    run, _ = _command(a, names, "--ins_seg_out_dir", a["O"], "--eval_ins_seg_pass", "True")          # (these files hold 'mask' only)
    assert run.returncode != 0 and f"{names[0]}.npy" in run.stderr and "has no 'score'" in run.stderr, run.stderr[-2000:]
    assert "Traceback" not in run.stderr
