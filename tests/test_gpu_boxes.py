"""ops.eval_boxes (csrc/boxes.hip) against the restatement in tests/oracle_boxes.py: the kept list, every field of the record
and the bits of box_miou, exactly -- everything is integer or correctly rounded, so there is no tolerance."""
import numpy as np
import pytest
import torch

import oracle_boxes as OB
from test_boxes_host import block7x9, checker8, dots, frame5x6, ring9, row7

pytestmark = pytest.mark.gpu


def comb():
    m = np.zeros((33, 65), bool)
    m[1, 1:64] = True
    m[1:32, 1:64:2] = True
    return m


def spiral(n=31):
    """a one-pixel-wide square spiral: one 4-connected path that winds inwards two pixels apart"""
    m = np.zeros((n, n), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    while True:
        moved = False
        while True:
            yy, xx = y + dy, x + dx
            y2, x2 = yy + dy, xx + dx
            if not (0 <= yy < n and 0 <= xx < n) or m[yy, xx] or (0 <= y2 < n and 0 <= x2 < n and m[y2, x2]):
                break
            y, x = yy, xx
            m[y, x] = True
            moved = True
        if not moved:
            return m
        dy, dx = dx, -dy


def cross(H=12, W=19):
    m = np.zeros((H, W), bool)
    m[H // 2, :] = True
    m[:, W // 2] = True
    return m


def _cases():
    out = [("block7x9", block7x9()), ("ring9", ring9()), ("frame5x6", frame5x6()), ("checker8", checker8()),
           ("dots16", dots(16)), ("one_zero", np.zeros((1, 1), bool)), ("one_one", np.ones((1, 1), bool)), ("row7", row7()),
           ("comb33x65", comb()), ("spiral31", spiral()), ("dots64", dots(64)), ("zeros", np.zeros((9, 70), bool)),
           ("ones", np.ones((9, 70), bool)), ("cross", cross())]
    for H, W in ((17, 23), (48, 64), (96, 128), (120, 160)):
        for seed in range(3):
            out.append((f"blob{H}x{W}s{seed}", OB.blob_mask(H, W, 100 * H + seed)))
    out.append(("blob427x640", OB.blob_mask(427, 640, 7, sigma=6.0)))
    return out


_CASES = _cases()
_REF = {}


def _reference(name, mask):
    """(gen, [(target, gt, argmax, expected record)]): computed once per case and left unchanged"""
    if name not in _REF:
        H, W = mask.shape
        rng = np.random.RandomState(sum(map(ord, name)))
        gen = OB.generate_bbox(mask, full=True)
        boxes = gen[0]
        inside = (min(int(boxes[-1][1] + boxes[-1][3]) // 2, H - 1), min(int(boxes[-1][0] + boxes[-1][2]) // 2, W - 1))
        cover = np.zeros((H + 1, W + 1), bool)
        for b in boxes:
            cover[int(b[1]):int(b[3]) + 1, int(b[0]):int(b[2]) + 1] = True
        free = np.argwhere(~cover[:H, :W])
        outside = tuple(int(v) for v in free[len(free) // 2]) if len(free) else (H - 1, W - 1)
        runs = []
        for am in (inside, outside):
            target = rng.rand(H, W) < 0.4
            x1, y1 = rng.randint(0, W), rng.randint(0, H)
            gt = [x1, y1, x1 + rng.randint(0, W), y1 + rng.randint(0, H)]
            if am == inside and boxes[-1][4] > 0:                      # once, a ground truth near a kept box: IoU > 0.5 is reached
                gt = [int(boxes[-1][0]), int(boxes[-1][1]), int(boxes[-1][2]) + 1, int(boxes[-1][3])]
            runs.append((target, gt, am, OB.sentence(mask, target, gt, am, gen=gen)))
        _REF[name] = (gen, runs)
    return _REF[name]


@pytest.mark.parametrize("name,mask", _CASES, ids=[c[0] for c in _CASES])
def test_eval_boxes_equals_the_restatement(name, mask):
    from tris_amd import ops
    H, W = mask.shape
    gen, runs = _reference(name, mask)
    # foreground at assorted positive values, background at 0, at values below the threshold and at the threshold itself
    rng = np.random.RandomState(1)
    cam = np.where(mask, rng.uniform(2e-9, 1.0, (H, W)), rng.choice([0.0, 1e-9, 5e-10, -0.3], (H, W))).astype(np.float32)
    assert ((cam > np.float32(1e-9)) == mask).all()
    cam_d = torch.from_numpy(cam).cuda()
    for target, gt, am, want in runs:
        iu = torch.tensor([0, 0, am[0] * W + am[1]], dtype=torch.int64, device="cuda")
        rec_d, boxes = ops.eval_boxes(cam_d, torch.from_numpy(target.astype(np.uint8)).cuda(), ops.eval_boxes_gt(gt)[0], iu,
                                      return_boxes=True)
        rec = ops.decode_boxes_record(rec_d.tolist())
        print(name, am, gt, {k: rec[k] for k in ("n_prop", "n_nms", "n_kept", "bbox_hit", "box_acc", "box_miou")})
        assert [tuple(b) for b in boxes] == want["boxes"]
        for k in ("hitm", "n_prop", "n_nms", "n_kept", "bbox_hit", "box_acc", "cmax"):
            assert rec[k] == want[k], (k, rec[k], want[k])
        assert np.float32(rec["box_miou"]).view(np.uint32) == np.float32(want["box_miou"]).view(np.uint32)
        assert rec_d.tolist()[12:] == [0, 0, 0, 0]


def test_expected_shapes_of_the_cases():
    """the cases are what they are meant to be (proposal counts of the hand cases; ties and holes among the blobs)"""
    assert _reference("dots64", dots(64))[1][0][3]["n_prop"] == 1024
    assert _reference("checker8", checker8())[1][0][3]["n_kept"] == 16
    assert _reference("cross", cross())[1][0][3]["n_prop"] == 1
    sp = spiral()
    assert OB.proposals(sp) == [(0, 0, 31, 31)] and 400 < sp.sum() < 560
    assert _reference("comb33x65", comb())[1][0][3]["n_prop"] == 1


def test_rejects_what_it_cannot_do():
    from tris_amd import ops
    cam = torch.zeros(4, 4, device="cuda")
    tgt = torch.zeros(4, 4, dtype=torch.uint8, device="cuda")
    iu = torch.zeros(3, dtype=torch.int64, device="cuda")
    with pytest.raises(TypeError):
        ops.eval_boxes(cam, tgt, torch.zeros(4, device="cuda"), iu)
    with pytest.raises(ValueError):
        ops.eval_boxes(cam, torch.zeros(4, 5, dtype=torch.uint8, device="cuda"), ops.eval_boxes_gt([0, 0, 1, 1])[0], iu)
    with pytest.raises(ops.NoGpuError):
        ops.eval_boxes(cam.cpu(), tgt, ops.eval_boxes_gt([0, 0, 1, 1])[0], iu)
