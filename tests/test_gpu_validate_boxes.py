"""validate / validate_same_sentence with cfg.eval_boxes: HitM, box_mIOU and box_Acc against the restatement
(tests/oracle_boxes.py) computed from the dumped cams, the old three numbers untouched, one host sync per group as before."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle_boxes as OB
from test_gpu_parity import _OneRefLoader, _args, refill

pytestmark = pytest.mark.gpu


def _loader(img_size, ann_sizes, S=3, seed0=40):
    from tris_amd.utils.synth import synthetic_batch, synthetic_ids
    rng = np.random.RandomState(3)
    loader = _OneRefLoader()
    for r, (oh, ow) in enumerate(ann_sizes):
        img = synthetic_batch(1, img_size, 20, 0, seed=seed0 + r)["img"]
        ids = torch.from_numpy(synthetic_ids(S, 20, rng))                     # [S, L]
        tgt = torch.zeros(1, oh, ow, dtype=torch.int64)
        tgt[0, oh // 8:oh // 2, ow // 6:ow // 2] = 1
        box = torch.tensor([[ow // 6, oh // 8, ow // 2, oh // 2]])
        loader.append(({"img": img, "word_ids": ids.t().reshape(1, 1, 20, S), "word_masks": torch.ones(1, 1, 20, S)},
                       {"target": tgt, "boxes": box, "img_path": torch.tensor([r]), "sentences": []}))
    return loader


def _aim(loader, model, tmp_path):
    """one plain validate pass, then the targets are laid out from the dumped cams: an even ref's target sits around the arg-max of
    its first sentence (it hits the mask) and its ground-truth box is the bounding box of that sentence's mask (a predicted box
    reaches IoU > 0.5); an odd ref's target and box sit in the image corner farthest from its arg-max points (no hit, low IoU)"""
    from tris_amd import validate as V
    args = _ns(tmp_path, "aim")
    V.validate(args, loader, model, 0, save_cam=True)
    for idx, (smp, tg) in enumerate(loader):
        cams = [np.load(f"{args.cam_save_dir}/{idx}_{j}_{int(tg['img_path'][0])}.npy") for j in range(smp["word_ids"].shape[-1])]
        oh, ow = cams[0].shape
        pts = [np.unravel_index(np.argmax(c), c.shape) for c in cams]
        if idx % 2 == 0:
            y, x = pts[0]
            y0, y1, x0, x1 = max(y - oh // 6, 0), min(y + oh // 5, oh - 1), max(x - ow // 6, 0), min(x + ow // 5, ow - 1)
            ys, xs = np.nonzero(cams[0] > np.float32(1e-9))
            box = [int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1]
        else:
            cy, cx = max(((cy, cx) for cy in (0, oh - 1) for cx in (0, ow - 1)),
                         key=lambda c: min(abs(c[0] - p[0]) + abs(c[1] - p[1]) for p in pts))
            y0, y1 = (0, oh // 6) if cy == 0 else (oh - 1 - oh // 6, oh - 1)
            x0, x1 = (0, ow // 6) if cx == 0 else (ow - 1 - ow // 6, ow - 1)
            box = [x0, y0, x1, y1]
        tg["target"] = torch.zeros(1, oh, ow, dtype=torch.int64)
        tg["target"][0, y0:y1 + 1, x0:x1 + 1] = 1
        tg["boxes"] = torch.tensor([box])
    return loader


def _ns(tmp, tag):
    return SimpleNamespace(print_freq=1000, cam_save_dir=str(tmp / f"cams_{tag}"), name_save_dir=None, dataset="refcocog",
                           save_cam=True, max_query_len=20)


def _restate(loader, cam_dir, S=3):
    """the reference's loop over the dumped cams (validate.py:191-208)"""
    mt = OB.Meters()
    seen = {"hitm": set(), "degenerate": set(), "acc": set()}
    for idx, (_, tg) in enumerate(loader):
        tgt = tg["target"][0].numpy() != 0
        for j in range(S):
            cam = np.load(f"{cam_dir}/{idx}_{j}_{int(tg['img_path'][0])}.npy")
            rec = OB.sentence(cam > np.float32(1e-9), tgt, tg["boxes"][0].tolist(), np.unravel_index(np.argmax(cam), cam.shape))
            print("  sentence", idx, j, {k: rec[k] for k in ("hitm", "n_prop", "n_kept", "bbox_hit", "box_acc", "box_miou")})
            mt.update(rec, 1)
            seen["hitm"].add(rec["hitm"])
            seen["degenerate"].add(rec["n_prop"] == 0)
            seen["acc"].add(rec["box_acc"])
    # the scenario is not a trivial one: masks with proposals, the arg-max on and off the ground-truth mask, boxes that reach
    # IoU > 0.5 and boxes that do not
    assert False in seen["degenerate"] and seen["hitm"] == {0, 1} and seen["acc"] == {0, 1}, seen
    return mt.result()


class _Syncs:
    """counts the device-to-host fetches validate makes (Tensor.tolist / Tensor.item of a device tensor)"""

    def __init__(self, monkeypatch):
        self.n = 0
        tl, it = torch.Tensor.tolist, torch.Tensor.item

        def tolist(t):
            self.n += int(t.is_cuda)
            return tl(t)

        def item(t):
            self.n += int(t.is_cuda)
            return it(t)
        monkeypatch.setattr(torch.Tensor, "tolist", tolist)
        monkeypatch.setattr(torch.Tensor, "item", item)


def _check(model, loader, tmp_path, monkeypatch):
    from tris_amd import ops, validate as V
    from tris_amd.config import cfg
    calls = {"n": 0}
    real = ops.eval_boxes

    def counted(*a, **k):
        calls["n"] += 1
        return real(*a, **k)
    monkeypatch.setattr(ops, "eval_boxes", counted)
    syncs = _Syncs(monkeypatch)

    def run(grp, on):
        args = _ns(tmp_path, f"{grp}_{int(on)}")
        with cfg.override(eval_group=grp, eval_boxes=on):
            n0 = syncs.n
            o, m, h = V.validate(args, loader, model, 0, save_cam=True)
            return (float(o), float(m), float(h)), V.last_metrics(), syncs.n - n0, args.cam_save_dir
    off = {g: run(g, False) for g in (1, 16)}
    assert calls["n"] == 0 and off[1][1] is None and off[16][1] is None and off[1][0] == off[16][0]
    on = {g: run(g, True) for g in (1, 16)}
    n_sent = 3 * len(loader)
    assert calls["n"] == 2 * n_sent
    want = _restate(loader, on[16][3])
    print("off", off[16][0], "on", on[16][0], "metrics", on[1][1], on[16][1], "restatement", want,
          "syncs off/on", [(off[g][2], on[g][2]) for g in (1, 16)])
    for g in (1, 16):
        assert on[g][0] == off[g][0]                               # (oIoU, mIoU, hit) bit for bit
        assert on[g][2] == off[g][2]                               # the records ride the I/U fetch
    assert on[1][1] == on[16][1] == want
    assert off[16][2] < off[1][2]                                  # (the grouped path does sync less: the counter sees them)
    V.validate(_ns(tmp_path, "last"), loader, model, 0)
    assert V.last_metrics() is None                                # the knob is off again


@pytest.fixture(scope="module")
def stage1():
    import warnings
    from tris_amd.model.model_stage1 import TRIS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = TRIS(_args()).cuda()
    refill(m)
    m.eval()
    # A seed-filled model answers every pixel with a positive score (an all-one mask: the default box list only).  Centre the
    # projected pixel features of the first image with the projection's bias: the scores then change sign across the image.
    from tris_amd.utils.synth import synthetic_batch
    seen = []
    hook = m.vis_project.register_forward_hook(lambda mod, inp, out: seen.append(out))
    with torch.no_grad():
        m.encode_visual(synthetic_batch(1, 320, 20, 0, seed=40)["img"].cuda())
        hook.remove()
        m.vis_project.bias.sub_(seen[0].reshape(-1, seen[0].shape[-1]).mean(0))
    return m


def test_stage1_validate_reports_hitm_and_the_box_metrics(stage1, tmp_path, monkeypatch):
    _check(stage1, _aim(_loader(320, [(120, 160), (97, 131)]), stage1, tmp_path), tmp_path, monkeypatch)


class _Shifted(torch.nn.Module):
    """a Stage-2 model whose logit maps are lowered by a constant, so that they change sign across the image (a seed-filled
    decoder answers with one sign everywhere).  validate reaches a signed-map model through these two methods only."""
    signed_maps = True

    def __init__(self, net, shift):
        super().__init__()
        self.net, self.shift = net, float(shift)

    def encode_visual(self, x):
        return self.net.encode_visual(x)

    def forward_pairs(self, vis_state, word_id, owner, out_size):
        return self.net.forward_pairs(vis_state, word_id, owner, out_size) - self.shift


def test_stage2_signed_maps(tmp_path, monkeypatch):
    from test_gpu_stage2 import _model
    m, _ = _model(64)
    m.eval()
    loader = _loader(64, [(48, 70), (64, 64)])
    with torch.no_grad():
        smp = loader[0][0]
        first = m.forward_pairs(m.encode_visual(smp["img"].cuda()), smp["word_ids"][0, 0].t()[:1].contiguous().cuda(), [0], 64)
    net = _Shifted(m, first.float().quantile(0.6).item()).eval()
    _check(net, _aim(loader, net, tmp_path), tmp_path, monkeypatch)


def test_same_sentence_reports_hitm_weighted_by_the_sentence_count(stage1, tmp_path):
    import warnings
    from tris_amd import validate as V
    from tris_amd.CLIP import clip
    from tris_amd.config import cfg
    from tris_amd.train_stage1 import freeze_aux
    from tris_amd.utils.synth import seed_fill
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        aux, _ = clip.load("ViT-B-32", device="cuda", txt_length=20)
    seed_fill(aux.state_dict(), 4321)
    aux = freeze_aux(aux)
    # refs with 3 and 2 sentences: the weighting shows
    loader = _loader(320, [(120, 160)], S=3) + _loader(320, [(97, 131)], S=2, seed0=41)
    args = _ns(tmp_path, "prms")
    V.validate_same_sentence(args, loader, stage1, 0, clip_model=aux)
    for idx, (_, tg) in enumerate(loader):       # the 3-sentence ref's target around its arg-max, the other's away from it
        cam = np.load(f"{args.cam_save_dir}/{idx}_{int(tg['img_path'][0])}.npy")
        y, x = np.unravel_index(np.argmax(cam), cam.shape)
        tg["target"] = torch.zeros(1, *cam.shape, dtype=torch.int64)
        if idx == 0:
            tg["target"][0, max(y - 9, 0):y + 10, max(x - 9, 0):x + 10] = 1
        else:
            tg["target"][0, (y + cam.shape[0] // 2) % cam.shape[0], :] = 1
    off = V.validate_same_sentence(args, loader, stage1, 0, clip_model=aux)
    assert V.last_metrics() is None
    with cfg.override(eval_boxes=True):
        on = V.validate_same_sentence(args, loader, stage1, 0, clip_model=aux)
    lm = V.last_metrics()
    assert tuple(float(v) for v in on) == tuple(float(v) for v in off)
    hitm = 0
    for idx, (smp, tg) in enumerate(loader):
        cam = np.load(f"{args.cam_save_dir}/{idx}_{int(tg['img_path'][0])}.npy")
        y, x = np.unravel_index(np.argmax(cam), cam.shape)
        hitm += int(tg["target"][0, y, x] != 0) * smp["word_ids"].shape[-1]
    print("PRMS HitM", lm, "restated", hitm / 5 * 100)
    assert hitm == 3                                                # (the first ref's three sentences)
    assert lm["n_sent"] == 5 and lm["hitm"] == hitm / 5 * 100 and lm["box_miou"] is None and lm["box_acc"] is None
