"""ReferIt evaluation on the MI355X (csrc/referit.hip, tris_amd.validate_referit, tris_amd.dataset.hbm_referit): the run-length
decoder byte for byte against cocomask, the grouped scoring bit for bit against K calls of the single-sentence entries, and
validate_referit.validate -- through the HBM cache and through DataLoader(ImageLoader) -- against the restated loop of
tests/oracle_referit.py over cams from a one-sentence-at-a-time pass.  Everything here is integer or bit-exact: no tolerance."""

import numpy as np
import pytest
import torch

import oracle_boxes as OB
import oracle_referit as O

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ decode
def _random_counts(rng, n, mean, zero_runs=0, first0=False):
    """run lengths that sum to n exactly, with `zero_runs` interior zero-length runs"""
    c, left = [], n
    while left > 0:
        r = min(int(rng.geometric(1.0 / mean)), left)
        c.append(r)
        left -= r
    for _ in range(zero_runs):                                  # (a zero run flips the value of everything behind it: still an RLE)
        c.insert(int(rng.randint(1, len(c) + 1)), 0)
    return ([0] + c) if first0 else c


def _sentences(H, W, K, seed):
    rng = np.random.RandomState(seed)
    n, mean = H * W, max(H * W / 40.0, 2.0)
    seg = lambda **kw: {"size": [H, W], "counts": _random_counts(rng, n, mean, **kw)}      # noqa: E731
    pool = [
        [seg(first0=True), seg(zero_runs=3)],                                   # first count 0; interior zero runs
        [],                                                                     # no segment, between two that have some
        [seg(), seg(first0=True), seg(zero_runs=2)],                            # three overlapping segments
        [{"size": [H, W], "counts": [n]}],                                      # all background
        [{"size": [H, W], "counts": [0, n]}],                                   # all foreground
        [{"size": [H, W], "counts": [H + 1, H, 2]}, {"size": [H, W], "counts": [0, min(3, n)]}],   # sums short of H*W
        [{"size": [H, W], "counts": O.counts_to_string(_random_counts(rng, n, mean))}, seg(zero_runs=4, first0=True)],
    ]
    return pool[:K]


def _decode_reference(sents, H, W):
    from tris_amd.dataset import cocomask
    return np.stack([cocomask.decode(s).sum(2).astype(np.uint8) if s else np.zeros((H, W), np.uint8) for s in sents])


@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("H,W", [(7, 5), (13, 9), (37, 50), (480, 360)])
def test_rle_decode_sum_equals_cocomask(H, W, K):
    from tris_amd import ops
    sents = _sentences(H, W, K, seed=H * 7 + K)
    got = ops.rle_decode_sum(sents, H, W)
    want = _decode_reference(sents, H, W)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (K, H, W)
    assert np.array_equal(got.cpu().numpy(), want)
    if K == 7:
        assert want[2].max() >= 2 and not want[1].any() and not want[3].any() and want[4].all() and want[5].sum() == H + min(3, H * W)


def test_rle_decode_sum_grid_stride_path():
    from tris_amd import ops
    H = W = 520                                                 # more than 1024 x 256 pixels
    sents = _sentences(H, W, 3, seed=5)
    assert np.array_equal(ops.rle_decode_sum(sents, H, W).cpu().numpy(), _decode_reference(sents, H, W))


def test_rle_decode_sum_from_a_shared_arena():
    """sentences of two images of different sizes in one arena, addressed by ranges -- the cache's form"""
    from tris_amd import ops
    from tris_amd.dataset.rle_arena import RleArena
    arena, ranges, sents = RleArena(), {}, {}
    for H, W in ((13, 9), (7, 5)):
        sents[H, W] = _sentences(H, W, 7, seed=H)
        ranges[H, W] = [arena.add_sentence(s, H, W) for s in sents[H, W]]
    ends, seg_off = arena.to("cuda")
    for (H, W), r in ranges.items():
        rng = torch.tensor(r, dtype=torch.int32).reshape(-1, 2).cuda()
        assert np.array_equal(ops.rle_decode_sum_arena(ends, seg_off, rng, H, W).cpu().numpy(), _decode_reference(sents[H, W], H, W))


# ------------------------------------------------------------------------------------------------------------------ scoring
def _maps(S, K, signed, seed):
    g = torch.Generator().manual_seed(seed)
    plateau = torch.zeros(S, S)
    plateau[2:, :] = 0.75                                       # many equal maxima: the first index must win
    rnd = lambda: torch.randn(S, S, generator=g) if signed else torch.randn(S, S, generator=g).relu()   # noqa: E731
    pool = [rnd(), torch.zeros(S, S), plateau, (-torch.rand(S, S, generator=g) - 0.5) if signed else rnd(), rnd(), rnd(), rnd()]
    return torch.stack(pool[:K]).cuda()


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("oH,oW", [(7, 5), (33, 47), (520, 520)])
@pytest.mark.parametrize("S", [8, 20])
def test_eval_post_group_equals_the_single_entries(S, oH, oW, K, signed):
    from tris_amd import ops
    maps = _maps(S, K, signed, seed=S + oH + K)
    targets = torch.from_numpy(np.random.RandomState(oH + K).randint(0, 3, size=(K, oH, oW)).astype(np.uint8)).cuda()
    records, cams = ops.eval_post_group(maps, targets, signed=signed)
    rec_only, none = ops.eval_post_group(maps, targets, signed=signed, cams=None)
    assert none is None and torch.equal(rec_only, records)
    assert records.dtype == torch.int64 and tuple(records.shape) == (K, 4) and tuple(cams.shape) == (K, oH, oW)
    single = ops.eval_post_signed if signed else ops.eval_post
    flat = targets.flatten(1)
    for k in range(K):
        iu, cam = single(maps[k:k + 1], (targets[k] != 0).to(torch.uint8))
        assert torch.equal(records[k, :3], iu), (k, records[k].tolist(), iu.tolist())
        assert torch.equal(cams[k].view(torch.int32), cam.view(torch.int32)), k            # bit for bit
        assert int(records[k, 3]) == int(flat[k, int(records[k, 2])])
    if K >= 3:
        assert int(records[1, 2]) == 0 and not cams[1].any()                              # the all-zero map
        c = cams[2].flatten().cpu().numpy()
        assert int(records[2, 2]) == int(np.argmax(c)) > 0 and (c == c.max()).sum() > 1   # equal maxima: the first
    if K >= 4 and signed:
        # a negative max flips the sign (validate_referit.py:163 divides by it): every pixel passes 1e-9
        assert float(maps[3].max()) < 0 and records[3, :2].tolist() == [int((targets[3] != 0).sum()), oH * oW]
    assert {0, 1, 2} <= set(targets.flatten().tolist()[:64])


# ------------------------------------------------------------------------------------------------------------------ end to end
def _args(size, root):
    from tris_amd.args import get_parser
    return get_parser().parse_args(["--backbone", "clip-RN50", "--size", str(size), "--max_query_len", "20", "--dataset", "referit",
                                    "--test_split", "test", "--refer_data_root", str(root), "--print-freq", "1000"])


def _dataset(size, root):
    from tris_amd.dataset.Dataset_referit import get_refit_dataset
    return get_refit_dataset(_args(size, root))[1]


def _single_pass(net, ds, post):
    """the reference's loop structure: the model called with ONE sentence at a time, ops.eval_post* on (mask != 0).
    -> (items, cams) for oracle_referit.restate"""
    from tris_amd import ops
    items, cams = [], []
    with torch.no_grad(), ops.batch_invariant():
        for n in range(len(ds)):
            img, out, (H, W), _ = ds[n]
            items.append([{"bbox": it["bbox"], "mask": it["mask"], "key": k} for k, it in out.items()])
            cams.append([])
            if not out:
                continue
            img = img.unsqueeze(0).cuda()
            vis = net.encode_visual(img)
            for it in out.values():
                wid = it["word_id"].reshape(1, -1).to(torch.int64).cuda()
                m = net.forward_cached(vis, wid, img.shape[2]) if hasattr(net, "forward_cached") else net.forward_pairs(vis, wid, [0], img.shape[2])
                _, cam = post(m, torch.from_numpy((it["mask"] != 0).astype(np.uint8)).cuda())
                cams[-1].append(cam.cpu().numpy())
    return items, cams


def _aimed_root(net, size, tmp_path, post):
    """a first pass over the default tree gives every aimed annotation's arg-max; the second tree lays its targets out around them"""
    ds0 = _dataset(size, O.synthetic_root(tmp_path / "first"))
    items, cams = _single_pass(net, ds0, post)
    aims = {}
    for n, (sents, cs) in enumerate(zip(items, cams)):
        for s, cam in zip(sents, cs):
            y, x = np.unravel_index(np.argmax(cam), cam.shape)
            aims[str(ds0.files[n]), int(s["key"])] = (int(y), int(x))
    assert set(O.AIMED) <= set(aims)
    return O.synthetic_root(tmp_path / "aimed", aims)


class _Syncs:
    """counts the device-to-host fetches (Tensor.tolist / Tensor.item of a device tensor), as tests/test_gpu_validate_boxes.py does"""

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


def _check(net, size, tmp_path, monkeypatch, signed):
    from torch.utils.data import DataLoader
    from tris_amd import ops, validate_referit as VR
    from tris_amd.config import cfg
    from tris_amd.dataset.hbm_referit import HbmReferitCache, HbmReferitLoader
    post = ops.eval_post_signed if signed else ops.eval_post
    root = _aimed_root(net, size, tmp_path, post)
    ds = _dataset(size, root)
    args = _args(size, root)
    items, cams = _single_pass(net, ds, post)
    want = O.restate(items, cams)
    print("restated", want)
    # both values of Hit and of HitM occur, and one HitM = 0 is an arg-max on a count-2 pixel
    assert {p[0] for p in want["pairs"]} == {0, 1} and {p[1] for p in want["pairs"]} == {0, 1}
    dbl, cam = items[0][1], cams[0][1]
    assert dbl["key"] == "2" and dbl["mask"][np.unravel_index(np.argmax(cam), cam.shape)] == 2 and want["pairs"][1] == (1, 0)
    assert want["pairs"][3 + 3] == (1, 0)                       # 1004/0: only the second box holds the point, the mask is elsewhere
    assert want["n_sent"] == 8

    calls = {"decode": 0, "group": 0}
    for name, key in (("rle_decode_sum_arena", "decode"), ("eval_post_group", "group")):
        real = getattr(ops, name)

        def counted(*a, _real=real, _key=key, **k):
            calls[_key] += 1
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, counted)
    syncs = _Syncs(monkeypatch)

    def run(loader):
        n0 = syncs.n
        o, m, h = VR.validate(args, loader, net, 0)
        assert isinstance(o, float) and torch.is_tensor(m) and m.dim() == 0 and isinstance(h, float)
        return (o, float(m), h), VR.last_metrics(), syncs.n - n0

    hbm = HbmReferitLoader(HbmReferitCache(ds, size))
    plain = DataLoader(ds, batch_size=1, shuffle=False, num_workers=0)
    assert len(hbm) == len(plain) == 4
    r_hbm, r_dl = run(hbm), run(plain)
    print("hbm", r_hbm, "dataloader", r_dl)
    assert calls == {"decode": 3, "group": 6}                   # per image with sentences: one decode (cache only), one scoring
    assert r_hbm[2] == r_dl[2] == 3                             # exactly one host sync per image that has sentences
    assert r_hbm[:2] == r_dl[:2]
    assert r_hbm[0] == (want["oiou"], float(torch.tensor(want["miou"])), want["hit"])
    assert r_hbm[1] == {"hitm": want["hitm"], "box_miou": None, "box_acc": None, "n_sent": 8}
    # box metrics: the same cams through the restatement of generate_bbox, against the FIRST ground-truth box
    mt = OB.Meters()
    for sents, cs in zip(items, cams):
        for s, cam in zip(sents, cs):
            mt.update(OB.sentence(cam > np.float32(1e-9), s["mask"] != 0, np.asarray(s["bbox"])[0].tolist(),
                                  np.unravel_index(np.argmax(cam), cam.shape)), 1)
    boxes = mt.result()
    with cfg.override(eval_boxes=True):
        b_hbm, b_dl = run(hbm), run(plain)
    print("boxes", b_hbm[1], "restated", boxes)
    assert b_hbm[0] == b_dl[0] == r_hbm[0] and b_hbm[2] == b_dl[2] == 3                    # the records ride the same sync
    assert b_hbm[1] == b_dl[1] == {"hitm": want["hitm"], "box_miou": boxes["box_miou"], "box_acc": boxes["box_acc"], "n_sent": 8}


def test_stage1_validate_referit_equals_the_restated_loop(tmp_path, monkeypatch):
    import warnings
    from test_gpu_parity import refill
    from tris_amd.model.model_stage1 import TRIS
    size = 224
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = TRIS(_args(size, tmp_path)).cuda()
    refill(m)
    m.eval()
    # a seed-filled model answers every pixel with a positive score: centre the projected pixel features of the first image with
    # the projection's bias, so that the scores change sign across the image (tests/test_gpu_validate_boxes.py does the same)
    ds = _dataset(size, O.synthetic_root(tmp_path / "centre"))
    seen = []
    hook = m.vis_project.register_forward_hook(lambda mod, inp, out: seen.append(out))
    with torch.no_grad():
        m.encode_visual(ds[0][0].unsqueeze(0).cuda())
        hook.remove()
        m.vis_project.bias.sub_(seen[0].reshape(-1, seen[0].shape[-1]).mean(0))
    _check(m, size, tmp_path, monkeypatch, signed=False)


def test_stage2_validate_referit_takes_the_signed_path(tmp_path, monkeypatch):
    from test_gpu_stage2 import _model
    from test_gpu_validate_boxes import _Shifted
    size = 64
    m, _ = _model(size)
    m.eval()
    ds = _dataset(size, O.synthetic_root(tmp_path / "shift"))
    with torch.no_grad():
        img, out, _, _ = ds[0]
        wid = out["0"]["word_id"].reshape(1, -1).to(torch.int64).cuda()
        first = m.forward_pairs(m.encode_visual(img.unsqueeze(0).cuda()), wid, [0], size)
    net = _Shifted(m, first.float().quantile(0.6).item()).eval()
    _check(net, size, tmp_path, monkeypatch, signed=True)


def test_cache_build_names_a_missing_image_and_a_malformed_rle(tmp_path):
    import os
    from tris_amd.dataset.hbm_referit import HbmReferitCache
    ds = _dataset(64, O.synthetic_root(tmp_path / "rle"))
    H, W = O.SIZES["1001"]
    ds.annotations["1001"]["annotations"][2]["segmentation"][1]["counts"] = [5, H * W]
    with pytest.raises(ValueError, match="1001 annotation 2 segment 1.*past H\\*W"):
        HbmReferitCache(ds, 64)
    root = O.synthetic_root(tmp_path / "img")
    os.remove(os.path.join(root, "images", "1004.jpg"))
    with pytest.raises(FileNotFoundError, match="1004.jpg"):
        HbmReferitCache(_dataset(64, root), 64)
