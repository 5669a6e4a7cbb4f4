"""tris_amd.predict.Predictor and tris_amd.demo.main on synthetic weights at 64 px, Stage 1 and Stage 2: the preprocessing is
get_transform(size, train=False) bit for bit, cam / mask / point are what validate computes for the same picture and sentences,
a sentence does not depend on its company, heat is ops.cam_paint of the model's own map, and the command writes that figure."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

import oracle_overlay as OV
from test_gpu_parity import _OneRefLoader

pytestmark = pytest.mark.gpu

SIZE, L = 64, 20
SENTENCES = ["man on the right", "the dog, left of the bench", "a red umbrella behind two people walking along the street in the rain"]


def _stage1():
    import warnings
    from test_gpu_stage2 import _args
    from tris_amd.model.model_stage1 import TRIS
    from tris_amd.utils.synth import seed_fill
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = TRIS(_args(SIZE)).cuda()
    seed_fill(m.state_dict(), 1234)
    return m.eval()


def _stage2():
    from test_gpu_stage2 import _model
    return _model(SIZE)[0].eval()


@pytest.fixture(scope="module", params=["stage1", "stage2"])
def predictor(request):
    from tris_amd.predict import Predictor
    return Predictor(_stage1() if request.param == "stage1" else _stage2(), size=SIZE, max_query_len=L)


def _picture(h=50, w=37):
    return OV.case_image(h, w, seed=h)


@pytest.mark.parametrize("hw", [(50, 37), (72, 60)])
def test_preprocessing_is_the_evaluation_transform(predictor, hw):
    from tris_amd.dataset.transform import get_transform
    pic = _picture(*hw)
    want, _ = get_transform(SIZE, train=False)(Image.fromarray(pic), Image.new("L", hw[::-1]))
    for src in (pic, torch.from_numpy(pic), Image.fromarray(pic)):
        dev, x = predictor.preprocess(src)
        assert dev.dtype == torch.uint8 and np.array_equal(dev.cpu().numpy(), pic)
        assert x.shape == (1, 3, SIZE, SIZE) and x.is_contiguous() and torch.equal(x[0].cpu(), want)
    grey = pic[:, :, 0].copy()
    assert torch.equal(predictor.preprocess(grey)[0].cpu(), torch.from_numpy(np.stack([grey] * 3, -1)))
    assert torch.equal(predictor.preprocess(Image.fromarray(grey))[0].cpu(), torch.from_numpy(np.stack([grey] * 3, -1)))


def test_segment_is_what_validate_scores(predictor, tmp_path):
    from tris_amd import ops, validate as V
    from tris_amd.CLIP import clip
    from tris_amd.dataset.transform import get_transform
    pic = _picture()
    H, W = pic.shape[:2]
    preds = predictor.segment(pic, SENTENCES)
    assert [p.sentence for p in preds] == SENTENCES
    # the same picture and sentences through validate's one-ref loader
    img, _ = get_transform(SIZE, train=False)(Image.fromarray(pic), Image.new("L", (W, H)))
    ids = torch.stack([clip.tokenize(s).squeeze(0)[:L] for s in SENTENCES]).to(torch.int64)             # [S, L]
    loader = _OneRefLoader()
    loader.append(({"img": img.unsqueeze(0), "word_ids": ids.t().reshape(1, 1, L, len(SENTENCES)),
                    "word_masks": torch.ones(1, 1, L, len(SENTENCES))},
                   {"target": torch.zeros(1, H, W, dtype=torch.int64), "boxes": torch.tensor([[0, 0, 1, 1]]),
                    "img_path": torch.tensor([0]), "sentences": []}))
    args = SimpleNamespace(print_freq=1000, cam_save_dir=str(tmp_path / "cams"), name_save_dir=None, dataset="refcocog",
                           save_cam=True, max_query_len=L)
    V.validate(args, loader, predictor.model, 0, save_cam=True)
    for j, p in enumerate(preds):
        cam = np.load(f"{args.cam_save_dir}/0_{j}_0.npy")
        r = p.numpy()
        assert r.cam.dtype == np.float32 and r.cam.shape == (H, W) and np.array_equal(r.cam, cam), j
        assert r.mask.dtype == bool and np.array_equal(r.mask, cam > np.float32(1e-9))
        assert p.point == tuple(int(v) for v in np.unravel_index(np.argmax(cam), cam.shape))
        assert p.cam.is_cuda and p.mask.is_cuda and p.heat.is_cuda and r.heat.shape == (H, W, 3) and r.heat.dtype == np.uint8
    # heat: the overlay kernel on the model's own maps, all sentences in one call
    with torch.no_grad(), ops.batch_invariant():
        dev, x = predictor.preprocess(pic)
        maps = predictor.net.forward_pairs(predictor.net.encode_visual(x), predictor.tokenize(SENTENCES), [0] * 3, SIZE)
    heat, _, rng, _ = ops.cam_paint(maps.contiguous(), dev, predictor.colormap)
    for j, p in enumerate(preds):
        assert torch.equal(p.heat, heat[j]) and p.range == tuple(float(v) for v in rng[j].tolist())
    # alone or among three: bit-identical
    for j in (0, 2):
        one = predictor.segment(Image.fromarray(pic), SENTENCES[j])[0]
        assert torch.equal(one.cam, preds[j].cam) and torch.equal(one.mask, preds[j].mask) and torch.equal(one.heat, preds[j].heat)
        assert one.point == preds[j].point and one.range == preds[j].range
    assert predictor.segment(pic, []) == []


def test_demo_main_writes_the_figure(tmp_path):
    from tris_amd import demo
    from tris_amd.args import get_parser
    from tris_amd.predict import Predictor
    model = _stage2()
    pic = _picture(72, 60)
    Image.fromarray(pic).save(tmp_path / "demo.png")
    torch.save({"model": model.state_dict()}, tmp_path / "ckpt.pth")
    text = "man, on the right"                                                  # one expression, the comma included
    args = get_parser().parse_args(["--img", str(tmp_path / "demo.png"), "--text", text, "--output", str(tmp_path), "--pretrain",
                                    "ckpt.pth", "--size", str(SIZE), "--max_query_len", str(L), "--vis_out", str(tmp_path / "vis")])
    path = demo.main(args)
    assert path == str(tmp_path / "vis" / f"demo_({text}).png")
    want = Predictor(model, size=SIZE, max_query_len=L).segment(pic, [text])[0]
    assert np.array_equal(np.asarray(Image.open(path)), want.heat.cpu().numpy())
    # visualize_cam / get_norm_cam: the two modes of the kernel at identity size, as the reference chains them
    norm = demo.get_norm_cam(want.cam.cpu() - 0.25)
    cam = np.maximum(want.cam.cpu().numpy() - np.float32(0.25), 0)
    assert norm.dtype == np.float32 and np.abs(norm - (cam - cam.min()) / (cam.max() - cam.min() + np.float32(1e-5))).max() <= OV.TOL
    fig = demo.visualize_cam(norm, pic)
    assert np.array_equal(fig, OV.blend(OV.jet_table()[np.uint8(norm * np.float32(255))], pic))
    demo.visualize_cam(norm, root=str(tmp_path / "plain.png"))
    assert np.array_equal(np.asarray(Image.open(tmp_path / "plain.png")), OV.jet_table()[np.uint8(norm * np.float32(255))])
    with pytest.raises(RuntimeError, match="unset"):                             # no silent random initialisation
        torch.save({"model": {k: v for k, v in model.state_dict().items() if not k.startswith("backbone.")}}, tmp_path / "part.pth")
        Predictor.from_checkpoint(tmp_path / "part.pth", args)
