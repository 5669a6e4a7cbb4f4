"""Stage-2 on the host (no GPU): the model's state-dict keys and parameter groups, the no-grad flags, the drop-in names, the
new ops' refusal of CPU tensors, the trainer's clear errors, and ReferDataset(pseudo_path) items."""
import os

import numpy as np
import pytest
import torch


def _args(extra=()):
    from tris_amd.args import get_parser
    return get_parser().parse_args(["--backbone", "clip-RN50", "--size", "320", "--max_query_len", "20"] + list(extra))


@pytest.fixture(scope="module")
def model():
    import warnings
    from tris_amd.CLIP import clip
    from tris_amd.model.model_stage2 import TRIS
    with warnings.catch_warnings(), clip.random_init():
        warnings.simplefilter("ignore")
        return TRIS(_args())


def test_state_dict_keys_and_shapes(model):
    sd = model.state_dict()
    assert len(sd) == 625
    want = {"reduced_c1.conv.weight": (64, 256, 3, 3), "reduced_c4.conv.weight": (512, 2048, 3, 3), "output1.conv.weight": (32, 64, 3, 3),
            "final_seg1.0.conv.weight": (32, 32, 3, 3), "final_seg4.0.conv.weight": (64, 256, 3, 3), "final_seg2.1.weight": (1, 32, 1, 1),
            "final_seg4.1.weight": (1, 64, 1, 1), "output3.relu.weight": (1,), "output3.bn.num_batches_tracked": (),
            "attention4.Wq.weight": (2048, 2048, 1, 1), "attention2.Wk.weight": (512, 512, 1)}
    for k, shp in want.items():
        assert tuple(sd[k].shape) == shp, k
    assert all(float(sd[k]) == 0.25 for k in sd if k.endswith(".relu.weight"))   # nn.PReLU() default slope
    assert sum(k.endswith(".relu.weight") for k in sd) == 12


def _golden_keys():
    import json
    from conftest import GOLDEN
    return json.load(open(os.path.join(GOLDEN, "g13_stage2_keys.json")))


def test_keys_and_shapes_equal_the_reference(model):
    """tests/golden/g13_stage2_keys.json, recorded from the reference (tools/gen_golden_stage2.py)"""
    g = _golden_keys()
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == g["keys"]


def test_parameter_groups_and_no_grad_flags(model):
    g = _golden_keys()
    named = dict(model.named_parameters())
    bb, hd = model.trainable_parameters()
    assert (len(bb), len(hd)) == (322, 102)
    assert [id(p) for p in bb] == [id(named[k]) for k in g["backbone_group"]]
    assert [id(p) for p in hd] == [id(named[k]) for k in g["head_group"]]
    assert "backbone.positional_embedding" in g["head_group"] and "backbone.visual.attnpool.positional_embedding" in g["head_group"]
    for k in ["backbone.text_projection", "backbone.logit_scale"] + [k for k in named if ".attnpool." in k]:
        assert getattr(named[k], "_tris_no_grad_path", False), k
    assert not getattr(named["reduced_c1.relu.weight"], "_tris_no_grad_path", False)


def test_restatement_matches_the_reference_recording(model):
    """tests/oracle_stage2.py -- the numerical reference of the GPU tests -- against the reference model itself (g13_stage2_model.npz:
    64 px, B = 2, seed-filled weights, PReLU slopes 0.25 +- 0.05).  The reference only runs in fp32 (its LayerNorm casts to fp32), so
    the bounds are those of two fp32 runs of the same algorithm: losses and the eval map agree to ~1e-6; the train maps and the
    gradients pass through train-mode BatchNorms over as few as 8 values (layer4 at 64 px is 2 x 2) that amplify round-off --
    measured 1.5e-4 on the maps and 0.3-2 % on the gradient heads; an operator that differs moves them by O(1)."""
    import sys
    sys.path.insert(0, os.path.dirname(__file__))
    import oracle_stage2 as S
    from conftest import GOLDEN
    from tris_amd.utils.synth import seed_fill
    g = np.load(os.path.join(GOLDEN, "g13_stage2_model.npz"))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    seed_fill(sd, 1234)
    S.reset_slopes(sd)
    probes = [k[len("grad_head."):] for k in g.files if k.startswith("grad_head.")]
    slopes = [k[len("grad_slope."):] for k in g.files if k.startswith("grad_slope.")]
    assert len(slopes) == 12
    s = {k: v.clone() for k, v in sd.items()}
    for k in probes + slopes:
        s[k].requires_grad_()
    img, ids, tgt = (torch.from_numpy(g[k]) for k in ("img", "word_ids", "target"))
    assert int(tgt.max()) == 2
    outs = S.forward(s, img, ids, True)
    ls = S.losses(outs, tgt)
    ls[0].backward()

    def rel(a, b):
        return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))
    assert rel(torch.stack(ls).detach().numpy(), g["losses"]) < 1e-6
    assert rel(torch.stack(outs).detach().numpy(), g["outs"]) < 1e-3
    for k in probes:
        assert abs(float(s[k].grad.norm()) - float(g["grad_norm." + k])) <= 1e-2 * float(g["grad_norm." + k]), k
        assert rel(s[k].grad.reshape(-1)[:16].numpy(), g["grad_head." + k]) < 5e-2, k
    for k in slopes:
        assert rel(s[k].grad.numpy(), g["grad_slope." + k]) < 5e-2, k
    for k in (x[len("running_mean."):] for x in g.files if x.startswith("running_mean.")):
        assert rel(s[k + ".running_mean"].numpy(), g["running_mean." + k]) < 1e-3, k
        assert rel(s[k + ".running_var"].numpy(), g["running_var." + k]) < 1e-3, k
    with torch.no_grad():
        ev = S.forward({k: v.clone() for k, v in sd.items()}, img, ids, False)
    assert rel(ev.numpy(), g["eval"]) < 1e-5


def test_backbones():
    import warnings
    from tris_amd.model.model_stage2 import TRIS
    with pytest.raises(ValueError):
        TRIS(_args(["--backbone", "clip-ViT-B/16"]))
    from tris_amd.model.model_stage2 import ConvBNRelu
    with pytest.raises(NotImplementedError):
        ConvBNRelu(8, 8, kernel_size=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert ConvBNRelu(8, 16, 3, 1, 1).relu.weight.shape == (1,)


def test_new_ops_refuse_cpu_tensors():
    from tris_amd import ops
    x = torch.randn(1, 4, 4, 32)
    c = torch.ones(32)
    with pytest.raises(ops.NoGpuError):
        ops.bn_prelu(x, c, c, c, c, torch.tensor([0.25]))
    with pytest.raises(ops.NoGpuError):
        ops.upsample_nhwc(x, (8, 8), skip=torch.randn(1, 8, 8, 32))
    with pytest.raises(ops.NoGpuError):
        ops.head1x1(x, torch.randn(1, 32, 1, 1))
    with pytest.raises(ops.NoGpuError):
        ops.bce4([torch.randn(1, 1, 4, 4)] * 4, torch.zeros(1, 1, 4, 4, dtype=torch.long))
    with pytest.raises(ops.NoGpuError):
        ops.eval_post_signed(torch.randn(1, 1, 4, 4), torch.zeros(4, 4, dtype=torch.uint8))


def test_trainer_refuses_ema_and_distributed():
    from tris_amd import train_stage2
    with pytest.raises(NotImplementedError, match="ema_pytorch"):
        train_stage2.main(_args(["--model_ema"]))
    with pytest.raises(NotImplementedError, match="single GPU"):
        train_stage2.main(_args(["--distributed"]))
    with pytest.raises(NotImplementedError, match="ema_pytorch"):
        train_stage2.train_one_epoch([], None, None, 0, 0, _args(["--model_ema"]))


def test_dropin_names_and_signatures():
    """argument lists equal the reference's, as recorded in g13_stage2_keys.json"""
    import inspect
    from tris_amd import dropin, train_stage2
    from tris_amd.model import model_stage2
    assert dropin.ALIASES["model.model_stage2"] == "tris_amd.model.model_stage2"
    assert dropin.ALIASES["train_stage2"] == "tris_amd.train_stage2"
    want = _golden_keys()["signatures"]

    def names(f):
        return list(inspect.signature(f).parameters)
    assert names(model_stage2.TRIS.__init__) == want["model_stage2.TRIS.__init__"]
    assert names(model_stage2.TRIS.forward) == want["model_stage2.TRIS.forward"]
    assert names(model_stage2.ConvBNRelu.__init__) == want["model_stage2.ConvBNRelu.__init__"]
    assert names(model_stage2.criterion) == want["model_stage2.criterion"]
    assert names(train_stage2.train_one_epoch) == want["train_stage2.train_one_epoch"]
    assert names(train_stage2.main)[:len(want["train_stage2.main"])] == want["train_stage2.main"]   # (+ tokenizer=None, as Stage-1)


def test_pseudo_items_equal_the_reference_recording(tmp_path):
    """ReferDataset(pseudo_path) training items against the reference's own (g13_stage2_pseudo.npz): the summed instance masks,
    NEAREST-resized, int64 [1,S,S] bit for bit, and the sentence draws of the same np.random sequence"""
    from conftest import GOLDEN
    from tris_amd.dataset.ReferDataset import ReferDataset
    from tris_amd.dataset.transform import get_transform
    from tris_amd.utils.synth import make_mini_refer, make_pseudo_masks, word_hash_tokenize
    g = np.load(os.path.join(GOLDEN, "g13_stage2_pseudo.npz"))
    n_images, ds_seed, mask_seed, size, rng_seed = (int(v) for v in g["params"])
    root = make_mini_refer(str(tmp_path / "data"), n_images=n_images, seed=ds_seed)
    pdir = make_pseudo_masks(root, str(tmp_path / "pseudo"), seed=mask_seed)
    ds = ReferDataset(root, "refcocog", "umd", image_transforms=get_transform(size, True), split="train", eval_mode=False,
                      size=size, max_tokens=20, pseudo_path=pdir, tokenizer=word_hash_tokenize)
    np.random.seed(rng_seed)
    items = [ds[i] for i in range(len(ds))]
    got = torch.stack([t["pseudo_gt"] for _, t in items]).numpy()
    assert got.dtype == np.int64 and np.array_equal(got, g["pseudo_gt"]) and got.max() == 2
    assert np.array_equal(torch.stack([s["word_ids"] for s, _ in items]).numpy(), g["word_ids"])
    assert np.array_equal(torch.stack([s["img"] for s, _ in items]).numpy(), g["img"])


def test_pseudo_targets_sum_instances(tmp_path):
    """ReferDataset.py:178-186: the sum of the instance masks (overlaps give 2), NEAREST to size x size, int64 [1,S,S]; the random
    draws of a training item are those of an item without pseudo masks"""
    from PIL import Image
    from tris_amd.dataset.ReferDataset import ReferDataset
    from tris_amd.dataset.transform import get_transform
    from tris_amd.utils.synth import make_mini_refer, word_hash_tokenize
    root = make_mini_refer(str(tmp_path / "data"), n_images=6, seed=1)
    plain = ReferDataset(root, "refcocog", "umd", image_transforms=get_transform(64, True), split="train", eval_mode=False,
                         size=64, tokenizer=word_hash_tokenize)
    d = str(tmp_path / "pseudo")
    os.makedirs(d)
    rng = np.random.RandomState(0)
    want = []
    for i in range(len(plain)):
        _, img_id, rec = plain.image_record(i)
        h, w = rec["height"], rec["width"]
        mk = rng.rand(2, h, w) > 0.5
        np.save(os.path.join(d, f"{i}_{img_id}.npy"), {"mask": mk}, allow_pickle=True)
        g = Image.fromarray((mk * 1.0).sum(0)).resize((64, 64), Image.NEAREST)
        want.append(torch.tensor(np.asarray(g), dtype=torch.int64).unsqueeze(0))
    ds = ReferDataset(root, "refcocog", "umd", image_transforms=get_transform(64, True), split="train", eval_mode=False, size=64,
                      pseudo_path=d, tokenizer=word_hash_tokenize)
    for i in range(len(ds)):
        np.random.seed(i)
        s, t = ds[i]
        np.random.seed(i)
        s0, t0 = plain[i]
        assert t["pseudo_gt"].dtype == torch.int64 and tuple(t["pseudo_gt"].shape) == (1, 64, 64)
        assert torch.equal(t["pseudo_gt"], want[i])
        assert torch.equal(s["word_ids"], s0["word_ids"]) and "pseudo_gt" not in t0
    assert any(int(w.max()) == 2 for w in want)
