"""Records tests/golden/g13_stage2_* from the REAL reference Stage-2 code (model/model_stage2.py, dataset/ReferDataset.py and the
signatures of train_stage2.py), imported through oracle/ref_shim.py.  Build-machine tool: the reference tree is not on the GPU
machines, and nothing that runs there reads it.

    python tools/gen_golden_stage2.py

  g13_stage2_keys.json   state-dict keys and shapes, parameter-group membership (trainable_parameters, :93-101), the argument
                         lists of TRIS / ConvBNRelu / criterion / TRIS.forward and train_stage2.train_one_epoch / main
  g13_stage2_model.npz   at 64 px, B = 2, T = 20, seed_fill weights with every PReLU slope reset to 0.25 +- 0.05: the four
                         train outputs, the eval output, the four losses against a {0, 1, 2} target, BatchNorm running statistics
                         after the train forward, and the first 16 gradient elements of trunk / text / PixelAttention / decoder
                         probes and of every PReLU slope.  fp32: the reference's LayerNorm casts to fp32 (CLIP/clip/model.py:357),
                         so it does not run in fp64
  g13_stage2_pseudo.npz  ReferDataset(pseudo_path) training items on make_mini_refer with make_pseudo_masks
"""
import ast
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")

SIZE, B, T, W_SEED, B_SEED, T_SEED, SLOPE_SEED = 64, 2, 20, 1234, 7, 9, 5
PROBES = ["backbone.visual.layer1.0.conv1.weight", "backbone.visual.layer4.2.conv3.weight",
          "backbone.transformer.resblocks.11.mlp.c_fc.weight", "backbone.token_embedding.weight", "attention3.Wq.weight",
          "attention2.Wk.weight", "reduced_c4.conv.weight", "output2.conv.weight", "reduced_c1.bn.weight", "final_seg1.1.weight",
          "final_seg4.0.bn.bias"]
BN_KEYS = ["backbone.visual.bn1", "reduced_c1.bn", "reduced_c4.bn", "output1.bn", "final_seg4.0.bn"]
PSEUDO = dict(n_images=6, ds_seed=1, mask_seed=0, size=32, rng_seed=3)


def arg_names(path, qualname):
    """argument names of a function / method in a reference source file (read with ast: importing train_stage2.py would pull
    packages this stack does not have)"""
    tree = ast.parse(open(path).read())
    parts = qualname.split(".")
    body = tree.body
    for i, name in enumerate(parts):
        node = next(n for n in body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name == name)
        body = node.body
    a = node.args
    return [x.arg for x in a.posonlyargs + a.args] + ([a.vararg.arg] if a.vararg else []) + [x.arg for x in a.kwonlyargs]


def reference_model():
    from oracle import ref_shim
    ref_shim.install()
    from model.model_stage2 import TRIS, criterion   # noqa: E402  (the reference's)
    args = ref_shim.make_args(["--size", str(SIZE)])
    return TRIS(args), criterion


def main_keys():
    ref = ref_shim_model = reference_model()[0]
    bb, hd = [], []
    for k, _ in ref_shim_model.named_parameters():
        (bb if k.startswith("backbone") and "positional_embedding" not in k else hd).append(k)
    rm = "/root/reference/model/model_stage2.py"
    rt = "/root/reference/train_stage2.py"
    out = {"keys": [[k, list(v.shape)] for k, v in ref.state_dict().items()],
           "backbone_group": bb, "head_group": hd,
           "signatures": {"model_stage2.TRIS.__init__": arg_names(rm, "TRIS.__init__"),
                          "model_stage2.TRIS.forward": arg_names(rm, "TRIS.forward"),
                          "model_stage2.ConvBNRelu.__init__": arg_names(rm, "ConvBNRelu.__init__"),
                          "model_stage2.criterion": arg_names(rm, "criterion"),
                          "train_stage2.train_one_epoch": arg_names(rt, "train_one_epoch"),
                          "train_stage2.main": arg_names(rt, "main")}}
    # the reference's own grouping function agrees with the predicate above
    g_bb, g_hd = ref.trainable_parameters()
    named = dict(ref.named_parameters())
    assert [id(p) for p in g_bb] == [id(named[k]) for k in bb] and [id(p) for p in g_hd] == [id(named[k]) for k in hd]
    with open(os.path.join(OUT, "g13_stage2_keys.json"), "w") as f:
        json.dump(out, f)
    print("g13 keys:", len(out["keys"]), len(bb), len(hd))


def main_model():
    from tris_amd.utils.synth import seed_fill, synthetic_batch
    ref, criterion = reference_model()
    sd = ref.state_dict()
    seed_fill(sd, W_SEED)
    g = torch.Generator().manual_seed(SLOPE_SEED)
    for k in sorted(k for k in sd if k.endswith(".relu.weight")):
        sd[k].copy_(0.25 + 0.05 * (2 * torch.rand(sd[k].shape, generator=g) - 1))
    ref.load_state_dict(sd)
    sd = {k: v.clone() for k, v in sd.items()}     # (state_dict() aliases the buffers the train forward updates)
    b = synthetic_batch(B, SIZE, T, 0, seed=B_SEED)
    tgt = torch.randint(0, 3, (B, 1, SIZE, SIZE), generator=torch.Generator().manual_seed(T_SEED))
    img = b["img"]
    ref.train()
    outs = ref(img, b["word_ids"])
    ls = [criterion(o, tgt) for o in outs]
    loss = ls[0] + ls[1] + ls[2] + ls[3] + torch.tensor(0)
    loss.backward()
    named = dict(ref.named_parameters())
    rec = {"img": img.numpy(), "word_ids": b["word_ids"].numpy(), "target": tgt.numpy(),
           "outs": torch.stack([o.detach() for o in outs]).numpy(), "losses": torch.stack([loss.detach()] + [l.detach() for l in ls]).numpy()}
    for k in PROBES:
        rec["grad_head." + k] = named[k].grad.reshape(-1)[:16].numpy()
        rec["grad_norm." + k] = np.array(float(named[k].grad.norm()))
    for k in sorted(k for k in named if k.endswith(".relu.weight")):
        rec["grad_slope." + k] = named[k].grad.numpy()
    after = ref.state_dict()
    for k in BN_KEYS:
        rec["running_mean." + k] = after[k + ".running_mean"].clone().numpy()
        rec["running_var." + k] = after[k + ".running_var"].clone().numpy()
    ref.load_state_dict(sd)
    ref.eval()
    with torch.no_grad():
        rec["eval"] = ref(img, b["word_ids"]).numpy()
    np.savez_compressed(os.path.join(OUT, "g13_stage2_model.npz"), **rec)
    print("g13 model:", os.path.getsize(os.path.join(OUT, "g13_stage2_model.npz")), rec["losses"])


def main_pseudo():
    from oracle import ref_shim
    RefDS, ref_tf = ref_shim.install_dataset()
    import CLIP.clip as ref_clip
    from tris_amd.utils.synth import make_mini_refer, make_pseudo_masks, word_hash_tokenize
    ref_clip.tokenize = word_hash_tokenize
    root = make_mini_refer(tempfile.mkdtemp(), n_images=PSEUDO["n_images"], seed=PSEUDO["ds_seed"])
    pdir = make_pseudo_masks(root, os.path.join(root, "pseudo"), seed=PSEUDO["mask_seed"])
    ds = RefDS(refer_data_root=root, dataset="refcocog", splitBy="umd", size=PSEUDO["size"], max_tokens=20,
               image_transforms=ref_tf(PSEUDO["size"], train=True), split="train", eval_mode=False, pseudo_path=pdir)
    np.random.seed(PSEUDO["rng_seed"])
    items = [ds[i] for i in range(len(ds))]
    rec = {"params": np.array([PSEUDO[k] for k in ("n_images", "ds_seed", "mask_seed", "size", "rng_seed")]),
           "pseudo_gt": torch.stack([t["pseudo_gt"] for _, t in items]).numpy(),
           "word_ids": torch.stack([s["word_ids"] for s, _ in items]).numpy(),
           "img": torch.stack([s["img"] for s, _ in items]).numpy()}
    assert rec["pseudo_gt"].dtype == np.int64 and rec["pseudo_gt"].max() == 2
    np.savez_compressed(os.path.join(OUT, "g13_stage2_pseudo.npz"), **rec)
    print("g13 pseudo:", rec["pseudo_gt"].shape, os.path.getsize(os.path.join(OUT, "g13_stage2_pseudo.npz")))


if __name__ == "__main__":
    os.environ.setdefault("TRIS_RANDOM_INIT", "1")
    main_keys()
    main_model()
    main_pseudo()
