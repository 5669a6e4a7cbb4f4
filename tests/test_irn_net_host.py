"""The IRNet edge / displacement network without a GPU: the torch restatement (tests/oracle_irn.py) against what the reference's own
EdgeDisplacement recorded (tests/golden/g15_irn_net.npz, tools/gen_golden_irn.py), the product module's names and shapes against
the recorded key list, state-dict loading with and without the reference's aliases, the normalisation table, the name -> image
file rule, the command line and the no-CPU-fallback rule."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import oracle_irn as O

NEW_ENTRY_POINTS = ["tris_irn_stem_f32", "tris_maxpool3s2_f32", "tris_subsample2_f32", "tris_gn_workspace_bytes", "tris_gn_stats_f32",
                    "tris_gn_apply_up_f32", "tris_irn_head_f32", "tris_irn_net_finish_f32", "tris_get_autotune"]


@pytest.fixture(scope="module")
def g15(golden):
    return golden("g15_irn_net.npz")


@pytest.fixture(scope="module")
def keys():
    with open(os.path.join(GOLDEN, "g15_irn_keys.json")) as f:
        return [(k, tuple(s)) for k, s in json.load(f)]


@pytest.fixture(scope="module")
def filled(g15):
    """the recording's seeded weights as a canonical state dict"""
    return O.filled_state_dict(int(g15["seed"]), float(g15["gain"]))


def test_golden_is_what_the_tests_rely_on(g15):
    """every crop bites somewhere: a map with both sides odd (the x2 / x4 upsampled maps overhang), a stride-8 map with an odd side, a
    grey image, and a size with H != W, both multiples of 16, where no crop bites"""
    assert int(g15["n_images"]) == len(O.IMAGES) == 3
    sizes = [(H, W) for H, W, _ in O.IMAGES]
    f4 = [((H - 1) // 4 + 1, (W - 1) // 4 + 1) for H, W in sizes]
    f8 = [((h - 1) // 2 + 1, (w - 1) // 2 + 1) for h, w in f4]
    assert any(h % 2 and w % 2 for h, w in f4) and any(h % 2 or w % 2 for h, w in f8)
    assert any(H != W and H % 16 == 0 and W % 16 == 0 for H, W in sizes) and any(g for _, _, g in O.IMAGES)
    for i, (h, w) in enumerate(f4):
        assert g15[f"i{i}_edge_out"].shape == (2, 1, h, w) and g15[f"i{i}_dp_out"].shape == (2, 2, h, w)
        assert g15[f"i{i}_edge"].shape == (1, h, w) and g15[f"i{i}_dp"].shape == (2, h, w)
        assert g15[f"i{i}_edge"].max() - g15[f"i{i}_edge"].min() > 0.05 and np.abs(g15[f"i{i}_dp"]).mean() > 0.05
    assert os.path.getsize(os.path.join(GOLDEN, "g15_irn_net.npz")) < 900_000


def test_restatement_against_the_recording(g15, filled):
    """fp32 restatement against the reference's fp32 run, both on the CPU with the same torch operators: the measured distance is 0
    on the build machine (same operators, same order).  The bound leaves room for a torch build whose convolution picks another
    summation order: 1e-5 of the tensor's largest magnitude, the class DESIGN.md section 8 records for fp32 outputs that do not pass
    through tiny-sample statistics."""
    for i, img in enumerate(O.images()):
        out = O.forward(filled, O.batch_of(img))
        for name in ("edge_out", "dp_out", "edge", "dp"):
            ref = g15[f"i{i}_{name}"]
            d = np.abs(out[name].numpy() - ref).max() / np.abs(ref).max()
            print(f"image {i} {name}: {d:.3e}")
            assert d < 1e-5, (i, name, d)
        if i == int(g15["tap_image"]):
            for k in range(5):
                ref = g15[f"tap{k + 1}"]
                assert tuple(out["taps"][k].shape) == tuple(g15[f"tap{k + 1}_shape"])
                d = np.abs(O.tap_sample(out["taps"][k]).numpy() - ref).max() / np.abs(ref).max()
                print(f"image {i} x{k + 1}: {d:.3e}")
                assert d < 1e-5, (k, d)


def test_keys_and_shapes(keys):
    """the module's canonical names and shapes are among the recorded ones, and every recorded name is an alias of one of them"""
    from tris_amd.irn_net import EdgeDisplacement, canonical_name
    own = {k: tuple(v.shape) for k, v in EdgeDisplacement().state_dict().items()}
    rec = dict(keys)
    assert len(rec) == len(keys) > len(own) > 300
    for k, s in own.items():
        assert rec.get(k) == s, k
    for k, s in keys:
        assert own.get(canonical_name(k)) == s, (k, canonical_name(k))
    assert {canonical_name(k) for k, _ in keys} == set(own)
    assert canonical_name("fc_dp7.4.running_mean") == canonical_name("dp_layers.6.4.running_mean") == "mean_shift.running_mean"
    assert canonical_name("backbone.1.0.0.conv1.weight") == "resnet50.layer1.0.conv1.weight"
    assert canonical_name("stage1.1.running_var") == "resnet50.bn1.running_var"
    assert canonical_name("edge_layers.5.bias") == "fc_edge6.bias"


def _with_aliases(filled, keys):
    from tris_amd.irn_net import canonical_name
    return {k: filled[canonical_name(k)].clone() for k, _ in keys}


def test_load_state_dict(keys, filled):
    from tris_amd.irn_net import EdgeDisplacement
    full = _with_aliases(filled, keys)
    assert len(full) > len(filled)
    for sd in (full, dict(filled)):
        m = EdgeDisplacement()
        m.load_state_dict(sd)
        got = m.state_dict()
        assert all(torch.equal(got[k], filled[k]) for k in filled)
    bad = dict(full)
    bad["backbone.2.0.1.conv2.weight"] = bad["backbone.2.0.1.conv2.weight"] + 1e-3
    with pytest.raises(ValueError, match="disagree"):
        EdgeDisplacement().load_state_dict(bad)
    bad = dict(full)
    bad["dp_layers.6.4.running_mean"] = bad["dp_layers.6.4.running_mean"] * 2
    with pytest.raises(ValueError, match="disagree"):
        EdgeDisplacement().load_state_dict(bad)
    short = {k: v for k, v in filled.items() if k != "fc_dp3.1.bias"}
    with pytest.raises(KeyError, match="fc_dp3.1.bias"):
        EdgeDisplacement().load_state_dict(short)
    extra = dict(filled)
    extra["resnet50.fc.weight"] = torch.zeros(1000, 2048)
    with pytest.raises(KeyError, match="unexpected"):
        EdgeDisplacement().load_state_dict(extra)
    EdgeDisplacement().load_state_dict(extra, strict=False)
    # a checkpoint of the training model carries its path-index buffers: passed over, as the reference's strict=False load does
    trained = dict(full, path_indices0=torch.zeros(3, 4, 5, dtype=torch.int64), path_indices11=torch.zeros(2, dtype=torch.int64),
                   disp_target=torch.zeros(1, 2, 6, 1))
    EdgeDisplacement().load_state_dict(trained)


def test_normalisation_table_is_bit_identical(g15):
    from tris_amd.irn_net import normalize_table
    lut = normalize_table().numpy()
    img = O.images()[int(g15["tap_image"])]
    got = np.stack([lut[c][img[..., c]] for c in range(3)])
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), g15["x_norm"].view(np.uint32))
    assert np.array_equal(O.normalize(img).numpy().view(np.uint32), g15["x_norm"].view(np.uint32))


def test_image_names():
    from tris_amd.make_ins_seg import image_file, image_id
    assert image_file("12_581857", "/data/coco/train2014") == "/data/coco/train2014/COCO_train2014_000000581857.jpg"
    assert image_file("refcocog_3_42", "imgs") == os.path.join("imgs", "COCO_train2014_000000000042.jpg")
    assert image_file("7_10243", "/data/referit/images") == "/data/referit/images/10243.jpg"
    assert image_id("5_99") == image_id("6_99") != image_id("5_98")


def test_parser_and_sources():
    from tris_amd.make_ins_seg import check_sources, get_parser, main
    base = ["--cam_out_dir", "D", "--ins_seg_out_dir", "O", "--train_list", "n.json"]
    a = get_parser().parse_args(base + ["--irn_weights_name", "W.pth", "--voc12_root", "IMG"])
    assert (a.irn_weights_name, a.voc12_root, a.irn_out_dir) == ("W.pth", "IMG", None)
    check_sources(a)
    a = get_parser().parse_args(base + ["--irn_out_dir", "E"])
    assert (a.irn_out_dir, a.irn_weights_name) == ("E", None)
    check_sources(a)
    with pytest.raises(ValueError, match="exactly one"):
        check_sources(get_parser().parse_args(base))
    with pytest.raises(ValueError, match="exactly one"):
        check_sources(get_parser().parse_args(base + ["--irn_out_dir", "E", "--irn_weights_name", "W.pth", "--voc12_root", "IMG"]))
    with pytest.raises(ValueError, match="voc12_root"):
        check_sources(get_parser().parse_args(base + ["--irn_weights_name", "W.pth"]))
    with pytest.raises(SystemExit):
        main(base)


def test_grey_image_becomes_three_equal_channels(tmp_path):
    from PIL import Image
    from tris_amd.make_ins_seg import load_image
    g = O.images()[1]
    assert g.ndim == 2
    Image.fromarray(g).save(tmp_path / "g.png")
    a = load_image(str(tmp_path / "g.png"))
    assert a.shape == g.shape + (3,) and all(np.array_equal(a[..., c], g) for c in range(3))
    c = O.images()[0]
    Image.fromarray(c).save(tmp_path / "c.png")
    assert np.array_equal(load_image(str(tmp_path / "c.png")), c)


def test_c_abi_exports_the_new_entry_points():
    from tris_amd import _lib
    lib = _lib.load()
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.DECLS and hasattr(lib, name), name
    assert _lib.query("tris_gn_workspace_bytes", 2, 17 * 25, 4) > 0
    assert lib.tris_get_autotune() in (0, 1)


def test_forward_without_a_gpu_raises():
    """no CPU path: without a GPU -- and, on a machine that has one, for a module left on the CPU -- forward raises NoGpuError"""
    from tris_amd import ops
    from tris_amd.irn_net import EdgeDisplacement
    m = EdgeDisplacement()
    with pytest.raises(ops.NoGpuError):
        m(O.images()[0])
    with pytest.raises(ops.NoGpuError):
        m(torch.from_numpy(O.images()[0]))
