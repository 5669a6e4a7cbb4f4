"""ops.cam_paint (csrc/overlay.hip) against the fp64 restatement tests/oracle_overlay.py: exact colour indices away from a
quantisation step, either neighbour within 2^-10 of one (at most 2 % of a case, asserted), norm and range at 2^-19, arg-max exact."""
import numpy as np
import pytest
import torch

import oracle_overlay as OV

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(key, maps, H, W, image, lut=None, mode=OV.MINMAX):
    """one restatement per case, shared by the tests that need it"""
    if key not in _REF:
        _REF[key] = OV.paint(maps, H, W, image, lut, mode)
    return _REF[key]


def _np(out):
    return tuple(None if t is None else t.cpu().numpy() for t in out)


@pytest.mark.parametrize("want_norm", [False, True])
@pytest.mark.parametrize("with_image", [False, True])
@pytest.mark.parametrize("shape", OV.SHAPES, ids=lambda s: "{}x{}-{}x{}-K{}".format(*s))
def test_cam_paint_against_the_oracle(shape, with_image, want_norm):
    from tris_amd import ops
    Sh, Sw, H, W, K = shape
    maps = OV.case_maps(Sh, Sw, K)
    image = OV.case_image(H, W) if with_image else None
    got = _np(ops.cam_paint(torch.from_numpy(maps).cuda(), None if image is None else torch.from_numpy(image).cuda(),
                            want_norm=want_norm, size=(H, W)))
    ref = _ref((shape, with_image), maps, H, W, image)
    print(shape, "near-step fraction", OV.near_fraction(ref), "pixels differing from the oracle's first choice",
          int((got[0] != ref["heat"]).any(-1).sum()))
    OV.check_all(got, ref, norm=want_norm)


@pytest.mark.parametrize("name", ["all_negative", "constant", "two_maxima", "signed"])
def test_special_maps(name):
    from tris_amd import ops
    maps, (H, W), mode = OV.special_cases()[name]
    image = OV.case_image(H, W, 3)
    got = _np(ops.cam_paint(torch.from_numpy(maps).cuda(), torch.from_numpy(image).cuda(), want_norm=True))
    ref = _ref(name, maps, H, W, image)
    OV.check_all(got, ref)
    if name in ("all_negative", "constant"):                                    # lo = hi, n = 0, lut[0] everywhere
        assert (got[2][:, 0] == got[2][:, 1]).all() and not got[1].any() and (got[3] == 0).all()
        assert np.array_equal(got[0], np.broadcast_to(OV.blend(OV.jet_table()[0], image), got[0].shape))
    if name == "two_maxima":
        assert got[3].tolist() == [300]                                         # the FIRST of the two equal maxima (np.argmax)


def test_unit_mode_at_identity_size_is_exact():
    from tris_amd import ops
    maps, (H, W), mode = OV.special_cases()["unit"]
    heat, norm, rng, arg = _np(ops.cam_paint(torch.from_numpy(maps).cuda(), mode="unit", want_norm=True))
    lut = OV.jet_table()
    assert np.array_equal(norm, maps)                                           # identity size: the samples are the map's own values
    assert np.array_equal(heat, lut[np.uint8(maps * np.float32(255))])          # visualize_cam's np.uint8(x * 255), demo.py:29
    assert np.array_equal(rng, np.stack([maps.reshape(2, -1).min(1), maps.reshape(2, -1).max(1)], 1))
    assert np.array_equal(arg, maps.reshape(2, -1).argmax(1))
    OV.check_all((heat, norm, rng, arg), _ref("unit", maps, H, W, None, mode=OV.UNIT))
    # values above 1 saturate at the last entry, negative ones at the first
    wide = torch.tensor([[[-0.5, 0.0, 0.999, 1.0], [1.5, 7.0, 0.5, 0.25]]], device="cuda")
    h = ops.cam_paint(wide, mode="unit")[0].cpu().numpy()
    assert np.array_equal(h[0], lut[[[0, 0, 254, 255], [255, 255, 127, 63]]])


def test_custom_lut():
    from tris_amd import ops
    Sh, Sw, H, W, K = OV.SHAPES[3]
    maps, image = OV.case_maps(Sh, Sw, K), OV.case_image(H, W)
    lut = np.random.RandomState(11).randint(0, 256, (256, 3)).astype(np.uint8)
    lut[1:] |= 1                                                                # (no entry equals lut[0] by accident)
    lut[0] = 0
    got = _np(ops.cam_paint(torch.from_numpy(maps).cuda(), torch.from_numpy(image).cuda(), torch.from_numpy(lut).cuda(), want_norm=True))
    OV.check_all(got, _ref("custom_lut", maps, H, W, image, lut))
    assert (got[0] != _ref((OV.SHAPES[3], True), maps, H, W, image)["heat"]).any()


def test_a_sentence_does_not_depend_on_its_company():
    from tris_amd import ops
    for Sh, Sw, H, W in ((10, 10, 37, 50), (20, 20, 333, 479), (2, 2, 7, 5)):   # H * W odd too: sentence boundaries inside a group
        maps = torch.from_numpy(OV.case_maps(Sh, Sw, 3, seed=4)).cuda()
        image = torch.from_numpy(OV.case_image(H, W, 4)).cuda()
        all3 = ops.cam_paint(maps, image, want_norm=True)
        for k in range(3):
            one = ops.cam_paint(maps[k:k + 1].contiguous(), image, want_norm=True)
            for a, b in zip(one, all3):
                assert torch.equal(a[0], b[k]), (H, W, k)


def test_no_sentence_and_refused_arguments():
    from tris_amd import ops
    heat, norm, rng, arg = ops.cam_paint(torch.zeros(0, 4, 4, device="cuda"), size=(6, 5), want_norm=True)
    assert heat.shape == (0, 6, 5, 3) and norm.shape == (0, 6, 5) and rng.shape == (0, 2) and arg.shape == (0,)
    maps = torch.zeros(2, 8, 8, device="cuda")
    image = torch.zeros(6, 5, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="maps must be contiguous"):
        ops.cam_paint(maps.transpose(1, 2), image)
    with pytest.raises(ValueError, match="image_u8 must be contiguous"):
        ops.cam_paint(maps, torch.zeros(6, 3, 5, dtype=torch.uint8, device="cuda").transpose(1, 2))
    with pytest.raises(TypeError, match="maps must be torch.float32"):
        ops.cam_paint(maps.double(), image)
    with pytest.raises(TypeError, match="image_u8 must be torch.uint8"):
        ops.cam_paint(maps, image.float())
    with pytest.raises(TypeError, match="lut must be torch.uint8"):
        ops.cam_paint(maps, image, torch.zeros(256, 3, device="cuda"))
    with pytest.raises(ValueError, match="lut is"):
        ops.cam_paint(maps, image, torch.zeros(255, 3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="mode"):
        ops.cam_paint(maps, image, mode="max")
    with pytest.raises(ops.NoGpuError):
        ops.cam_paint(maps.cpu(), image)


def test_the_call_can_be_captured():
    """no host synchronisation and no allocation inside tris_cam_paint_f32: a captured replay repaints new maps"""
    from tris_amd import _lib, ops
    Sh, Sw, H, W, K = OV.SHAPES[3]
    maps = torch.from_numpy(OV.case_maps(Sh, Sw, K)).cuda()
    image = torch.from_numpy(OV.case_image(H, W)).cuda()
    lut = torch.from_numpy(OV.jet_table()).cuda()
    heat = torch.zeros(K, H, W, 3, dtype=torch.uint8, device="cuda")
    rng, arg = torch.zeros(K, 2, device="cuda"), torch.zeros(K, dtype=torch.int64, device="cuda")
    ws = torch.zeros(_lib.query("tris_cam_paint_workspace_bytes", K, H, W) // 4, device="cuda")
    want = ops.cam_paint(maps, image)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.call("tris_cam_paint_f32", maps.data_ptr(), K, Sh, Sw, image.data_ptr(), H, W, lut.data_ptr(), 0, heat.data_ptr(), None,
                  rng.data_ptr(), arg.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    g.replay()
    assert torch.equal(heat, want[0]) and torch.equal(rng, want[2]) and torch.equal(arg, want[3])
