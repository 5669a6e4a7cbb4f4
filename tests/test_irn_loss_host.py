"""IRNet's affinity / displacement training losses without a GPU: the torch restatement of the contract (tests/oracle_irn_loss.py)
against what the reference's own code recorded (tests/golden/g16_irn_loss.npz, tools/gen_golden_irn_loss.py), the tie rule of the
path maximum, the argument checks of tris_amd.irn_loss, the no-CPU-fallback rule and the C ABI of csrc/irnloss.hip."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

import oracle_irn_loss as O

ENTRY_POINTS = ["tris_irn_loss_workspace_bytes", "tris_irn_loss_fwd_f32", "tris_irn_loss_bwd_f32"]


@pytest.fixture(scope="module")
def g16(golden):
    return golden("g16_irn_loss.npz")


def test_golden_is_what_the_tests_rely_on(g16):
    """the three shapes of the helper, every pair class present in each, the plateau case, a small file"""
    for i, shape in enumerate(O.GOLDEN_SHAPES):
        assert tuple(g16[f"s{i}_shape"]) == shape
        assert (g16[f"s{i}_counts"] > 0).all()
        B, h, w, _ = shape
        assert g16[f"s{i}_d_edge"].shape == (B, 1, h, w) and g16[f"s{i}_d_dp"].shape == (B, 2, h, w)
        assert g16[f"s{i}_d_edge"].dtype == np.float32 and g16[f"s{i}_losses"].dtype == np.float32
    assert tuple(g16["s1_counts"]) == (210262, 57306, 48676)
    assert tuple(g16["plateau_shape"]) == O.PLATEAU_SHAPE
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g16_irn_loss.npz")) < 200_000


def test_inputs_have_no_near_ties():
    """what the inputs are built for: distinct logits per image, no displacement difference at a kink of |.|"""
    for B, h, w, radius in O.GOLDEN_SHAPES:
        edge, dp, label = O.inputs(B, h, w)
        for b in range(B):
            v = np.sort(edge[b].reshape(-1).astype(np.float64))
            assert np.diff(v).min() > 0.5 * 12.0 / (h * w)
        frac = np.modf(np.abs(dp.astype(np.float64)) * 8)[0]
        assert np.all(frac == 0.5)                                  # odd multiples of 1/16: differences are multiples of 1/8 ...
        assert set(np.unique(label)) == {0, 1, 255}


@pytest.mark.parametrize("i", range(len(O.GOLDEN_SHAPES)))
def test_restatement_fp32_equals_the_reference(g16, i):
    """both sides are one fp32 CPU computation of the same formulas: losses <= 1e-6 relative, gradients <= 1e-6 relative L2,
    counts equal"""
    B, h, w, radius = O.GOLDEN_SHAPES[i]
    edge, dp, label = O.inputs(B, h, w)
    l, n, ge, gd = O.restated(edge, dp, label, radius, torch.float32)
    assert np.array_equal(n, g16[f"s{i}_counts"])
    rel = np.abs(l.astype(np.float64) - g16[f"s{i}_losses"]) / np.abs(g16[f"s{i}_losses"])
    e_edge, e_dp = O.rel_l2(ge, g16[f"s{i}_d_edge"]), O.rel_l2(gd, g16[f"s{i}_d_dp"])
    print(f"shape {(B, h, w, radius)}: losses {rel}, d_edge {e_edge:.3e}, d_dp {e_dp:.3e}")
    assert (rel <= 1e-6).all(), rel
    assert e_edge <= 1e-6 and e_dp <= 1e-6, (e_edge, e_dp)


def test_tie_rule_on_the_plateau_case(g16):
    """logits from {-0.5, 0, 0.5}: every path has equal maxima, and the gradient goes to the first of them in the reference's
    path order (indexing.py:48); the gradient of (l0 + l1) / 2 against the reference's max_pool2d backward"""
    B, h, w, radius = O.PLATEAU_SHAPE
    edge, dp, label = O.plateau_inputs()
    assert set(np.unique(edge)) == {-0.5, 0.0, 0.5} and not dp.any()
    l, n, ge, _ = O.restated(edge, dp, label, radius, torch.float32, weights=(0.5, 0.5, 0.0, 0.0))
    assert np.array_equal(n, g16["plateau_counts"])
    assert np.abs(l - g16["plateau_losses"]).max() <= 1e-6 * np.abs(g16["plateau_losses"]).max()
    e = O.rel_l2(ge, g16["plateau_d_edge"])
    print(f"plateau d_edge {e:.3e}")
    assert e <= 1e-6, e
    # the rule matters here: sending the gradient to the first maximum in SCAN order instead gives another map
    from tris_amd import irn
    scan = [(d, list(c)) for d, c in irn.search_paths(radius)]
    ref = O.reference_paths(radius)
    assert [d for d, _ in scan] == [d for d, _ in ref] and all(set(a) == set(b) for (_, a), (_, b) in zip(scan, ref))
    _, _, g_scan, _ = O.restated(edge, dp, label, radius, torch.float32, weights=(0.5, 0.5, 0.0, 0.0), scan_order=True)
    assert O.rel_l2(g_scan, g16["plateau_d_edge"]) > 0.1


def test_reference_order_is_l1_then_scan():
    """larger |cy| + |cx| first, then smaller cy, then smaller cx: what the kernel's comparison implements on the scan-ordered
    table"""
    for radius in (5, 10):
        for (dy, dx), cells in O.reference_paths(radius):
            key = [(-(abs(cy) + abs(cx)), cy, cx) for cy, cx in cells]
            assert key == sorted(key)
            assert cells[0] == (dy, dx) and cells[-1] == (0, 0)


def test_module_has_no_cpu_fallback():
    from tris_amd import irn, irn_loss, ops
    with pytest.raises(ops.NoGpuError):
        irn_loss.reduce_label(torch.zeros(50, 61, dtype=torch.uint8))
    with pytest.raises(ops.NoGpuError):
        irn_loss.reduce_label(torch.zeros(2, 50, 61, dtype=torch.uint8))
    e, d, l = torch.zeros(2, 1, 21, 23), torch.zeros(2, 2, 21, 23), torch.zeros(2, 21, 23, dtype=torch.uint8)
    with pytest.raises(ops.NoGpuError):
        irn_loss.affinity_displacement_losses(e, d, l)
    paths = irn.search_paths(10)
    tables = [torch.zeros(len(paths), 2, dtype=torch.int32), torch.zeros(len(paths) + 1, dtype=torch.int32),
              torch.zeros(sum(len(c) for _, c in paths), 2, dtype=torch.int32)]
    with pytest.raises(ops.NoGpuError):
        ops.irn_aff_losses(e, d, l, *tables)
    assert float(irn_loss.total_loss(torch.tensor([1.0, 2.0, 3.0, 5.0]))) == 5.5


def test_value_errors_name_the_shapes():
    from tris_amd import irn_loss
    e, d, l = torch.zeros(2, 1, 21, 23), torch.zeros(2, 2, 21, 23), torch.zeros(2, 21, 23, dtype=torch.uint8)
    bad = [((e, d[:, :1], l), "[2, 1, 21, 23]|(2, 1, 21, 23)"),                    # dp_out with one channel
           ((e, d, l[:, :20]), "(2, 20, 23)"),                                    # a label of another size
           ((e[:1], d, l), "(1, 1, 21, 23)"),                                     # another batch
           ((e[:, 0], d, l), "(2, 21, 23)"),                                      # edge_out without its channel dimension
           ((e.double(), d, l), "float64"), ((e, d, l.long()), "int64"),           # dtypes
           ((e[..., :9, :], d[..., :9, :], l[:, :9]), "(2, 1, 9, 23)"),            # h < r + 1
           ((e[..., :18], d[..., :18], l[..., :18]), "(2, 1, 21, 18)")]            # w < 2 r + 1
    for args, names in bad:
        with pytest.raises(ValueError) as err:
            irn_loss.affinity_displacement_losses(*args)
        assert any(n in str(err.value) for n in names.split("|")), (names, str(err.value))
    irn_loss_small = (e[..., :10, :19], d[..., :10, :19], l[:, :10, :19])          # the smallest map radius 10 takes: not a ValueError
    from tris_amd import ops
    with pytest.raises(ops.NoGpuError):
        irn_loss.affinity_displacement_losses(*irn_loss_small)
    with pytest.raises(ValueError):
        irn_loss.affinity_displacement_losses(*irn_loss_small, radius=17)
    for x in (torch.zeros(5, dtype=torch.uint8), torch.zeros(8, 8), np.zeros((8, 8), np.uint8)):
        with pytest.raises(ValueError):
            irn_loss.reduce_label(x)


def test_header_declares_and_library_exports_the_entry_points():
    from tris_amd import _lib
    decls, _ = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIBPATH)
    for name in ENTRY_POINTS:
        assert name in decls, f"{name} is not declared in include/tris_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    # 5 fp64 sums + 3 integer counts per 16 x 16 tile of source pixels: (128 - 9) x (128 - 18) per image -> 8 x 7 tiles
    assert _lib.query("tris_irn_loss_workspace_bytes", 32, 128, 128, 10) == 32 * 8 * 7 * 64
    assert _lib.query("tris_irn_loss_workspace_bytes", 1, 9, 19, 10) == 0           # a map without a source pixel
    src = open(os.path.join(ROOT, "include", "tris_hip.h")).read()
    part = src[src.index("csrc/irnloss.hip"):]
    assert part.count("irn.py:") >= 3 and part.count("train_irn.py:") >= 2 and part.count("dataloader.py:") >= 2
    assert "irnloss" in open(os.path.join(ROOT, "tris_amd", "csrc", "build.sh")).read()
