"""The polygon run-length arena without a GPU: runs_numpy (the numpy statement of csrc/polymask.hip) against the unchanged
dataset/cocomask.py, the arena's refusals and host route, the knob's default and the C ABI declarations.  All comparisons exact."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import poly_cases
from tris_amd.dataset import cocomask
from tris_amd.dataset.rle_arena import decode_sum_numpy, segment_ends


def _check(name, xy, h, w):
    from tris_amd.dataset.poly_arena import runs_numpy, upsample
    ends = runs_numpy(upsample(xy), h, w)
    assert ends.dtype == np.int32 and ends[-1] == h * w and (np.diff(ends) >= 0).all() and ends[0] >= 0, name
    mask = decode_sum_numpy(ends, np.array([0, ends.size]), [(0, 1)], h, w)[0]
    assert np.array_equal(mask, poly_cases.oracle_mask(xy, h, w)), name
    counts = cocomask._poly_to_counts(xy, h, w)
    assert poly_cases.merge_zero_runs(np.diff(np.concatenate([[0], ends.astype(np.int64)]))) == counts, name


def test_runs_numpy_equals_cocomask_on_the_random_family():
    for i, (xy, h, w) in enumerate(poly_cases.random_family(3000, seed=20240611)):
        _check(f"random {i}", xy, h, w)


@pytest.mark.parametrize("case", poly_cases.named_cases(), ids=lambda c: c[0])
def test_runs_numpy_equals_cocomask_on_named_cases(case):
    _check(*case)


def test_named_cases_hold_what_their_names_say():
    from tris_amd.dataset.poly_arena import runs_numpy, upsample
    by = {c[0]: c[1:] for c in poly_cases.named_cases()}
    xy, h, w = by["clips to yc == h"]
    ends = runs_numpy(upsample(xy), h, w)
    assert ((ends[:-1] % h == 0) & (ends[:-1] > 0)).any()            # a boundary on the first pixel of the next column
    assert poly_cases.oracle_mask(xy, h, w)[h - 1].any()
    for name in ("all negative", "below the canvas", "right of the canvas", "one vertex", "1x1 missed"):
        assert not poly_cases.oracle_mask(*by[name]).any(), name
    assert poly_cases.oracle_mask(*by["rectangle on all four borders"]).all()
    assert poly_cases.oracle_mask(*by["1x1 covered"]).all()


def test_upsample_is_cocomasks_cast():
    from tris_amd.dataset.poly_arena import upsample
    xy = [0.1, -0.1, -0.3, 7.49, 2.5, 2.7, -3.9, 1e3]
    v = upsample(xy)
    a = np.asarray(xy)
    assert np.array_equal(v[:, 0], (5.0 * a[0::2] + 0.5).astype(np.int64)) and np.array_equal(v[:, 1], (5.0 * a[1::2] + 0.5).astype(np.int64))
    assert v[0].tolist() == [1, 0] and v[1, 0] == -1        # truncation toward zero, not floor


def test_arena_layout_ranges_and_host_route():
    from tris_amd.dataset.poly_arena import COORD_MAX, PolyArena, upsample
    a = PolyArena()
    tri, sq = [1.0, 1.0, 6.0, 1.5, 3.0, 5.0], [2, 2, 5, 2, 5, 5, 2, 5]
    assert a.add_ref([tri, sq], 8, 9, "r0") == (0, 2)
    rle = {"size": [8, 9], "counts": [3, 5, 10, 2]}
    assert a.add_ref([rle], 8, 9, "r1") == (2, 3)                 # the form REFER.getMask reads: a list of RLE dicts
    assert a.add_ref(rle, 8, 9, "r2") == (3, 4)                   # ... and a bare dict
    far = [1.0, 1.0, float(COORD_MAX // 5 + 10), 2.0, 3.0, 6.0]   # upsampled: just beyond the device's bound
    assert a.add_ref([far, tri], 8, 9, "r3") == (4, 6)
    assert a.n_segments == 6 and a.n_host_segments == 3
    verts, off, hw, ranges = a.arrays()
    assert verts.dtype == np.int32 and off.dtype == np.int64 and hw.dtype == np.int32 and ranges.dtype == np.int32
    assert off.tolist() == [0, 3, 7, 7, 7, 7, 10] and (hw == [8, 9]).all() and ranges.tolist() == [[0, 2], [2, 3], [3, 4], [4, 6]]
    assert np.array_equal(verts[:3], upsample(tri)) and np.array_equal(verts[7:], upsample(tri))
    assert np.array_equal(a._host[2], segment_ends(rle, 8, 9)) and np.array_equal(a._host[3], a._host[2])
    # the host route of a polygon decodes to cocomask's mask
    e = a._host[4]
    m = decode_sum_numpy(e, np.array([0, e.size]), [(0, 1)], 8, 9)[0]
    assert np.array_equal(m, poly_cases.oracle_mask(far, 8, 9))


def test_arena_refusals_name_the_offender():
    from tris_amd.dataset.poly_arena import PolyArena
    a = PolyArena()
    sq = [2, 2, 5, 2, 5, 5, 2, 5]
    with pytest.raises(ValueError, match="ref 7.*256 segments"):
        a.add_ref([sq] * 256, 8, 9, "ref 7")
    with pytest.raises(ValueError, match="ref 8.*2\\^24"):
        a.add_ref([sq], 4097, 4096, "ref 8")
    with pytest.raises(ValueError, match="ref 9 segment 1.*7 numbers"):
        a.add_ref([sq, sq[:7]], 8, 9, "ref 9")
    with pytest.raises(ValueError, match="ref 10 segment 0.*0 numbers"):
        a.add_ref([[]], 8, 9, "ref 10")
    with pytest.raises(ValueError, match="ref 11 segment 0.*not finite"):
        a.add_ref([[1.0, float("nan"), 2.0, 2.0]], 8, 9, "ref 11")
    with pytest.raises(ValueError, match="ref 12 segment 0.*beyond"):
        a.add_ref([[1.0, 1e9, 2.0, 2.0]], 8, 9, "ref 12")
    with pytest.raises(ValueError, match="ref 13 segment 0.*past H\\*W"):
        a.add_ref([{"size": [8, 9], "counts": [70, 5]}], 8, 9, "ref 13")
    assert a.n_segments == 0 and a.add_ref([sq], 8, 9) == (0, 1)      # a refused ref leaves nothing behind


def test_knob_defaults_off_and_is_documented(monkeypatch):
    from tris_amd import config
    monkeypatch.delenv("TRIS_POLY_TARGETS", raising=False)
    assert config._Config().poly_targets is False
    monkeypatch.setenv("TRIS_POLY_TARGETS", "1")
    assert config._Config().poly_targets is True
    assert "TRIS_POLY_TARGETS" in config.__doc__
    assert "TRIS_POLY_TARGETS" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_header_declares_the_entry_points_with_citations():
    from tris_amd import _lib
    decls, _ = _lib.parse_header()
    for name in ("tris_poly_count_runs", "tris_poly_emit_runs", "tris_rle_target_nearest_u8", "tris_poly_sort_capacity"):
        assert name in decls, name
    assert len(decls["tris_poly_emit_runs"][1]) == 7 and len(decls["tris_rle_target_nearest_u8"][1]) == 12
    src = open(os.path.join(ROOT, "include", "tris_hip.h")).read()
    sec = src[src.index("csrc/polymask.hip"):src.index("tris_rle_target_nearest_u8(")]
    assert "dataset/refer.py:279-291" in sec and "load_mask" in sec
    assert "polymask" in open(os.path.join(ROOT, "tris_amd", "csrc", "build.sh")).read().split("for f in ")[1].split(";")[0].split()
    assert _lib.query("tris_poly_sort_capacity") >= 1024


def test_ops_refuse_to_run_without_the_gpu():
    from tris_amd import ops
    from tris_amd.dataset.poly_arena import PolyArena
    verts, off, hw = torch.zeros(4, 2, dtype=torch.int32), torch.tensor([0, 3]), torch.tensor([[8, 9]], dtype=torch.int32)
    with pytest.raises(ops.NoGpuError):
        ops.poly_runs(verts, off, hw)
    with pytest.raises(ops.NoGpuError):
        ops.rle_target_nearest((torch.zeros(3, dtype=torch.int32), torch.tensor([0, 2])), 0, 1, 8, 9, 4)
    if not torch.cuda.is_available():
        a = PolyArena()
        a.add_ref([[2, 2, 5, 2, 5, 5]], 8, 9)
        with pytest.raises(ops.NoGpuError):
            a.build()
