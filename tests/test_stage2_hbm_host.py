"""Stage-2 pseudo masks in the HBM loader, on the host (no GPU): the new op refuses CPU tensors and over-long stacks before any
launch, the header declares its entry point and the built library exports it, and the loader builder keeps its signature."""
import inspect
import re

import pytest
import torch


def test_mask_sum_nearest_u8_refuses_cpu_tensors():
    from tris_amd import ops
    with pytest.raises(ops.NoGpuError):
        ops.mask_sum_nearest_u8(torch.zeros(2, 5, 7, dtype=torch.uint8), 4, 4)
    with pytest.raises(ops.NoGpuError):
        ops.mask_sum_nearest_u8(torch.zeros(0, 5, 7, dtype=torch.uint8), 4, 4)


def test_mask_sum_nearest_u8_refuses_more_than_255_masks_without_a_device():
    from tris_amd import ops
    with pytest.raises(ValueError, match="256"):
        ops.mask_sum_nearest_u8(torch.zeros(256, 3, 5, dtype=torch.uint8), 4, 4)
    with pytest.raises(ValueError):
        ops.mask_sum_nearest_u8(torch.zeros(5, 7, dtype=torch.uint8), 4, 4)      # not a [K,h,w] stack


def test_header_declares_and_library_exports_the_entry_point():
    from tris_amd import _lib
    assert "tris_mask_sum_nearest_u8" in _lib.DECLS
    src = open(_lib.HEADER).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int tris_mask_sum_nearest_u8\(", src, re.S)
    assert m and "ReferDataset.py:178-186" in m.group(1)       # the reference citation the other entries carry
    assert hasattr(_lib.load(), "tris_mask_sum_nearest_u8")


def test_build_loader_and_cache_signatures():
    """existing callers are untouched: the new arguments are optional and last"""
    from tris_amd.dataset.hbm import HbmReferCache
    from tris_amd.train_stage1 import build_loader
    p = list(inspect.signature(build_loader).parameters.values())
    assert [q.name for q in p] == ["args", "dataset", "batch_size", "shuffle", "distributed", "images_from"] and p[-1].default is None
    c = list(inspect.signature(HbmReferCache.__init__).parameters.values())
    assert [q.name for q in c] == ["self", "dataset", "size", "device", "images_from"] and c[-1].default is None
