"""Run-length targets for the device decoder (csrc/referit.hip, tris_rle_decode_sum_u8): the host side.

A COCO RLE segment is a list of counts in column-major order, background first.  The arena keeps, for every segment, the
inclusive prefix sums of its counts -- the column-major position where each run ends -- so that the value of a pixel is the
parity of a binary search: the run that holds position p is the first one whose end lies beyond p, odd runs are foreground, and a
position past the last run is background (what `cocomask._decode_counts` and pycocotools' zero-initialised buffer give for counts
that stop short of H*W).  Compressed-string counts go through `cocomask._counts_from_string` here, once.

Everything the kernel would otherwise have to trust is refused here, naming the offender: a negative count, counts that sum past
H*W, more than 255 segments for one sentence (the sum is a byte), H*W > 2^24.
"""
import numpy as np

from . import cocomask

MAX_PIXELS = 1 << 24
MAX_SEGMENTS = 255


def segment_ends(rle, H, W, name="segment"):
    """one RLE dict -> int32 run ends (inclusive prefix sums of its counts); ValueError naming `name` on a malformed one"""
    if not isinstance(rle, dict) or "counts" not in rle:
        raise ValueError(f"{name}: not an RLE dict with 'counts'")
    size = rle.get("size")
    if size is not None and tuple(int(v) for v in size) != (int(H), int(W)):
        raise ValueError(f"{name}: RLE size {list(size)} is not the image's [{H}, {W}]")
    c = rle["counts"]
    if isinstance(c, (str, bytes)):
        try:
            c = cocomask._counts_from_string(c)
        except IndexError:
            raise ValueError(f"{name}: truncated compressed RLE string") from None
    c = np.asarray(c)
    if c.ndim != 1 or (c.size and not np.issubdtype(c.dtype, np.integer)):
        raise ValueError(f"{name}: counts are not a list of integers")
    c = c.astype(np.int64)
    if (c < 0).any():
        j = int(np.nonzero(c < 0)[0][0])
        raise ValueError(f"{name}: negative count {int(c[j])} at run {j}")
    ends = np.cumsum(c)
    if ends.size and ends[-1] > H * W:
        raise ValueError(f"{name}: counts sum to {int(ends[-1])}, past H*W = {H * W}")
    return ends.astype(np.int32)


class RleArena:
    """Builder: add_sentence() per sentence, arrays() / to(device) at the end."""

    def __init__(self):
        self._ends, self._seg_off, self._n = [], [0], 0

    @property
    def n_segments(self):
        return len(self._seg_off) - 1

    def add_sentence(self, rles, H, W, name="sentence"):
        """the segments of one sentence (a list of RLE dicts, or one dict) -> (first segment, one past the last)"""
        if H < 1 or W < 1 or H * W > MAX_PIXELS:
            raise ValueError(f"{name}: {H}x{W} is empty or beyond 2^24 pixels")
        if isinstance(rles, dict):
            rles = [rles]
        if len(rles) > MAX_SEGMENTS:
            raise ValueError(f"{name}: {len(rles)} segments, their sum does not fit the uint8 target (at most {MAX_SEGMENTS})")
        lo = self.n_segments
        new = [segment_ends(r, H, W, f"{name} segment {j}") for j, r in enumerate(rles)]   # (all checked before any is added)
        for e in new:
            self._ends.append(e)
            self._n += e.size
            self._seg_off.append(self._n)
        return lo, self.n_segments

    def arrays(self):
        """-> (ends int32 [total runs], seg_off int64 [segments + 1])"""
        ends = np.concatenate(self._ends) if self._ends else np.zeros(0, np.int32)
        return ends.astype(np.int32), np.asarray(self._seg_off, np.int64)

    def to(self, device):
        import torch
        ends, seg_off = self.arrays()
        # (one spare word: an arena without runs still has an address)
        return (torch.from_numpy(np.concatenate([ends, np.zeros(1, np.int32)])).to(device), torch.from_numpy(seg_off).to(device))


def decode_sum_numpy(ends, seg_off, ranges, H, W):
    """numpy statement of the kernel: parity of searchsorted -> uint8 [K,H,W]"""
    ys, xs = np.mgrid[0:H, 0:W]
    p = xs * H + ys
    out = np.zeros((len(ranges), H, W), np.int64)
    for k, (lo, hi) in enumerate(ranges):
        for s in range(lo, hi):
            e = ends[seg_off[s]:seg_off[s + 1]]
            r = np.searchsorted(e, p, side="right")
            out[k] += (r < e.size) & (r % 2 == 1)
    return out.astype(np.uint8)
