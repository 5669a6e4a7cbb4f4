"""REFER segmentation targets as a run-length arena built on the device (csrc/polymask.hip): the host side.

`REFER.getMask` (dataset/refer.py:279-291) rasterises every polygon of a ref with `cocomask.frPyObjects` and decodes it to a
full-size mask.  Here the polygons of a whole split are handed to the device once; what comes back is the `(ends, seg_off)` arena
of dataset/rle_arena.py -- for every segment the column-major positions where its runs end -- which `tris_rle_decode_sum_u8` and
`tris_rle_target_nearest_u8` read.  A ref is a range of segments, as a ReferIt sentence is.

The host forms the x5 upsampled integer vertices exactly as cocomask.py:18-19 does (double arithmetic, truncation toward zero), so
no coordinate rounding reaches the device.  `runs_numpy` states what the kernels compute from them.

Everything the kernels would otherwise have to trust is settled here.  Through the host route (`cocomask.frPyObjects` ->
`rle_arena.segment_ends`, into the same arena): an RLE-dict segmentation, and a polygon with an upsampled coordinate beyond
+-COORD_MAX (the device walks max(dx, dy) steps per edge; the bound keeps a chunk of step counts inside int32).  Refused, naming
the offender: more than 255 segments for one ref (the decoded sum is a byte), H*W > 2^24, a coordinate list that is empty, odd or
not finite (cocomask.py would drop the last number or fail on it), a coordinate beyond +-HOST_COORD_MAX / 5 pixels.  No slice is refused for its length: the device sorts slices
beyond its LDS capacity in global memory.

The arena inherits cocomask.py's caveat: it is pinned to this project's restatement of maskApi.c, not to pycocotools.
"""
import numpy as np

from . import cocomask
from .rle_arena import MAX_PIXELS, MAX_SEGMENTS, segment_ends

COORD_MAX = 1 << 20        # |upsampled coordinate| the device producer takes: +-209715 pixels
HOST_COORD_MAX = 1 << 24   # ... and the host route, whose walk allocates one array element per step


def upsample(xy):
    """[x0,y0,x1,y1,...] -> int64 [k,2] upsampled vertices (cocomask.py:16-19)"""
    xy = np.asarray(xy, np.float64)
    k = xy.size // 2
    x = (5.0 * xy[0:2 * k:2] + 0.5).astype(np.int64)
    y = (5.0 * xy[1:2 * k:2] + 0.5).astype(np.int64)
    return np.stack([x, y], 1)


def runs_numpy(verts, h, w):
    """numpy statement of tris_poly_count_runs / tris_poly_emit_runs for one polygon: upsampled vertices int [k,2] -> the sorted
    int32 run ends, the closing h*w included.  Every step pair (d - 1, d) of every edge on its own, in integers but for the rounded
    point of a step."""
    verts = np.asarray(verts, np.int64).reshape(-1, 2)
    k = verts.shape[0]
    out = [np.array([h * w], np.int64)]
    for j in range(k):
        xs, ys = (int(c) for c in verts[j])
        xe, ye = (int(c) for c in verts[(j + 1) % k])
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        n = max(dx, dy)
        if n == 0:
            continue
        d = np.arange(n + 1)
        t = n - d if flip else d
        if dx >= dy:
            s = (ye - ys) / dx
            u = t + xs
            v = (ys + s * t + 0.5).astype(np.int64)
        else:
            s = (xe - xs) / dy
            v = t + ys
            u = (xs + s * t + 0.5).astype(np.int64)
        u1, u0, v1, v0 = u[1:], u[:-1], v[1:], v[:-1]
        xk = np.where(u1 < u0, u1, u1 - 1)
        keep = (u1 != u0) & (xk >= 2) & ((xk - 2) % 5 == 0) & ((xk - 2) // 5 <= w - 1)
        vk = np.minimum(v1, v0)[keep]
        yc = np.clip(np.where(vk <= 2, 0, (vk + 2) // 5), 0, h)
        out.append((xk[keep] - 2) // 5 * h + yc)
    return np.sort(np.concatenate(out)).astype(np.int32)


class DeviceArena:
    """what PolyArena.build leaves on the device: ends int32 [runs + 1], seg_off int64 [segments + 1], ranges int32 [refs, 2]"""

    def __init__(self, ends, seg_off, ranges):
        self.ends, self.seg_off, self.ranges = ends, seg_off, ranges

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.ends, self.seg_off, self.ranges))


class PolyArena:
    """Builder: add_ref() per ref, build(device) at the end."""

    def __init__(self):
        self._verts, self._hw, self._host, self._ranges = [], [], {}, []

    @property
    def n_segments(self):
        return len(self._verts)

    @property
    def n_host_segments(self):
        return len(self._host)

    def add_ref(self, segmentation, H, W, name="ref"):
        """the segments of one ref (a list of polygons [x0,y0,x1,y1,...], a list of RLE dicts, or one RLE dict) -> (first segment,
        one past the last)"""
        H, W = int(H), int(W)
        if H < 1 or W < 1 or H * W > MAX_PIXELS:
            raise ValueError(f"{name}: {H}x{W} is empty or beyond 2^24 pixels")
        seg = [segmentation] if isinstance(segmentation, dict) else list(segmentation)
        if len(seg) > MAX_SEGMENTS:
            raise ValueError(f"{name}: {len(seg)} segments, their sum does not fit the uint8 target (at most {MAX_SEGMENTS})")
        new = []                                    # (all checked before any is added)
        for j, s in enumerate(seg):
            who = f"{name} segment {j}"
            if isinstance(s, dict):
                new.append((None, segment_ends(cocomask.frPyObjects(s, H, W), H, W, who)))
                continue
            try:
                xy = np.asarray(s, np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"{who}: neither a coordinate list nor an RLE dict") from None
            if xy.ndim != 1 or xy.size == 0 or xy.size % 2:
                raise ValueError(f"{who}: {xy.size} numbers in shape {xy.shape} are not a list of x, y pairs")
            if not np.isfinite(xy).all():
                raise ValueError(f"{who}: coordinate {float(xy[~np.isfinite(xy)][0])} is not finite")
            if np.abs(xy).max() > HOST_COORD_MAX / 5.0:
                raise ValueError(f"{who}: coordinate {float(xy[np.abs(xy).argmax()])} is beyond +-{HOST_COORD_MAX // 5} pixels")
            v = upsample(xy)
            if np.abs(v).max() > COORD_MAX:
                new.append((None, segment_ends(cocomask.frPyObjects([xy], H, W)[0], H, W, who)))
            else:
                new.append((v.astype(np.int32), None))
        lo = self.n_segments
        for v, host in new:
            if v is None:
                self._host[self.n_segments] = host
                v = np.zeros((0, 2), np.int32)
            self._verts.append(v)
            self._hw.append((H, W))
        self._ranges.append((lo, self.n_segments))
        return lo, self.n_segments

    def arrays(self):
        """-> (verts int32 [V,2], poly_off int64 [P+1], hw int32 [P,2], ranges int32 [refs,2])"""
        verts = np.concatenate(self._verts) if self._verts else np.zeros((0, 2), np.int32)
        off = np.zeros(self.n_segments + 1, np.int64)
        off[1:] = np.cumsum([v.shape[0] for v in self._verts])
        return (verts.astype(np.int32), off, np.asarray(self._hw, np.int32).reshape(-1, 2),
                np.asarray(self._ranges, np.int32).reshape(-1, 2))

    def build(self, device="cuda"):
        """count -> scan -> emit for the whole split, the host-route segments placed into their slices -> DeviceArena"""
        import torch
        from .. import ops
        if not torch.cuda.is_available():
            raise ops.NoGpuError("PolyArena.build needs the GPU; there is no CPU fallback")
        verts, off, hw, ranges = self.arrays()
        host = None
        if self._host:
            idx = np.fromiter(self._host.keys(), np.int64)
            vals = list(self._host.values())
            host = (torch.from_numpy(idx).to(device), torch.tensor([e.size for e in vals], dtype=torch.int64, device=device),
                    torch.from_numpy(np.concatenate(vals + [np.zeros(0, np.int32)]).astype(np.int32)).to(device))
        # (one spare row: a split without vertices still has an address)
        verts_d = torch.from_numpy(np.concatenate([verts, np.zeros((1, 2), np.int32)])).to(device)
        ends, seg_off = ops.poly_runs(verts_d, torch.from_numpy(off).to(device), torch.from_numpy(hw).to(device), host=host)
        return DeviceArena(ends, seg_off, torch.from_numpy(ranges).to(device))
