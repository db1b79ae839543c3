"""Travel-distance fields on the free space of a 2-D obstacle map and their decay maps (csrc/avl_travel.hip):
the counterpart of the Euclidean distance transform of image2d.py that goes around walls.  Upstream has no counterpart."""
from __future__ import annotations

import numpy as np

from .. import _lib
from ..device import DeviceArray, as_device
from ._args import _image_shape, _image_u8, _is_dev, _result, _workspace
from .fields import _check_decay

TRAVEL_MAX_SIDE = 16384      # EDT_MAX_SIDE: the decay maps of both families cover the same crops
TRAVEL_TILE = 32             # kTravelTile: cells per tile side of the kernel
TRAVEL_SWEEPS = 64           # kTravelSweeps: the in-tile sweep cap of one round
UNREACHED = -1

# the order in which descend() looks at the neighbours of a cell, (d_row, d_col): E, NE, N, NW, W, SW, S, SE -- the kernel's order
TRAVEL_NEIGHBOURS = ((0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1))


class _PairField:
    """What TravelField and CostField share: the two int32 planes of a field of pairs, host or device, the length a + b * sqrt(2)
    and the walk back to a source.  _what names the field in the messages."""
    _what = "travel"

    def __init__(self, straight, diagonal, shape, reached, rounds, tile_runs, stream):
        self.straight, self.diagonal, self.shape = straight, diagonal, tuple(shape)
        self.reached, self.rounds, self.tile_runs = int(reached), int(rounds), int(tile_runs)
        self._stream, self._host = stream, None

    def planes(self):
        """(straight, diagonal) as host arrays (a device field is copied once and kept)"""
        if self._host is None:
            if isinstance(self.straight, np.ndarray):
                self._host = (self.straight, self.diagonal)
            else:
                self._host = (self.straight.numpy(self._stream), self.diagonal.numpy(self._stream))
        return self._host

    def _length(self) -> np.ndarray:
        a, b = self.planes()
        d = a.astype(np.float64) + b.astype(np.float64) * np.sqrt(2.0)
        d[a < 0] = np.inf
        return d

    def reachable(self) -> np.ndarray:
        """(H, W) bool: the cells a walk from a source ends on, the sources included"""
        return self.planes()[0] >= 0

    def _host_map(self, name):
        """the host plane kept under `name`, fetched once when it was given as a function"""
        v = getattr(self, name)
        if callable(v):
            v = v()
            setattr(self, name, v)
        return v

    def _descend(self, cell, passable, price=None):
        """the walk of descend(): a step into v adds price[v] (1 without a price plane) to the straight or to the diagonal sum, and a
        diagonal step needs both edge-sharing cells passable"""
        a, b = self.planes()
        H, W = self.shape
        r, c = int(cell[0]), int(cell[1])
        if not (0 <= r < H and 0 <= c < W):
            raise ValueError(f"descend: cell {(r, c)} lies outside the {H} x {W} map")
        if a[r, c] < 0:
            raise ValueError(f"descend: cell {(r, c)} is not reached from any source")
        walk = [(r, c)]
        while a[r, c] or b[r, c]:
            p = 1 if price is None else int(price[r, c])
            for dr, dc in TRAVEL_NEIGHBOURS:
                ur, uc = r + dr, c + dc
                if not (0 <= ur < H and 0 <= uc < W) or a[ur, uc] < 0:
                    continue
                diag = dr != 0 and dc != 0
                if a[ur, uc] + (0 if diag else p) != a[r, c] or b[ur, uc] + (p if diag else 0) != b[r, c]:
                    continue
                if diag and not (passable[ur, c] and passable[r, uc]):
                    continue
                r, c = ur, uc
                break
            else:
                raise RuntimeError(f"descend: no predecessor at {(r, c)}: the planes are not a {self._what} field of this map")
            walk.append((r, c))
        return walk


class TravelField(_PairField):
    """travel_field's result.  straight, diagonal: (H, W) int32 host arrays or DeviceArrays, the numbers a and b of straight and
    diagonal steps of the shortest legal walk from the nearest source (length a + b * sqrt(2)); (0, 0) on a source, UNREACHED in
    both where no walk ends.  reached: the number of reached cells.  rounds, tile_runs: how many rounds had an active tile and how
    many tiles ran in all -- information about the schedule, not part of the result."""

    def __init__(self, straight, diagonal, shape, reached, rounds, tile_runs, free, stream=None):
        super().__init__(straight, diagonal, shape, reached, rounds, tile_runs, stream)
        self._free = free

    def distance(self) -> np.ndarray:
        """(H, W) float64: float64(a) + float64(b) * sqrt(2), inf where unreached"""
        return self._length()

    def descend(self, cell):
        """The cells of a shortest walk from `cell` back to a source, [(row, col), ...] from `cell` to the source, on the host.  At
        each cell it takes the first neighbour in the order TRAVEL_NEIGHBOURS (E, NE, N, NW, W, SW, S, SE) whose pair plus the
        step equals the cell's pair and from which the step is legal.  ValueError from an unreached cell or one outside the map."""
        return self._descend(cell, self._host_map("_free"))


def _source_mask(sources, H, W):
    """a host (H, W) uint8 mask from a host mask or from (M, 2) integer cells; a device mask is passed through"""
    if _is_dev(sources):
        if _image_shape(sources) != (H, W):
            raise ValueError(f"travel_field: the source mask is {_image_shape(sources)}, the map {(H, W)}")
        return sources
    s = np.asarray(sources)
    if s.shape == (H, W):
        mask = np.ascontiguousarray(s != 0).view(np.uint8)
    elif s.ndim == 2 and s.shape[1] == 2 and s.dtype.kind in "iu":
        if len(s) and (s.min() < 0 or s[:, 0].max() >= H or s[:, 1].max() >= W):
            raise ValueError(f"travel_field: a source cell lies outside the {H} x {W} map")
        mask = np.zeros((H, W), dtype=np.uint8)
        mask[s[:, 0], s[:, 1]] = 1
    else:
        raise ValueError(f"travel_field: sources must be an ({H}, {W}) mask or (M, 2) integer cells, got {s.dtype} {s.shape}")
    if not mask.any():
        raise ValueError("travel_field: there is no source")
    return mask


def _field_front(who, free, window, sources=None):
    """The front end of travel_field, cost_field and travel_fields: the shape check, the window, and the source mask or cells.
    -> (free, shape, (r0, r1, c0, c1), source): free with a numeric host image turned into a bool one; source = (mask, its row
    length, the window's offset in it), None without `sources`.  `who` names the caller in the messages."""
    shape = _image_shape(free)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"expected a non-empty 2-D free map, got shape {shape}")
    r0, r1, c0, c1 = (0, shape[0], 0, shape[1]) if window is None else (int(v) for v in window)
    if not (0 <= r0 < r1 <= shape[0] and 0 <= c0 < c1 <= shape[1]):
        raise ValueError(f"window [{r0}:{r1}, {c0}:{c1}] is not inside the {shape} map")
    if isinstance(free, np.ndarray) and free.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        free = free != 0
    source = None
    if sources is not None:
        H, W = r1 - r0, c1 - c0
        s = np.asarray(sources) if not _is_dev(sources) else sources
        if not _is_dev(s) and s.shape != shape and s.ndim == 2 and s.shape[1] == 2:      # cells, relative to the window
            source = (_source_mask(s, H, W), W, 0)
        else:
            source = (_source_mask(s, shape[0], shape[1]), shape[1], r0 * shape[1] + c0)
            if isinstance(source[0], np.ndarray) and window is not None and not source[0][r0:r1, c0:c1].any():
                raise ValueError(f"{who}: there is no source")
    return free, shape, (r0, r1, c0, c1), source


def _host_window(image, keep, stream, win):
    """the window of a plane on the host: `image` as the caller gave it, `keep` what _image_u8 kept of a device image"""
    h = image if isinstance(image, np.ndarray) else (keep.numpy(stream) if isinstance(keep, DeviceArray) else keep.cpu().numpy())
    return np.asarray(h)[win[0]:win[1], win[2]:win[3]]


def travel_field(free, sources, device=False, stream=None, window=None) -> TravelField:
    """The multi-source travel-distance field of DESIGN.md 4.26.  free: 2-D bool / uint8 / numeric image, nonzero = free (the
    convention of Map.obstacles_cropped), host or device.  sources: a mask of the same shape, nonzero = source (a source may lie on
    an obstacle cell), host or device, or (M, 2) integer (row, col) cells on the host.  window=(r0, r1, c0, c1): work on
    free[r0:r1, c0:c1] and on the same window of a source mask without copying; cells are then relative to the window.
    A step u -> v between 8-neighbours is legal when v is free, u is free or a source and, for a diagonal step, both cells that
    share an edge with u and with v are free.  -> TravelField with host planes, or with DeviceArrays (device=True).
    ValueError without a source, for a shape mismatch and for cells outside the map; a side above TRAVEL_MAX_SIDE raises AvlError
    before any device work.  The call synchronises the stream."""
    lib = _lib.load()
    free, shape, win, (smask, s_ld, s_off) = _field_front("travel_field", free, window, sources)
    H, W = win[1] - win[0], win[3] - win[2]
    off = win[0] * shape[1] + win[2]
    ws, nws = _workspace(lib.avl_travel2d_workspace_bytes, "avl_travel2d", H, W)
    fp, _, fkeep = _image_u8(free, stream)
    sp, _, skeep = _image_u8(smask, stream)
    straight, diagonal = DeviceArray((H, W), np.int32), DeviceArray((H, W), np.int32)
    stats = DeviceArray((4,), np.int64)
    _lib.check(lib.avl_travel2d(fp + off, shape[1], sp + s_off, s_ld, H, W, straight.ptr, diagonal.ptr, stats.ptr, ws.ptr, nws, stream),
               "avl_travel2d")
    rounds, tile_runs, reached, any_source = (int(v) for v in stats.numpy(stream))
    if not any_source:
        raise ValueError("travel_field: there is no source")

    def free_host():
        return _host_window(free, fkeep, stream, win) != 0

    if not device:                                   # (device: the stream is drained, nothing queued still reads the inputs or the workspace)
        straight, diagonal = straight.numpy(stream), diagonal.numpy(stream)
    return TravelField(straight, diagonal, (H, W), reached, rounds, tile_runs, free_host, stream)


def travel_decay_2d(field: TravelField, decay_rate, cell_size=1.0, normalize=False, device=False, stream=None):
    """The decay map of a travel field, NumPy's float64 bits (mask_decay_2d's expression with the travel distance):
        d = field.distance();  t = 1 - (d / cell_size) * decay_rate;  t[t < 0] = 0;  t[unreached] = 0
        normalize:  (t - t.min()) / (t.max() - t.min()) over the whole map
    -> (H, W) float64 or the DeviceArray.  ValueError: normalize on a constant map."""
    lib = _lib.load()
    H, W = field.shape
    decay = _check_decay(decay_rate)
    cs = float(cell_size)
    if not (np.isfinite(cs) and cs > 0.0):
        raise ValueError(f"cell_size must be finite and > 0, got {cell_size!r}")
    _lib.require_gpu()
    ap, ashape, k1 = as_device(field.straight, np.int32, stream)
    bp, bshape, k2 = as_device(field.diagonal, np.int32, stream)
    if tuple(ashape) != (H, W) or tuple(bshape) != (H, W):
        raise ValueError(f"travel_decay_2d: planes of {tuple(ashape)} and {tuple(bshape)} for a field of {(H, W)}")
    ws, flag, out = DeviceArray((512,), np.uint8), DeviceArray((1,), np.int32), DeviceArray((H, W), np.float64)
    _lib.check(lib.avl_travel_decay_2d(ap, bp, H, W, cs, decay, int(bool(normalize)), out.ptr, flag.ptr, ws.ptr, ws.nbytes, stream),
               "avl_travel_decay_2d")
    if normalize and int(flag.numpy(stream)[0]):
        raise ValueError("travel_decay_2d: the 2-D map is constant, its min-max normalisation is undefined")
    return _result(out, device, stream, keep=(k1, k2, ws, flag))
