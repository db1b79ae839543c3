"""Rooms and doorways on the free space of a 2-D obstacle map (csrc/avl_rooms.hip): label growth along the travel
field, the morphological room segmentation built on it with its room and door tables, and the lift of a label image onto voxels.
Upstream has no counterpart.  Every result is integers and the same bytes on every run."""
from __future__ import annotations

import numpy as np

from .. import _lib
from ..device import DeviceArray, as_device
from ._args import _image_shape, _image_u8, _is_dev, _result, _workspace
from .image2d import distance_transform_edt
from .travel import TravelField

ROOM_TABLE_COLS = 10        # cells, rmin, rmax, cmin, cmax, sum of rows, sum of cols, seed cells, centre row, centre col
DOOR_TABLE_COLS = 10        # i, j, contacts, rmin, rmax, cmin, cmax, door row, door col, 0 (reserved)
ROOMS_MAX = 1 << 24         # kRoomMaxRooms


class LabelGrowth:
    """grow_labels' result.  owner: (H, W) int32 host array or DeviceArray -- the seed on a source, 0 where the travel field does not
    reach, else the smallest label of any source from which a shortest legal walk ends on the cell.  field: the TravelField the
    labels grew along.  rounds, tile_runs: the label phase's schedule (the distance phase's are field.rounds, field.tile_runs) --
    information about the schedule, not part of the result."""

    def __init__(self, owner, field, rounds, tile_runs):
        self.owner, self.field, self.rounds, self.tile_runs = owner, field, int(rounds), int(tile_runs)
        self.shape = field.shape


class RoomSegmentation:
    """segment_rooms' result.  n: the number of rooms K.  labels: (H, W) int32, 0 = obstacle or a free cell no seed reaches, 1 .. K.
    rooms: (K, ROOM_TABLE_COLS) int64 host table, doors: (D, DOOR_TABLE_COLS) int64 host table sorted by (i, j).  clearance: the
    (H, W) float64 distance transform of the free map.  field: the TravelField of the growth (None when K == 0).  seeds: the
    (H, W) int32 seed image.  labels, clearance and seeds are host arrays, or DeviceArrays with device=True."""

    def __init__(self, n, labels, rooms, doors, clearance, field, seeds, shape, growth=None):
        self.n, self.labels, self.rooms, self.doors = int(n), labels, rooms, doors
        self.clearance, self.field, self.seeds, self.shape, self.growth = clearance, field, seeds, tuple(shape), growth


def _seed_image(seeds, shape, stream):
    """(H, W) int32 seed image, host or device -> (ptr, keepalive); the host checks of grow_labels"""
    if _is_dev(seeds):
        if _image_shape(seeds) != shape:
            raise ValueError(f"grow_labels: the seed image is {_image_shape(seeds)}, the map {shape}")
        ptr, _, keep = as_device(seeds, np.int32, stream)
        return ptr, keep
    s = np.asarray(seeds)
    if s.shape != shape:
        raise ValueError(f"grow_labels: the seed image is {s.shape}, the map {shape}")
    if s.dtype.kind not in "iub":
        raise TypeError(f"grow_labels: seeds are integer labels, got {s.dtype}")
    if s.size and (s.min() < 0 or s.max() > np.iinfo(np.int32).max):
        raise ValueError("grow_labels: a seed label is negative or above 2^31 - 1")
    ptr, _, keep = as_device(np.ascontiguousarray(s, dtype=np.int32), np.int32, stream)
    return ptr, keep


def grow_labels(free, seeds, device=False, stream=None, window=None) -> LabelGrowth:
    """Label growth along the travel field: a geodesic Voronoi partition of the free space with exact ties.
    free: 2-D bool / uint8 / numeric image, nonzero = free, host or device.  seeds: int32 image of the same shape, host or device; a
    seed is > 0 and is a label, it may lie on an obstacle cell.  window=(r0, r1, c0, c1): work on that window of both images
    without copying.  First ops.travel_field's field from the sources seeds > 0, then on the fixed field
        owner[c] = seeds[c] on a source, 0 where unreached, else min(owner[u]) over the tight predecessors u
    (the step u -> c is legal and field[u] + step == field[c]).  -> LabelGrowth with host arrays, or DeviceArrays (device=True).
    ValueError without a seed, for negative labels and for a shape mismatch; a side above TRAVEL_MAX_SIDE raises AvlError before any
    device work.  The call synchronises the stream."""
    lib = _lib.load()
    shape = _image_shape(free)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"expected a non-empty 2-D free map, got shape {shape}")
    r0, r1, c0, c1 = (0, shape[0], 0, shape[1]) if window is None else (int(v) for v in window)
    if not (0 <= r0 < r1 <= shape[0] and 0 <= c0 < c1 <= shape[1]):
        raise ValueError(f"window [{r0}:{r1}, {c0}:{c1}] is not inside the {shape} map")
    H, W = r1 - r0, c1 - c0
    if not _is_dev(seeds):
        s = np.asarray(seeds)
        if s.shape != shape:
            raise ValueError(f"grow_labels: the seed image is {s.shape}, the map {shape}")
        if s.dtype.kind not in "iub":
            raise TypeError(f"grow_labels: seeds are integer labels, got {s.dtype}")
        if s.size and s.min() < 0:
            raise ValueError("grow_labels: a seed label is negative")
        if not (s[r0:r1, c0:c1] > 0).any():
            raise ValueError("grow_labels: there is no seed")
    elif _image_shape(seeds) != shape:
        raise ValueError(f"grow_labels: the seed image is {_image_shape(seeds)}, the map {shape}")
    ws, nws = _workspace(lib.avl_grow_labels_workspace_bytes, "avl_grow_labels", H, W)
    if isinstance(free, np.ndarray) and free.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        free = free != 0
    fp, _, fkeep = _image_u8(free, stream)
    sp, skeep = _seed_image(seeds, shape, stream)
    off = r0 * shape[1] + c0
    straight, diagonal, owner = (DeviceArray((H, W), np.int32) for _ in range(3))
    stats = DeviceArray((8,), np.int64)
    _lib.check(lib.avl_grow_labels(fp + off, shape[1], sp + 4 * off, shape[1], H, W, straight.ptr, diagonal.ptr, owner.ptr, stats.ptr,
                                   ws.ptr, nws, stream), "avl_grow_labels")
    rounds, tile_runs, reached, any_source, lrounds, ltiles, negative, _ = (int(v) for v in stats.numpy(stream))
    if negative:
        raise ValueError("grow_labels: a seed label is negative")
    if not any_source:
        raise ValueError("grow_labels: there is no seed")

    def free_host():
        f = free if isinstance(free, np.ndarray) else (fkeep.numpy(stream) if isinstance(fkeep, DeviceArray) else fkeep.cpu().numpy())
        return np.asarray(f)[r0:r1, c0:c1] != 0

    if device:                                       # the stream is drained: nothing queued still reads the inputs or the workspace
        field = TravelField(straight, diagonal, (H, W), reached, rounds, tile_runs, free_host, stream)
        return LabelGrowth(owner, field, lrounds, ltiles)
    field = TravelField(straight.numpy(stream), diagonal.numpy(stream), (H, W), reached, rounds, tile_runs, free_host, stream)
    return LabelGrowth(owner.numpy(stream), field, lrounds, ltiles)


def room_seeds(clearance, radius, min_seed_cells=1, stream=None):
    """The seeds of the room segmentation: the 8-connected islands of `clearance > radius` (float64) in SciPy's numbering, those with
    fewer than min_seed_cells cells dropped, the rest renumbered 1 .. K in their old order.  clearance: (H, W) float64, host or
    device.  -> ((H, W) int32 DeviceArray, K)."""
    lib = _lib.load()
    shape = _image_shape(clearance)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"expected a non-empty 2-D clearance image, got shape {shape}")
    H, W = shape
    radius, least = float(radius), int(min_seed_cells)
    if not (np.isfinite(radius) and radius >= 0.0):
        raise ValueError(f"radius must be finite and >= 0, got {radius!r}")
    if least < 1:
        raise ValueError(f"min_seed_cells must be >= 1, got {min_seed_cells!r}")
    ws, nws = _workspace(lib.avl_room_seeds_workspace_bytes, "avl_room_seeds", H, W)
    ep, _, ekeep = as_device(clearance, np.float64, stream)
    seeds, k = DeviceArray((H, W), np.int32), DeviceArray((1,), np.int32)
    _lib.check(lib.avl_room_seeds(ep, H, W, radius, least, seeds.ptr, k.ptr, ws.ptr, nws, stream), "avl_room_seeds")
    n = int(k.numpy(stream)[0])                      # drains the stream: the workspace and the input may go
    return seeds, n


def room_tables(labels, seeds, clearance, n, stream=None):
    """The room table (n, ROOM_TABLE_COLS) and the door table (D, DOOR_TABLE_COLS) of a label image with labels 0 .. n, both int64
    host arrays.  labels, seeds: (H, W) int32; clearance: (H, W) float64; host or device."""
    lib = _lib.load()
    shape = _image_shape(labels)
    if len(shape) != 2 or _image_shape(seeds) != shape or _image_shape(clearance) != shape:
        raise ValueError(f"room_tables: labels {shape}, seeds {_image_shape(seeds)} and clearance {_image_shape(clearance)} must be one 2-D shape")
    H, W = shape
    n = int(n)
    if not 0 <= n <= ROOMS_MAX:
        raise ValueError(f"room_tables: {n} rooms (0 .. {ROOMS_MAX})")
    if n == 0:
        return np.zeros((0, ROOM_TABLE_COLS), np.int64), np.zeros((0, DOOR_TABLE_COLS), np.int64)
    ws, nws = _workspace(lib.avl_room_doors_workspace_bytes, "avl_room_doors", n)
    lp, _, k1 = as_device(labels, np.int32, stream)
    sp, _, k2 = as_device(seeds, np.int32, stream)
    ep, _, k3 = as_device(clearance, np.float64, stream)
    rooms, count = DeviceArray((n, ROOM_TABLE_COLS), np.int64), DeviceArray((2,), np.int64)
    _lib.check(lib.avl_room_table(lp, sp, ep, H, W, n, rooms.ptr, stream), "avl_room_table")
    _lib.check(lib.avl_room_doors(lp, ep, H, W, n, count.ptr, ws.ptr, nws, stream), "avl_room_doors")
    D, overflow = (int(v) for v in count.numpy(stream))
    if overflow:
        raise _lib.AvlError(f"room_tables: more touching pairs than the pair table of {n} rooms holds")
    doors = DeviceArray((D, DOOR_TABLE_COLS), np.int64)
    if D:
        _lib.check(lib.avl_room_door_table(ws.ptr, nws, n, W, D, doors.ptr, stream), "avl_room_door_table")
    return rooms.numpy(stream), (doors.numpy(stream) if D else np.zeros((0, DOOR_TABLE_COLS), np.int64))


def segment_rooms(free, radius, min_seed_cells=1, device=False, stream=None) -> RoomSegmentation:
    """Morphological room segmentation of a free map (Bormann et al., ICRA 2016), a chain of device passes:
        E = distance_transform_edt(free);  core = E > radius (float64, radius in cells)
        seeds = the 8-connected islands of core, those below min_seed_cells cells dropped, the rest renumbered 1 .. K
        labels = grow_labels(free, seeds).owner  (a free cell no seed reaches keeps 0)
    and the room and door tables.  K == 0 is no error: the labels are zero and the tables empty.  A map without an obstacle cell
    raises distance_transform_edt's ValueError.  -> RoomSegmentation."""
    shape = _image_shape(free)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"expected a non-empty 2-D free map, got shape {shape}")
    radius, least = float(radius), int(min_seed_cells)
    if not (np.isfinite(radius) and radius >= 0.0):
        raise ValueError(f"radius must be finite and >= 0, got {radius!r}")
    if least < 1:
        raise ValueError(f"min_seed_cells must be >= 1, got {min_seed_cells!r}")
    _lib.load()
    if isinstance(free, np.ndarray) and free.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        free = free != 0
    if not _is_dev(free):
        _lib.require_gpu()
        free = DeviceArray.from_numpy(np.ascontiguousarray(free).astype(np.uint8, copy=False), stream)      # one upload for the chain
    E = distance_transform_edt(free, device=True, stream=stream)
    seeds, n = room_seeds(E, radius, least, stream)
    if n == 0:
        labels, field, growth = seeds, None, None    # all zero
    else:
        growth = grow_labels(free, seeds, device=True, stream=stream)
        labels, field = growth.owner, growth.field
    rooms, doors = room_tables(labels, seeds, E, n, stream)
    if not device:
        labels, E, seeds = labels.numpy(stream), E.numpy(stream), seeds.numpy(stream)
        if field is not None:
            field.straight, field.diagonal = field.planes()
    return RoomSegmentation(n, labels, rooms, doors, E, field, seeds, shape, growth)


def lift_labels_2d(labels, grid_pos, window, device=False, stream=None):
    """voxel_room[n] = labels[row - rmin, col - cmin] for grid_pos (N, 3) int32 = (row, col, height), host or device; 0 outside
    the crop.  labels: (H, W) int32 over the crop, window = (rmin, cmin) of the crop in the full map.  -> (N,) int32."""
    lib = _lib.load()
    shape = _image_shape(labels)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"expected a non-empty 2-D label image, got shape {shape}")
    gshape = _image_shape(grid_pos)
    if len(gshape) != 2 or gshape[1] != 3:
        raise ValueError(f"lift_labels_2d: grid_pos must be (N, 3), got {gshape}")
    rmin, cmin = (int(v) for v in tuple(window)[:2])
    _lib.require_gpu()
    lp, _, k1 = as_device(labels if _is_dev(labels) else np.ascontiguousarray(labels, dtype=np.int32), np.int32, stream)
    gp, _, k2 = as_device(grid_pos if _is_dev(grid_pos) else np.ascontiguousarray(grid_pos, dtype=np.int32), np.int32, stream)
    N = int(gshape[0])
    out = DeviceArray((N,), np.int32)
    _lib.check(lib.avl_lift_labels_2d(lp, shape[0], shape[1], gp, N, rmin, cmin, out.ptr, stream), "avl_lift_labels_2d")
    return _result(out, device, stream, keep=(k1, k2))
