"""Layered costmaps and cost-weighted travel fields on a 2-D obstacle map (csrc/avl_costfield.hip): the price of
entering a cell from distance planes and lookup tables, and the cheapest 8-connected walk under those prices -- travel.py's field
with a price per cell.  Upstream has no counterpart (it dilates the obstacle map by a fixed number of cells)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from ..device import DeviceArray, as_device
from ._args import _image_shape, _image_u8, _is_dev, _result, _workspace
from .travel import _field_front, _host_window, _PairField

COST_MAX_CELLS = 1 << 22     # kCostMaxCells: H * W of a cost field, which keeps both sums of prices below 2^30
COST_MAX_LAYERS = 8          # kCostMaxLayers
COST_LETHAL = 255            # a table entry that makes the cell impassable; in a costmap a lethal cell has price 0
COST_MAX = 254               # the largest price a costmap gives a passable cell


class _CostLayerC(C.Structure):
    """avl_cost_layer of include/avlmaps_hip.h"""
    _fields_ = [("d_distance", C.c_void_p), ("d_table", C.c_void_p), ("n_table", C.c_int32)]


def _table_length(reach):
    """entries of a table over d^2 that covers every d <= reach and ends with one entry beyond it"""
    return int(np.floor(float(reach) ** 2)) + 2


def inflation_table(inscribed_cells, inflation_cells, scaling, peak=100) -> np.ndarray:
    """The inflation layer's uint8 table over the SQUARED clearance d^2 (in cells), computed on the host in float64 with d = sqrt(d^2):
    COST_LETHAL where d < inscribed_cells (the robot's centre cannot be there), floor(peak * exp(-scaling * (d - inscribed_cells)))
    for inscribed_cells <= d <= inflation_cells, 0 beyond.  The last entry lies beyond both radii, so it serves every larger d^2.
    scaling is per cell; 0 <= peak <= COST_MAX."""
    inscribed, inflation, scaling, peak = float(inscribed_cells), float(inflation_cells), float(scaling), float(peak)
    if not (np.isfinite(inscribed) and inscribed >= 0.0 and np.isfinite(inflation) and inflation >= 0.0):
        raise ValueError(f"inflation_table: radii must be finite and >= 0, got {inscribed_cells!r} and {inflation_cells!r}")
    if not (np.isfinite(scaling) and scaling >= 0.0):
        raise ValueError(f"inflation_table: scaling must be finite and >= 0, got {scaling!r}")
    if not 0.0 <= peak <= COST_MAX:
        raise ValueError(f"inflation_table: peak must lie in [0, {COST_MAX}], got {peak!r}")
    d = np.sqrt(np.arange(_table_length(max(inscribed, inflation)), dtype=np.float64))
    t = np.floor(peak * np.exp(-scaling * (d - inscribed)))
    t[d > inflation] = 0.0
    t[d < inscribed] = COST_LETHAL
    return t.astype(np.uint8)


def penalty_table(radius_cells, penalty, lethal=False) -> np.ndarray:
    """An avoidance layer's uint8 table over the SQUARED distance d^2 (in cells) to the thing to avoid: floor(penalty * (1 - d / radius))
    for d < radius_cells -- the penalty itself at distance 0 -- and 0 from the radius on.  lethal=True: the entry at d^2 = 0, the
    thing's own cells, is COST_LETHAL.  0 <= penalty <= COST_MAX."""
    radius, penalty = float(radius_cells), float(penalty)
    if not (np.isfinite(radius) and radius >= 0.0):
        raise ValueError(f"penalty_table: radius must be finite and >= 0, got {radius_cells!r}")
    if not 0.0 <= penalty <= COST_MAX:
        raise ValueError(f"penalty_table: penalty must lie in [0, {COST_MAX}], got {penalty!r}")
    d = np.sqrt(np.arange(_table_length(radius), dtype=np.float64))
    t = np.zeros(len(d), dtype=np.float64)
    inside = d < radius
    t[inside] = np.floor(penalty * (1.0 - d[inside] / radius))
    t[0] = penalty
    if lethal:
        t[0] = COST_LETHAL
    return t.astype(np.uint8)


def distance_to_mask(mask, window=None, stream=None):
    """The distance plane of an avoidance layer: per cell of mask[r0:r1, c0:c1] (window, default the whole mask) the float64
    distance to the nearest NONZERO cell of the window, 0 on those cells -- distance_transform_edt(mask == 0) on the window
    in place (avl_edt2d with invert).  mask: bool / uint8 host image or uint8 device image.  -> float64 DeviceArray, or None when the
    window holds no nonzero cell (nothing to avoid)."""
    from .image2d import _edt_workspace
    lib = _lib.load()
    shape = _image_shape(mask)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"expected a non-empty 2-D mask, got shape {shape}")
    r0, r1, c0, c1 = (0, shape[0], 0, shape[1]) if window is None else (int(v) for v in window)
    if not (0 <= r0 < r1 <= shape[0] and 0 <= c0 < c1 <= shape[1]):
        raise ValueError(f"window [{r0}:{r1}, {c0}:{c1}] is not inside the {shape} mask")
    H, W = r1 - r0, c1 - c0
    ws, nws, found = _edt_workspace(lib, H, W, "avl_edt2d")
    if isinstance(mask, np.ndarray) and mask.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        mask = mask != 0
    mp, _, keep = _image_u8(mask, stream)
    out = DeviceArray((H, W), np.float64)
    _lib.check(lib.avl_edt2d(mp + r0 * shape[1] + c0, shape[1], H, W, 1, out.ptr, found.ptr, ws.ptr, nws, stream), "avl_edt2d")
    if not int(found.numpy(stream)[0]):             # drains the stream: the mask and the workspace are no longer read
        return None
    return out


def build_costmap(free, layers, device=False, stream=None):
    """The layered costmap (avl_costmap2d): (H, W) uint8 prices of entering a cell, or the DeviceArray (device=True).
    free: 2-D bool / uint8 / numeric image, nonzero = free, host or device.  layers: up to COST_MAX_LAYERS pairs
    (distance plane, table) -- the plane an (H, W) float64 image from ops.distance_transform_edt(..., device=True) (clearance:
    the EDT of the free map) or distance_to_mask (nearness to things to avoid), host or device; the table uint8 over the squared
    distance (inflation_table, penalty_table), the last entry serving every larger distance.  Per cell: 0 where not free or where
    any layer's entry is COST_LETHAL, else min(COST_MAX, 1 + the sum of the layers' entries).  Price 0 means impassable."""
    lib = _lib.load()
    shape = _image_shape(free)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"expected a non-empty 2-D free map, got shape {shape}")
    H, W = shape
    layers = list(layers)
    if len(layers) > COST_MAX_LAYERS:
        raise ValueError(f"build_costmap: {len(layers)} layers, at most {COST_MAX_LAYERS}")
    tables = []
    for k, (plane, table) in enumerate(layers):
        if _image_shape(plane) != (H, W):
            raise ValueError(f"build_costmap: the distance plane of layer {k} is {_image_shape(plane)}, the map {(H, W)}")
        if not _is_dev(table):
            table = np.asarray(table)
            if table.ndim != 1 or len(table) < 1 or table.dtype != np.uint8:
                raise ValueError(f"build_costmap: the table of layer {k} must be a non-empty 1-D uint8 array, got {table.dtype} {table.shape}")
        elif len(_image_shape(table)) != 1 or _image_shape(table)[0] < 1:
            raise ValueError(f"build_costmap: the table of layer {k} must be a non-empty 1-D uint8 array, got shape {_image_shape(table)}")
        tables.append(table)
    if H > 16384 or W > 16384:                       # the library's own message, before any device work
        _lib.check(lib.avl_costmap2d(None, W, H, W, None, 0, None, stream), "avl_costmap2d")
    _lib.require_gpu()
    if isinstance(free, np.ndarray) and free.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        free = free != 0
    fp, _, fkeep = _image_u8(free, stream)
    arr, keep = (_CostLayerC * max(len(layers), 1))(), [fkeep]
    for k, ((plane, _), table) in enumerate(zip(layers, tables)):
        pp, _, pkeep = as_device(plane, np.float64, stream)
        tp, tshape, tkeep = as_device(table, np.uint8, stream)
        arr[k] = _CostLayerC(pp, tp, int(tshape[0]))
        keep += [pkeep, tkeep]
    out = DeviceArray((H, W), np.uint8)
    _lib.check(lib.avl_costmap2d(fp, W, H, W, arr, len(layers), out.ptr, stream), "avl_costmap2d")
    return _result(out, device, stream, keep=tuple(keep))


def drop_collinear(walk):
    """the two ends of a walk of 8-neighbour steps and the cells where its direction changes, in order"""
    if len(walk) <= 2:
        return list(walk)
    keep = [walk[0]]
    for p0, p1, p2 in zip(walk[:-2], walk[1:-1], walk[2:]):
        if (p1[0] - p0[0], p1[1] - p0[1]) != (p2[0] - p1[0], p2[1] - p1[1]):
            keep.append(p1)
    keep.append(walk[-1])
    return keep


class CostField(_PairField):
    """cost_field's result.  straight, diagonal: (H, W) int32 host arrays or DeviceArrays, the summed prices A of the straight and
    B of the diagonal steps of the cheapest legal walk from the nearest source (price A + B * sqrt(2)); (0, 0) on a source, -1 in
    both where no walk ends.  reached: the number of reached cells.  rounds, tile_runs: how many rounds had an active tile and how
    many tiles ran in all -- information about the schedule, not part of the result."""
    _what = "cost"

    def __init__(self, straight, diagonal, shape, reached, rounds, tile_runs, passable, prices, stream=None):
        super().__init__(straight, diagonal, shape, reached, rounds, tile_runs, stream)
        self._passable, self._prices = passable, prices

    def cost(self) -> np.ndarray:
        """(H, W) float64: float64(A) + float64(B) * sqrt(2), inf where unreached"""
        return self._length()

    def descend(self, cell, waypoints=False):
        """The cells of a cheapest walk from `cell` back to a source, [(row, col), ...] from `cell` to the source, on the host:
        TravelField.descend with the entered cell's price in the predecessor test.  At each cell v it takes the first neighbour u in
        the order TRAVEL_NEIGHBOURS (E, NE, N, NW, W, SW, S, SE) whose pair plus price[v] -- on the straight sum for a straight step,
        on the diagonal sum for a diagonal one -- equals v's pair and from which the step is legal.  waypoints=True keeps the two
        ends and the cells where the direction changes.  ValueError from an unreached cell or one outside the map."""
        walk = self._descend(cell, self._host_map("_passable"), self._host_map("_prices"))
        return drop_collinear(walk) if waypoints else walk


def _cost_u8(cost, shape):
    """the price plane as uint8: a device image must be uint8 already, a host image any integer or bool dtype with values 0 .. 255"""
    if _image_shape(cost) != tuple(shape):
        raise ValueError(f"cost_field: the cost plane is {_image_shape(cost)}, the map {tuple(shape)}")
    if _is_dev(cost):
        return cost
    c = np.asarray(cost)
    if c.dtype == np.uint8:
        return c
    if c.dtype.kind not in "iub":
        raise ValueError(f"cost_field: prices must be integers 0 .. 255, got dtype {c.dtype}")
    if c.size and (c.min() < 0 or c.max() > 255):
        raise ValueError("cost_field: prices must be integers 0 .. 255")
    return c.astype(np.uint8)


def cost_field(free, cost, sources, device=False, stream=None, window=None) -> CostField:
    """The multi-source cost-weighted travel field of DESIGN.md 4.29.  free, sources, window, device and stream are travel_field's;
    cost: a 2-D image of free's shape with the integer price 0 .. 255 of entering each cell, host or device (uint8 there); the
    window applies to all three planes.  A cell is passable when it is free and its price is not 0.  A step u -> v between
    8-neighbours is legal when v is passable, u is passable or a source and, for a diagonal step, both cells that share an edge with
    u and with v are passable; it adds price[v] to the straight or to the diagonal sum.  -> CostField with host planes, or with
    DeviceArrays (device=True).  With price 1 everywhere the planes are travel_field's.  ValueError without a source, for a shape
    mismatch and for cells outside the map; more than COST_MAX_CELLS cells or a side above TRAVEL_MAX_SIDE raises AvlError before
    any device work.  The call synchronises the stream."""
    lib = _lib.load()
    free, shape, win, (smask, s_ld, s_off) = _field_front("cost_field", free, window, sources)
    H, W = win[1] - win[0], win[3] - win[2]
    off = win[0] * shape[1] + win[2]
    cost = _cost_u8(cost, shape)
    if H * W > COST_MAX_CELLS:                       # the library's own refusal: it looks at the shape before any pointer
        _lib.check(lib.avl_costfield2d(None, W, None, W, None, W, H, W, None, None, None, None, 0, stream), "avl_costfield2d")
    ws, nws = _workspace(lib.avl_travel2d_workspace_bytes, "avl_costfield2d", H, W)      # the travel field's workspace serves
    fp, _, fkeep = _image_u8(free, stream)
    cp, _, ckeep = _image_u8(cost, stream)
    sp, _, skeep = _image_u8(smask, stream)
    straight, diagonal = DeviceArray((H, W), np.int32), DeviceArray((H, W), np.int32)
    stats = DeviceArray((4,), np.int64)
    _lib.check(lib.avl_costfield2d(fp + off, shape[1], cp + off, shape[1], sp + s_off, s_ld, H, W, straight.ptr, diagonal.ptr, stats.ptr,
                                   ws.ptr, nws, stream), "avl_costfield2d")
    rounds, tile_runs, reached, any_source = (int(v) for v in stats.numpy(stream))
    if not any_source:
        raise ValueError("cost_field: there is no source")

    def prices_host():
        return _host_window(cost, ckeep, stream, win).astype(np.uint8)

    def passable_host():
        return (_host_window(free, fkeep, stream, win) != 0) & (prices_host() != 0)

    if not device:                                   # (device: the stream is drained, nothing queued still reads the inputs or the workspace)
        straight, diagonal = straight.numpy(stream), diagonal.numpy(stream)
    return CostField(straight, diagonal, (H, W), reached, rounds, tile_runs, passable_host, prices_host, stream)
