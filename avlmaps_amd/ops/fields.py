"""Area / sound / image goal fields (csrc/avl_field2d.hip) and the fused cross-modal goal (csrc/avl_goal.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from ..device import DeviceArray, DeviceView, as_device, _is_torch
from ._args import _is_dev


class GoalField:
    """A 2-D goal field on the device: `field` (gs, gs) float64 (area) or float32 (sound) and `minmax` (2,) of the same type,
    [min, max] of the whole grid, both DeviceArrays (csrc/avl_field2d.hip)."""

    def __init__(self, field, minmax):
        self.field, self.minmax = field, minmax
        self.gs = field.shape[0]
        self.is_f64 = field.dtype == np.float64

    def bounds(self, stream=None):
        """(min, max) on the host (synchronises the stream)"""
        mm = self.minmax.numpy(stream)
        return mm[0], mm[1]


def _check_decay(decay_rate):
    d = float(decay_rate)
    if not (np.isfinite(d) and d >= 0.0):
        raise ValueError(f"decay_rate must be finite and >= 0, got {decay_rate!r}")
    return d


def area_field(cells, peaks, gs, decay_rate=0.1, stream=None) -> GoalField:
    """avlmap.py:78-96 (index_area_2d before its normalisation): the float64 maximum of clipped cones
    clip(peak_i - decay * ||cell - cell_i||, 0, 1) over the poses whose cell lies inside the (gs, gs) grid, on a field of zeros.
    cells (P, 2) int32 (row, col), peaks (P,) float64 finite: host arrays or device arrays."""
    lib = _lib.load()
    _lib.require_gpu()
    decay = _check_decay(decay_rate)
    if isinstance(peaks, np.ndarray) and not np.all(np.isfinite(peaks)):
        raise ValueError("area peaks must be finite")
    cp, cshape, k1 = as_device(cells, np.int32, stream)
    pp, pshape, k2 = as_device(peaks, np.float64, stream)
    P = int(pshape[0]) if len(pshape) else 0
    if tuple(cshape) != (P, 2):
        raise ValueError(f"cells must be ({P}, 2), got {tuple(cshape)}")
    field, mm = DeviceArray((gs, gs), np.float64), DeviceArray((2,), np.float64)
    _lib.check(lib.avl_field_area(cp, pp, P, int(gs), decay, field.ptr, mm.ptr, stream), "avl_field_area")
    if isinstance(cells, np.ndarray) or isinstance(peaks, np.ndarray):
        _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")      # the uploaded temporaries die here
    return GoalField(field, mm)


def sound_field(offsets, cells, peaks, gs, decay_rate=0.01, stream=None) -> GoalField:
    """avlmap.py:111-131 (index_sound_2d before its normalisation): for every segment in order, the float64 term
    max(p - (p * d) * decay, 0), d = distance to the nearest of the segment's locations, added into a float32 field.
    offsets (S + 1,) int64 CSR offsets into cells (L, 2) int32 (row, col), peaks (S,) float32 >= 0 (host arrays).  Every
    location must lie inside the grid."""
    lib = _lib.load()
    _lib.require_gpu()
    decay = _check_decay(decay_rate)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    cells = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 2)
    peaks = np.ascontiguousarray(peaks, dtype=np.float32)
    S, L = len(peaks), len(cells)
    if offsets.shape != (S + 1,) or offsets[0] != 0 or offsets[-1] != L or np.any(np.diff(offsets) < 1):
        raise ValueError("offsets must be (S + 1,) CSR offsets from 0 to len(cells), every segment with >= 1 location")
    if not np.all(np.isfinite(peaks)) or np.any(peaks < 0):
        raise ValueError("sound peaks must be finite and >= 0")
    if L and (cells.min() < 0 or cells.max() >= gs):
        raise ValueError(f"a sound location lies outside the {gs} x {gs} grid")
    op, _, k1 = as_device(offsets, np.int64, stream)
    cp, _, k2 = as_device(cells, np.int32, stream)
    pp, _, k3 = as_device(peaks, np.float32, stream)
    field, mm = DeviceArray((gs, gs), np.float32), DeviceArray((2,), np.float32)
    _lib.check(lib.avl_field_sound(op, cp, L, pp, S, int(gs), decay, field.ptr, mm.ptr, stream), "avl_field_sound")
    _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")
    return GoalField(field, mm)


def field_lift(gf: GoalField, grid_pos, vh, stream=None):
    """avlmap.py:97 + 100-109 (area) / :132 + 135-144 (sound): heat[i] = f32(normalised field[row_i, col_i]), 0 for voxels outside
    the (gs, gs, vh) grid.  grid_pos (N, 3) int32 host or device (VLMap._device_pos()) -> (N,) float32 DeviceArray."""
    lib = _lib.load()
    gp, gshape, keep = as_device(grid_pos, np.int32, stream)
    N = int(gshape[0])
    heat = DeviceArray((N,), np.float32)
    _lib.check(lib.avl_field_lift(gf.field.ptr, int(gf.is_f64), gf.minmax.ptr, int(gf.gs), int(vh), gp, N, heat.ptr, stream),
               "avl_field_lift")
    if isinstance(grid_pos, np.ndarray):
        _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")
    return heat


def field_normalize(gf: GoalField, stream=None):
    """(field - min) / (max - min) over the whole grid, in the field's precision -> (gs, gs) DeviceArray"""
    lib = _lib.load()
    out = DeviceArray((gf.gs, gf.gs), gf.field.dtype)
    _lib.check(lib.avl_field_normalize(gf.field.ptr, int(gf.is_f64), gf.minmax.ptr, int(gf.gs), out.ptr, stream), "avl_field_normalize")
    return out


def planar_decay(grid_pos, row, col, decay_rate=0.01, stream=None):
    """avlmap.py:154-161: clip(1 - decay * ||grid_pos[:, :2] - (row, col)||, 0, 1) in float64 -> (N,) float64 DeviceArray"""
    lib = _lib.load()
    _lib.require_gpu()
    gp, gshape, keep = as_device(grid_pos, np.int32, stream)
    N = int(gshape[0])
    sim = DeviceArray((N,), np.float64)
    _lib.check(lib.avl_planar_decay(gp, N, int(row), int(col), float(decay_rate), sim.ptr, stream), "avl_planar_decay")
    if isinstance(grid_pos, np.ndarray):
        _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")
    return sim


# ---------------------------------------------------------------------------------------- cross-modal goals
GOAL_DENSE_F32, GOAL_DENSE_F64, GOAL_FIELD_F32, GOAL_FIELD_F64, GOAL_CONES = 0, 1, 2, 3, 4
GOAL_MAX_TERMS = 8


class _GoalTermC(C.Structure):
    """avl_goal_term of include/avlmaps_hip.h"""
    _fields_ = [("kind", C.c_int32), ("gs", C.c_int32), ("vh", C.c_int32), ("reserved", C.c_int32), ("d_data", C.c_void_p),
                ("d_aux", C.c_void_p), ("n_points", C.c_int64), ("decay", C.c_double)]


class GoalTerm:
    """One factor of a fused goal (csrc/avl_goal.hip): build it with dense(), field() or cones().  `n` is the number of voxels a
    dense term covers (None for the other kinds); `keep` holds the device buffers the term points into."""

    def __init__(self, kind, data=0, aux=0, gs=0, vh=0, n_points=0, decay=0.0, n=None, keep=()):
        self.kind, self.data, self.aux, self.gs, self.vh = int(kind), data, aux, int(gs), int(vh)
        self.n_points, self.decay, self.n, self.keep = int(n_points), float(decay), n, keep

    @classmethod
    def dense(cls, heat, stream=None):
        """an (N,) float32 or float64 heat: a device array (DeviceArray, torch CUDA tensor) is used in place, a host array is
        uploaded in its own type (anything but float32 / float64 is converted to float64 first)"""
        if isinstance(heat, (DeviceArray, DeviceView)):
            dt = heat.dtype
        elif _is_torch(heat):
            dt = np.dtype(str(heat.dtype).split(".")[-1])
        else:
            heat = np.asarray(heat)
            dt = heat.dtype if heat.dtype in (np.float32, np.float64) else np.dtype(np.float64)
        if dt not in (np.float32, np.float64):
            raise TypeError(f"a dense goal term is float32 or float64, got {dt}")
        ptr, shape, keep = as_device(heat, dt, stream)
        if len(shape) != 1:
            raise ValueError(f"a dense goal term is an (N,) vector, got shape {tuple(shape)}")
        return cls(GOAL_DENSE_F64 if dt == np.float64 else GOAL_DENSE_F32, data=ptr, n=int(shape[0]), keep=(keep,))

    @classmethod
    def field(cls, gf: "GoalField", vh):
        """the lift of a GoalField (area_field / sound_field) to the voxels of a (gs, gs, vh) grid: field_lift's value"""
        vh = int(vh)
        if vh < 0:
            raise ValueError(f"vh must be >= 0, got {vh}")
        return cls(GOAL_FIELD_F64 if gf.is_f64 else GOAL_FIELD_F32, data=gf.field.ptr, aux=gf.minmax.ptr, gs=gf.gs, vh=vh, keep=(gf,))

    @classmethod
    def cones(cls, cells, peaks, decay_rate, stream=None):
        """max over the points of clip(peak - decay_rate * ||(row, col) - cell||, 0, 1): cells (P, 2) int32, peaks (P,) float64
        finite, P >= 1 (host or device arrays).  One point with peak 1 is planar_decay."""
        decay = _check_decay(decay_rate)
        if not _is_dev(peaks):
            peaks = np.ascontiguousarray(peaks, dtype=np.float64).reshape(-1)
            if not np.all(np.isfinite(peaks)):
                raise ValueError("cone peaks must be finite")
        if not _is_dev(cells):
            cells = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 2)
        P = int(peaks.shape[0])
        if P < 1 or tuple(cells.shape) != (P, 2):
            raise ValueError(f"cones need P >= 1 points: cells (P, 2) and peaks (P,), got {tuple(cells.shape)} and {tuple(peaks.shape)}")
        cp, _, k1 = as_device(cells, np.int32, stream)
        pp, _, k2 = as_device(peaks, np.float64, stream)
        return cls(GOAL_CONES, data=cp, aux=pp, n_points=P, decay=decay, keep=(k1, k2))

    def _c(self):
        return _GoalTermC(self.kind, self.gs, self.vh, 0, self.data or None, self.aux or None, self.n_points, self.decay)


class GoalResult:
    """goal_fuse's result: heat (N,) float64 DeviceArray or None, index of the first maximum, the product there, grid_pos there"""
    __slots__ = ("heat", "index", "value", "pos")

    def __init__(self, heat, index, value, pos):
        self.heat, self.index, self.value, self.pos = heat, index, value, pos


def goal_terms_array(terms):
    """the C array of avl_goal_term that avl_goal_fuse reads (host side only)"""
    terms = list(terms)
    if not 1 <= len(terms) <= GOAL_MAX_TERMS:
        raise ValueError(f"a goal is the product of 1 to {GOAL_MAX_TERMS} terms, got {len(terms)}")
    return (_GoalTermC * len(terms))(*[t._c() for t in terms])


def goal_fuse(terms, grid_pos, want_heat=True, stream=None) -> GoalResult:
    """habitat_lang_robot.py:377-430: heat = ((t0 * t1) * t2) ... in float64 over the voxels, and the first voxel of its maximum
    (np.argmax), in one pass (csrc/avl_goal.hip).  terms: 1 to 8 GoalTerms, multiplied in the order given; grid_pos (N, 3) int32
    host or device.  Only index / value / pos come back to the host; want_heat=False stores nothing of size N."""
    lib = _lib.load()
    arr = goal_terms_array(terms)
    _lib.require_gpu()
    gp, gshape, keep = as_device(grid_pos, np.int32, stream)
    if len(gshape) != 2 or gshape[1] != 3:
        raise ValueError(f"grid_pos must be (N, 3), got {tuple(gshape)}")
    N = int(gshape[0])
    for t in terms:
        if t.n is not None and t.n != N:
            raise ValueError(f"a dense term has {t.n} values, the map {N} voxels")
    if N == 0:
        raise ValueError("an empty map has no goal")
    heat = DeviceArray((N,), np.float64) if want_heat else None
    idx, val = C.c_int64(), C.c_double()
    pos = np.empty((3,), dtype=np.int32)
    _lib.check(lib.avl_goal_fuse(arr, len(arr), gp, N, heat.ptr if want_heat else None, C.byref(idx), C.byref(val), pos.ctypes.data,
                                 stream), "avl_goal_fuse")
    return GoalResult(heat, int(idx.value), float(val.value), pos)
