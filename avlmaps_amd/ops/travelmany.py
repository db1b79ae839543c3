"""K travel-distance fields on one free map in one batch, the set-to-set arrivals read from their planes, and the sound field that
decays around walls (csrc/avl_travel_many.hip).  Upstream has no counterpart."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from ..device import DeviceArray, DeviceView, as_device
from ._args import _image_u8
from .fields import _check_decay, GoalField
from .travel import _field_front, _host_window, TravelField

TRAVEL_MANY_MAX_FIELDS = 1024    # kManyMaxFields
TRAVEL_MANY_MAX_PAIRS = 1 << 28  # kManyMaxPairs: (field, tile) pairs of one batch


class _PlaneView(DeviceView):
    """one (H, W) plane of a (K, H, W) DeviceArray that `owner` keeps alive; numpy() copies it to the host"""
    __slots__ = ("owner",)

    def __init__(self, owner, k, shape, dtype):
        super().__init__(owner.ptr + k * int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize, shape, dtype)
        self.owner = owner

    def numpy(self, stream=None):
        out = np.empty(self.shape, dtype=self.dtype)
        _lib.check(_lib.load().avl_memcpy_d2h(out.ctypes.data, self.ptr, self.nbytes, stream), "avl_memcpy_d2h")
        return out


def _csr_sets(what, offsets, cells, H, W):
    """host CSR sets checked against an (H, W) map -> (offsets int64 (K + 1,), cells int32 (L, 2)); ValueError otherwise"""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    c = np.asarray(cells)
    if c.size and c.dtype.kind not in "iu":
        raise ValueError(f"{what}: cells must be integers, got {c.dtype}")
    cells = np.ascontiguousarray(c, dtype=np.int32).reshape(-1, 2)
    K, L = len(offsets) - 1, len(cells)
    if K < 1 or offsets[0] != 0 or offsets[-1] != L or np.any(np.diff(offsets) < 1):
        raise ValueError(f"{what}: offsets must be (K + 1,) CSR offsets from 0 to len(cells) = {L}, every set with one cell or more")
    if cells.min() < 0 or cells[:, 0].max() >= H or cells[:, 1].max() >= W:
        raise ValueError(f"{what}: a cell lies outside the {H} x {W} map")
    return offsets, cells


def _sets_to_device(offsets, cells, stream):
    """one upload for both: (K + 1) int64 offsets, then the (L, 2) int32 cells -> (offsets pointer, cells pointer, keepalive)"""
    packed = np.empty(len(offsets) + len(cells), dtype=np.int64)
    packed[:len(offsets)] = offsets
    packed[len(offsets):].view(np.int32)[:] = cells.ravel()
    d = DeviceArray.from_numpy(packed, stream)
    return d.ptr, d.ptr + 8 * len(offsets), d


class TravelFields:
    """travel_fields' result.  straight, diagonal: (K, H, W) int32 host arrays or DeviceArrays, field k the TravelField planes of
    set k; reached (K,) int64: the reached cells of each field.  rounds, tile_runs: how many rounds had an active (field, tile) pair
    and how many pairs ran in all -- information about the schedule, not part of the result."""

    def __init__(self, straight, diagonal, shape, reached, rounds, tile_runs, free, free_dev, stream=None):
        self.straight, self.diagonal, self.shape = straight, diagonal, tuple(shape)
        self.K = int(straight.shape[0])
        self.reached, self.rounds, self.tile_runs = np.asarray(reached, dtype=np.int64), int(rounds), int(tile_runs)
        self._free, self._free_dev, self._stream, self._host = free, free_dev, stream, None

    def planes(self):
        """(straight, diagonal) as (K, H, W) host arrays (device planes are copied once and kept)"""
        if self._host is None:
            if isinstance(self.straight, np.ndarray):
                self._host = (self.straight, self.diagonal)
            else:
                self._host = (self.straight.numpy(self._stream), self.diagonal.numpy(self._stream))
        return self._host

    def _free_host(self):
        f = self._free() if callable(self._free) else self._free
        self._free = f
        return f

    def field(self, k) -> TravelField:
        """field k as a TravelField that travel_decay_2d and descend take as they are (views of this batch's planes, no copy)"""
        k = int(k)
        if not 0 <= k < self.K:
            raise IndexError(f"field {k} of {self.K}")
        if isinstance(self.straight, np.ndarray):
            a, b = self.straight[k], self.diagonal[k]
        else:
            a, b = _PlaneView(self.straight, k, self.shape, np.int32), _PlaneView(self.diagonal, k, self.shape, np.int32)
        f = TravelField(a, b, self.shape, self.reached[k], self.rounds, self.tile_runs, self._free_host, self._stream)
        if self._host is not None:
            f._host = (self._host[0][k], self._host[1][k])
        return f


def travel_fields(free, offsets, cells, device=False, stream=None, window=None) -> TravelFields:
    """K travel-distance fields of DESIGN.md 4.26 on one free map in one batch: field k is travel_field(free,
    cells[offsets[k]:offsets[k + 1]]), byte for byte.  free: 2-D bool / uint8 / numeric image, nonzero = free, host or device.
    offsets (K + 1,) and cells (L, 2) integer (row, col): host arrays, CSR from 0 to L, every set with one cell or more; a set may
    repeat a cell and its cells may lie on obstacles.  window=(r0, r1, c0, c1): work on free[r0:r1, c0:c1] without copying; cells are
    then relative to the window.  -> TravelFields with host planes, or with DeviceArrays (device=True).  ValueError for bad CSR
    offsets, an empty set, and a cell outside the map or the window; more than TRAVEL_MANY_MAX_FIELDS sets or a side above
    TRAVEL_MAX_SIDE raise AvlError before any device work.  The call synchronises the stream."""
    lib = _lib.load()
    free, shape, win, _ = _field_front("travel_fields", free, window)
    H, W = win[1] - win[0], win[3] - win[2]
    off = win[0] * shape[1] + win[2]
    offsets, cells = _csr_sets("travel_fields", offsets, cells, H, W)
    K, L = len(offsets) - 1, len(cells)
    if K > TRAVEL_MANY_MAX_FIELDS:
        raise _lib.AvlError(f"travel_fields: {K} sets (1 .. {TRAVEL_MANY_MAX_FIELDS})")
    one = C.c_size_t(0)
    _lib.check(lib.avl_travel2d_workspace_bytes(H, W, C.byref(one)), "avl_travel2d_many")
    _lib.require_gpu()
    nws = K * one.value
    ws = DeviceArray((nws,), np.uint8)
    fp, _, fkeep = _image_u8(free, stream)
    op, cp, k1 = _sets_to_device(offsets, cells, stream)
    straight, diagonal = DeviceArray((K, H, W), np.int32), DeviceArray((K, H, W), np.int32)
    stats = DeviceArray((2 + K,), np.int64)
    _lib.check(lib.avl_travel2d_many(fp + off, shape[1], H, W, op, cp, K, L, straight.ptr, diagonal.ptr, stats.ptr, ws.ptr,
                                     nws, stream), "avl_travel2d_many")
    st = stats.numpy(stream)

    def free_host():
        return _host_window(free, fkeep, stream, win) != 0

    if not device:                                   # (device: the stream is drained, nothing queued still reads the inputs or the workspace)
        straight, diagonal = straight.numpy(stream), diagonal.numpy(stream)
    return TravelFields(straight, diagonal, (H, W), st[2:], st[0], st[1], free_host, (fkeep, fp + off, shape[1]), stream)


class TravelArrivals:
    """travel_arrivals' result, (K, M) int32 host arrays: a, b the pair of field k's arrival at target set j; cell the index into the
    target cells of the first cell in CSR order that attains it; from_ (also under the key "from" of as_dict()) the index in
    TRAVEL_NEIGHBOURS of the neighbour the arrival steps from, the first among ties, -1 when the target cell is a source of the
    field.  -1 in all four where no walk arrives."""

    def __init__(self, a, b, cell, from_):
        self.a, self.b, self.cell, self.from_ = a, b, cell, from_

    def __getitem__(self, key):
        return self.as_dict()[key]

    def as_dict(self):
        return {"a": self.a, "b": self.b, "cell": self.cell, "from": self.from_}

    def length(self) -> np.ndarray:
        """(K, M) float64: float64(a) + float64(b) * sqrt(2), inf where unreachable"""
        d = self.a.astype(np.float64) + self.b.astype(np.float64) * np.sqrt(2.0)
        d[self.a < 0] = np.inf
        return d


def travel_arrivals(fields: TravelFields, offsets, cells, stream=None) -> TravelArrivals:
    """The arrivals of every field of `fields` at M target sets (host CSR offsets (M + 1,) and cells (L, 2), checked like
    travel_fields').  For a target cell t, arrive_k(t) is (0, 0) when t is a source of field k, else the exact minimum over the
    eight neighbours u of t of pair_k(u) + step(u -> t) over the reached u for which, on a diagonal step, both cells that share an
    edge with u and t are free; t itself need not be free, which mirrors "a source may lie on an obstacle" and makes the matrix of a
    family of sets symmetric.  A set's arrival is the minimum over its cells, the first in CSR order among ties."""
    lib = _lib.load()
    H, W = fields.shape
    offsets, cells = _csr_sets("travel_arrivals", offsets, cells, H, W)
    M, L = len(offsets) - 1, len(cells)
    if M > TRAVEL_MANY_MAX_FIELDS:
        raise _lib.AvlError(f"travel_arrivals: {M} target sets (1 .. {TRAVEL_MANY_MAX_FIELDS})")
    _lib.require_gpu()
    stream = fields._stream if stream is None else stream
    K = fields.K
    ap, _, k1 = as_device(fields.straight, np.int32, stream)
    bp, _, k2 = as_device(fields.diagonal, np.int32, stream)
    fkeep, fptr, fld = fields._free_dev
    op, cp, k3 = _sets_to_device(offsets, cells, stream)
    out = [DeviceArray((K, M), np.int32) for _ in range(4)]
    _lib.check(lib.avl_travel_arrive(fptr, fld, H, W, ap, bp, K, op, cp, M, L, out[0].ptr, out[1].ptr, out[2].ptr, out[3].ptr, stream),
               "avl_travel_arrive")
    return TravelArrivals(*[o.numpy(stream) for o in out])


def sound_travel_field(free, offsets, cells, peaks, decay_rate, chunk=64, window=None, stream=None) -> GoalField:
    """sound_field with the travel distance: for every segment in order the float64 term max(p - (p * d) * decay, 0),
    d = the travel distance to the nearest of the segment's locations (0 where no walk ends), added into a float32 field of the
    free map's (or the window's) shape.  offsets (S + 1,), cells (L, 2), peaks (S,) float32 >= 0: host arrays.  Segments go through
    in chunks of at most `chunk` fields, each one travel_fields call and one accumulate call; the result does not depend on
    `chunk`.  Segments with peak 0 add exactly +0 and are skipped.  -> GoalField, field (H, W) float32 and its [min, max]."""
    lib = _lib.load()
    decay = _check_decay(decay_rate)
    _, _, win, _ = _field_front("sound_travel_field", free, window)
    H, W = win[1] - win[0], win[3] - win[2]
    peaks = np.ascontiguousarray(peaks, dtype=np.float32).reshape(-1)
    offsets, cells = _csr_sets("sound_travel_field", offsets, cells, H, W)
    if len(offsets) - 1 != len(peaks):
        raise ValueError(f"sound_travel_field: {len(offsets) - 1} segments and {len(peaks)} peaks")
    if not np.all(np.isfinite(peaks)) or np.any(peaks < 0):
        raise ValueError("sound peaks must be finite and >= 0")
    chunk = int(chunk)
    if not 1 <= chunk <= TRAVEL_MANY_MAX_FIELDS:
        raise ValueError(f"chunk must be 1 .. {TRAVEL_MANY_MAX_FIELDS}, got {chunk}")
    _lib.require_gpu()
    if isinstance(free, np.ndarray):                 # uploaded once for all chunks
        fdev = DeviceArray.from_numpy(np.ascontiguousarray(free != 0).view(np.uint8), stream)
    else:
        fdev = free
    field, mm = DeviceArray((H, W), np.float32), DeviceArray((2,), np.float32)
    field.zero_(stream)
    mm.zero_(stream)
    live = np.flatnonzero(peaks != 0)
    for at in range(0, len(live), chunk):
        seg = live[at:at + chunk]
        sizes = offsets[seg + 1] - offsets[seg]
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        cs = np.concatenate([cells[offsets[s]:offsets[s + 1]] for s in seg])
        tf = travel_fields(fdev, offs, cs, device=True, stream=stream, window=win)
        pp, _, keep = as_device(peaks[seg], np.float32, stream)
        _lib.check(lib.avl_travel_sound2d(tf.straight.ptr, tf.diagonal.ptr, len(seg), H, W, pp, decay, int(at == 0), field.ptr, mm.ptr,
                                          stream), "avl_travel_sound2d")
        _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")      # the chunk's planes and peaks die here
    return GoalField(field, mm)


def sound_travel_normalize(gf: GoalField, stream=None):
    """(field - min) / (max - min) over the whole (H, W) field in float32, field_normalize's expression -> (H, W) DeviceArray"""
    lib = _lib.load()
    H, W = gf.field.shape
    out = DeviceArray((H, W), np.float32)
    _lib.check(lib.avl_travel_sound_normalize(gf.field.ptr, gf.minmax.ptr, H, W, out.ptr, stream), "avl_travel_sound_normalize")
    return out
