"""Rooms: what Map.get_rooms returns -- the room segmentation of the obstacle crop (ops.segment_rooms) with its
crop window, read in full-map coordinates.  Upstream has no counterpart: its "kitchen" is a CLIP score per camera pose."""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np


def room_parameters(door_width: float, min_core_area: float, cs: float):
    """-> (radius in cells, min_seed_cells): radius = door_width / (2 cs), min_seed_cells = ceil(min_core_area / cs^2), at least 1"""
    door_width, min_core_area, cs = float(door_width), float(min_core_area), float(cs)
    if not (np.isfinite(cs) and cs > 0.0):
        raise ValueError(f"cell size {cs} m (finite and > 0)")
    if not (np.isfinite(door_width) and door_width >= 0.0):
        raise ValueError(f"door_width {door_width} m (finite and >= 0)")
    if not (np.isfinite(min_core_area) and min_core_area >= 0.0):
        raise ValueError(f"min_core_area {min_core_area} m^2 (finite and >= 0)")
    return door_width / (2.0 * cs), max(int(math.ceil(min_core_area / (cs * cs))), 1)


class Rooms:
    """n rooms of an (h, w) crop whose cell (0, 0) is full-map cell window = (rmin, cmin).  labels (h, w) int32: 0 = obstacle or a
    free cell no room reaches, 1 .. n; room_table (n, 10) and door_table (D, 10) int64 as ops.segment_rooms returns them, in crop
    coordinates; clearance (h, w) float64: the distance transform of the free map, in cells; cs: the cell size in metres; params:
    door_width, min_core_area, radius, min_seed_cells.  Positions taken and returned by the methods are full-map (row, col)."""

    def __init__(self, labels, room_table, door_table, clearance, window, cs, params=None, field=None):
        self.labels = np.ascontiguousarray(labels, dtype=np.int32)
        self.room_table = np.asarray(room_table, dtype=np.int64).reshape(-1, 10)
        self.door_table = np.asarray(door_table, dtype=np.int64).reshape(-1, 10)
        self.clearance = None if clearance is None else np.asarray(clearance, dtype=np.float64)
        self.window = (int(window[0]), int(window[1]))
        self.cs, self.params, self.field = float(cs), dict(params or {}), field
        if self.labels.ndim != 2:
            raise ValueError(f"Rooms: labels of shape {self.labels.shape} (expected 2-D)")

    @property
    def n(self) -> int:
        return int(self.room_table.shape[0])

    @property
    def shape(self):
        return self.labels.shape

    def _check(self, k) -> int:
        k = int(k)
        if not 1 <= k <= self.n:
            raise ValueError(f"room {k}: the map has rooms 1 .. {self.n}")
        return k

    def room_of(self, pos) -> int:
        """the room of the cell of full-map position pos = (row, col) (its int() cell); 0 on an obstacle, on a free cell no room
        reaches and outside the crop"""
        r, c = int(pos[0]) - self.window[0], int(pos[1]) - self.window[1]
        h, w = self.labels.shape
        return int(self.labels[r, c]) if 0 <= r < h and 0 <= c < w else 0

    def centre(self, k) -> List[int]:
        """the room's cell farthest from every obstacle (the first in raster order among equals): the "go to this room" goal"""
        row = self.room_table[self._check(k) - 1]
        return [int(row[8]) + self.window[0], int(row[9]) + self.window[1]]

    def mask(self, k, gs: Optional[int] = None) -> np.ndarray:
        """bool mask of room k: over the crop, or over the (gs, gs) full map when gs is given"""
        m = self.labels == self._check(k)
        if gs is None:
            return m
        full = np.zeros((int(gs), int(gs)), dtype=bool)
        h, w = m.shape
        full[self.window[0]:self.window[0] + h, self.window[1]:self.window[1] + w] = m
        return full

    def area_m2(self, k) -> float:
        return float(self.room_table[self._check(k) - 1, 0]) * self.cs * self.cs

    @property
    def doors(self) -> np.ndarray:
        """the door table with its rows and columns moved into the full map: i, j, contacts, rmin, rmax, cmin, cmax, door row,
        door col, 0"""
        d = self.door_table.copy()
        d[:, [3, 4, 7]] += self.window[0]
        d[:, [5, 6, 8]] += self.window[1]
        return d

    def door(self, a, b) -> Optional[List[int]]:
        """the door cell between rooms a and b, None when they do not touch"""
        i, j = sorted((self._check(a), self._check(b)))
        for row in self.door_table:
            if (int(row[0]), int(row[1])) == (i, j):
                return [int(row[7]) + self.window[0], int(row[8]) + self.window[1]]
        return None

    def neighbours(self, k) -> List[int]:
        """the rooms that touch room k, ascending"""
        k = self._check(k)
        out = {int(j) for i, j in self.door_table[:, :2] if i == k} | {int(i) for i, j in self.door_table[:, :2] if j == k}
        return sorted(out)

    def route(self, a, b) -> Optional[List[int]]:
        """the room sequence from a to b through the fewest doors: a breadth-first search on the host that visits neighbours in
        ascending id; [a] when a == b, None when the rooms are not connected"""
        a, b = self._check(a), self._check(b)
        prev, queue, head = {a: 0}, [a], 0
        while head < len(queue):
            k = queue[head]
            head += 1
            if k == b:
                out = []
                while k:
                    out.append(k)
                    k = prev[k]
                return out[::-1]
            for m in self.neighbours(k):
                if m not in prev:
                    prev[m] = k
                    queue.append(m)
        return None

    def save(self, path) -> None:
        np.savez_compressed(path, labels=self.labels, room_table=self.room_table, door_table=self.door_table,
                            clearance=self.clearance if self.clearance is not None else np.zeros((0, 0)),
                            window=np.asarray(self.window, np.int64), cs=np.float64(self.cs),
                            **{f"param_{k}": np.float64(v) for k, v in self.params.items()})

    @classmethod
    def load(cls, path) -> "Rooms":
        with np.load(path, allow_pickle=False) as z:
            params = {k[len("param_"):]: z[k].item() for k in z.files if k.startswith("param_")}
            clearance = z["clearance"] if z["clearance"].size else None
            return cls(z["labels"], z["room_table"], z["door_table"], clearance, z["window"].tolist(), z["cs"].item(), params)


def majority_room(counts) -> np.ndarray:
    """counts (n, K + 1): per object the number of its voxels in no room (column 0) and in rooms 1 .. K.  -> (n,) int32: the room
    with the most voxels, the smallest id among equals, 0 when no voxel lies in a room"""
    counts = np.asarray(counts)
    if counts.ndim != 2 or counts.shape[1] < 1:
        raise ValueError(f"majority_room: counts of shape {counts.shape}")
    out = np.zeros(counts.shape[0], dtype=np.int32)
    if counts.shape[1] > 1 and counts.shape[0]:
        inside = counts[:, 1:]
        best = np.argmax(inside, axis=1)                       # the first maximum: the smallest room id
        has = inside[np.arange(len(inside)), best] > 0
        out[has] = best[has].astype(np.int32) + 1
    return out
