"""SceneObjects: what VLMap.get_objects returns -- every object of every category of a map, with the score rows of its voxels pooled.
Upstream has no counterpart: vlmap_3d.py:75-100 and habitat_lang_robot.py:242-265 stop at one category's voxel mask."""
from __future__ import annotations

import json
from typing import List

import numpy as np


class SceneObjects:
    """voxel_objects: the ops.VoxelObjects of the labelling (labels on the device, table, best_score, classes_of; closed with
    close()); names: the Q column names of scores_mat; mean_scores (n, Q) float64 = the pooled sums / count; voted (n,) int32: the
    first maximum of every row of mean_scores; margin (n,) float64: its largest value minus the second largest, inf for Q = 1;
    objects: the ops.Object3D of the objects with at least min_voxels voxels, in label order, with their scene-wide labels."""

    def __init__(self, voxel_objects, mean_scores, argmax, names, min_voxels=50, connectivity=26, exclude=()):
        from .. import ops
        self.voxel_objects, self.names = voxel_objects, [str(s) for s in names]
        self.mean_scores = np.asarray(mean_scores, np.float64).reshape(voxel_objects.n, len(self.names))
        self.min_voxels, self.connectivity, self.exclude = int(min_voxels), int(connectivity), tuple(exclude)
        self._argmax, self._labels = argmax, None
        self.positions, self.rooms = None, None         # the (N, 3) cells of the voxels (VLMap.get_objects sets them); assign_rooms' result
        self.voted, self.margin = ops.vote_rows(self.mean_scores)
        table, best, classes = voxel_objects.table, voxel_objects.best_score, voxel_objects.classes_of
        self.objects: List[ops.Object3D] = [
            ops.Object3D.from_row(k + 1, table[k], best[k], classes[k], self.mean_scores[k], self.names)
            for k in range(voxel_objects.n) if table[k, 0] >= self.min_voxels]

    @property
    def n(self) -> int:
        """all objects of the labelling, listed or not"""
        return self.voxel_objects.n

    def _host_labels(self) -> np.ndarray:
        if self._labels is None:                         # copied back once
            lab = self.voxel_objects.labels
            self._labels = lab if isinstance(lab, np.ndarray) else lab.numpy(self.voxel_objects.stream)
        return self._labels

    def vote_labels(self) -> np.ndarray:
        """(N,) int32: the row argmax of every voxel, with the voxels of every LISTED object replaced by that object's voted
        category -- a chair with a few "table" voxels on its seat is those voxels' objects too, so only objects of min_voxels or
        more re-vote, and a small island inside a large object keeps its own argmax.  Host NumPy on the labels."""
        labels = self._host_labels()
        out = np.array(self._argmax, dtype=np.int32, copy=True)
        if out.shape != labels.shape:
            raise ValueError(f"the argmax has shape {out.shape}, the labels {labels.shape}")
        vote_of = np.full(self.n + 1, -1, np.int32)
        for it in self.objects:
            vote_of[it.label] = it.voted
        v = vote_of[labels]
        out[v >= 0] = v[v >= 0]
        return out

    def assign_rooms(self, rooms, positions=None) -> np.ndarray:
        """(len(objects),) int32: per listed object the room that holds most of its voxels -- the smallest room id among equals,
        0 when no voxel of the object lies in a room.  rooms: Map.get_rooms' result.  The voxels' rooms are ops.lift_labels_2d of
        the rooms' labels on `positions` ((N, 3) cells, by default those VLMap.get_objects left here); the votes are one
        ops.label_confusion over the object labels and the voxels' rooms.  Kept as self.rooms for in_room."""
        from .. import ops
        from .rooms import majority_room
        positions = self.positions if positions is None else positions
        if positions is None:
            raise ValueError("assign_rooms: no voxel positions (pass positions=vlmap.grid_pos)")
        vo = self.voxel_objects
        voxel_room = ops.lift_labels_2d(rooms.labels, positions, rooms.window, device=True)
        labels = vo.labels_dev if getattr(vo, "labels_dev", None) is not None else self._host_labels()
        conf, _ = ops.label_confusion(labels, voxel_room, self.n + 1, rooms.n + 1)
        listed = np.array([it.label for it in self.objects], dtype=np.int64)
        self.rooms = majority_room(conf[listed].astype(np.int64)) if len(listed) else np.zeros((0,), np.int32)
        return self.rooms

    def in_room(self, k) -> list:
        """the listed objects of room k (0: those in no room), in label order; assign_rooms must have run"""
        if self.rooms is None:
            raise ValueError("in_room: call assign_rooms(rooms) first")
        return [it for it, room in zip(self.objects, self.rooms) if int(room) == int(k)]

    def to_json(self) -> str:
        """the listed objects as JSON text; objects_from_json reads them back.  A margin of inf (Q = 1) is written as null"""
        doc = dict(categories=self.names, min_voxels=self.min_voxels, connectivity=self.connectivity, exclude=list(self.exclude),
                   n_objects=self.n, objects=[_object_dict(it) for it in self.objects])
        return json.dumps(doc, indent=1)

    def save(self, path) -> None:
        with open(path, "w") as f:
            f.write(self.to_json())

    def close(self) -> None:
        self.voxel_objects.close()


def _object_dict(it) -> dict:
    d = it._asdict()
    d["bbox"], d["center"], d["cell"] = list(it.bbox), list(it.center), list(it.cell)
    d["margin"] = None if np.isinf(it.margin) else it.margin
    return d


def objects_from_json(text: str):
    """the ops.Object3D list of SceneObjects.to_json's text, equal to SceneObjects.objects field by field"""
    from .. import ops
    out = []
    for d in json.loads(text)["objects"]:
        d = dict(d, bbox=tuple(d["bbox"]), center=tuple(d["center"]), cell=tuple(d["cell"]),
                 margin=float("inf") if d["margin"] is None else d["margin"])
        out.append(ops.Object3D(**d))
    return out
