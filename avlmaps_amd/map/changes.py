"""What changed between two voxel maps of one place: VLMap.compare's result and the objects among the changed voxels
(ops/mapdiff.py, csrc/avl_mapdiff.hip).  Upstream has no counterpart: its maps are static.

Map A is the earlier map (`self` of VLMap.compare), map B the later one (`other`).  A voxel of A without a voxel of B within the
radius has VANISHED; a voxel of B without one of A has APPEARED; a voxel of B whose nearest voxel of A holds a feature row with a
cosine below the threshold has CHANGED (a chair swapped for a plant in the same cells).  With a visibility audit of a map made from
the OTHER session's frames, an unmatched voxel that session never looked at is UNSEEN instead: nothing is known about it."""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

import numpy as np

KINDS = ("vanished", "appeared", "changed", "moved")
_SIDE = {"vanished": "a", "unseen": "a", "changed_a": "a", "appeared": "b", "changed": "b", "unseen_b": "b"}
_MASKS = tuple(_SIDE)
MOVED_MAX_RATIO = 2.0


class Change(NamedTuple):
    """One object-sized change (MapChanges.objects), in full-map cells.  kind: "vanished" (bbox, center on map A), "appeared",
    "changed" (on map B) or "moved" (where it is now, on map B; from_* where it was, on map A).  bbox: (rmin, rmax, cmin, cmax,
    hmin, hmax), inclusive; center: the mean cell of its voxels; mean_cosine: the mean cosine of a changed component's voxels
    against their matches, NaN for the other kinds; category / name: the voted category of its voxels (-1 / "" when the maps hold
    no scores of one category list)."""
    kind: str
    count: int
    bbox: Tuple[int, int, int, int, int, int]
    center: Tuple[float, float, float]
    mean_cosine: float = float("nan")
    category: int = -1
    name: str = ""
    from_count: Optional[int] = None
    from_bbox: Optional[Tuple[int, int, int, int, int, int]] = None
    from_center: Optional[Tuple[float, float, float]] = None

    def to_json(self) -> dict:
        d = {k: (list(v) if isinstance(v, tuple) else v) for k, v in self._asdict().items() if v is not None}
        if d["mean_cosine"] != d["mean_cosine"]:
            del d["mean_cosine"]
        return d


def pair_moved(vanished: List[Change], appeared: List[Change], max_ratio: float = MOVED_MAX_RATIO):
    """Host pairing of vanished and appeared components into moves: a pair qualifies when both carry the same voted category
    (>= 0) and the larger voxel count is at most max_ratio times the smaller; qualifying pairs are taken nearest centres first
    (ties: the earlier vanished, then the earlier appeared component), each component at most once.  Returns (moved, the vanished
    left over, the appeared left over), the left-overs in their input order."""
    cand = []
    for i, v in enumerate(vanished):
        for j, a in enumerate(appeared):
            if v.category >= 0 and v.category == a.category and max(v.count, a.count) <= max_ratio * min(v.count, a.count):
                d2 = sum((float(x) - float(y)) ** 2 for x, y in zip(v.center, a.center))
                cand.append((d2, i, j))
    cand.sort()
    used_v, used_a, moved = set(), set(), []
    for _, i, j in cand:
        if i in used_v or j in used_a:
            continue
        used_v.add(i)
        used_a.add(j)
        v, a = vanished[i], appeared[j]
        moved.append(Change("moved", a.count, a.bbox, a.center, float("nan"), a.category, a.name, v.count, v.bbox, v.center))
    return (moved, [v for i, v in enumerate(vanished) if i not in used_v], [a for j, a in enumerate(appeared) if j not in used_a])


def check_comparable(a: dict, b: dict) -> None:
    """ValueError unless two maps' (gs, cs, vh, D) agree: the comparison is cell by cell and row by row"""
    for key, what in (("gs", "grid sizes"), ("cs", "cell sizes"), ("vh", "height cells"), ("D", "feature widths")):
        if a[key] != b[key]:
            raise ValueError(f"compare: the maps' {what} differ ({a[key]} and {b[key]}); whole-cell shifts of one grid are all that is compared")


class MapChanges:
    """VLMap.compare's result.  Bool masks: vanished, unseen, changed_a over map A's voxels; appeared, changed, unseen_b over map
    B's.  cosine_a / cosine_b: (N,) float64, a voxel's cosine against its match, NaN where unmatched.  pos_a / pos_b: the maps'
    cells; params: gs, cs, vh, radius, threshold, shift, min_rays.  scores_a / scores_b / categories: the maps' scores_mat when both
    hold one of the same category list (not saved: a loaded MapChanges lists its objects without categories)."""

    def __init__(self, pos_a, pos_b, masks: dict, cosine_a, cosine_b, params: dict, scores_a=None, scores_b=None, categories=None):
        self.pos_a = np.ascontiguousarray(pos_a, dtype=np.int32).reshape(-1, 3)
        self.pos_b = np.ascontiguousarray(pos_b, dtype=np.int32).reshape(-1, 3)
        n = {"a": len(self.pos_a), "b": len(self.pos_b)}
        for name in _MASKS:
            m = np.ascontiguousarray(masks[name], dtype=bool)
            if m.shape != (n[_SIDE[name]],):
                raise ValueError(f"MapChanges: {name} has shape {m.shape}, map {_SIDE[name].upper()} {n[_SIDE[name]]} voxels")
            setattr(self, name, m)
        self.cosine_a = np.ascontiguousarray(cosine_a, dtype=np.float64)
        self.cosine_b = np.ascontiguousarray(cosine_b, dtype=np.float64)
        if self.cosine_a.shape != (n["a"],) or self.cosine_b.shape != (n["b"],):
            raise ValueError("MapChanges: one cosine per voxel")
        self.params = dict(params)
        self.scores_a, self.scores_b, self.categories = scores_a, scores_b, categories

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_diff(cls, diff, pos_a, pos_b, params, **kw) -> "MapChanges":
        """from an ops.MapDiff with host arrays"""
        from .. import ops
        sa, sb = np.asarray(diff.a.status), np.asarray(diff.b.status)
        masks = dict(vanished=sa == ops.DIFF_NO_MATCH, unseen=sa == ops.DIFF_UNSEEN, changed_a=sa == ops.DIFF_CHANGED,
                     appeared=sb == ops.DIFF_NO_MATCH, unseen_b=sb == ops.DIFF_UNSEEN, changed=sb == ops.DIFF_CHANGED)
        return cls(pos_a, pos_b, masks, diff.a.cosine, diff.b.cosine, params, **kw)

    # ------------------------------------------------------------------ queries
    def mask(self, kinds, side: str = None) -> np.ndarray:
        """the union of the masks named in `kinds`, which must lie over one map's voxels (`side`: "a" / "b" when given)"""
        kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
        if not kinds or any(k not in _SIDE for k in kinds):
            raise ValueError(f"kinds {kinds!r}: one or more of {_MASKS}")
        sides = {_SIDE[k] for k in kinds}
        if len(sides) != 1 or (side is not None and sides != {side}):
            raise ValueError(f"kinds {kinds!r} lie over different maps' voxels: vanished / unseen / changed_a are map A's, "
                             "appeared / changed / unseen_b map B's")
        out = np.zeros_like(getattr(self, kinds[0]))
        for k in kinds:
            out |= getattr(self, k)
        return out

    def summary(self) -> dict:
        """counts of every mask, the voxels of both maps, and the changed volume in m^3: the cells that vanished, appeared or
        changed (a changed cell counted once, on map B), times cs^3"""
        cs = float(self.params["cs"])
        out = {"voxels_a": int(len(self.pos_a)), "voxels_b": int(len(self.pos_b))}
        out.update({name: int(np.count_nonzero(getattr(self, name))) for name in _MASKS})
        out["changed_volume_m3"] = (out["vanished"] + out["appeared"] + out["changed"]) * cs ** 3
        return out

    def objects(self, min_voxels: int = 20, connectivity: int = 26) -> List[Change]:
        """The object-sized changes: the connected components (ops.label_voxels, connectivity 6 / 18 / 26) of the vanished voxels
        on map A's list and of the appeared and of the changed voxels on map B's list with at least min_voxels voxels, each with
        its box, centre and -- changed only -- mean cosine.  When both maps hold a scores_mat of one category list every component
        also carries the voted category of its voxels (ops.pool_rows, ops.vote_rows), and a vanished and an appeared component of
        one category and similar size become one "moved" change (pair_moved).  Order: moved, vanished, appeared, changed; label
        order within each."""
        from .. import ops
        voted = self.scores_a is not None and self.scores_b is not None and self.categories is not None
        lists = {}
        for kind, pos, mask, scores, cosine in (("vanished", self.pos_a, self.vanished, self.scores_a, None),
                                                ("appeared", self.pos_b, self.appeared, self.scores_b, None),
                                                ("changed", self.pos_b, self.changed, self.scores_b, self.cosine_b)):
            lists[kind] = []
            if not mask.any():
                continue
            with ops.label_voxels(pos, mask, connectivity=connectivity, device=True) as inst:
                table = inst.table
                category = None
                if voted and inst.n:
                    sums = ops.pool_rows(scores, inst.labels_dev, inst.n)
                    category = ops.vote_rows(sums / table[:, 0:1].astype(np.float64))[0]
                mean_cos = None
                if cosine is not None and inst.n:
                    labels = inst.labels_dev.numpy()
                    mean_cos = np.bincount(labels, weights=np.where(labels > 0, np.nan_to_num(cosine), 0.0), minlength=inst.n + 1)[1:] \
                        / table[:, 0].astype(np.float64)
                for k in range(inst.n):
                    row = [int(v) for v in table[k]]
                    if row[0] < int(min_voxels):
                        continue
                    cat = -1 if category is None else int(category[k])
                    lists[kind].append(Change(kind, row[0], tuple(row[1:7]), tuple(float(s) / row[0] for s in row[7:10]),
                                              float("nan") if mean_cos is None else float(mean_cos[k]), cat,
                                              "" if cat < 0 else str(self.categories[cat])))
        moved, vanished, appeared = pair_moved(lists["vanished"], lists["appeared"])
        return moved + vanished + appeared + lists["changed"]

    # ------------------------------------------------------------------ file
    def save(self, path) -> None:
        p = self.params
        np.savez_compressed(path, pos_a=self.pos_a, pos_b=self.pos_b, cosine_a=self.cosine_a, cosine_b=self.cosine_b,
                            shift=np.asarray(p["shift"], np.int64), **{name: getattr(self, name) for name in _MASKS},
                            **{k: v for k, v in p.items() if k != "shift"})

    @classmethod
    def load(cls, path) -> "MapChanges":
        arrays = ("pos_a", "pos_b", "cosine_a", "cosine_b", "shift") + _MASKS
        with np.load(path, allow_pickle=False) as z:
            params = {k: z[k].item() for k in z.files if k not in arrays}
            params["shift"] = tuple(int(s) for s in z["shift"])
            return cls(z["pos_a"], z["pos_b"], {name: z[name] for name in _MASKS}, z["cosine_a"], z["cosine_b"], params)


def _map_dims(vm, who):
    if vm.grid_pos is None or vm.grid_feat is None or vm.occupied_ids is None:
        raise ValueError(f"compare: {who} has no map loaded")
    return dict(gs=int(vm.gs), cs=float(vm.cs), vh=int(np.asarray(vm.occupied_ids).shape[2]), D=int(np.asarray(vm.grid_feat).shape[1]))


def _through(audit, n, who):
    """a VisibilityAudit's ray counts as the int32 the status kernel compares (a count past 2^31 - 1 saturates)"""
    if audit is None:
        return None
    if audit.N != n:
        raise ValueError(f"compare: {who} is of {audit.N} voxels, the map has {n}")
    return np.minimum(audit.through, np.uint32(2 ** 31 - 1)).astype(np.int32)


def compare_maps(a, b, radius=1, threshold=0.8, shift=(0, 0, 0), audit=None, other_audit=None, min_rays=3) -> MapChanges:
    """VLMap.compare(a, b, ...): see there"""
    from .. import ops
    da, db = _map_dims(a, "this map"), _map_dims(b, "the other map")
    check_comparable(da, db)
    pos_a = np.ascontiguousarray(a.grid_pos, dtype=np.int32)
    pos_b = np.ascontiguousarray(b.grid_pos, dtype=np.int32)
    through_a = _through(audit, len(pos_a), "audit")
    through_b = _through(other_audit, len(pos_b), "other_audit")
    diff = ops.map_diff(pos_a, np.ascontiguousarray(a.grid_feat, dtype=np.float32), pos_b, np.ascontiguousarray(b.grid_feat, dtype=np.float32),
                        da["gs"], da["vh"], radius=radius, threshold=threshold, shift=shift, through_a=through_a, through_b=through_b,
                        min_rays=min_rays)
    params = dict(gs=da["gs"], cs=da["cs"], vh=da["vh"], radius=diff.radius, threshold=diff.threshold, shift=diff.shift, min_rays=diff.min_rays)
    kw = {}
    sa, sb, ca, cb = getattr(a, "scores_mat", None), getattr(b, "scores_mat", None), getattr(a, "categories", None), getattr(b, "categories", None)
    if sa is not None and sb is not None and ca is not None and list(ca) == list(cb or ()) and np.shape(sa)[1:] == np.shape(sb)[1:] \
            and len(sa) == len(pos_a) and len(sb) == len(pos_b):
        Q = int(np.shape(sa)[1])
        names = list(ca)[:Q] + ["other"] * (Q - len(ca))       # the "other" column that init_categories appends
        kw = dict(scores_a=np.ascontiguousarray(sa, dtype=np.float32), scores_b=np.ascontiguousarray(sb, dtype=np.float32), categories=names)
    return MapChanges.from_diff(diff, pos_a, pos_b, params, **kw)
