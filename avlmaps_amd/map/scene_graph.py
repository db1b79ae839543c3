"""SceneGraph: what VLMap.get_scene_graph returns -- the objects of a scene (SceneObjects) and, for every pair of them that come
within a radius of each other, the nearest gap, who rests on whom and how much they touch (ops.object_relations,
csrc/avl_relations.hip).  Upstream has no counterpart: map/map.py:183-240 relates the 2-D islands of one category's
top-down mask and needs a viewpoint for left / right; nothing there tells a mug on the table from a mug under it.

Everything here is host arithmetic on the (P, 8) integer table: every order below is an integer ranking with the labels as the last
key, so the same map gives the same lists on every run."""
from __future__ import annotations

import json
import math
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

RELATIONS = ("near", "on", "under", "touching")


class Relation(NamedTuple):
    """One pair of related objects, seen from `a`.  d2: the smallest squared cell distance between a voxel of one and a voxel of the
    other (0: they share a cell); distance = sqrt(d2) * cs in metres; voxel_a, voxel_b: the rows of the two voxels of that gap (the
    table's witness, put on the right sides); a_on_b: the voxels of a with a cell of b directly beneath them, b_on_a the converse;
    contacts: the 26-neighbour voxel pairs of the two objects, counted from both sides."""
    a: int
    b: int
    d2: int
    distance: float
    voxel_a: int
    voxel_b: int
    a_on_b: int
    b_on_a: int
    contacts: int

    def rests(self) -> bool:
        """a rests on b: at least one voxel of a lies directly on b, and more of a on b than of b on a"""
        return self.a_on_b >= 1 and self.a_on_b > self.b_on_a

    def mirrored(self) -> "Relation":
        return Relation(self.b, self.a, self.d2, self.distance, self.voxel_b, self.voxel_a, self.b_on_a, self.a_on_b, self.contacts)


class SceneGraph:
    """objects: the SceneObjects of the labelling (its `objects` are the LISTED ones, those of at least min_voxels voxels);
    relations: the ops.ObjectRelations over ALL n objects; cs: the cell size in metres; R: the radius in cells.  labels: the (N,)
    host labels the witnesses are put on their sides with (default: the SceneObjects' own, copied back once).  edges: the
    Relation (a < b) of every row of the table whose two objects are both listed, in (a, b) order."""

    def __init__(self, objects, relations, cs, R, labels=None):
        self.objects, self.relations, self.cs, self.R = objects, relations, float(cs), int(R)
        self._labels = None if labels is None else np.asarray(labels)
        self._listed = {it.label: it for it in objects.objects}
        table = np.asarray(relations.host_table()).reshape(-1, 8)
        self.edges: List[Relation] = [self._relation(row) for row in table if int(row[0]) in self._listed and int(row[1]) in self._listed]
        self._by_label = {}
        for e in self.edges:
            self._by_label.setdefault(e.a, []).append(e)
            self._by_label.setdefault(e.b, []).append(e.mirrored())

    def _host_labels(self):
        if self._labels is None:
            self._labels = self.objects._host_labels()
        return self._labels

    def _relation(self, row) -> Relation:
        lo, hi, d2, i, j, lo_on_hi, hi_on_lo, contacts = (int(v) for v in row)
        if int(self._host_labels()[i]) != lo:            # the scanning voxel of the witness belongs to hi
            i, j = j, i
        return Relation(lo, hi, d2, math.sqrt(d2) * self.cs, i, j, lo_on_hi, hi_on_lo, contacts)

    def relation(self, a, b) -> Optional[Relation]:
        """the Relation of objects a and b as seen from a; None when they are not within R cells of each other.  Any two objects
        of the labelling, listed or not."""
        row = self.relations.pair(a, b)
        if row is None:
            return None
        rel = self._relation(row)
        return rel if rel.a == int(a) else rel.mirrored()

    def neighbors(self, label) -> List[Relation]:
        """the listed objects within R cells of `label`, nearest first: by (d2, the other label)"""
        return sorted(self._by_label.get(int(label), []), key=lambda e: (e.d2, e.b))

    def rests_on(self, label) -> List[Relation]:
        """the listed objects x that `label` rests on -- label_on_x >= 1 and label_on_x > x_on_label -- most support first: by
        (-label_on_x, x)"""
        return sorted((e for e in self._by_label.get(int(label), []) if e.rests()), key=lambda e: (-e.a_on_b, e.b))

    def supports(self, label) -> List[Relation]:
        """the converse: the listed objects x that rest on `label`, by (-x_on_label, x)"""
        return sorted((e for e in self._by_label.get(int(label), []) if e.mirrored().rests()), key=lambda e: (-e.b_on_a, e.b))

    def touching(self, label) -> List[Relation]:
        """the listed objects with at least one voxel in the 26-neighbourhood of a voxel of `label`: by (-contacts, the other label)"""
        return sorted((e for e in self._by_label.get(int(label), []) if e.contacts > 0), key=lambda e: (-e.contacts, e.b))

    def find(self, subject: str, relation: str, anchor: str) -> List[Tuple[object, object, Relation]]:
        """"the mug on the table": (subject Object3D, anchor Object3D, Relation seen from the subject) for every pair of LISTED
        objects whose voted names (Object3D.voted_name, compared as lower-case strings) are `subject` and `anchor` and that stand
        in `relation`:
            "near"      within R cells of each other;                      ordered by (d2, subject label, anchor label)
            "on"        the subject rests on the anchor (rests_on's rule); by (-subject_on_anchor, subject label, anchor label)
            "under"     the anchor rests on the subject;                   by (-anchor_on_subject, subject label, anchor label)
            "touching"  contacts > 0;                                      by (-contacts, subject label, anchor label)
        An object is never related to itself.  ValueError for another relation."""
        if relation not in RELATIONS:
            raise ValueError(f"relation {relation!r}: one of {RELATIONS}")
        want_s, want_a = str(subject).strip().lower(), str(anchor).strip().lower()
        test, rank = {
            "near": (lambda e: True, lambda e: e.d2),
            "on": (lambda e: e.rests(), lambda e: -e.a_on_b),
            "under": (lambda e: e.mirrored().rests(), lambda e: -e.b_on_a),
            "touching": (lambda e: e.contacts > 0, lambda e: -e.contacts),
        }[relation]
        hits = []
        for s in self.objects.objects:
            if s.voted_name.lower() != want_s:
                continue
            for e in self._by_label.get(s.label, []):
                t = self._listed[e.b]
                if t.voted_name.lower() == want_a and test(e):
                    hits.append((rank(e), s.label, t.label, s, t, e))
        hits.sort(key=lambda h: h[:3])
        return [h[3:] for h in hits]

    def to_json(self) -> str:
        """the listed objects' labels and the edges as JSON text, a document of its own (SceneObjects.to_json has the objects);
        relations_from_json reads the edges back"""
        doc = dict(radius_cells=self.R, cell_size=self.cs, n_objects=self.objects.n, n_pairs=self.relations.P,
                   min_voxels=getattr(self.objects, "min_voxels", None), labels=sorted(self._listed),
                   names={str(k): it.voted_name for k, it in sorted(self._listed.items())}, edges=[e._asdict() for e in self.edges])
        return json.dumps(doc, indent=1)

    def save(self, path) -> None:
        with open(path, "w") as f:
            f.write(self.to_json())


def relations_from_json(text: str) -> List[Relation]:
    """the Relation list of SceneGraph.to_json's text, equal to SceneGraph.edges field by field"""
    return [Relation(**d) for d in json.loads(text)["edges"]]
