#!/usr/bin/env python3
"""G12: the spatial-relation goals of the reference's Map (avlmaps/map/map.py:243-485), EXECUTED on prepared islands.

Run:  python tools/gen_golden_relations.py        (needs the reference checkout, see tools/ref_import.py; never runs on the GPU box)
Writes tests/golden/g12_relations.npz: arrays only -- the islands of two categories per scene, the (position, heading) cases and
what every reference method returned for them, None / "stop" / a raised error encoded as flags.  Map.get_pos is replaced by a
function that hands out the prepared islands; everything else is the reference's own code, imported from where it lies.

Scenes
  0  rectangles around a robot at (60, 80) + the crop offset: boxes with extent area exactly 50 (dropped by filter_small_objects'
     default threshold) and 51 (kept), an object exactly behind the robot at heading 0, objects in all four quadrants, a two-pixel
     island.  The lists are bottom-up, so at heading 0 the front objects are the LAST entries: get_pos_in_between's use of front
     indices on the full centre lists picks other objects' centres.
  1  category a empty: every "nothing in front" convention, and get_delta_angle_to's error on an empty list.
  2  irregular islands (unions of random rectangles) in both categories.
Cases: headings in all four quadrants, +-90, +-180 and beyond +-180 (the wrap-around branches of select_front_objs), from two
robot positions per scene.
"""
import contextlib
import importlib.util
import io
import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
from ref_import import REF_ROOT, import_reference  # noqa: E402

OUT = HERE.parent / "tests" / "golden"
SHAPE = (120, 160)
RMIN, CMIN = 37, 21
HEADINGS = [0.0, 45.0, 135.0, -45.0, -135.0, 90.0, -90.0, 180.0, -180.0, 30.0, 200.0, -200.0]
COMPASS = ("north", "south", "west", "east")


def rect_mask(rects):
    m = np.zeros(SHAPE, np.uint8)
    for r0, r1, c0, c1 in rects:
        m[r0:r1 + 1, c0:c1 + 1] = 1
    return m


def islands_of(mask):
    """(contours, centers, boxes) as VLMap.get_pos returns them: the project's host island step plus the crop offset"""
    from avlmaps_amd.utils.navigation_utils import get_segment_islands_pos
    contours, centers, boxes, _ = get_segment_islands_pos(mask, 1)
    for k in range(len(contours)):
        contours[k] = contours[k] + np.array([RMIN, CMIN])
        centers[k] = [centers[k][0] + RMIN, centers[k][1] + CMIN]
        boxes[k] = [boxes[k][0] + RMIN, boxes[k][1] + RMIN, boxes[k][2] + CMIN, boxes[k][3] + CMIN]
    return contours, centers, boxes


def scenes(rng):
    a0 = rect_mask([(10, 15, 75, 85), (20, 23, 100, 117), (58, 62, 120, 140), (100, 110, 78, 82), (55, 70, 10, 30), (40, 40, 40, 41)])
    b0 = rect_mask([(30, 40, 60, 70), (80, 95, 100, 120), (50, 52, 150, 158), (5, 8, 5, 30)])

    def blobs(count):
        rects = []
        for _ in range(count):
            r0, c0 = int(rng.integers(2, SHAPE[0] - 30)), int(rng.integers(2, SHAPE[1] - 30))
            rects.append((r0, r0 + int(rng.integers(1, 22)), c0, c0 + int(rng.integers(1, 22))))
        return rect_mask(rects)
    return [dict(a=a0, b=b0, robots=[(60.0 + RMIN, 80.0 + CMIN), (20.5 + RMIN, 33.25 + CMIN)]),
            dict(a=np.zeros(SHAPE, np.uint8), b=b0, robots=[(60.0 + RMIN, 80.0 + CMIN), (20.5 + RMIN, 33.25 + CMIN)]),
            dict(a=blobs(14), b=blobs(12), robots=[(50.0 + RMIN, 70.0 + CMIN), (101.5 + RMIN, 12.0 + CMIN)])]


def pack(contours):
    lengths = np.array([len(c) for c in contours], np.int64)
    points = np.concatenate(contours).astype(np.int64) if contours else np.zeros((0, 2), np.int64)
    return points, lengths


def main():
    rng = np.random.default_rng(1212)
    all_scenes = scenes(rng)
    for sc in all_scenes:                               # before import_reference: it replaces cv2 by a stub the host step would pick up
        sc["islands"] = {k: islands_of(sc[k]) for k in "ab"}
    m = import_reference()
    spec = importlib.util.spec_from_file_location("ref_navigation_utils", os.path.join(REF_ROOT, "avlmaps", "utils", "navigation_utils.py"))
    nav = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(nav)
    m["map"].get_dist_to_bbox_2d = nav.get_dist_to_bbox_2d
    Map = m["map"].Map
    out = dict(rmin=np.int64(RMIN), cmin=np.int64(CMIN), compass=np.array(COMPASS))
    sink = io.StringIO()
    out["n_scenes"] = np.int64(len(all_scenes))
    for s, sc in enumerate(all_scenes):
        isl = sc["islands"]
        ref = object.__new__(Map)
        ref.rmin, ref.cmin = RMIN, CMIN
        ref.get_pos = lambda name, isl=isl: tuple(list(x) for x in isl[name])
        for k in "ab":
            pts, lens = pack(isl[k][0])
            out[f"s{s}_{k}_points"], out[f"s{s}_{k}_lengths"] = pts, lens
            out[f"s{s}_{k}_centers"] = np.array(isl[k][1], np.float64).reshape(-1, 2)
            out[f"s{s}_{k}_boxes"] = np.array(isl[k][2], np.int64).reshape(-1, 4)
        cases = [(p, h) for p in sc["robots"] for h in (HEADINGS if p == sc["robots"][0] else HEADINGS[:6])]
        n = len(cases)
        na = len(isl["a"][1])
        r = dict(pos=np.zeros((n, 2)), heading=np.zeros(n), front=np.zeros((n, na), bool),
                 nearest_none=np.zeros(n, bool), nearest=np.zeros((n, 2)),
                 box_none=np.zeros(n, bool), box_center=np.zeros((n, 2)), box=np.zeros((n, 4), np.int64),
                 left_none=np.zeros(n, bool), left=np.zeros((n, 2)), right_none=np.zeros(n, bool), right=np.zeros((n, 2)),
                 between_none=np.zeros(n, bool), between=np.zeros((n, 2)),
                 delta_error=np.zeros(n, bool), delta=np.zeros(n),
                 compass_stop=np.zeros((n, 4), bool), compass=np.zeros((n, 4, 2)),
                 side_left=np.zeros((n, na, 2)), side_right=np.zeros((n, na, 2)))
        with contextlib.redirect_stdout(sink), np.errstate(all="ignore"):
            for c, (pos, h) in enumerate(cases):
                pos = list(pos)
                r["pos"][c], r["heading"][c] = pos, h
                r["front"][c, ref.select_front_objs(isl["a"][1], pos, h)] = True
                v = ref.get_front_nearest_obj_pos(pos, h, "a")
                r["nearest_none"][c] = v is None
                if v is not None:
                    r["nearest"][c] = v
                cen, box = ref.get_front_nearest_obj_pos_box(pos, h, "a")
                r["box_none"][c] = cen is None
                if cen is not None:
                    r["box_center"][c], r["box"][c] = cen, box
                for key, fn in (("left", ref.get_left_pos), ("right", ref.get_right_pos)):
                    v = fn(pos, h, "a")
                    r[key + "_none"][c] = v[0] is None
                    if v[0] is not None:
                        r[key][c] = v
                v = ref.get_pos_in_between(pos, h, "a", "b")
                r["between_none"][c] = v is None
                if v is not None:
                    r["between"][c] = v
                try:
                    r["delta"][c] = ref.get_delta_angle_to(pos, h, "a")
                except ValueError:
                    r["delta_error"][c] = True
                for q, name in enumerate(COMPASS):
                    v = getattr(ref, f"get_{name}_pos")(pos, h, "a")
                    r["compass_stop"][c, q] = v == ["stop"]
                    if v != ["stop"]:
                        r["compass"][c, q] = v
                for k in range(na):
                    r["side_left"][c, k] = ref._get_left_pos(pos, isl["a"][1][k], isl["a"][2][k])
                    r["side_right"][c, k] = ref._get_right_pos(pos, isl["a"][1][k], isl["a"][2][k])
            # the contour midpoint for every pair of the first few islands
            pa, pb = isl["a"][0][:4], isl["b"][0][:4]
            mid = np.zeros((len(pa), len(pb), 2))
            for i, ca in enumerate(pa):
                for j, cb in enumerate(pb):
                    mid[i, j] = ref.find_middle_bewteen_contours(ca, cb)
            out[f"s{s}_middle"] = mid
        for key, v in r.items():
            out[f"s{s}_{key}"] = v
    OUT.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT / "g12_relations.npz", **out)
    print("wrote", OUT / "g12_relations.npz", (OUT / "g12_relations.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
