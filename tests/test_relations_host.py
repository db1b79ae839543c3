"""Map's spatial-relation goals (map.py:243-485 upstream) against g12_relations.npz: what the reference's own methods returned on
prepared islands (tools/gen_golden_relations.py).  CPU only: get_pos hands out the fixture's islands and ops.contour_nearest_pair is
replaced by its NumPy definition.

Everything is compared with array_equal: the methods are the same NumPy float64 expressions as upstream's.  That includes the values
that pass through arctan2 / sin / cos: the reference run that wrote the fixture and this mirror agree bit for bit where the fixture
was generated, so no margin for libm versions that differ in the last ulp (1e-12 would be the one) is taken."""
import numpy as np
import pytest

COMPASS = ("north", "south", "west", "east")


def numpy_nearest_pair(a, b, stream=None):
    a, b = np.asarray(a), np.asarray(b)
    d = np.linalg.norm(a.reshape((-1, 1, 2)) - b.reshape((1, -1, 2)), axis=2)
    i, j = np.unravel_index(np.argmin(d), d.shape)
    return int(i), int(j), int(((a[i] - b[j]) ** 2).sum())


def islands(g, s, k):
    lengths = g[f"s{s}_{k}_lengths"]
    ends = np.cumsum(lengths)
    pts = g[f"s{s}_{k}_points"]
    contours = [pts[e - n:e].copy() for e, n in zip(ends, lengths)]
    centers = [[c[0], c[1]] for c in g[f"s{s}_{k}_centers"]]
    boxes = [[b[0], b[1], b[2], b[3]] for b in g[f"s{s}_{k}_boxes"]]
    return contours, centers, boxes


@pytest.fixture(scope="module")
def scenes(golden):
    from avlmaps_amd.map.map import Map
    g = golden("g12_relations.npz")
    out = []
    for s in range(int(g["n_scenes"])):
        isl = {k: islands(g, s, k) for k in "ab"}
        m = object.__new__(Map)
        m.rmin, m.cmin = int(g["rmin"]), int(g["cmin"])
        m.get_pos = lambda name, isl=isl: tuple(list(x) for x in isl[name])
        out.append((s, m, isl, {k[len(f"s{s}_"):]: g[k] for k in g.files if k.startswith(f"s{s}_")}))
    return out


@pytest.fixture(autouse=True)
def host_nearest_pair(monkeypatch):
    from avlmaps_amd import ops
    monkeypatch.setattr(ops, "contour_nearest_pair", numpy_nearest_pair)


def cases(r):
    return [(c, list(r["pos"][c]), float(r["heading"][c])) for c in range(len(r["heading"]))]


def test_fixture_covers_what_it_should(scenes):
    """the cases the fixture exists for are in it: every branch answer, both sides of the area threshold, an empty list"""
    _, m, isl, r = scenes[0]
    areas = [(b[1] - b[0]) * (b[3] - b[2]) for b in isl["a"][2]]
    assert 50 in areas and 51 in areas
    assert r["box_none"].any() and not r["box_none"].all()
    assert r["between_none"].any() and not r["between_none"].all()
    assert {0.0, 45.0, 135.0, -45.0, -135.0, 90.0, -90.0, 180.0, -180.0} <= set(r["heading"].tolist())
    behind = [c for c in isl["a"][1] if c[1] == r["pos"][0][1] and c[0] > r["pos"][0][0]]
    assert behind and r["heading"][0] == 0.0                   # an object exactly behind the first case's robot
    assert len(scenes[1][2]["a"][1]) == 0 and scenes[1][3]["delta_error"].all()


def test_select_front_objs_and_nearest(scenes):
    for s, m, isl, r in scenes:
        for c, pos, h in cases(r):
            front = np.zeros(len(isl["a"][1]), bool)
            front[m.select_front_objs(isl["a"][1], pos, h)] = True
            assert np.array_equal(front, r["front"][c]), (s, c)
            v = m.get_front_nearest_obj_pos(pos, h, "a")
            assert (v is None) == bool(r["nearest_none"][c]), (s, c)
            if v is not None:
                assert np.array_equal(v, r["nearest"][c]), (s, c)
            cen, box = m.get_front_nearest_obj_pos_box(pos, h, "a")
            assert (cen is None) == (box is None) == bool(r["box_none"][c]), (s, c)
            if cen is not None:
                assert np.array_equal(cen, r["box_center"][c]) and np.array_equal(box, r["box"][c]), (s, c)


def test_left_right(scenes):
    for s, m, isl, r in scenes:
        for c, pos, h in cases(r):
            for key, fn, side in (("left", m.get_left_pos, m._get_left_pos), ("right", m.get_right_pos, m._get_right_pos)):
                v = fn(pos, h, "a")
                if r[key + "_none"][c]:
                    assert v == [None, None], (s, c, key)
                else:
                    assert np.array_equal(v, r[key][c]), (s, c, key)
                for k in range(len(isl["a"][1])):
                    assert np.array_equal(side(pos, isl["a"][1][k], isl["a"][2][k]), r["side_" + key][c, k]), (s, c, key, k)


def test_left_is_two_cells_farther_out_than_right(scenes):
    """upstream's left distance is half the box diagonal + 2 (the value that overwrites its first estimate), the right one half
    the diagonal: about the target's centre the two points are opposite and their distances differ by exactly that margin"""
    _, m, isl, r = scenes[0]
    pos = list(r["pos"][0])
    for cen, box in zip(isl["a"][1], isl["a"][2]):
        left, right = np.array(m._get_left_pos(pos, cen, box)), np.array(m._get_right_pos(pos, cen, box))
        half = 0.5 * np.hypot(box[1] - box[0], box[3] - box[2])
        assert abs(np.linalg.norm(left - cen) - (half + 2)) < 1e-9 and abs(np.linalg.norm(right - cen) - half) < 1e-9


def test_in_between_and_contour_middle(scenes):
    for s, m, isl, r in scenes:
        for c, pos, h in cases(r):
            v = m.get_pos_in_between(pos, h, "a", "b")
            assert (v is None) == bool(r["between_none"][c]), (s, c)
            if v is not None:
                assert np.array_equal(v, r["between"][c]), (s, c)
        mid = r["middle"]
        for i in range(mid.shape[0]):
            for j in range(mid.shape[1]):
                assert np.array_equal(m.find_middle_bewteen_contours(isl["a"][0][i], isl["b"][0][j]), mid[i, j]), (s, i, j)


def test_in_between_keeps_the_index_mix_up(scenes):
    """the surviving FRONT indices select centres from the FULL lists upstream: at least one case of the fixture must differ from
    what front centres would give, or the fixture would not pin the convention"""
    differs = 0
    for s, m, isl, r in scenes:
        for c, pos, h in cases(r):
            if r["between_none"][c]:
                continue
            fa, fb = m.select_front_objs(isl["a"][1], pos, h), m.select_front_objs(isl["b"][1], pos, h)
            ka = m.filter_small_objects([isl["a"][2][i] for i in fa])
            kb = m.filter_small_objects([isl["b"][2][i] for i in fb])
            ca = np.array([isl["a"][1][fa[i]] for i in ka]).reshape((-1, 1, 2))
            cb = np.array([isl["b"][1][fb[i]] for i in kb]).reshape((1, -1, 2))
            d = np.linalg.norm((ca + cb) / 2 - np.array(pos).reshape((1, 1, 2)), axis=-1)
            row, col = np.unravel_index(np.argmin(d), d.shape)
            fixed = m.find_middle_bewteen_contours(isl["a"][0][fa[ka[row]]], isl["b"][0][fb[kb[col]]])
            differs += not np.array_equal(fixed, r["between"][c])
    assert differs > 0


def test_delta_angle_and_compass(scenes):
    for s, m, isl, r in scenes:
        for c, pos, h in cases(r):
            if r["delta_error"][c]:
                with pytest.raises(ValueError):
                    m.get_delta_angle_to(pos, h, "a")
            else:
                assert m.get_delta_angle_to(pos, h, "a") == r["delta"][c], (s, c)
            for q, name in enumerate(COMPASS):
                v = getattr(m, f"get_{name}_pos")(pos, h, "a")
                if r["compass_stop"][c, q]:
                    assert v == ["stop"], (s, c, name)
                else:
                    assert np.array_equal(np.asarray(v, np.float64), r["compass"][c, q]), (s, c, name)
