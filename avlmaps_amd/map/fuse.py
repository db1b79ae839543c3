"""One map out of two sessions: VLMap.resample and VLMap.fuse (ops/mapfuse.py, csrc/avl_mapfuse.hip; the backward
resampling: ops/mappull.py, csrc/avl_mappull.hip).  Upstream has no counterpart: a revisit can only be folded in there by building one map from both
recordings."""
from __future__ import annotations

import numpy as np

from .changes import check_comparable, MapChanges, _map_dims


def fuse_masks(changes: MapChanges, drop_vanished: bool = True, replace_changed: bool = True):
    """(use_a, use_b) bool masks over the voxels of map A and map B from a MapChanges: A's vanished voxels leave (drop_vanished), A's
    voxels whose content was replaced give way to B's (replace_changed); of B only the voxels that A's session never looked at
    (unseen_b) stay out"""
    if not isinstance(changes, MapChanges):
        raise TypeError(f"fuse: changes is a {type(changes).__name__}, expected a MapChanges (VLMap.compare)")
    leave = np.zeros(len(changes.pos_a), dtype=bool)
    if drop_vanished:
        leave |= changes.vanished
    if replace_changed:
        leave |= changes.changed_a
    return ~leave, ~changes.unseen_b


def _arrays(vm, who):
    """(grid_pos int32, grid_feat float32, weight float32, grid_rgb uint8 or zeros, whether the map holds colours)"""
    n = len(vm.grid_pos)
    if vm.weight is None or len(vm.weight) != n:
        raise ValueError(f"{who}: the map holds no weight per voxel")
    rgb = vm.grid_rgb
    has_rgb = rgb is not None
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(n, 3) if has_rgb else np.zeros((n, 3), np.uint8)
    return (np.ascontiguousarray(vm.grid_pos, dtype=np.int32).reshape(n, 3), np.ascontiguousarray(vm.grid_feat, dtype=np.float32),
            np.ascontiguousarray(vm.weight, dtype=np.float32).reshape(n), rgb, has_rgb)


def _shift_tuple(shift):
    return tuple(int(s) for s in np.asarray(shift).reshape(-1))


RESAMPLE_METHODS = ("forward", "nearest", "linear")


def resample_map(vm, transform=None, shift=(0, 0, 0), method="forward", min_support=0.5):
    """VLMap.resample: see there"""
    from .. import ops
    if method not in RESAMPLE_METHODS:
        raise ValueError(f"resample: method {method!r} (one of {', '.join(RESAMPLE_METHODS)})")
    ops.check_min_support(min_support, "resample")
    dims = _map_dims(vm, "this map")
    pos, feat, weight, rgb, has_rgb = _arrays(vm, "resample")
    D = dims["D"]
    if method == "forward":
        res = ops.fuse_maps(np.zeros((0, 3), np.int32), np.zeros((0, D), np.float32), np.zeros((0,), np.float32), np.zeros((0, 3), np.uint8),
                            pos, feat, weight, rgb, dims["gs"], dims["cs"], dims["vh"], transform=transform, shift=shift)
    else:
        res = ops.pull_map(pos, feat, weight, rgb, dims["gs"], dims["cs"], dims["vh"], transform=transform, shift=shift, interp=method,
                           min_support=min_support)
    out = type(vm)(vm.map_config, data_dir=str(getattr(vm, "data_dir", "") or ""))
    out.prefetch_device, out.compact_map = vm.prefetch_device, vm.compact_map
    out.grid_pos, out.grid_feat, out.weight, out.occupied_ids = res.grid_pos, res.grid_feat, res.weight, res.occupied_ids
    out.grid_rgb = res.grid_rgb if has_rgb else None
    out.mapped_iter_list = None if vm.mapped_iter_list is None else list(vm.mapped_iter_list)
    out.categories = None if vm.categories is None else list(vm.categories)
    out.resample_counts = dict(res.counts)
    return out


def fuse_into(vm, other, transform=None, shift=(0, 0, 0), changes=None, drop_vanished=True, replace_changed=True, gain=1.0) -> dict:
    """VLMap.fuse: see there"""
    from .. import ops
    da, db = _map_dims(vm, "this map"), _map_dims(other, "the other map")
    check_comparable(da, db)
    T = ops.check_transform(transform, "fuse")
    gain = ops.check_gain(gain, "fuse")
    shift = _shift_tuple(shift)
    if len(shift) != 3:
        raise ValueError(f"fuse: shift is three whole cells (row, col, h), got {shift!r}")
    use_a = use_b = None
    if changes is not None:
        use_a, use_b = fuse_masks(changes, drop_vanished, replace_changed)
        if T is not None:
            raise ValueError("fuse: changes are those of two maps on one grid; resample the other map first (other.resample(transform)), "
                             "compare against that and fuse it with transform=None")
        if _shift_tuple(changes.params["shift"]) != shift:
            raise ValueError(f"fuse: the changes were found under shift {tuple(changes.params['shift'])}, the fusion asks for {shift}")
        if len(use_a) != len(vm.grid_pos) or len(use_b) != len(other.grid_pos):
            raise ValueError(f"fuse: the changes are of {len(use_a)} and {len(use_b)} voxels, the maps hold {len(vm.grid_pos)} and "
                             f"{len(other.grid_pos)}")
    pos_a, feat_a, w_a, rgb_a, has_a = _arrays(vm, "fuse")
    pos_b, feat_b, w_b, rgb_b, has_b = _arrays(other, "fuse")
    # compare's convention: A's cell c corresponds to B's cell c + shift, so B's cells come over by -shift
    res = ops.fuse_maps(pos_a, feat_a, w_a, rgb_a, pos_b, feat_b, w_b, rgb_b, da["gs"], da["cs"], da["vh"], transform=T,
                        shift=tuple(-s for s in shift), use_a=use_a, use_b=use_b, gain_a=1.0, gain_b=gain)
    with vm._dev_lock:
        vm.grid_pos, vm.grid_feat, vm.weight, vm.occupied_ids = res.grid_pos, res.grid_feat, res.weight, res.occupied_ids
        vm.grid_rgb = res.grid_rgb if (has_a or has_b) else None
        vm.scores_mat = None
        vm._drop_derived()
    out = dict(res.counts)
    out.update(voxels_a=len(pos_a), voxels_b=len(pos_b), voxels=int(res.n_out))
    return out
