"""The 3-D heat of a voxel mask and its per-map plan (csrc/avl_heat.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from ..device import DeviceArray, as_device, _is_torch

_HOST_PLANS = []          # [(weakref to the host array, fingerprint, HeatPlan)]: most recent first, at most two maps


def _fingerprint(a: np.ndarray) -> int:
    """hash of the WHOLE array (a fingerprint of sampled rows misses an in-place edit elsewhere and the stale cell order
    gives a silently wrong heat).  xxh3 runs at ~10 GB/s (2 ms for a 2 M-voxel map's 24 MB); zlib.crc32 is the fall-back."""
    buf = memoryview(a).cast("B")
    try:
        import xxhash
        return xxhash.xxh3_64_intdigest(buf)
    except ImportError:
        import zlib
        return zlib.crc32(buf)


def _host_heat_plan(grid_pos: np.ndarray, stream=None):
    """HeatPlan for a HOST position array that is passed again and again (upstream's AVLMap.index_object and the navigator hand
    the map's grid_pos to get_heatmap_from_mask_3d on every query): kept per array object, checked against a hash of ALL of
    its contents so that an array edited in place gets a new plan.  Only for arrays that reach the library unchanged (int32,
    C-contiguous): a converted temporary is a new object on every call and would build -- and keep alive -- a plan per query.
    None if the map cannot have one."""
    import weakref
    fp = (len(grid_pos), grid_pos.__array_interface__["data"][0], _fingerprint(grid_pos))
    for k, (ref, f, plan) in enumerate(_HOST_PLANS):
        if ref() is grid_pos and f == fp:
            if k:
                _HOST_PLANS.insert(0, _HOST_PLANS.pop(k))
            return plan
    stale = [e for e in _HOST_PLANS if e[0]() is None or e[0]() is grid_pos]
    _HOST_PLANS[:] = [e for e in _HOST_PLANS if e[0]() is not None and e[0]() is not grid_pos]
    for _, _, old in stale:                    # the array died or was edited in place: its plan's device buffers go now
        if old is not None:
            old.close()
    plan = HeatPlan.for_positions(DeviceArray.from_numpy(grid_pos), stream)
    try:
        _HOST_PLANS.insert(0, (weakref.ref(grid_pos), fp, plan))
    except TypeError:
        return plan
    for _, _, old in _HOST_PLANS[2:]:
        if old is not None:
            old.close()
    del _HOST_PLANS[2:]
    return plan


def heatmap_from_mask(grid_pos, mask, cell_size=0.05, decay_rate=0.01, stream=None, reuse_plan=False):
    """visualize_utils.py:29-49 on the GPU.  grid_pos (N,3) int32, mask (N,) bool/uint8 -> (N,) float32.
    reuse_plan (host grid_pos only, int32 and C-contiguous, i.e. the SAME array object on every call): keep the map's positions
    and their cell order on the device between calls (HeatPlan) -- the second query on the same array uploads the mask alone and
    runs the 3-4x faster planned kernel; same bits.  The whole array is hashed per call (~2 ms at 2 M voxels), so an in-place
    edit gets a fresh plan; VLMap / AVLMap.index_object hold their own plan and skip the hash."""
    lib = _lib.load()
    _lib.require_gpu()
    if (reuse_plan and isinstance(grid_pos, np.ndarray) and grid_pos.ndim == 2 and len(grid_pos) > 0 and grid_pos.dtype == np.int32
            and grid_pos.flags.c_contiguous):
        plan = _host_heat_plan(grid_pos, stream)
        if plan is not None:
            return plan(np.asarray(mask), cell_size, decay_rate, stream).numpy(stream)
    if _is_torch(mask):
        import torch
        if mask.dtype == torch.bool:
            mask = mask.to(torch.uint8)
    elif isinstance(mask, np.ndarray):
        mask = mask.astype(np.uint8)
    pp, pshape, k1 = as_device(grid_pos, np.int32, stream)
    mp, mshape, k2 = as_device(mask, np.uint8, stream)
    N = pshape[0]
    if _is_torch(grid_pos):
        import torch
        heat = torch.empty((N,), dtype=torch.float32, device=grid_pos.device)
        _lib.check(lib.avl_heatmap_from_mask(pp, mp, N, float(cell_size), float(decay_rate), heat.data_ptr(), stream),
                   "avl_heatmap_from_mask")
        return heat
    heat = DeviceArray((N,), np.float32)
    _lib.check(lib.avl_heatmap_from_mask(pp, mp, N, float(cell_size), float(decay_rate), heat.ptr, stream),
               "avl_heatmap_from_mask")
    return heat.numpy(stream) if isinstance(grid_pos, np.ndarray) else heat


class HeatPlan:
    """The part of heatmap_from_mask that depends on the voxel positions only, kept for a map that is queried repeatedly
    (avl_heat_plan: bounding box, voxels in cell order, zeroed grid buffers).  plan(mask, cell_size, decay_rate) returns the same
    bits as heatmap_from_mask(grid_pos, mask, ...), ~3x sooner.  grid_pos: DeviceArray or CUDA tensor (N,3) int32, kept alive here.
    HeatPlan.for_positions returns None when the map's bounding box is too large for a plan (>= 2^32 cells)."""

    def __init__(self, grid_pos, stream=None):
        lib = _lib.load()
        _lib.require_gpu()
        if isinstance(grid_pos, np.ndarray):
            grid_pos = DeviceArray.from_numpy(np.ascontiguousarray(grid_pos, dtype=np.int32))
        pp, pshape, self._keep = as_device(grid_pos, np.int32, stream)
        self.grid_pos, self.N = grid_pos, int(pshape[0])
        self._torch = _is_torch(grid_pos)
        h = C.c_void_p()
        _lib.check(lib.avl_heat_plan_create(C.byref(h), pp, self.N, stream), "avl_heat_plan_create")
        self._h, self._lib = h, lib

    @classmethod
    def for_positions(cls, grid_pos, stream=None):
        try:
            return cls(grid_pos, stream)
        except _lib.AvlError as e:
            if "2^32" in str(e):
                return None
            raise

    def __call__(self, mask, cell_size=0.05, decay_rate=0.01, stream=None):
        if self._h is None:
            raise RuntimeError("HeatPlan used after close()")
        if _is_torch(mask):
            import torch
            if mask.dtype == torch.bool:
                mask = mask.to(torch.uint8)
        elif isinstance(mask, np.ndarray):
            mask = mask.astype(np.uint8)
        mp, mshape, keep = as_device(mask, np.uint8, stream)
        if int(np.prod(mshape)) != self.N:
            raise ValueError(f"mask has {int(np.prod(mshape))} entries, the plan {self.N} voxels")
        if self._torch:
            import torch
            heat = torch.empty((self.N,), dtype=torch.float32, device=self.grid_pos.device)
            hp = heat.data_ptr()
        else:
            heat = DeviceArray((self.N,), np.float32)
            hp = heat.ptr
        _lib.check(self._lib.avl_heatmap_from_mask_planned(self._h, mp, float(cell_size), float(decay_rate), hp, stream),
                   "avl_heatmap_from_mask_planned")
        return heat

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            self._lib.avl_heat_plan_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
