"""The voxel map under construction and its finalisation (csrc/avl_builder.hip, avl_finalize.hip, avl_replay.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from ..device import DeviceArray, as_device, _is_torch


def _global_depth(depth, stream):
    """-> (ptr, shape, keepalive, is_u16) of the depth image of the multi-floor builder: uint16 (metres = value / depth_div) or
    float32 metres, nothing else.  The kernels read one of these two; converting anything else here would round it quietly (a
    float64 image in metres, what the reference's PNG / 1000.0 is, would lose bits and move voxel ids at cell edges)."""
    if _is_torch(depth):
        dt = str(depth.dtype)
        is_u16 = dt in ("torch.uint16", "torch.int16")
        if not (is_u16 or dt == "torch.float32"):
            raise TypeError(f"depth must be uint16 (value / depth_div metres) or float32 metres, got {dt}")
        if not depth.is_cuda:
            raise TypeError("torch tensors passed to avlmaps_amd must live on the GPU")
        depth = depth.contiguous()
        return depth.data_ptr(), tuple(depth.shape), depth, is_u16
    dt = getattr(depth, "dtype", None)
    dt = np.dtype(object) if dt is None else np.dtype(dt)
    if dt not in (np.dtype(np.uint16), np.dtype(np.float32)):
        raise TypeError(f"depth must be uint16 (value / depth_div metres) or float32 metres, got {dt}")
    if dt == np.uint16:
        if isinstance(depth, np.ndarray):
            return (*as_device(depth.view(np.int16), np.int16, stream), True)
        return depth.ptr, depth.shape, depth, True           # DeviceArray / DeviceView of uint16
    return (*as_device(depth, np.float32, stream), False)


class BatchPlan:
    """resolved device-pointer tables of one batch of frames (VoxelAccumulator.make_batch_plan)"""
    __slots__ = ("B", "H", "W", "Hf", "Wf", "P", "depth", "samples", "feat", "rgb", "keep")

    def __init__(self, B, H, W, Hf, Wf, P, depth, samples, feat, rgb, keep):
        self.B, self.H, self.W, self.Hf, self.Wf, self.P = B, H, W, Hf, Wf, P
        self.depth, self.samples, self.feat, self.rgb, self.keep = depth, samples, feat, rgb, keep


class VoxelAccumulator:
    """Device-resident map under construction (handle over avl_builder_*).

    One instance = the state the reference keeps in grid_feat / grid_pos / weight / grid_rgb / occupied_ids
    inside VLMapBuilder.create_mobile_base_map (vlmap_builder.py:86-95), living in HBM.
    """

    def __init__(self, gs, cs, vh, D, capacity=None, n_rows=None, max_capacity=None, deferred_fuse=False):
        """grid (gs, gs, vh) -- or (n_rows, gs, vh) for the rectangular global multi-floor map.
        capacity: voxels the accumulators hold initially (default gs * n_rows like the reference, vlmap_builder.py:202-206);
        max_capacity: like the reference's _reserve_map_space (:286-311) the accumulators DOUBLE when the map outgrows them,
        up to this many voxels (default: every cell of the grid, capped at 2^31 - 1); max_capacity=0 keeps the capacity fixed.
        deferred_fuse: frame-by-frame calls take ONE launch each (avl_builder_set_deferred_fuse): the features of a frame are
        read by the NEXT call's launch, so this object keeps them alive until then; same map, bit for bit (K3 sums a voxel's
        samples in ascending sample order in either mode)."""
        lib = _lib.load()
        _lib.require_gpu()
        self.gs, self.cs, self.vh, self.D = int(gs), float(cs), int(vh), int(D)
        self.n_rows = int(n_rows) if n_rows else self.gs
        ncell = self.n_rows * self.gs * self.vh
        cap0 = int(capacity) if capacity else min(self.n_rows * self.gs, ncell)
        h = C.c_void_p()
        _lib.check(lib.avl_builder_create_grid(C.byref(h), self.n_rows, self.gs, self.vh, self.cs, self.D, cap0),
                   "avl_builder_create_grid")
        self._h = h
        self._has_log = False
        self._max_frame, self._imported = 0, False          # bounds of the first-touch keys (key_bits)
        if max_capacity is None:
            max_capacity = min(ncell, (1 << 31) - 1)
        if max_capacity and max_capacity > cap0:
            _lib.check(lib.avl_builder_set_max_capacity(h, int(max_capacity)), "avl_builder_set_max_capacity")
        if deferred_fuse:
            self.set_deferred_fuse(True)

    def _retain(self, keeps, stream):
        """Keep the inputs of a launch alive until the GPU is done with them.  With deferred fuse the features of frame i are read
        by the launch of frame i + 1, so two generations are always held.  Buffers this module staged itself (NumPy inputs ->
        pooled DeviceArrays) go back to a pool that other threads and streams allocate from (map upload, checkpoint writer):
        those are released only behind an event recorded after the launch that reads them last (at most 4 generations wait, the
        oldest is synchronised -- this path already pays a blocking host-to-device copy per input); torch tensors return to
        torch's own stream-ordered allocator and need no event."""
        self._keep_prev, self._keep = getattr(self, "_keep", None), keeps
        if not any(isinstance(k, DeviceArray) for k in keeps):
            return
        lib = _lib.load()
        q = self.__dict__.setdefault("_keep_events", [])
        free = self.__dict__.setdefault("_free_events", [])
        if free:
            ev = free.pop()
        else:
            ev = C.c_void_p()
            _lib.check(lib.avl_event_create(C.byref(ev)), "avl_event_create")
        _lib.check(lib.avl_event_record(ev, stream), "avl_event_record")
        q.append((ev, keeps))
        while len(q) > 4:
            old_ev, _old = q.pop(0)
            # the launches that read _old must have completed: its own launch -- or, with deferred fuse, the NEXT one, which
            # fuses that frame's features (an event later in the stream covers the earlier one)
            _lib.check(lib.avl_event_sync(q[0][0] if getattr(self, "_deferred", False) else old_ev), "avl_event_sync")
            free.append(old_ev)

    def _calib_pair(self, calib, calib_inv):
        """(K, inv(K)) as contiguous float64; the inverse of an unchanged calibration is computed once (np.linalg.inv is
        ~8 us, most of the host cost of a frame-by-frame call)"""
        K = np.ascontiguousarray(np.asarray(calib, dtype=np.float64).reshape(3, 3))
        if calib_inv is not None:
            return K, np.ascontiguousarray(np.asarray(calib_inv, dtype=np.float64).reshape(3, 3))
        key = K.tobytes()
        c = getattr(self, "_kinv_cache", None)
        if c is None or c[0] != key:
            c = self._kinv_cache = (key, np.ascontiguousarray(np.linalg.inv(K)))
        return K, c[1]

    def key_bits(self) -> int:
        """first-touch keys of this map lie below 2^key_bits: frame index << 32 | sample index, bit 62 once a map was imported
        (avl_builder_import_map: new voxels order after every imported one) -- the bits the merge's key sort has to look at"""
        return 63 if self._imported else 32 + max(1, int(self._max_frame).bit_length())

    def set_deferred_fuse(self, on, stream=None):
        _lib.check(_lib.load().avl_builder_set_deferred_fuse(self._h, int(bool(on)), stream), "avl_builder_set_deferred_fuse")
        self._deferred = bool(on)
        return self

    def flush(self, stream=None):
        """run the feature fusion a deferred-fuse accumulator still owes (every read of the map does this by itself)"""
        _lib.check(_lib.load().avl_builder_flush(self._h, stream), "avl_builder_flush")
        return self

    def release_scratch(self, keep_bytes=0, stream=None):
        """drop the cached sorted replay log and trim the library's stream-ordered pool to keep_bytes (after the last merge /
        save of a build that shares the GPU with a feature extractor)"""
        _lib.check(_lib.load().avl_builder_release_scratch(self._h, int(keep_bytes), stream), "avl_builder_release_scratch")
        return self

    @property
    def capacity(self):
        c = C.c_int64()
        _lib.check(_lib.load().avl_builder_capacity(self._h, C.byref(c)), "avl_builder_capacity")
        return c.value

    def has_replay_log(self):
        return self._has_log

    def drop_replay_cache(self):
        """forget the log sorted by voxel that avl_builder_replay_chain keeps until the next frame (bench.py: a second merge of the
        same map should pay for the sort again)"""
        from ..device import torch_stream_ptr
        _lib.check(_lib.load().avl_builder_drop_replay_cache(self._h, torch_stream_ptr()), "avl_builder_drop_replay_cache")

    def close(self):
        if getattr(self, "_h", None):
            try:
                lib = _lib.load()
                lib.avl_builder_destroy(self._h)          # synchronises: nothing reads the retained inputs any more
                for ev in [e for e, _ in self.__dict__.pop("_keep_events", [])] + self.__dict__.pop("_free_events", []):
                    lib.avl_event_destroy(ev)
            except Exception:      # interpreter shutdown: the module globals are already gone, the driver frees the memory
                pass
            self._h = None

    __del__ = close

    def reset(self, stream=None):
        _lib.check(_lib.load().avl_builder_reset(self._h, stream), "avl_builder_reset")
        self._max_frame, self._imported = 0, False

    def enable_replay_log(self, max_samples):
        """log every sampled pixel so that finalize() replays the reference's sequential weight / grid_rgb exactly"""
        _lib.check(_lib.load().avl_builder_enable_replay_log(self._h, int(max_samples)), "avl_builder_enable_replay_log")
        self._has_log = True
        return self

    def integrate_frame(self, depth, calib, pc_transform, sample_idx, feat_hwc, rgb, frame_idx, calib_inv=None,
                        min_depth=0.1, max_depth=6.0, sigma_sq=0.6, stream=None):
        """Fuse one frame.  depth (H,W) f32, feat_hwc (Hf,Wf,D) f32 channels-last, rgb (H,W,3) u8,
        sample_idx (P,) i32 in sampling order; calib 3x3 and pc_transform 4x4 are host float64."""
        lib = _lib.load()
        dp, dshape, k1 = as_device(depth, np.float32, stream)
        fp_, fshape, k2 = as_device(feat_hwc, np.float32, stream)
        rp, rshape, k3 = as_device(rgb, np.uint8, stream)
        sp, sshape, k4 = as_device(sample_idx, np.int32, stream)
        if len(dshape) != 2 or len(fshape) != 3 or fshape[2] != self.D or tuple(rshape) != (dshape[0], dshape[1], 3):
            raise ValueError(f"bad frame shapes depth {dshape} feat {fshape} rgb {rshape}")
        K, Kinv = self._calib_pair(calib, calib_inv)
        T = np.ascontiguousarray(np.asarray(pc_transform, dtype=np.float64).reshape(4, 4))
        rc = lib.avl_builder_integrate_frame(self._h, dp, dshape[0], dshape[1], K.ctypes.data, Kinv.ctypes.data, T.ctypes.data,
                                             sp, int(np.prod(sshape)), fp_, fshape[0], fshape[1], rp, int(frame_idx),
                                             float(min_depth), float(max_depth), float(sigma_sq), stream)
        _lib.check(rc, "avl_builder_integrate_frame")
        self._max_frame = max(self._max_frame, int(frame_idx))
        self._retain((k1, k2, k3, k4), stream)   # inputs must outlive the asynchronous launches
        return self

    def integrate_batch(self, depths, calib, pc_transforms, sample_idxs=None, feats_hwc=None, rgbs=None, frame_idx0=0, calib_inv=None,
                        min_depth=0.1, max_depth=6.0, sigma_sq=0.6, stream=None):
        """Fuse len(depths) consecutive frames with one launch pair (avl_builder_integrate_batch).  Arguments are lists of
        per-frame arrays (numpy / DeviceArray / torch CUDA) with identical shapes; results equal frame-by-frame fusion."""
        if isinstance(depths, BatchPlan):
            plan = depths
        else:
            plan = self.make_batch_plan(depths, sample_idxs, feats_hwc, rgbs, stream)
        return self._integrate_plan(plan, calib, pc_transforms, frame_idx0, calib_inv, min_depth, max_depth, sigma_sq, stream)

    def integrate_frames(self, plan, calib, pc_transforms, frame_idx0=0, calib_inv=None, min_depth=0.1, max_depth=6.0, sigma_sq=0.6,
                         stream=None):
        """The frame-by-frame loop from C (avl_builder_integrate_frames): the frames of `plan` (make_batch_plan) one after the other,
        one launch pair -- with deferred fuse one launch -- per frame, exactly like len(plan) integrate_frame calls without the
        ~12 us of Python / ctypes per call.  Not a batch: no two frames share a launch."""
        lib = _lib.load()
        B = plan.B
        K, Kinv = self._calib_pair(calib, calib_inv)
        T = np.ascontiguousarray(np.asarray(pc_transforms, dtype=np.float64).reshape(B, 16))
        rc = lib.avl_builder_integrate_frames(self._h, B, plan.depth, plan.H, plan.W, K.ctypes.data, Kinv.ctypes.data, T.ctypes.data,
                                              plan.samples, plan.P, plan.feat, plan.Hf, plan.Wf, plan.rgb, int(frame_idx0),
                                              float(min_depth), float(max_depth), float(sigma_sq), stream)
        _lib.check(rc, "avl_builder_integrate_frames")
        self._max_frame = max(self._max_frame, int(frame_idx0) + B)
        self._retain(plan.keep, stream)
        return self

    def make_batch_plan(self, depths, sample_idxs, feats_hwc, rgbs, stream=None):
        """Resolve the per-frame device pointers of a batch once.  A pipeline that cycles through a ring of frame buffers can
        keep the plan and pass it as `depths` to integrate_batch (sample_idxs / feats_hwc / rgbs are then ignored)."""
        B = len(depths)
        assert B > 0 and len(sample_idxs) == len(feats_hwc) == len(rgbs) == B
        keep, dptr, sptr, fptr, rptr = [], [], [], [], []
        shapes = None
        for i in range(B):
            dp, dshape, k1 = as_device(depths[i], np.float32, stream)
            fp_, fshape, k2 = as_device(feats_hwc[i], np.float32, stream)
            rp, rshape, k3 = as_device(rgbs[i], np.uint8, stream)
            sp, sshape, k4 = as_device(sample_idxs[i], np.int32, stream)
            sh = (tuple(dshape), tuple(fshape), tuple(rshape), int(np.prod(sshape)))
            if shapes is None:
                shapes = sh
            elif sh != shapes:
                raise ValueError("all frames of a batch must share their shapes")
            keep += [k1, k2, k3, k4]
            dptr.append(dp); fptr.append(fp_); rptr.append(rp); sptr.append(sp)
        (H, W), (Hf, Wf, D), _, P = shapes
        if D != self.D:
            raise ValueError(f"feature dim {D} != {self.D}")
        arr = lambda ptrs: (C.c_void_p * B)(*ptrs)
        return BatchPlan(B, H, W, Hf, Wf, P, arr(dptr), arr(sptr), arr(fptr), arr(rptr), keep)

    def _integrate_plan(self, plan, calib, pc_transforms, frame_idx0, calib_inv, min_depth, max_depth, sigma_sq, stream):
        lib = _lib.load()
        B = plan.B
        K, Kinv = self._calib_pair(calib, calib_inv)
        T = np.ascontiguousarray(np.asarray(pc_transforms, dtype=np.float64).reshape(B, 16))
        rc = lib.avl_builder_integrate_batch(self._h, B, plan.depth, plan.H, plan.W, K.ctypes.data, Kinv.ctypes.data, T.ctypes.data,
                                             plan.samples, plan.P, plan.feat, plan.Hf, plan.Wf, plan.rgb, int(frame_idx0),
                                             float(min_depth), float(max_depth), float(sigma_sq), stream)
        _lib.check(rc, "avl_builder_integrate_batch")
        self._max_frame = max(self._max_frame, int(frame_idx0) + B)
        self._retain(plan.keep, stream)
        return self

    def integrate_frame_global(self, depth, calib, transform, sample_idx, feat_hwc, rgb, frame_idx, pcd_min, depth_div=1000.0,
                               calib_inv=None, min_depth=0.1, max_depth=100.0, sigma_sq=0.6, stream=None):
        """Global (multi-floor) fusion, vlmap_builder_multi_floor.py:137-199.  depth: (H,W) uint16 (metres = value /
        depth_div, like the reference's PNG / 1000.0) or float32 metres (any other dtype raises TypeError);
        transform = camera_pose_tf @ habitat2cam_rot_tf."""
        lib = _lib.load()
        dp, dshape, k1, is_u16 = _global_depth(depth, stream)
        fp_, fshape, k2 = as_device(feat_hwc, np.float32, stream)
        rp, rshape, k3 = as_device(rgb, np.uint8, stream)
        sp, sshape, k4 = as_device(sample_idx, np.int32, stream)
        K, Kinv = self._calib_pair(calib, calib_inv)
        T = np.ascontiguousarray(np.asarray(transform, dtype=np.float64).reshape(4, 4))
        pm = np.ascontiguousarray(pcd_min, dtype=np.float64)
        rc = lib.avl_builder_integrate_frame_global(self._h, dp, int(is_u16), float(depth_div), dshape[0], dshape[1], K.ctypes.data,
                                                    Kinv.ctypes.data, T.ctypes.data, sp, int(np.prod(sshape)), fp_, fshape[0],
                                                    fshape[1], rp, int(frame_idx), float(min_depth), float(max_depth),
                                                    float(sigma_sq), pm.ctypes.data, stream)
        _lib.check(rc, "avl_builder_integrate_frame_global")
        self._max_frame = max(self._max_frame, int(frame_idx))
        self._retain((k1, k2, k3, k4), stream)
        return self

    def import_map(self, grid_feat, grid_pos, weight, grid_rgb=None, stream=None):
        """seed an empty accumulator from a finished map (resume, vlmap_builder.py:212-222)"""
        lib = _lib.load()
        fp_, fshape, k1 = as_device(np.asarray(grid_feat, dtype=np.float32) if isinstance(grid_feat, np.ndarray) else grid_feat,
                                    np.float32, stream)
        pp, _, k2 = as_device(np.asarray(grid_pos, dtype=np.int32) if isinstance(grid_pos, np.ndarray) else grid_pos, np.int32, stream)
        wp, _, k3 = as_device(np.asarray(weight, dtype=np.float32) if isinstance(weight, np.ndarray) else weight, np.float32, stream)
        rp = None
        if grid_rgb is not None:
            rgb8 = np.clip(np.asarray(grid_rgb), 0, 255).astype(np.uint8) if isinstance(grid_rgb, np.ndarray) else grid_rgb
            rp, _, k4 = as_device(rgb8, np.uint8, stream)
        _lib.check(lib.avl_builder_import_map(self._h, fshape[0], fp_, pp, wp, rp, stream), "avl_builder_import_map")
        self._imported = True
        return self

    def mark_resumed(self, stream=None):
        """this (empty) accumulator continues a map another rank imported: same first-touch key space as that rank, so that in the
        merge the voxels of new frames order after every imported one (avl_builder_import_map with n = 0)"""
        _lib.check(_lib.load().avl_builder_import_map(self._h, 0, None, None, None, None, stream), "avl_builder_import_map")
        self._imported = True
        return self

    def num_voxels(self, stream=None):
        n = C.c_int64()
        _lib.check(_lib.load().avl_builder_num_voxels(self._h, C.byref(n), stream), "avl_builder_num_voxels")
        return n.value

    def num_points(self, stream=None):
        n = C.c_int64()
        _lib.check(_lib.load().avl_builder_num_points(self._h, C.byref(n), stream), "avl_builder_num_points")
        return n.value

    def num_groups(self, stream=None):
        n = C.c_int64()
        _lib.check(_lib.load().avl_builder_num_groups(self._h, C.byref(n), stream), "avl_builder_num_groups")
        return n.value

    def finalize(self, stream=None, want_occupied=True, as_numpy=True, as_torch=False, want_dirty=False):
        """-> dict(grid_feat, grid_pos, weight, grid_rgb, occupied_ids) in the reference's voxel-id order
        (numpy arrays; DeviceArrays with as_numpy=False; torch CUDA tensors with as_torch=True).
        want_dirty: also 'row_dirty' (n,) uint8 = rows whose voxel was fused since the previous finalize(want_dirty=True)
        (the flags are cleared): what an incremental checkpoint has to rewrite (avl_builder_finalize_ex)."""
        lib = _lib.load()
        n = self.num_voxels(stream)
        if as_torch:
            import torch
            dev = torch.device("cuda", torch.cuda.current_device())
            out = dict(grid_feat=torch.empty((n, self.D), dtype=torch.float32, device=dev),
                       grid_pos=torch.empty((n, 3), dtype=torch.int32, device=dev),
                       weight=torch.empty((n,), dtype=torch.float32, device=dev),
                       grid_rgb=torch.empty((n, 3), dtype=torch.uint8, device=dev),
                       occupied_ids=torch.empty((self.n_rows, self.gs, self.vh), dtype=torch.int32, device=dev) if want_occupied else None)
            _lib.check(lib.avl_builder_finalize(self._h, n, out["grid_feat"].data_ptr(), out["grid_pos"].data_ptr(), out["weight"].data_ptr(),
                                                out["grid_rgb"].data_ptr(),
                                                out["occupied_ids"].data_ptr() if want_occupied else None, stream), "avl_builder_finalize")
            return out
        gf = DeviceArray((n, self.D), np.float32)
        gp = DeviceArray((n, 3), np.int32)
        w = DeviceArray((n,), np.float32)
        rgb = DeviceArray((n, 3), np.uint8)
        occ = DeviceArray((self.n_rows, self.gs, self.vh), np.int32) if want_occupied else None
        dirty = DeviceArray((n,), np.uint8) if want_dirty else None
        _lib.check(lib.avl_builder_finalize_ex(self._h, n, gf.ptr, gp.ptr, w.ptr, rgb.ptr, occ.ptr if occ else None,
                                               dirty.ptr if dirty else None, 1 if want_dirty else 0, stream), "avl_builder_finalize")
        out = dict(grid_feat=gf, grid_pos=gp, weight=w, grid_rgb=rgb, occupied_ids=occ)
        if want_dirty:
            out["row_dirty"] = dirty
        if as_numpy:
            out = {k: (v.numpy(stream) if v is not None else None) for k, v in out.items()}
        return out

    def finalize_rows(self, n_saved, stream=None):
        """Lean checkpoint: finalise on the device, then bring to the host ONLY the rows a checkpoint has to write -- the rows
        below n_saved whose voxel was fused since the previous finalize(want_dirty=True) / finalize_rows, and the new rows
        [n_saved, n) -- gathered on the device (avl_gather_rows) and copied into a page-locked staging buffer.  A full
        finalize() copies the whole map (4.8 GB at 2.25 M voxels: 0.3-0.5 s on the builder's thread, as much as LSeg needs for
        the 100 frames between two checkpoints).
        -> dict(n, n_saved, idx (k,) int64 ascending row indices, rows {grid_feat, grid_pos, weight, grid_rgb: (k, ...) host arrays})
        The row arrays alias this accumulator's staging buffer: they are valid until its next finalize_rows call."""
        from ..device import PinnedBuffer
        lib = _lib.load()
        dev = self.finalize(stream=stream, want_occupied=False, as_numpy=False, want_dirty=True)
        n = int(dev["grid_pos"].shape[0])
        n_saved = min(int(n_saved), n)
        dirty = dev["row_dirty"].numpy(stream)
        idx = np.concatenate([np.flatnonzero(dirty[:n_saved]), np.arange(n_saved, n)]).astype(np.int64)
        names = ("grid_feat", "grid_pos", "weight", "grid_rgb")
        sizes = {}
        for k in names:
            row_shape = tuple(dev[k].shape[1:])
            sizes[k] = (row_shape, int(np.prod(row_shape, dtype=np.int64)) * dev[k].dtype.itemsize)
        stage = getattr(self, "_stage", None)
        if stage is None:
            stage = self._stage = PinnedBuffer()
        total = sum((idx.size * rb + 255) // 256 * 256 for _, rb in sizes.values())
        stage.reserve(max(total, 256))
        rows, off = {}, 0
        if idx.size:
            d_idx = DeviceArray.from_numpy(idx, stream)
            for k in names:
                row_shape, rb = sizes[k]
                dst = DeviceArray((idx.size,) + row_shape, dev[k].dtype)
                _lib.check(lib.avl_gather_rows(dev[k].ptr, rb, d_idx.ptr, idx.size, dst.ptr, stream), "avl_gather_rows")
                rows[k] = stage.view(off, (idx.size,) + row_shape, dev[k].dtype)
                _lib.check(lib.avl_memcpy_d2h(rows[k].ctypes.data, dst.ptr, dst.nbytes, stream), "avl_memcpy_d2h")
                off += (dst.nbytes + 255) // 256 * 256
        else:
            for k in names:
                rows[k] = np.empty((0,) + sizes[k][0], dev[k].dtype)
        return dict(n=n, n_saved=n_saved, idx=idx, rows=rows)

    def export_raw(self, stream=None, as_numpy=True):
        """raw accumulators of all voxels (see avl_builder_export_raw) for the multi-GPU merge"""
        lib = _lib.load()
        n = self.num_voxels(stream)
        arrs = dict(cell=DeviceArray((n,), np.int32), first_key=DeviceArray((n,), np.uint64),
                    sum_feat=DeviceArray((n, self.D), np.float64), sum_w4=DeviceArray((n, 4), np.float64),
                    first_feat=DeviceArray((n, self.D), np.float32), first_alpha=DeviceArray((n,), np.float64))
        _lib.check(lib.avl_builder_export_raw(self._h, n, *(a.ptr for a in arrs.values()), stream), "avl_builder_export_raw")
        _lib.check(lib.avl_stream_sync(stream))
        return {k: v.numpy(stream) for k, v in arrs.items()} if as_numpy else arrs


def points_bbox(minmax, depth, calib, transform, sample_idx, depth_div=1000.0, min_depth=0.1, max_depth=100.0, stream=None):
    """Pass 1 of the global builder (vlmap_builder_multi_floor.py:97-118): fold one frame's transformed sampled points into
    minmax (6,) float64 [min xyz, max xyz] in place.  depth: uint16 (value / depth_div metres) or float32 metres; any other dtype
    raises TypeError."""
    lib = _lib.load()
    dp, dshape, k1, is_u16 = _global_depth(depth, stream)
    sp, sshape, k2 = as_device(sample_idx, np.int32, stream)
    Kinv = np.ascontiguousarray(np.linalg.inv(np.asarray(calib, dtype=np.float64).reshape(3, 3)))
    T = np.ascontiguousarray(np.asarray(transform, dtype=np.float64).reshape(4, 4))
    assert minmax.dtype == np.float64 and minmax.flags["C_CONTIGUOUS"] and minmax.shape == (6,)
    rc = lib.avl_points_bbox(dp, int(is_u16), float(depth_div), dshape[0], dshape[1], Kinv.ctypes.data, T.ctypes.data, sp,
                             int(np.prod(sshape)), float(min_depth), float(max_depth), minmax.ctypes.data, stream)
    _lib.check(rc, "avl_points_bbox")
    return minmax


def finalize_raw(raw, D, gs, vh, stream=None, n_rows=None):
    """Stateless finalisation of (merged) raw accumulators -> the reference's arrays (numpy in, numpy out)."""
    lib = _lib.load()
    n = len(raw["cell"])
    dev = {k: as_device(raw[k], dt, stream) for k, dt in (("cell", np.int32), ("sum_feat", np.float64), ("sum_w4", np.float64),
                                                          ("first_feat", np.float32), ("first_alpha", np.float64))}
    gf, gp = DeviceArray((n, D), np.float32), DeviceArray((n, 3), np.int32)
    w, rgb = DeviceArray((n,), np.float32), DeviceArray((n, 3), np.uint8)
    occ = DeviceArray((n_rows or gs, gs, vh), np.int32)
    _lib.check(lib.avl_memset(occ.ptr, 0xFF, occ.nbytes, stream))
    rc = lib.avl_finalize_raw(n, D, gs, vh, dev["cell"][0], dev["sum_feat"][0], dev["sum_w4"][0], dev["first_feat"][0],
                              dev["first_alpha"][0], gf.ptr, gp.ptr, w.ptr, rgb.ptr, occ.ptr, stream)
    _lib.check(rc, "avl_finalize_raw")
    return dict(grid_feat=gf.numpy(stream), grid_pos=gp.numpy(stream), weight=w.numpy(stream), grid_rgb=rgb.numpy(stream),
                occupied_ids=occ.numpy(stream))


def finalize_merged(merged, D, gs, vh, stream=None, n_rows=None):
    """Finalise accumulators merged by parallel.merge_raw / merge_raw_local: merged = dict(cell (M,) int32, acc (M, D+4) f64)
    in voxel-id order with the first-touch term folded in (avl_finalize_merged).  numpy / torch in, numpy out."""
    lib = _lib.load()
    M = len(merged["cell"])
    cp, _, k1 = as_device(merged["cell"], np.int32, stream)
    ap, ashape, k2 = as_device(merged["acc"], np.float64, stream)
    assert tuple(ashape) == (M, D + 4), ashape
    gf, gp = DeviceArray((M, D), np.float32), DeviceArray((M, 3), np.int32)
    w, rgb = DeviceArray((M,), np.float32), DeviceArray((M, 3), np.uint8)
    occ = DeviceArray((n_rows or gs, gs, vh), np.int32)
    _lib.check(lib.avl_memset(occ.ptr, 0xFF, occ.nbytes, stream))
    _lib.check(lib.avl_finalize_merged(M, 0, D, gs, vh, cp, ap, D + 4, gf.ptr, gp.ptr, w.ptr, rgb.ptr, occ.ptr, stream),
               "avl_finalize_merged")
    return dict(grid_feat=gf.numpy(stream), grid_pos=gp.numpy(stream), weight=w.numpy(stream), grid_rgb=rgb.numpy(stream),
                occupied_ids=occ.numpy(stream))


def export_raw_torch(acc: "VoxelAccumulator", device=None, stream=None):
    """VoxelAccumulator.export_raw into torch tensors on the GPU (input of parallel.merge_raw)."""
    import torch
    lib = _lib.load()
    n = acc.num_voxels(stream)
    device = device or torch.device("cuda", torch.cuda.current_device())
    t = dict(cell=torch.empty((n,), dtype=torch.int32, device=device),
             first_key=torch.empty((n,), dtype=torch.int64, device=device),
             sum_feat=torch.empty((n, acc.D), dtype=torch.float64, device=device),
             sum_w4=torch.empty((n, 4), dtype=torch.float64, device=device),
             first_feat=torch.empty((n, acc.D), dtype=torch.float32, device=device),
             first_alpha=torch.empty((n,), dtype=torch.float64, device=device))
    _lib.check(lib.avl_builder_export_raw(acc._h, n, *(v.data_ptr() for v in t.values()), stream), "avl_builder_export_raw")
    _lib.check(lib.avl_stream_sync(stream))
    return t
