"""Python face of the hot-path kernels (thin: argument marshalling only, all compute in HIP)."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import _lib
from .device import DeviceArray, DeviceView, as_device, _is_torch

PRECISION = {"auto": _lib.SIM_AUTO, "exact": _lib.SIM_EXACT, "split_f16": _lib.SIM_SPLIT_F16, "exact_valu": _lib.SIM_EXACT_VALU,
             "prepared": _lib.SIM_PREPARED}


def query_col_support(queries):
    """(begin, end) int32 arrays: the non-zero column window of every row of a HOST query matrix"""
    q = np.asarray(queries)
    nz = q != 0
    any_nz = nz.any(axis=1)
    begin = np.where(any_nz, nz.argmax(axis=1), 0).astype(np.int32)
    end = np.where(any_nz, q.shape[1] - nz[:, ::-1].argmax(axis=1), 0).astype(np.int32)
    return begin, end


def sim_scores(feat, queries, want_scores=True, want_argmax=True, want_best=False, precision="auto", stream=None,
               out_scores=None, out_argmax=None, out_best=None, col_support="auto"):
    """scores = feat @ queries.T (raw dot product, clip_utils.py:227-229) and argmax(axis=1) (vlmap.py:123).

    feat (N, D) float32, queries (Q, D) float32: numpy arrays, DeviceArrays or torch CUDA tensors.
    Returns (scores, argmax, best): numpy arrays for numpy inputs, otherwise device-side objects of
    the same kind as `feat` (entries are None when not requested).
    col_support: (begin, end) per-query non-zero column windows for block-structured query sets (e.g. text queries living
    in the visual columns and audio queries in the audio columns of a fused map): queries are then scored against their own
    columns only (avl_sim_scores_blocks).  "auto" derives the windows when `queries` is a host array; None = dense.
    """
    lib = _lib.load()
    _lib.require_gpu()
    prepared = None
    if isinstance(feat, PreparedMap):
        prepared, feat, precision = feat, feat.feat, "prepared"
        if prepared.compact:
            return _sim_scores_compact(lib, prepared, queries, want_scores, want_argmax, want_best, stream, out_scores, out_argmax, out_best,
                                       col_support)
    if stream is None and _is_torch(feat):
        from .device import torch_stream_ptr
        stream = torch_stream_ptr()           # launch on torch's current stream so torch-side ordering holds
    fptr, fshape, fkeep = as_device(feat, np.float32, stream)
    qptr, qshape, qkeep = as_device(queries, np.float32, stream)
    if len(fshape) != 2 or len(qshape) != 2 or fshape[1] != qshape[1]:
        raise ValueError(f"shape mismatch: feat {fshape}, queries {qshape}")
    N, D = fshape
    Q = qshape[0]
    torch_mode = _is_torch(feat)

    def alloc(shape, dtype, given):
        if given is not None:
            p, s, k = as_device(given, dtype, stream)
            if tuple(s) != tuple(shape):
                raise ValueError(f"output buffer shape {s} != {shape}")
            return p, k
        if torch_mode:
            import torch
            t = torch.empty(shape, dtype={np.float32: torch.float32, np.int32: torch.int32}[dtype], device=feat.device)
            return t.data_ptr(), t
        d = DeviceArray(shape, dtype)
        return d.ptr, d

    sp = sk = ap = ak = bp = bk = None
    if want_scores or out_scores is not None:
        sp, sk = alloc((N, Q), np.float32, out_scores)
    if want_argmax or out_argmax is not None:
        ap, ak = alloc((N,), np.int32, out_argmax)
    if want_best or out_best is not None:
        bp, bk = alloc((N,), np.float32, out_best)
    rsp = None
    if prepared is not None and prepared.row_scale is not None:
        rs = prepared.row_scale
        rsp = rs.data_ptr() if _is_torch(rs) else rs.ptr
    if isinstance(col_support, str):
        col_support = query_col_support(queries) if (col_support == "auto" and isinstance(queries, np.ndarray) and D > 128) else None
    if col_support is not None and precision in ("auto", "split_f16", "prepared"):
        cb = np.ascontiguousarray(col_support[0], dtype=np.int32)
        ce = np.ascontiguousarray(col_support[1], dtype=np.int32)
        if cb.shape != (Q,) or ce.shape != (Q,):
            raise ValueError("col_support must be two (Q,) integer arrays")
        wsp, wsb = _sim_workspace(lib, N, D, Q, stream)
        rc = lib.avl_sim_scores_blocks(fptr, rsp, N, D, D, qptr, Q, D, cb.ctypes.data, ce.ctypes.data, sp, ap, bp, PRECISION[precision],
                                       wsp, wsb, stream)
    elif rsp is not None:
        wsp, wsb = _sim_workspace(lib, N, D, Q, stream)
        rc = lib.avl_sim_scores_prepared(fptr, rsp, N, D, D, qptr, Q, D, sp, ap, bp, wsp, wsb, stream)
    else:
        wsp, wsb = _sim_workspace(lib, N, D, Q, stream)
        rc = lib.avl_sim_scores_ws(fptr, N, D, D, qptr, Q, D, sp, ap, bp, PRECISION[precision], wsp, wsb, stream)
    _lib.check(rc, "avl_sim_scores")
    if isinstance(feat, np.ndarray):
        _lib.check(lib.avl_stream_sync(stream))
        res = tuple(k.numpy(stream) if k is not None else None for k in (sk, ak, bk))
        return res
    return sk, ak, bk


_WS_CACHE: dict = {}


def _sim_workspace(lib, N, D, Q, stream):
    """per-stream scratch of the similarity kernels (query image + range-guard words + column-block gather), grown on demand
    and reused: the library then allocates nothing per call (avl_sim_workspace_bytes_n)"""
    need = C.c_size_t()
    _lib.check(lib.avl_sim_workspace_bytes_n(int(N), int(D), int(Q), C.byref(need)), "avl_sim_workspace_bytes_n")
    key = int(stream or 0)
    ws = _WS_CACHE.get(key)
    if ws is None or ws.nbytes < need.value:
        ws = _WS_CACHE[key] = DeviceArray((max(need.value, 1 << 20),), np.uint8)
    return ws.ptr, ws.nbytes


class PreparedMap:
    """a device-resident map converted in place by avl_sim_prepare_map: `feat` (N, D) now holds fp16 hi | lo groups,
    `row_scale` (N,) float32 the per-row 2^-s (None: prepared without scaling).  Pass it to sim_scores as `feat`.
    compact=True: `feat` is the separate (N, 3 D) uint8 buffer of avl_sim_prepare_map24 (fp16 hi + one residual byte per element)."""
    __slots__ = ("feat", "row_scale", "shape", "compact")

    def __init__(self, feat, row_scale, shape, compact=False):
        self.feat, self.row_scale, self.shape, self.compact = feat, row_scale, tuple(shape), bool(compact)


def _sim_scores_compact(lib, pm, queries, want_scores, want_argmax, want_best, stream, out_scores, out_argmax, out_best, col_support="auto"):
    """sim_scores on a compact prepared map (avl_sim_scores_prepared24, or avl_sim_scores_blocks with AVL_SIM_PREPARED24 for
    block-structured query sets); results as DeviceArrays / torch tensors like the map"""
    torch_mode = _is_torch(pm.feat)
    if stream is None and torch_mode:
        from .device import torch_stream_ptr
        stream = torch_stream_ptr()
    N, D = pm.shape
    qptr, qshape, qkeep = as_device(queries, np.float32, stream)
    if len(qshape) != 2 or qshape[1] != D:
        raise ValueError(f"shape mismatch: map {pm.shape}, queries {qshape}")
    Q = qshape[0]

    def alloc(shape, dtype, given):
        if given is not None:
            p, s, k = as_device(given, dtype, stream)
            if tuple(s) != tuple(shape):
                raise ValueError(f"output buffer shape {s} != {shape}")
            return p, k
        if torch_mode:
            import torch
            t = torch.empty(shape, dtype={np.float32: torch.float32, np.int32: torch.int32}[dtype], device=pm.feat.device)
            return t.data_ptr(), t
        d = DeviceArray(shape, dtype)
        return d.ptr, d
    sp = sk = ap = ak = bp = bk = None
    if want_scores or out_scores is not None:
        sp, sk = alloc((N, Q), np.float32, out_scores)
    if want_argmax or out_argmax is not None:
        ap, ak = alloc((N,), np.int32, out_argmax)
    if want_best or out_best is not None:
        bp, bk = alloc((N,), np.float32, out_best)
    fptr = pm.feat.data_ptr() if torch_mode else pm.feat.ptr
    rsp = pm.row_scale.data_ptr() if _is_torch(pm.row_scale) else pm.row_scale.ptr
    wsp, wsb = _sim_workspace(lib, N, D, Q, stream)
    if isinstance(col_support, str):
        col_support = query_col_support(queries) if (col_support == "auto" and isinstance(queries, np.ndarray) and D > 128) else None
    if col_support is not None:
        cb = np.ascontiguousarray(col_support[0], dtype=np.int32)
        ce = np.ascontiguousarray(col_support[1], dtype=np.int32)
        if cb.shape != (Q,) or ce.shape != (Q,):
            raise ValueError("col_support must be two (Q,) integer arrays")
        _lib.check(lib.avl_sim_scores_blocks(fptr, rsp, N, D, D, qptr, Q, D, cb.ctypes.data, ce.ctypes.data, sp, ap, bp, _lib.SIM_PREPARED24,
                                             wsp, wsb, stream), "avl_sim_scores_blocks")
    else:
        _lib.check(lib.avl_sim_scores_prepared24(fptr, rsp, N, D, qptr, Q, D, sp, ap, bp, wsp, wsb, stream), "avl_sim_scores_prepared24")
    return sk, ak, bk


def prepare_map(feat_dev, scaled=True, stream=None, compact=False):
    """Convert a DEVICE-resident float32 map in place into the split-fp16 layout (avl_sim_prepare_map) and return a
    PreparedMap for sim_scores.  scaled=True (default): every row gets its own power-of-two scale, so rows of any magnitude
    -- e.g. voxels observed once from far away, feat * exp(-r^2/1.2) -- score with float32-class accuracy.  scaled=False:
    scores bit-identical to the on-the-fly split of the raw map.  feat_dev: DeviceArray or torch CUDA tensor (N, D), D % 64 == 0.
    compact=True (D % 128 == 0): out of place into the 3-byte form (avl_sim_prepare_map24: a plane of fp16 hi values + a plane of
    residual bytes in units of ulp(hi)/256 per row, always row-scaled): a quarter less HBM traffic per query pass, max score error
    2.3e-6 instead of 1.4e-6 (float32-class); the float32 map is left untouched and can be freed by the caller."""
    lib = _lib.load()
    if isinstance(feat_dev, np.ndarray):
        raise TypeError("prepare_map works on a device-resident map (DeviceArray / torch CUDA tensor), not a host array")
    if stream is None and _is_torch(feat_dev):
        from .device import torch_stream_ptr
        stream = torch_stream_ptr()
    fptr, fshape, _ = as_device(feat_dev, np.float32, stream)
    if compact:
        N, D = fshape
        if D % 128:
            raise ValueError(f"the compact form needs a feature width that is a multiple of 128 (D = {D}); use the 4-byte prepared form")
        if _is_torch(feat_dev):
            import torch
            buf = torch.empty((N, 3 * D), dtype=torch.uint8, device=feat_dev.device)
            rs = torch.empty((N,), dtype=torch.float32, device=feat_dev.device)
            bptr, rptr = buf.data_ptr(), rs.data_ptr()
        else:
            buf, rs = DeviceArray((N, 3 * D), np.uint8), DeviceArray((N,), np.float32)
            bptr, rptr = buf.ptr, rs.ptr
        _lib.check(lib.avl_sim_prepare_map24(fptr, N, D, D, bptr, rptr, stream), "avl_sim_prepare_map24")
        return PreparedMap(buf, rs, fshape, compact=True)
    rs = None
    if scaled:
        if _is_torch(feat_dev):
            import torch
            rs = torch.empty((fshape[0],), dtype=torch.float32, device=feat_dev.device)
        else:
            rs = DeviceArray((fshape[0],), np.float32)
    rptr = None if rs is None else (rs.data_ptr() if _is_torch(rs) else rs.ptr)
    _lib.check(lib.avl_sim_prepare_map(fptr, fshape[0], fshape[1], fshape[1], rptr, stream), "avl_sim_prepare_map")
    return PreparedMap(feat_dev, rs, fshape)


def mask_from_argmax(argmax, cat_id, stream=None):
    lib = _lib.load()
    ap, ashape, ak = as_device(argmax, np.int32, stream)
    N = ashape[0]
    if _is_torch(argmax):
        import torch
        m = torch.empty((N,), dtype=torch.uint8, device=argmax.device)
        _lib.check(lib.avl_mask_from_argmax(ap, N, int(cat_id), m.data_ptr(), stream), "avl_mask_from_argmax")
        return m.bool()
    m = DeviceArray((N,), np.uint8)
    _lib.check(lib.avl_mask_from_argmax(ap, N, int(cat_id), m.ptr, stream), "avl_mask_from_argmax")
    return m.numpy(stream).astype(bool) if isinstance(argmax, np.ndarray) else m


def mask_bool_from_argmax(argmax, cat_id, stream=None) -> np.ndarray:
    """host bool mask (N,) = (argmax == cat_id) of a DEVICE-resident argmax (DeviceArray / torch tensor): the comparison and a
    64-to-1 bit packing run on the GPU (avl_mask_bits_from_argmax), N / 8 bytes cross PCIe instead of 4 N, np.unpackbits expands
    them -- what VLMap.index_map returns (vlmap.py:123-124)"""
    lib = _lib.load()
    ap, ashape, ak = as_device(argmax, np.int32, stream)
    N = int(ashape[0])
    bits = DeviceArray(((N + 63) // 64,), np.uint64)
    _lib.check(lib.avl_mask_bits_from_argmax(ap, N, int(cat_id), bits.ptr, stream), "avl_mask_bits_from_argmax")
    packed = bits.numpy(stream)
    bits.free()
    return np.unpackbits(packed.view(np.uint8), count=N, bitorder="little").view(np.bool_)


def argmax_f32(vals, stream=None):
    """(index, value) of the first maximum of a float32 vector (habitat_lang_robot.py:427-430).  NaN is ignored: with at least
    one value that is not NaN the index is np.nanargmax's (not np.argmax's, which returns the first NaN); an all-NaN vector
    returns index 0."""
    lib = _lib.load()
    vp, vshape, vk = as_device(vals, np.float32, stream)
    idx, val = C.c_int64(), C.c_float()
    _lib.check(lib.avl_argmax_f32(vp, int(np.prod(vshape)), C.byref(idx), C.byref(val), stream), "avl_argmax_f32")
    return idx.value, val.value


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
        from .device import torch_stream_ptr
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
        from .device import PinnedBuffer
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


# ---------------------------------------------------------------------------------------- top-down 2-D products
def _dev_u8(x, stream):
    """bool / uint8 host array, DeviceArray or torch tensor -> uint8 device pointer"""
    if isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x).astype(np.uint8, copy=False)
    elif _is_torch(x):
        import torch
        if x.dtype == torch.bool:
            x = x.to(torch.uint8)
    return as_device(x, np.uint8, stream)


def pool_label_2d(mask_3d, grid_pos, gs, stream=None, device=False):
    """(gs, gs) bool: mask_2d[row, col] |= mask_3d[i]  (visualize_utils.py:77-83).  Inputs host or device-resident.
    device=True: the (gs, gs) uint8 DeviceArray instead (nothing crosses PCIe)."""
    lib = _lib.load()
    _lib.require_gpu()
    pp, pshape, k1 = as_device(grid_pos, np.int32, stream)
    mp, mshape, k2 = _dev_u8(mask_3d, stream)
    out = DeviceArray((gs, gs), np.uint8)
    _lib.check(lib.avl_pool_label_2d(pp, mp, pshape[0], int(gs), out.ptr, stream), "avl_pool_label_2d")
    if device:
        return out
    return out.numpy(stream).astype(bool)


def rgb_topdown(grid_pos, grid_rgb, gs, stream=None):
    """(gs, gs, 3) uint8 colour map, last voxel of a column wins  (map.py:106-113)"""
    lib = _lib.load()
    _lib.require_gpu()
    pp, pshape, k1 = as_device(grid_pos, np.int32, stream)
    rgb8 = np.ascontiguousarray(grid_rgb).astype(np.uint8) if isinstance(grid_rgb, np.ndarray) else grid_rgb
    rp, _, k2 = as_device(rgb8, np.uint8, stream)
    out = DeviceArray((gs, gs, 3), np.uint8)
    _lib.check(lib.avl_rgb_topdown(pp, rp, pshape[0], int(gs), out.ptr, stream), "avl_rgb_topdown")
    return out.numpy(stream)


def obstacle_map(occupied_ids, cs, h_min=0, h_max=1.5, stream=None):
    """(n0, n1) bool, True = free: no voxel id > 0 with h_min < height < h_max  (map.py:79-95)"""
    lib = _lib.load()
    _lib.require_gpu()
    op, oshape, k1 = as_device(occupied_ids, np.int32, stream)
    n0, n1, vh = oshape
    heights = np.arange(0, vh) * cs                                     # float64, exactly as upstream
    sel = np.flatnonzero(np.logical_and(heights > h_min, heights < h_max))
    h0, h1 = (int(sel[0]), int(sel[-1]) + 1) if sel.size else (0, 0)   # heights ascend: the mask is one index range
    out = DeviceArray((n0, n1), np.uint8)
    _lib.check(lib.avl_obstacle_map(op, n0, n1, vh, h0, h1, out.ptr, stream), "avl_obstacle_map")
    return out.numpy(stream).astype(bool)


def obstacle_scatter(grid_pos, predict, obs_inds, n_classes, obstacles_cropped, rmin, cmin, stream=None):
    """index_utils.py:163-177: cropped map, True = free, after marking the voxels whose class is in obs_inds.
    predict may be the device-resident argmax of sim_scores."""
    lib = _lib.load()
    _lib.require_gpu()
    pp, pshape, k1 = as_device(grid_pos, np.int32, stream)
    cp, cshape, k2 = as_device(predict, np.int32, stream)
    crop = np.ascontiguousarray(np.asarray(obstacles_cropped) != 0).astype(np.uint8)
    H, W = crop.shape
    fp_, _, k3 = as_device(crop, np.uint8, stream)
    table = np.zeros((int(n_classes),), dtype=np.uint8)
    table[list(obs_inds)] = 1
    out = DeviceArray((H, W), np.uint8)
    _lib.check(lib.avl_obstacle_scatter(pp, cp, pshape[0], table.ctypes.data, int(n_classes), int(rmin), int(cmin), H, W, fp_, out.ptr,
                                        stream), "avl_obstacle_scatter")
    return out.numpy(stream).astype(bool)


# ---------------------------------------------------------------------------------------- headless rendering (csrc/avl_render.hip)
RENDER_MAX_SIDE = 8192


def jet_table() -> np.ndarray:
    """(256, 3) uint8 RGB: OpenCV's COLORMAP_JET built from its published definition, the piecewise-linear
    red(x) = clip(1.5 - |4 x - 3|, 0, 1), green(x) = clip(1.5 - |4 x - 2|, 0, 1), blue(x) = clip(1.5 - |4 x - 1|, 0, 1) at
    x = i / 255, scaled by 255 and rounded to the nearest byte, halves to even (dark blue (0, 0, 128) at 0, dark red (128, 0, 0)
    at 255).  NOT compared with the library: OpenCV is not installed where this project is built and tested, so single entries may
    differ from cv2's by a rounding step.  The kernels take the table as data; with OpenCV at hand pass
    cv2.applyColorMap(np.arange(256, dtype=np.uint8), cv2.COLORMAP_JET)[:, 0, ::-1] instead."""
    i = np.arange(256, dtype=np.int64)
    # in integers, doubled so that the half steps stay exact: 2 * 255 * channel = clip(765 - |8 i - 510 c|, 0, 510), c = 3, 2, 1
    twice = np.stack([np.clip(765 - np.abs(8 * i - 510 * c), 0, 510) for c in (3, 2, 1)], axis=1)
    half = twice // 2
    return (half + ((twice & 1) & (half & 1))).astype(np.uint8)          # an odd `twice` is a half: it goes to the even neighbour


def _heat_arg(heat, stream):
    """(N,) float32 / float64 heat, host or device -> (ptr, N, is_f64, keepalive); other dtypes are a TypeError (the index
    (heat * 255).astype(uint8) is computed in the heat's own dtype, so nothing is converted silently)"""
    if not (isinstance(heat, (DeviceArray, DeviceView)) or _is_torch(heat)):
        heat = np.asarray(heat)
    dt = np.dtype(str(heat.dtype).replace("torch.", ""))
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"heat must be float32 or float64, got {dt}")
    ptr, shape, keep = as_device(heat, dt, stream)
    n = int(np.prod(shape, dtype=np.int64))
    return ptr, n, int(dt == np.float64), keep


def _table_arg(table, stream):
    if table is None:
        table = jet_table()
    if isinstance(table, np.ndarray):
        if table.dtype != np.uint8 or table.shape != (256, 3):
            raise ValueError(f"the colour table must be (256, 3) uint8, got {table.dtype} {table.shape}")
    ptr, shape, keep = as_device(table, np.uint8, stream)
    if tuple(shape) != (256, 3):
        raise ValueError(f"the colour table must be (256, 3) uint8, got shape {tuple(shape)}")
    return ptr, keep


def _rgb_arg(rgb, n, stream):
    """(n, 3) uint8 colours, host or device; a host array of another dtype is cast like ops.rgb_topdown casts grid_rgb"""
    if isinstance(rgb, np.ndarray):
        rgb = np.ascontiguousarray(rgb).astype(np.uint8, copy=False)
    ptr, shape, keep = as_device(rgb, np.uint8, stream)
    if int(np.prod(shape, dtype=np.int64)) != 3 * n:
        raise ValueError(f"expected {n} RGB triples, got shape {tuple(shape)}")
    return ptr, keep


def _background3(background):
    bg = np.ascontiguousarray(np.asarray(background, dtype=np.uint8).reshape(3))
    return bg


def colorize_heat(heat, grid_rgb, transparency=0.5, table=None, as_uint8=False, device=False, stream=None):
    """convert_heatmap_to_rgb (visualize_utils.py:59-64) per voxel on the GPU, NumPy 2's bits:
        idx = (heat * 255).astype(np.uint8)                       (the product in the heat's dtype, float32 or float64)
        out = table[idx].astype(np.float32) * transparency + grid_rgb * (1 - transparency)          -> (N, 3) float64
    as_uint8=True: out.astype(np.uint8) instead, the truncation visualize_rgb_map_2d applies, (N, 3) uint8.
    table: (256, 3) uint8 RGB, default jet_table().  A heat outside [0, 1] or NaN raises AvlError (the uint8 cast is undefined
    there; nothing is clamped).  Inputs host or device-resident; device=True returns the DeviceArray."""
    lib = _lib.load()
    _lib.require_gpu()
    hp, n, is_f64, k1 = _heat_arg(heat, stream)
    rp, k2 = _rgb_arg(grid_rgb, n, stream)
    tp, k3 = _table_arg(table, stream)
    out = DeviceArray((n, 3), np.uint8 if as_uint8 else np.float64)
    _lib.check(lib.avl_render_colorize(hp, is_f64, rp, tp, n, float(transparency), None if as_uint8 else out.ptr,
                                       out.ptr if as_uint8 else None, stream), "avl_render_colorize")
    return _result(out, device, stream, keep=(k1, k2, k3))


def render_topdown(grid_pos, heat, grid_rgb, gs, window=None, transparency=0.5, table=None, background=(0, 0, 0), device=False,
                   stream=None):
    """The heat over the top-down colour map, (rmax - rmin + 1, cmax - cmin + 1, 3) uint8, without a dense heat image: per cell of
    window = (rmin, rmax, cmin, cmax) (inclusive, default the whole (gs, gs) map) the colour of the column's HIGHEST voxel blended
    with table[idx(the column's largest heat)] as colorize_heat(as_uint8=True) blends; cells without a voxel are `background`.
    Negative positions wrap once and a position outside the map raises AvlError, as ops.rgb_topdown; so does a heat outside [0, 1].
    Not upstream's behaviour: upstream has no such function (visualize_heatmap_2d takes a dense 2-D heat, and its colour map keeps
    the LAST voxel of a column, ops.rgb_topdown)."""
    lib = _lib.load()
    _lib.require_gpu()
    gs = int(gs)
    rmin, rmax, cmin, cmax = (0, gs - 1, 0, gs - 1) if window is None else (int(v) for v in window)
    H, W = rmax - rmin + 1, cmax - cmin + 1
    nws = C.c_size_t(0)
    _lib.check(lib.avl_render_topdown_work_bytes(H, W, C.byref(nws)), "avl_render_topdown")      # rejects a bad window before any device work
    pp, pshape, k1 = as_device(grid_pos, np.int32, stream)
    n = int(pshape[0])
    hp, nh, is_f64, k2 = _heat_arg(heat, stream)
    if nh != n:
        raise ValueError(f"{n} voxels but {nh} heat values")
    rp, k3 = _rgb_arg(grid_rgb, n, stream)
    tp, k4 = _table_arg(table, stream)
    bg = _background3(background)
    ws = DeviceArray((nws.value,), np.uint8)
    out = DeviceArray((H, W, 3), np.uint8)
    _lib.check(lib.avl_render_topdown(pp, hp, is_f64, rp, tp, n, gs, rmin, rmax, cmin, cmax, float(transparency), bg.ctypes.data, out.ptr,
                                      ws.ptr, nws.value, stream), "avl_render_topdown")
    return _result(out, device, stream, keep=(k1, k2, k3, k4, ws))


def render_view(grid_pos, color, T, fx, fy, cx, cy, size, znear=0.5, smax=16, background=(0, 0, 0), device=False, stream=None):
    """A z-buffered splat of the voxels from a pinhole camera, (H, W, 3) uint8 for size = (W, H), each <= RENDER_MAX_SIDE.
    color: (N, 3) uint8 per voxel, normally colorize_heat(..., as_uint8=True, device=True).  T: (3, 4) float64 from cell
    coordinates (row, col, h, 1) to the camera frame (x right, y down, z forward, in cells): utils.visualize_utils.look_at or
    camera_of_frame.  Per voxel, in float64: p = T (row, col, h, 1); culled unless z > znear; u = fx * x / z + cx,
    v = fy * y / z + cy; a square of half-side min(0.5 * fx / z, 0.5 * smax) pixels around (u, v), i.e. pixels floor(u - half) ..
    floor(u + half) by floor(v - half) .. floor(v + half) clipped to the image.  A pixel shows the voxel with the smallest
    (float32(z), id); pixels no voxel covers are `background`.  No shading, no anti-aliasing."""
    lib = _lib.load()
    _lib.require_gpu()
    W, H = int(size[0]), int(size[1])
    nws = C.c_size_t(0)
    _lib.check(lib.avl_render_view_work_bytes(W, H, C.byref(nws)), "avl_render_view")
    Tm = np.ascontiguousarray(np.asarray(T, dtype=np.float64))
    if Tm.shape != (3, 4):
        raise ValueError(f"T must be (3, 4), got {Tm.shape}")
    pp, pshape, k1 = as_device(grid_pos, np.int32, stream)
    n = int(pshape[0])
    cp, k2 = _rgb_arg(color, n, stream)
    bg = _background3(background)
    ws = DeviceArray((nws.value,), np.uint8)
    out = DeviceArray((H, W, 3), np.uint8)
    _lib.check(lib.avl_render_view(pp, cp, n, Tm.ctypes.data, float(fx), float(fy), float(cx), float(cy), W, H, float(znear), float(smax),
                                   bg.ctypes.data, out.ptr, ws.ptr, nws.value, stream), "avl_render_view")
    return _result(out, device, stream, keep=(k1, k2, ws))


# ---------------------------------------------------------------------------------------- 2-D image morphology (csrc/avl_morph2d.hip)
_MORPH_OPS = {"dilate": _lib.MORPH_DILATE, "erode": _lib.MORPH_ERODE}
_MORPH_STRUCTURES = {"cross": _lib.MORPH_CROSS, "box": _lib.MORPH_BOX}


def _image_u8(x, stream):
    """2-D bool / uint8 image, host or device -> (ptr, (H, W), keepalive)"""
    ptr, shape, keep = _dev_u8(x, stream)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"expected a non-empty 2-D image, got shape {tuple(shape)}")
    return ptr, (int(shape[0]), int(shape[1])), keep


def _image_any(x, stream):
    """2-D image -> (ptr, (H, W), is_u8, keepalive): float64 stays float64, everything else becomes uint8 (nonzero = true)"""
    dt = np.dtype(x.dtype) if isinstance(x, (np.ndarray, DeviceArray, DeviceView)) else None
    if dt is None and not _is_torch(x):
        x = np.asarray(x)
        dt = x.dtype
    if dt is not None and dt == np.float64:
        ptr, shape, keep = as_device(x, np.float64, stream)
        if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"expected a non-empty 2-D image, got shape {tuple(shape)}")
        return ptr, (int(shape[0]), int(shape[1])), 0, keep
    if _is_torch(x):
        import torch
        if x.dtype == torch.float64:
            ptr, shape, keep = as_device(x, np.float64, stream)
            return ptr, (int(shape[0]), int(shape[1])), 0, keep
    if isinstance(x, np.ndarray) and x.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        x = x != 0
    ptr, shape, keep = _image_u8(x, stream)
    return ptr, shape, 1, keep


def _result(out, device, stream, as_bool=False, keep=()):
    if device:
        out._keep = keep          # inputs and workspaces of the queued launches live as long as their result
        return out
    a = out.numpy(stream)
    return a.astype(bool) if as_bool else a


def gaussian_weights(sigma, truncate=4.0):
    """(weights (2 * radius + 1,) float64, radius): scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, radius) with
    gaussian_filter1d's radius = int(truncate * sigma + 0.5), operation for operation"""
    sd = float(sigma)
    radius = int(float(truncate) * sd + 0.5)
    sigma2 = sd * sd
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    return phi_x / phi_x.sum(), radius


def binary_morph(image, op, structure="cross", iterations=1, device=False, stream=None):
    """scipy.ndimage.binary_dilation / binary_erosion(image, structure, iterations) with border_value 0: op 'dilate' | 'erode',
    structure 'cross' (SciPy's default) | 'box' (np.ones((3, 3))).  -> (H, W) bool, or the uint8 DeviceArray (device=True)."""
    lib = _lib.load()
    _lib.require_gpu()
    ip, (H, W), keep = _image_u8(image, stream)
    out = DeviceArray((H, W), np.uint8)
    tmp = DeviceArray((H, W), np.uint8) if iterations > 4 else None
    _lib.check(lib.avl_morph_binary(ip, H, W, _MORPH_OPS[op], _MORPH_STRUCTURES[structure], int(iterations), out.ptr,
                                    tmp.ptr if tmp is not None else None, stream), "avl_morph_binary")
    return _result(out, device, stream, as_bool=True, keep=(keep, tmp))


def gaussian_filter2d(image, sigma, truncate=4.0, threshold=None, device=False, stream=None):
    """scipy.ndimage.gaussian_filter(image.astype(float), sigma, truncate=truncate) (mode 'reflect'), SciPy's bits: (H, W) float64.
    With `threshold` the mask `value > threshold` is returned as well: (values, mask)."""
    lib = _lib.load()
    _lib.require_gpu()
    ip, (H, W), is_u8, keep = _image_any(image, stream)
    w, radius = gaussian_weights(sigma, truncate)
    out = DeviceArray((H, W), np.float64)
    tmp = DeviceArray((H, W), np.float64)
    gt = DeviceArray((H, W), np.uint8) if threshold is not None else None
    _lib.check(lib.avl_gauss2d_f64(ip, is_u8, H, W, w.ctypes.data, radius, out.ptr, gt.ptr if gt is not None else None,
                                   float(threshold if threshold is not None else 0.0), tmp.ptr, stream), "avl_gauss2d_f64")
    vals = _result(out, device, stream, keep=(keep, tmp))
    if gt is None:
        return vals
    return vals, _result(gt, device, stream, as_bool=True, keep=(keep, tmp))


def resize2x_up(image, device=False, stream=None):
    """cv2.resize(image.astype(float), (2 * W, 2 * H)) with the default INTER_LINEAR: (2 * H, 2 * W) float64"""
    lib = _lib.load()
    _lib.require_gpu()
    ip, (H, W), is_u8, keep = _image_any(image, stream)
    out = DeviceArray((2 * H, 2 * W), np.float64)
    _lib.check(lib.avl_resize2x_up_f64(ip, is_u8, H, W, out.ptr, stream), "avl_resize2x_up_f64")
    return _result(out, device, stream, keep=(keep,))


def resize2x_down(image, device=False, stream=None):
    """cv2.resize(image.astype(float), (W // 2, H // 2)) of an image with even sides: the 2 x 2 block means, float64"""
    lib = _lib.load()
    _lib.require_gpu()
    ip, (H2, W2), is_u8, keep = _image_any(image, stream)
    if H2 % 2 or W2 % 2:
        raise ValueError(f"resize2x_down needs even sides, got {(H2, W2)}")
    out = DeviceArray((H2 // 2, W2 // 2), np.float64)
    _lib.check(lib.avl_resize2x_down_f64(ip, is_u8, H2 // 2, W2 // 2, out.ptr, stream), "avl_resize2x_down_f64")
    return _result(out, device, stream, keep=(keep,))


def dilate_map(binary_map, dilate_iter=0, gaussian_sigma=1.0, want_values=True, want_zero=True, device=False, stream=None):
    """Map._dilate_map (map.py:169-181) on the GPU -> (values (H, W) float64, zero (H, W) bool = values == 0); an output that is
    not wanted is None.  binary_map: bool / uint8 image, host or device."""
    lib = _lib.load()
    _lib.require_gpu()
    ip, (H, W), keep = _image_u8(binary_map, stream)
    n = C.c_size_t(0)
    _lib.check(lib.avl_dilate_map_work_bytes(H, W, C.byref(n)), "avl_dilate_map_work_bytes")
    ws = DeviceArray((n.value,), np.uint8)
    vals = DeviceArray((H, W), np.float64) if want_values else None
    zero = DeviceArray((H, W), np.uint8) if want_zero else None
    _lib.check(lib.avl_dilate_map(ip, H, W, int(dilate_iter), float(gaussian_sigma), vals.ptr if vals is not None else None,
                                  zero.ptr if zero is not None else None, ws.ptr, n.value, stream), "avl_dilate_map")
    return (None if vals is None else _result(vals, device, stream, keep=(keep, ws)),
            None if zero is None else _result(zero, device, stream, as_bool=True, keep=(keep, ws)))


def mask_foreground(mask_2d, r0=0, r1=None, c0=0, c1=None, device=False, stream=None):
    """The mask chain of VLMap.get_pos (vlmap.py:166-171) on the crop [r0:r1, c0:c1] of mask_2d: binary_closing(iterations=3),
    gaussian_filter(0.8, truncate=3), > 0.5, binary_dilation -> (r1 - r0, c1 - c0) bool, or the uint8 DeviceArray."""
    lib = _lib.load()
    _lib.require_gpu()
    ip, (Hf, Wf), keep = _image_u8(mask_2d, stream)
    r1 = Hf if r1 is None else int(r1)
    c1 = Wf if c1 is None else int(c1)
    r0, c0 = int(r0), int(c0)
    if not (0 <= r0 < r1 <= Hf and 0 <= c0 < c1 <= Wf):
        raise ValueError(f"crop [{r0}:{r1}, {c0}:{c1}] is not inside the {(Hf, Wf)} mask")
    H, W = r1 - r0, c1 - c0
    n = C.c_size_t(0)
    _lib.check(lib.avl_mask_foreground_work_bytes(H, W, C.byref(n)), "avl_mask_foreground_work_bytes")
    ws = DeviceArray((n.value,), np.uint8)
    out = DeviceArray((H, W), np.uint8)
    _lib.check(lib.avl_mask_foreground(ip, Wf, r0, r1, c0, c1, out.ptr, ws.ptr, n.value, stream), "avl_mask_foreground")
    return _result(out, device, stream, as_bool=True, keep=(keep, ws))


# ---------------------------------------------------------------------------------------- 2-D distance transform (csrc/avl_edt2d.hip)
EDT_MAX_SIDE = 16384


def _edt_workspace(lib, H, W, what):
    """(workspace, its size, the `found` flag): avl_edt2d_work_bytes rejects a side above EDT_MAX_SIDE before any device work"""
    n = C.c_size_t(0)
    _lib.check(lib.avl_edt2d_work_bytes(int(H), int(W), C.byref(n)), what)
    _lib.require_gpu()
    return DeviceArray((n.value,), np.uint8), n.value, DeviceArray((1,), np.int32)


def _image_shape(x):
    """shape of a host or device image without touching the device"""
    return tuple(int(s) for s in (x.shape if hasattr(x, "shape") else np.asarray(x).shape))


def distance_transform_edt(image, device=False, stream=None):
    """scipy.ndimage.distance_transform_edt(image) for a 2-D image, SciPy's bits: per non-zero cell the float64 distance to the nearest
    zero cell, 0 on zero cells.  image: bool / uint8 / numeric host array (nonzero = true) or a uint8 DeviceArray.  -> (H, W)
    float64, or the DeviceArray (device=True; the check below then synchronises the stream all the same).
    An image without a zero cell raises ValueError (SciPy measures to an imaginary cell at (-1, 0) there); a side above
    EDT_MAX_SIDE raises AvlError before any device work.  return_indices is not supported."""
    lib = _lib.load()
    shape = _image_shape(image)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"expected a non-empty 2-D image, got shape {shape}")
    H, W = shape
    ws, nws, found = _edt_workspace(lib, H, W, "avl_edt2d")
    if isinstance(image, np.ndarray) and image.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        image = image != 0
    ip, _, keep = _image_u8(image, stream)
    out = DeviceArray((H, W), np.float64)
    _lib.check(lib.avl_edt2d(ip, W, H, W, 0, out.ptr, found.ptr, ws.ptr, nws, stream), "avl_edt2d")
    if not int(found.numpy(stream)[0]):
        raise ValueError("distance_transform_edt: the image has no zero cell to measure to")
    return _result(out, device, stream, keep=(keep, ws))


def mask_decay_2d(mask, decay_rate, cell_size=1.0, normalize=False, smooth_sigma=None, device=False, stream=None, window=None):
    """The decay map of a 2-D mask (nonzero = target), NumPy's float64 bits:
        d = distance_transform_edt(mask == 0);  t = 1 - (d / cell_size) * decay_rate;  t[t < 0] = 0
        normalize:  (t - t.min()) / (t.max() - t.min())
    cell_size=1, normalize=True is habitat_lang_robot.py:233-236; cell_size=cs, normalize=False is get_heatmap_from_mask_2d
    (visualize_utils.py:97-102).  smooth_sigma: first mask = gaussian_filter(mask.astype(np.float32), smooth_sigma) > 0.5 in float32
    storage (habitat_lang_robot.py:231-232).  window=(r0, r1, c0, c1): work on mask[r0:r1, c0:c1] without copying it.
    -> (H, W) float64 or the DeviceArray.  ValueError: a mask without a target (after the smoothing), or normalize on a constant map."""
    lib = _lib.load()
    shape = _image_shape(mask)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"expected a non-empty 2-D mask, got shape {shape}")
    r0, r1, c0, c1 = (0, shape[0], 0, shape[1]) if window is None else (int(v) for v in window)
    if not (0 <= r0 < r1 <= shape[0] and 0 <= c0 < c1 <= shape[1]):
        raise ValueError(f"window [{r0}:{r1}, {c0}:{c1}] is not inside the {shape} mask")
    H, W, ld = r1 - r0, c1 - c0, shape[1]
    decay = _check_decay(decay_rate)
    cs = float(cell_size)
    if not (np.isfinite(cs) and cs > 0.0):
        raise ValueError(f"cell_size must be finite and > 0, got {cell_size!r}")
    ws, nws, found = _edt_workspace(lib, H, W, "avl_mask_decay_2d")
    if isinstance(mask, np.ndarray) and mask.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        mask = mask != 0
    mp, _, keep = _image_u8(mask, stream)
    mp += r0 * ld + c0
    keep = [keep, ws]
    if smooth_sigma is not None:
        w, radius = gaussian_weights(smooth_sigma)
        gt, tmp = DeviceArray((H, W), np.uint8), DeviceArray((H, W), np.float32)
        _lib.check(lib.avl_gauss2d_f32(mp, 1, ld, H, W, w.ctypes.data, radius, None, gt.ptr, 0.5, tmp.ptr, stream), "avl_gauss2d_f32")
        keep += [gt, tmp]
        mp, ld = gt.ptr, W
    out, mm = DeviceArray((H, W), np.float64), DeviceArray((2,), np.float64)
    _lib.check(lib.avl_mask_decay_2d(mp, ld, H, W, cs, decay, int(bool(normalize)), out.ptr, mm.ptr, found.ptr, ws.ptr, nws, stream),
               "avl_mask_decay_2d")
    if not int(found.numpy(stream)[0]):
        raise ValueError("mask_decay_2d: the mask has no target cell" + (" after the smoothing" if smooth_sigma is not None else ""))
    if normalize:
        lo, hi = mm.numpy(stream)
        if not hi > lo:
            raise ValueError(f"mask_decay_2d: the 2-D map is constant ({lo}), its min-max normalisation is undefined")
    return _result(out, device, stream, keep=tuple(keep))


def gaussian_filter2d_f32(image, sigma, truncate=4.0, threshold=None, device=False, stream=None):
    """scipy.ndimage.gaussian_filter(image.astype(np.float32), sigma, truncate=truncate), SciPy's float32 bits: (H, W) float32 -- every
    line accumulated in double, the intermediate and the result rounded to float32.  image: bool / uint8 (nonzero = 1) or float32.
    With `threshold` the mask `value > threshold` is returned as well: (values, mask)."""
    lib = _lib.load()
    _lib.require_gpu()
    dt = np.dtype(image.dtype) if hasattr(image, "dtype") and not _is_torch(image) else None
    if dt is not None and dt == np.float32:
        ip, shape, keep = as_device(image, np.float32, stream)
        if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"expected a non-empty 2-D image, got shape {tuple(shape)}")
        (H, W), is_u8 = (int(shape[0]), int(shape[1])), 0
    else:
        if isinstance(image, np.ndarray) and image.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
            raise TypeError(f"gaussian_filter2d_f32 takes a bool, uint8 or float32 image, got {image.dtype}")
        ip, (H, W), keep = _image_u8(image, stream)
        is_u8 = 1
    w, radius = gaussian_weights(sigma, truncate)
    out, tmp = DeviceArray((H, W), np.float32), DeviceArray((H, W), np.float32)
    gt = DeviceArray((H, W), np.uint8) if threshold is not None else None
    _lib.check(lib.avl_gauss2d_f32(ip, is_u8, W, H, W, w.ctypes.data, radius, out.ptr, gt.ptr if gt is not None else None,
                                   float(threshold if threshold is not None else 0.0), tmp.ptr, stream), "avl_gauss2d_f32")
    vals = _result(out, device, stream, keep=(keep, tmp))
    if gt is None:
        return vals
    return vals, _result(gt, device, stream, as_bool=True, keep=(keep, tmp))


class _WindowTermC(C.Structure):
    """avl_window_term of include/avlmaps_hip.h"""
    _fields_ = [("d_data", C.c_void_p), ("ld", C.c_int64), ("is_f64", C.c_int32), ("reserved", C.c_int32)]


class Window:
    """The window [r0:r1, c0:c1] of a 2-D float32 / float64 image (host array or DeviceArray) as a term of product_argmax_2d: a
    device image is read in place."""

    def __init__(self, image, r0, r1, c0, c1):
        self.image, self.r0, self.r1, self.c0, self.c1 = image, int(r0), int(r1), int(c0), int(c1)
        shape = _image_shape(image)
        if len(shape) != 2 or not (0 <= self.r0 < self.r1 <= shape[0] and 0 <= self.c0 < self.c1 <= shape[1]):
            raise ValueError(f"window [{r0}:{r1}, {c0}:{c1}] is not inside an image of shape {shape}")
        self.shape = (self.r1 - self.r0, self.c1 - self.c0)


class ProductResult:
    """product_argmax_2d's result: heat (h, w) float64 DeviceArray or None, cell = (row, col) of the first maximum in raster order
    within the window, value = the product there"""
    __slots__ = ("heat", "cell", "value")

    def __init__(self, heat, cell, value):
        self.heat, self.cell, self.value = heat, cell, value


def product_argmax_2d(terms, want_heat=True, stream=None) -> ProductResult:
    """habitat_lang_robot.py:357-375 + 419-425: heat = ((t0 * t1) * t2) ... in float64 over 1 to 8 (h, w) maps, and np.argmax +
    np.unravel_index of it, in one pass.  terms: float32 / float64 2-D host arrays or DeviceArrays, or ops.Window views of them, all
    of one (h, w); anything else is converted to float64 first.  want_heat=False stores nothing of size h * w."""
    lib = _lib.load()
    terms = list(terms)
    if not 1 <= len(terms) <= GOAL_MAX_TERMS:
        raise ValueError(f"a product has 1 to {GOAL_MAX_TERMS} terms, got {len(terms)}")
    wins = []
    for t in terms:
        if not isinstance(t, Window):
            shape = _image_shape(t)
            if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
                raise ValueError(f"a term is a non-empty 2-D map, got shape {shape}")
            t = Window(t, 0, shape[0], 0, shape[1])
        wins.append(t)
    h, w = wins[0].shape
    if any(t.shape != (h, w) for t in wins):
        raise ValueError(f"the terms differ in shape: {[t.shape for t in wins]}")
    _lib.require_gpu()
    arr, keep = (_WindowTermC * len(wins))(), []
    for k, t in enumerate(wins):
        img = t.image
        if isinstance(img, (DeviceArray, DeviceView)):
            dt = img.dtype
        else:
            img = np.asarray(img)
            dt = img.dtype if img.dtype in (np.float32, np.float64) else np.dtype(np.float64)
        if dt not in (np.float32, np.float64):
            raise TypeError(f"a term is float32 or float64, got {dt}")
        ptr, shape, kp = as_device(img, dt, stream)
        keep.append(kp)
        ld = int(shape[1])
        arr[k] = _WindowTermC(ptr + (t.r0 * ld + t.c0) * dt.itemsize, ld, int(dt == np.float64), 0)
    heat = DeviceArray((h, w), np.float64) if want_heat else None
    idx, val = C.c_int64(), C.c_double()
    _lib.check(lib.avl_product_argmax_2d(arr, len(wins), h, w, heat.ptr if want_heat else None, C.byref(idx), C.byref(val), stream),
               "avl_product_argmax_2d")
    return ProductResult(heat, (int(idx.value) // w, int(idx.value) % w), float(val.value))


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


def topk_f32(vals, k, stream=None):
    """(indices (k,) int64, values (k,) float32) of the k largest entries, descending, ties by ascending index."""
    lib = _lib.load()
    vp, vshape, vk = as_device(vals, np.float32, stream)
    idx = np.empty((k,), dtype=np.int64)
    val = np.empty((k,), dtype=np.float32)
    _lib.check(lib.avl_topk_f32(vp, int(np.prod(vshape)), int(k), idx.ctypes.data, val.ctypes.data, stream), "avl_topk_f32")
    return idx, val


# ---------------------------------------------------------------------------------------- area / sound / image goal fields
class GoalField:
    """A 2-D goal field on the device: `field` (gs, gs) float64 (area) or float32 (sound) and `minmax` (2,) of the same type,
    [min, max] of the whole grid, both DeviceArrays (csrc/avl_field2d.hip)."""

    def __init__(self, field, minmax):
        self.field, self.minmax = field, minmax
        self.gs = field.shape[0]
        self.is_f64 = field.dtype == np.float64

    def bounds(self, stream=None):
        """(min, max) on the host (synchronises the stream)"""
        mm = self.minmax.numpy(stream)
        return mm[0], mm[1]


def _check_decay(decay_rate):
    d = float(decay_rate)
    if not (np.isfinite(d) and d >= 0.0):
        raise ValueError(f"decay_rate must be finite and >= 0, got {decay_rate!r}")
    return d


def area_field(cells, peaks, gs, decay_rate=0.1, stream=None) -> GoalField:
    """avlmap.py:78-96 (index_area_2d before its normalisation): the float64 maximum of clipped cones
    clip(peak_i - decay * ||cell - cell_i||, 0, 1) over the poses whose cell lies inside the (gs, gs) grid, on a field of zeros.
    cells (P, 2) int32 (row, col), peaks (P,) float64 finite: host arrays or device arrays."""
    lib = _lib.load()
    _lib.require_gpu()
    decay = _check_decay(decay_rate)
    if isinstance(peaks, np.ndarray) and not np.all(np.isfinite(peaks)):
        raise ValueError("area peaks must be finite")
    cp, cshape, k1 = as_device(cells, np.int32, stream)
    pp, pshape, k2 = as_device(peaks, np.float64, stream)
    P = int(pshape[0]) if len(pshape) else 0
    if tuple(cshape) != (P, 2):
        raise ValueError(f"cells must be ({P}, 2), got {tuple(cshape)}")
    field, mm = DeviceArray((gs, gs), np.float64), DeviceArray((2,), np.float64)
    _lib.check(lib.avl_field_area(cp, pp, P, int(gs), decay, field.ptr, mm.ptr, stream), "avl_field_area")
    if isinstance(cells, np.ndarray) or isinstance(peaks, np.ndarray):
        _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")      # the uploaded temporaries die here
    return GoalField(field, mm)


def sound_field(offsets, cells, peaks, gs, decay_rate=0.01, stream=None) -> GoalField:
    """avlmap.py:111-131 (index_sound_2d before its normalisation): for every segment in order, the float64 term
    max(p - (p * d) * decay, 0), d = distance to the nearest of the segment's locations, added into a float32 field.
    offsets (S + 1,) int64 CSR offsets into cells (L, 2) int32 (row, col), peaks (S,) float32 >= 0 (host arrays).  Every
    location must lie inside the grid."""
    lib = _lib.load()
    _lib.require_gpu()
    decay = _check_decay(decay_rate)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    cells = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 2)
    peaks = np.ascontiguousarray(peaks, dtype=np.float32)
    S, L = len(peaks), len(cells)
    if offsets.shape != (S + 1,) or offsets[0] != 0 or offsets[-1] != L or np.any(np.diff(offsets) < 1):
        raise ValueError("offsets must be (S + 1,) CSR offsets from 0 to len(cells), every segment with >= 1 location")
    if not np.all(np.isfinite(peaks)) or np.any(peaks < 0):
        raise ValueError("sound peaks must be finite and >= 0")
    if L and (cells.min() < 0 or cells.max() >= gs):
        raise ValueError(f"a sound location lies outside the {gs} x {gs} grid")
    op, _, k1 = as_device(offsets, np.int64, stream)
    cp, _, k2 = as_device(cells, np.int32, stream)
    pp, _, k3 = as_device(peaks, np.float32, stream)
    field, mm = DeviceArray((gs, gs), np.float32), DeviceArray((2,), np.float32)
    _lib.check(lib.avl_field_sound(op, cp, L, pp, S, int(gs), decay, field.ptr, mm.ptr, stream), "avl_field_sound")
    _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")
    return GoalField(field, mm)


def field_lift(gf: GoalField, grid_pos, vh, stream=None):
    """avlmap.py:97 + 100-109 (area) / :132 + 135-144 (sound): heat[i] = f32(normalised field[row_i, col_i]), 0 for voxels outside
    the (gs, gs, vh) grid.  grid_pos (N, 3) int32 host or device (VLMap._device_pos()) -> (N,) float32 DeviceArray."""
    lib = _lib.load()
    gp, gshape, keep = as_device(grid_pos, np.int32, stream)
    N = int(gshape[0])
    heat = DeviceArray((N,), np.float32)
    _lib.check(lib.avl_field_lift(gf.field.ptr, int(gf.is_f64), gf.minmax.ptr, int(gf.gs), int(vh), gp, N, heat.ptr, stream),
               "avl_field_lift")
    if isinstance(grid_pos, np.ndarray):
        _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")
    return heat


def field_normalize(gf: GoalField, stream=None):
    """(field - min) / (max - min) over the whole grid, in the field's precision -> (gs, gs) DeviceArray"""
    lib = _lib.load()
    out = DeviceArray((gf.gs, gf.gs), gf.field.dtype)
    _lib.check(lib.avl_field_normalize(gf.field.ptr, int(gf.is_f64), gf.minmax.ptr, int(gf.gs), out.ptr, stream), "avl_field_normalize")
    return out


def planar_decay(grid_pos, row, col, decay_rate=0.01, stream=None):
    """avlmap.py:154-161: clip(1 - decay * ||grid_pos[:, :2] - (row, col)||, 0, 1) in float64 -> (N,) float64 DeviceArray"""
    lib = _lib.load()
    _lib.require_gpu()
    gp, gshape, keep = as_device(grid_pos, np.int32, stream)
    N = int(gshape[0])
    sim = DeviceArray((N,), np.float64)
    _lib.check(lib.avl_planar_decay(gp, N, int(row), int(col), float(decay_rate), sim.ptr, stream), "avl_planar_decay")
    if isinstance(grid_pos, np.ndarray):
        _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")
    return sim


# ---------------------------------------------------------------------------------------- cross-modal goals
GOAL_DENSE_F32, GOAL_DENSE_F64, GOAL_FIELD_F32, GOAL_FIELD_F64, GOAL_CONES = 0, 1, 2, 3, 4
GOAL_MAX_TERMS = 8


def _on_device(x):
    return isinstance(x, (DeviceArray, DeviceView)) or _is_torch(x)


class _GoalTermC(C.Structure):
    """avl_goal_term of include/avlmaps_hip.h"""
    _fields_ = [("kind", C.c_int32), ("gs", C.c_int32), ("vh", C.c_int32), ("reserved", C.c_int32), ("d_data", C.c_void_p),
                ("d_aux", C.c_void_p), ("n_points", C.c_int64), ("decay", C.c_double)]


class GoalTerm:
    """One factor of a fused goal (csrc/avl_goal.hip): build it with dense(), field() or cones().  `n` is the number of voxels a
    dense term covers (None for the other kinds); `keep` holds the device buffers the term points into."""

    def __init__(self, kind, data=0, aux=0, gs=0, vh=0, n_points=0, decay=0.0, n=None, keep=()):
        self.kind, self.data, self.aux, self.gs, self.vh = int(kind), data, aux, int(gs), int(vh)
        self.n_points, self.decay, self.n, self.keep = int(n_points), float(decay), n, keep

    @classmethod
    def dense(cls, heat, stream=None):
        """an (N,) float32 or float64 heat: a device array (DeviceArray, torch CUDA tensor) is used in place, a host array is
        uploaded in its own type (anything but float32 / float64 is converted to float64 first)"""
        if isinstance(heat, (DeviceArray, DeviceView)):
            dt = heat.dtype
        elif _is_torch(heat):
            dt = np.dtype(str(heat.dtype).split(".")[-1])
        else:
            heat = np.asarray(heat)
            dt = heat.dtype if heat.dtype in (np.float32, np.float64) else np.dtype(np.float64)
        if dt not in (np.float32, np.float64):
            raise TypeError(f"a dense goal term is float32 or float64, got {dt}")
        ptr, shape, keep = as_device(heat, dt, stream)
        if len(shape) != 1:
            raise ValueError(f"a dense goal term is an (N,) vector, got shape {tuple(shape)}")
        return cls(GOAL_DENSE_F64 if dt == np.float64 else GOAL_DENSE_F32, data=ptr, n=int(shape[0]), keep=(keep,))

    @classmethod
    def field(cls, gf: "GoalField", vh):
        """the lift of a GoalField (area_field / sound_field) to the voxels of a (gs, gs, vh) grid: field_lift's value"""
        vh = int(vh)
        if vh < 0:
            raise ValueError(f"vh must be >= 0, got {vh}")
        return cls(GOAL_FIELD_F64 if gf.is_f64 else GOAL_FIELD_F32, data=gf.field.ptr, aux=gf.minmax.ptr, gs=gf.gs, vh=vh, keep=(gf,))

    @classmethod
    def cones(cls, cells, peaks, decay_rate, stream=None):
        """max over the points of clip(peak - decay_rate * ||(row, col) - cell||, 0, 1): cells (P, 2) int32, peaks (P,) float64
        finite, P >= 1 (host or device arrays).  One point with peak 1 is planar_decay."""
        decay = _check_decay(decay_rate)
        if not _on_device(peaks):
            peaks = np.ascontiguousarray(peaks, dtype=np.float64).reshape(-1)
            if not np.all(np.isfinite(peaks)):
                raise ValueError("cone peaks must be finite")
        if not _on_device(cells):
            cells = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 2)
        P = int(peaks.shape[0])
        if P < 1 or tuple(cells.shape) != (P, 2):
            raise ValueError(f"cones need P >= 1 points: cells (P, 2) and peaks (P,), got {tuple(cells.shape)} and {tuple(peaks.shape)}")
        cp, _, k1 = as_device(cells, np.int32, stream)
        pp, _, k2 = as_device(peaks, np.float64, stream)
        return cls(GOAL_CONES, data=cp, aux=pp, n_points=P, decay=decay, keep=(k1, k2))

    def _c(self):
        return _GoalTermC(self.kind, self.gs, self.vh, 0, self.data or None, self.aux or None, self.n_points, self.decay)


class GoalResult:
    """goal_fuse's result: heat (N,) float64 DeviceArray or None, index of the first maximum, the product there, grid_pos there"""
    __slots__ = ("heat", "index", "value", "pos")

    def __init__(self, heat, index, value, pos):
        self.heat, self.index, self.value, self.pos = heat, index, value, pos


def goal_terms_array(terms):
    """the C array of avl_goal_term that avl_goal_fuse reads (host side only)"""
    terms = list(terms)
    if not 1 <= len(terms) <= GOAL_MAX_TERMS:
        raise ValueError(f"a goal is the product of 1 to {GOAL_MAX_TERMS} terms, got {len(terms)}")
    return (_GoalTermC * len(terms))(*[t._c() for t in terms])


def goal_fuse(terms, grid_pos, want_heat=True, stream=None) -> GoalResult:
    """habitat_lang_robot.py:377-430: heat = ((t0 * t1) * t2) ... in float64 over the voxels, and the first voxel of its maximum
    (np.argmax), in one pass (csrc/avl_goal.hip).  terms: 1 to 8 GoalTerms, multiplied in the order given; grid_pos (N, 3) int32
    host or device.  Only index / value / pos come back to the host; want_heat=False stores nothing of size N."""
    lib = _lib.load()
    arr = goal_terms_array(terms)
    _lib.require_gpu()
    gp, gshape, keep = as_device(grid_pos, np.int32, stream)
    if len(gshape) != 2 or gshape[1] != 3:
        raise ValueError(f"grid_pos must be (N, 3), got {tuple(gshape)}")
    N = int(gshape[0])
    for t in terms:
        if t.n is not None and t.n != N:
            raise ValueError(f"a dense term has {t.n} values, the map {N} voxels")
    if N == 0:
        raise ValueError("an empty map has no goal")
    heat = DeviceArray((N,), np.float64) if want_heat else None
    idx, val = C.c_int64(), C.c_double()
    pos = np.empty((3,), dtype=np.int32)
    _lib.check(lib.avl_goal_fuse(arr, len(arr), gp, N, heat.ptr if want_heat else None, C.byref(idx), C.byref(val), pos.ctypes.data,
                                 stream), "avl_goal_fuse")
    return GoalResult(heat, int(idx.value), float(val.value), pos)


# ---------------------------------------------------------------------------------------- visibility-graph navigation
NAV_MAX_VERTICES = 65536
NAV_MAX_SIDE = 32768
NAV_MANY_MAX = 1 << 20          # points per snap / goals per plan_many


class NavGraph:
    """The navigation graph of one obstacle map, resident on the device (csrc/avl_nav.hip): the padded obstacle raster, the path
    vertices and their V x V visibility bitset.  Node ids of a plan: vertices 0 .. V-1 (raster order), V = start, V + 1 = goal.
    Release the device memory with close() (also on garbage collection)."""

    def __init__(self, handle, shape, V):
        self._h = handle
        self.shape = shape
        self.V = V
        self.W64 = (V + 63) // 64
        self._verts = None
        self._many = 0              # serial of the last plan_many: its NavPlanMany alone may read paths

    def _handle(self):
        if self._h is None:
            raise ValueError("the navigation graph has been closed")
        return self._h

    def vertices(self) -> np.ndarray:
        """(V, 2) int32 (row, col) of the path vertices, raster order (cached on the host)"""
        if self._verts is None:
            out = np.zeros((self.V, 2), np.int32)
            if self.V:
                _lib.check(_lib.load().avl_nav_vertices(self._handle(), out.ctypes.data, None), "avl_nav_vertices")
            self._verts = out
        return self._verts

    def visibility_words(self) -> np.ndarray:
        """(V, ceil(V / 64)) uint64: bit b % 64 of word (a, b // 64) = a and b see each other"""
        out = np.zeros((self.V, self.W64), np.uint64)
        if self.V:
            _lib.check(_lib.load().avl_nav_export_visibility(self._handle(), out.ctypes.data, None), "avl_nav_export_visibility")
        return out

    def visibility(self) -> np.ndarray:
        """(V, V) bool, symmetric, False on the diagonal"""
        return unpack_rows(self.visibility_words(), self.V)

    def plan(self, start, goal):
        """float64 shortest path from start (row, col) to goal over the graph -> (distance, node ids start .. goal); (inf, [])
        when the goal is unreachable.  Both points must lie inside the map."""
        s = [float(start[0]), float(start[1])]
        t = [float(goal[0]), float(goal[1])]
        H, W = self.shape
        for r, c in (s, t):
            if not (np.isfinite(r) and np.isfinite(c) and 0.0 <= r <= H - 1 and 0.0 <= c <= W - 1):
                raise ValueError(f"point ({r}, {c}) lies outside the {H} x {W} map")
        cap = self.V + 2
        ids = np.zeros(cap, np.int32)
        dist, n = C.c_double(0.0), C.c_int(0)
        _lib.check(_lib.load().avl_nav_plan(self._handle(), s[0], s[1], t[0], t[1], C.byref(dist), ids.ctypes.data, C.byref(n), cap,
                                            None), "avl_nav_plan")
        return dist.value, ids[:n.value].tolist()

    def last_plan(self) -> dict:
        """the last plan's internals: dist (V + 2,) float64, pred (V + 2,) int32, qvis (2, V) bool (start row, goal row), sg bool"""
        N = self.V + 2
        dist, pred = np.zeros(N, np.float64), np.zeros(N, np.int32)
        q = np.zeros((2, max(self.W64, 1)), np.uint64)
        sg = np.zeros(1, np.int32)
        _lib.check(_lib.load().avl_nav_last_plan(self._handle(), dist.ctypes.data, pred.ctypes.data, q.ctypes.data, sg.ctypes.data,
                                                 None), "avl_nav_last_plan")
        return dict(dist=dist, pred=pred, qvis=unpack_rows(q[:, :self.W64], self.V), sg=bool(sg[0]))

    def _points(self, points, what):
        """(M, 2) float64 points checked like plan's: finite and inside the map"""
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 2))
        if len(pts) > NAV_MANY_MAX:
            raise ValueError(f"{len(pts)} {what}: at most {NAV_MANY_MAX} per call")
        H, W = self.shape
        ok = np.isfinite(pts).all(axis=1) & (pts[:, 0] >= 0.0) & (pts[:, 0] <= H - 1) & (pts[:, 1] >= 0.0) & (pts[:, 1] <= W - 1)
        if not ok.all():
            k = int(np.argmin(ok))
            raise ValueError(f"point ({pts[k, 0]}, {pts[k, 1]}) lies outside the {H} x {W} map")
        return pts

    def snap(self, points):
        """navigation_utils._in_obstacle + _nearest_free for (M, 2) points, on the device -> (points_out (M, 2) float64, moved (M,)
        bool): a point inside the obstacle set (an obstacle cell, or strictly inside a triangle fill) moves to the free cell with
        the smallest squared distance, the first in raster order on ties; the others come back unchanged.  AvlError when the map
        has no free cell."""
        pts = self._points(points, "points")
        out = np.empty_like(pts)
        moved = np.zeros(len(pts), np.uint8)
        _lib.check(_lib.load().avl_navmany_snap(self._handle(), pts.ctypes.data, len(pts), out.ctypes.data, moved.ctypes.data, None),
                   "avl_navmany_snap")
        return out, moved.astype(bool)

    def plan_many(self, start, goals) -> "NavPlanMany":
        """the shortest-path tree from start (row, col), computed once, and every goal of (M, 2) `goals` against it in one launch:
        dist, via and best of avl_navmany_plan.  dist[k] and path(k) equal plan(start, goals[k]) exactly."""
        handle = self._handle()
        s = self._points([start], "points")[0]
        pts = self._points(goals, "goals")
        M = len(pts)
        dist = np.empty(M, np.float64)
        via = np.empty(M, np.int32)
        best = C.c_int64(-1)
        _lib.check(_lib.load().avl_navmany_plan(handle, float(s[0]), float(s[1]), pts.ctypes.data, M, dist.ctypes.data,
                                                via.ctypes.data, C.byref(best), None), "avl_navmany_plan")
        self._many += 1
        return NavPlanMany(self, self._many, dist, via, int(best.value))

    def count_walks(self, on=True):
        """have the following plan_many calls count their walks for many_stats (off by default: counting costs a little per word)"""
        _lib.check(_lib.load().avl_navmany_count_walks(self._handle(), 1 if on else 0), "avl_navmany_count_walks")

    def many_stats(self) -> dict:
        """the pruning of the last plan_many (after count_walks()): walks started, and goal-vertex pairs with a finite candidate
        (the walks without pruning)"""
        n = np.zeros(2, np.uint64)
        _lib.check(_lib.load().avl_navmany_stats(self._handle(), n.ctypes.data), "avl_navmany_stats")
        return dict(walks=int(n[0]), candidates=int(n[1]))

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            try:
                _lib.load().avl_nav_destroy(h)
            except Exception:
                pass

    def __del__(self):
        self.close()


class NavPlanMany:
    """One NavGraph.plan_many: dist (M,) float64 (inf = unreachable), via (M,) int32 (the node each goal hangs on: a vertex id,
    V = the start, -1 = unreachable), best (the first goal with the smallest finite distance, -1 = none) and path(k), the node ids
    start .. goal k (V = start, V + 1 = goal; [] when unreachable).  path() reads the tree kept on the graph, so it answers only
    until the graph's next plan_many."""

    def __init__(self, graph, serial, dist, via, best):
        self._g, self._serial = graph, serial
        self.dist, self.via, self.best = dist, via, best

    def path(self, k):
        k = int(k)
        if not 0 <= k < len(self.dist):
            raise IndexError(f"goal {k} of {len(self.dist)}")
        if self._g._many != self._serial:
            raise ValueError("the graph has planned another batch since: this one's paths are gone")
        cap = self._g.V + 2
        ids = np.zeros(cap, np.int32)
        n = C.c_int(0)
        _lib.check(_lib.load().avl_navmany_path(self._g._handle(), k, ids.ctypes.data, C.byref(n), cap, None), "avl_navmany_path")
        return ids[:n.value].tolist()


def unpack_rows(words: np.ndarray, n: int) -> np.ndarray:
    """(R, ceil(n / 64)) uint64 bit rows -> (R, n) bool (bit b % 64 of word b // 64)"""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    bits = np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder="little")
    return bits[:, :n].astype(bool)


def nav_graph(obstacle_map) -> NavGraph:
    """navigation_utils.py:77-127 build_visgraph_with_obs_map on the GPU: obstacle_map (H, W), nonzero / True = free, 0 = obstacle
    (Map.obstacles_cropped).  Raises AvlError above NAV_MAX_VERTICES path vertices."""
    obs = np.asarray(obstacle_map)
    if obs.ndim != 2 or obs.shape[0] < 1 or obs.shape[1] < 1:
        raise ValueError(f"the obstacle map must be a non-empty 2-D array, got shape {obs.shape}")
    if max(obs.shape) > NAV_MAX_SIDE:
        raise ValueError(f"the obstacle map is {obs.shape[0]} x {obs.shape[1]}; at most {NAV_MAX_SIDE} per side")
    if obs.dtype.kind not in "biuf":
        raise TypeError(f"the obstacle map must be boolean or numeric, got {obs.dtype}")
    free = np.ascontiguousarray(obs != 0, dtype=np.uint8)
    lib = _lib.load()
    _lib.require_gpu()
    h = C.c_void_p()
    _lib.check(lib.avl_nav_create(free.ctypes.data, free.shape[0], free.shape[1], None, C.byref(h)), "avl_nav_create")
    V = C.c_int64(0)
    rc = lib.avl_nav_num_vertices(h, C.byref(V))
    g = NavGraph(h, free.shape, int(V.value))
    _lib.check(rc, "avl_nav_num_vertices")
    return g


# ---------------------------------------------------------------------------------------- object islands (csrc/avl_islands.hip)
ISLANDS_MAX_SIDE = 16384
ISLAND_TABLE_COLS = 8       # area, rmin, rmax, cmin, cmax, first_row, first_col, contour length (0 until trace_islands has run)
NEAREST_PAIR_MAX_COORD = 1 << 15


class Islands:
    """label_islands' result: n islands of an (H, W) mask.  labels: (H, W) int32, 0 = background, 1 .. n in raster order of the first
    pixel (host array, or the DeviceArray with device=True); table: (n, 8) int32 host array, one row per label (ISLAND_TABLE_COLS).
    The device copies of both live until close()."""

    def __init__(self, n, shape, labels_dev, table_dev, device, stream, keep):
        self.n, self.shape, self.stream = int(n), shape, stream
        self.labels_dev, self.table_dev, self._keep = labels_dev, table_dev, keep
        self.labels = labels_dev if device else labels_dev.numpy(stream)
        self._table = None

    @property
    def table(self) -> np.ndarray:
        if self._table is None:
            self._table = self.table_dev.numpy(self.stream) if self.n else np.zeros((0, ISLAND_TABLE_COLS), np.int32)
        return self._table

    def close(self):
        for a in (self.labels_dev, self.table_dev):
            if a is not None:
                a.free()
        self.labels_dev = self.table_dev = self._keep = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def label_islands(mask, device=False, stream=None) -> Islands:
    """8-connected islands of a 2-D mask (bool / uint8, host or DeviceArray; nonzero = foreground):
    scipy.ndimage.label(mask, structure=np.ones((3, 3))) with its numbering, plus the per-island table.  The island count is read
    back once to size the table."""
    lib = _lib.load()
    shape = _image_shape(mask)
    if len(shape) != 2:
        raise ValueError(f"expected a 2-D mask, got shape {shape}")
    H, W = shape
    nws = C.c_size_t(0)
    _lib.check(lib.avl_label_islands_work_bytes(H, W, C.byref(nws)), "avl_label_islands")      # rejects a bad shape before any device work
    _lib.require_gpu()
    if isinstance(mask, np.ndarray) and mask.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        mask = mask != 0
    mp, _, keep = _image_u8(mask, stream)
    ws = DeviceArray((nws.value,), np.uint8)
    labels, n_dev = DeviceArray((H, W), np.int32), DeviceArray((1,), np.int32)
    _lib.check(lib.avl_label_islands(mp, W, H, W, labels.ptr, n_dev.ptr, ws.ptr, nws.value, stream), "avl_label_islands")
    n = int(n_dev.numpy(stream)[0])
    table = DeviceArray((n, ISLAND_TABLE_COLS), np.int32) if n else None
    if n:
        _lib.check(lib.avl_island_table(labels.ptr, H, W, n, table.ptr, stream), "avl_island_table")
    return Islands(n, (H, W), labels, table, device, stream, (keep, ws))


def trace_islands(islands: Islands):
    """The outer contour of every island, in label order: a list of (len, 2) int32 arrays of (row, col), each what
    utils.navigation_utils._trace_boundary returns for that island.  Two device passes: count, then write into one packed buffer."""
    lib = _lib.load()
    n, (H, W), stream = islands.n, islands.shape, islands.stream
    if n == 0:
        return []
    if islands.labels_dev is None:
        raise ValueError("trace_islands: the islands have been closed")
    lp, tp = islands.labels_dev.ptr, islands.table_dev.ptr
    _lib.check(lib.avl_trace_islands(lp, H, W, n, tp, None, None, 0, stream), "avl_trace_islands")
    islands._table = None
    lengths = islands.table[:, 7].astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    total = int(offsets[-1])
    off_dev = DeviceArray.from_numpy(offsets[:-1], stream)
    points = DeviceArray((total, 2), np.int32)
    _lib.check(lib.avl_trace_islands(lp, H, W, n, tp, off_dev.ptr, points.ptr, total, stream), "avl_trace_islands")
    pts = points.numpy(stream)
    return [pts[offsets[k]:offsets[k + 1]] for k in range(n)]


def _points_i32(x, what, stream):
    """an (n, 2) list of integer points, host or int32 DeviceArray -> (ptr, n, keepalive)"""
    if isinstance(x, (DeviceArray, DeviceView)):
        ptr, shape, keep = as_device(x, np.int32, stream)
        if len(shape) != 2 or shape[1] != 2 or shape[0] < 1:
            raise ValueError(f"{what}: expected (n >= 1, 2) points, got shape {tuple(shape)}")
        return ptr, int(shape[0]), keep
    a = np.asarray(x)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1:
        raise ValueError(f"{what}: expected (n >= 1, 2) points, got shape {a.shape}")
    if a.dtype.kind not in "iu":
        if a.dtype.kind != "f" or not np.array_equal(a, np.rint(a)):
            raise TypeError(f"{what}: contour points are integer cells, got {a.dtype}")
    if np.abs(a).max() > NEAREST_PAIR_MAX_COORD:
        raise ValueError(f"{what}: coordinates beyond +-{NEAREST_PAIR_MAX_COORD}")
    ptr, _, keep = as_device(np.ascontiguousarray(a, dtype=np.int32), np.int32, stream)
    return ptr, int(a.shape[0]), keep


def contour_nearest_pair(a, b, stream=None):
    """-> (i, j, d2): the points a[i], b[j] of two (n, 2) integer point lists with the smallest squared distance d2, the first in
    row-major (i, j) order among equals = np.unravel_index(np.argmin(np.linalg.norm(a[:, None] - b[None], axis=2)), (na, nb)),
    without the na x nb matrix (map.py:351-358)."""
    lib = _lib.load()
    _lib.require_gpu()
    ap, na, k1 = _points_i32(a, "contour_nearest_pair: a", stream)
    bp, nb, k2 = _points_i32(b, "contour_nearest_pair: b", stream)
    nws = C.c_size_t(0)
    _lib.check(lib.avl_nearest_pair_work_bytes(na, nb, C.byref(nws)), "avl_nearest_pair_work_bytes")
    ws, out = DeviceArray((nws.value,), np.uint8), DeviceArray((3,), np.int64)
    _lib.check(lib.avl_nearest_pair_i32(ap, na, bp, nb, out.ptr, ws.ptr, nws.value, stream), "avl_nearest_pair_i32")
    i, j, d2 = (int(v) for v in out.numpy(stream))
    return i, j, d2


# ---------------------------------------------------------------------------------------- image localization (csrc/avl_pnp.hip)
PNP_DEFAULT_HYPOTHESES = 9216     # trials for confidence 0.9999 at inlier ratio 0.1: ln(1e-4) / ln(1 - 0.1^3) = 9206, up to a multiple of 64
PNP_MAX_ERROR = 12.0              # localization_utils.py:485
PNP_MAX_ITERATIONS = 50
PNP_STEP_TOLERANCE = 1e-10


def pnp_lds_stage() -> int:
    """the number of correspondences the RANSAC and scoring kernels stage in LDS at a time"""
    return int(_lib.load().avl_pnp_lds_stage())


def _mix32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def pnp_sample_indices(seed, n_hyp, m) -> np.ndarray:
    """(n_hyp, 3) int32: the three distinct correspondence indices hypothesis h of pnp_ransac draws from [0, m), the hash of
    csrc/avl_pnp.hip restated in NumPy's wrapping uint32 arithmetic.  Row h depends on (seed, h, m) alone."""
    m = int(m)
    if m < 3:
        raise ValueError(f"three distinct samples need m >= 3, got {m}")
    with np.errstate(over="ignore"):
        h = np.arange(int(n_hyp), dtype=np.uint32)
        base = _mix32(_mix32(np.uint32((int(seed) ^ 0x9e3779b9) & 0xffffffff)) + h)
        w0, w1, w2 = (_mix32(base + np.uint32(d)) for d in range(3))
    i0 = (w0 % np.uint32(m)).astype(np.int64)
    i1 = (w1 % np.uint32(m - 1)).astype(np.int64)
    i1 += i1 >= i0
    k = (w2 % np.uint32(m - 2)).astype(np.int64)
    k += k >= np.minimum(i0, i1)
    k += k >= np.maximum(i0, i1)
    return np.stack([i0, i1, k], axis=1).astype(np.int32)


class Correspondences:
    """what loc_lift keeps: points (M', 3) in the reference camera's frame and pixels (M', 2) in the query image, float64 on the
    device (views of buffers this object owns), count = M'"""
    __slots__ = ("points", "pixels", "count", "_keep")

    def __init__(self, points, pixels, count, keep=()):
        self.points, self.pixels, self.count, self._keep = points, pixels, int(count), keep

    def numpy(self, stream=None):
        if self.count == 0:
            return np.zeros((0, 3)), np.zeros((0, 2))
        full_p, full_x = self._keep[0].numpy(stream), self._keep[1].numpy(stream)
        return full_p[:self.count].copy(), full_x[:self.count].copy()


def _f64_2d(x, cols, what, stream):
    if isinstance(x, np.ndarray) or not (isinstance(x, (DeviceArray, DeviceView)) or _is_torch(x)):
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    ptr, shape, keep = as_device(x, np.float64, stream)
    if len(shape) != 2 or shape[1] != cols:
        raise ValueError(f"{what}: expected (n, {cols}) float64, got shape {tuple(shape)}")
    return ptr, int(shape[0]), keep


def _camera3(K):
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"the query intrinsic matrix must be (3, 3), got {K.shape}")
    return float(K[0, 0]), float(K[0, 2]), float(K[1, 2])


def _corr_args(points, pixels, stream):
    if isinstance(points, Correspondences):
        points, pixels = points.points, points.pixels
    pp, m, k1 = _f64_2d(points, 3, "points", stream)
    xp, m2, k2 = _f64_2d(pixels, 2, "pixels", stream)
    if m != m2:
        raise ValueError(f"{m} points but {m2} pixels")
    return pp, xp, m, (k1, k2)


def loc_lift(depth, K_ref, kp_ref, kp_query, stream=None) -> Correspondences:
    """localization_utils.py:461-473: the matched key points of the reference frame lifted to 3-D with its depth image.
    depth (H, W) float32 or float64 metres, host or device; K_ref (3, 3); kp_ref, kp_query (M, 2) (x, y) pixel pairs.  kp_ref is
    truncated like astype(np.int32); the point is inv(K_ref) @ (x + 0.5, y + 0.5, 1) * z and is kept when 0.1 < p_z < 10.  The kept
    pairs come back in input order.  A key point outside the image raises AvlError (upstream's IndexError)."""
    lib = _lib.load()
    _lib.require_gpu()
    if not (isinstance(depth, (DeviceArray, DeviceView)) or _is_torch(depth)):
        depth = np.asarray(depth)
        if depth.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            depth = depth.astype(np.float64)
    dt = np.dtype(str(depth.dtype).replace("torch.", ""))
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"depth must be float32 or float64, got {dt}")
    dp, dshape, k0 = as_device(depth, dt, stream)
    if len(dshape) != 2:
        raise ValueError(f"depth must be (H, W), got shape {tuple(dshape)}")
    Kinv = np.ascontiguousarray(np.linalg.inv(np.asarray(K_ref, dtype=np.float64).reshape(3, 3)))
    rp, m, k1 = _f64_2d(kp_ref, 2, "kp_ref", stream)
    qp, m2, k2 = _f64_2d(kp_query, 2, "kp_query", stream)
    if m != m2:
        raise ValueError(f"{m} reference key points but {m2} query key points")
    pts, pix, counter = DeviceArray((max(m, 1), 3), np.float64), DeviceArray((max(m, 1), 2), np.float64), DeviceArray((2,), np.int32)
    n = C.c_int64(0)
    _lib.check(lib.avl_loc_lift(dp, int(dt == np.float64), int(dshape[0]), int(dshape[1]), Kinv.ctypes.data, rp, qp, m, pts.ptr, pix.ptr,
                                counter.ptr, C.byref(n), stream), "avl_loc_lift")
    return Correspondences(DeviceView(pts.ptr, (n.value, 3), np.float64), DeviceView(pix.ptr, (n.value, 2), np.float64), n.value,
                           keep=(pts, pix, k0, k1, k2))


class PnpRansacResult:
    """pose (3, 4) float64 [R|t] (query camera from reference camera), count, hyp_counts (n_hyp,) int32, triples (n_hyp, 3) int32 or
    None; hyp_poses (n_hyp, 3, 4) or None: the best pose of every hypothesis ([I|0] without a solution); pose_dev: the pose on the
    device"""
    __slots__ = ("pose", "count", "hyp_counts", "triples", "hyp_poses", "pose_dev")

    def __init__(self, pose, count, hyp_counts, triples, hyp_poses, pose_dev):
        self.pose, self.count, self.hyp_counts, self.triples, self.hyp_poses, self.pose_dev = pose, int(count), hyp_counts, triples, hyp_poses, pose_dev


def pnp_ransac(points, pixels, K_query, max_error=PNP_MAX_ERROR, n_hyp=PNP_DEFAULT_HYPOTHESES, seed=0, want_triples=False,
               want_poses=False, stream=None) -> PnpRansacResult:
    """n_hyp P3P hypotheses scored against all correspondences (the estimation half of pycolmap.absolute_pose_estimation,
    localization_utils.py:478-498).  points (M, 3) / pixels (M, 2) float64, host or device, or a Correspondences as `points`.
    The winner has the largest inlier count, ties to the smallest hypothesis index; the same seed gives the same bits.  Fewer
    than three correspondences: count 0 and the pose [I|0], without a launch."""
    lib = _lib.load()
    _lib.require_gpu()
    f, cx, cy = _camera3(K_query)
    n_hyp = int(n_hyp)
    pp, xp, m, keep = _corr_args(points, pixels, stream)
    if m < 3:
        return PnpRansacResult(np.eye(3, 4), 0, np.zeros(n_hyp, np.int32), None, None, None)
    nws = C.c_size_t(0)
    _lib.check(lib.avl_pnp_ransac_work_bytes(n_hyp, C.byref(nws)), "avl_pnp_ransac_work_bytes")
    ws = DeviceArray((n_hyp, 3, 4), np.float64)      # after the call: the best pose of every hypothesis
    assert ws.nbytes == nws.value
    counts, pose, count = DeviceArray((n_hyp,), np.int32), DeviceArray((3, 4), np.float64), DeviceArray((1,), np.int32)
    triples = DeviceArray((n_hyp, 3), np.int32) if want_triples else None
    _lib.check(lib.avl_pnp_ransac(pp, xp, m, f, cx, cy, float(max_error), int(seed) & 0xffffffff, n_hyp, triples.ptr if want_triples else None,
                                  counts.ptr, pose.ptr, count.ptr, ws.ptr, nws.value, stream), "avl_pnp_ransac")
    res = PnpRansacResult(pose.numpy(stream), int(count.numpy(stream)[0]), counts.numpy(stream),
                          triples.numpy(stream) if want_triples else None, ws.numpy(stream) if want_poses else None, pose)
    return res


def pnp_score(points, pixels, poses, K_query, max_error=PNP_MAX_ERROR, want_mask=False, stream=None):
    """inlier counts (P,) int32 of poses (P, 3, 4) (or one (3, 4) pose) with the RANSAC kernel's own inlier test; want_mask=True:
    (counts, mask) with the (M,) bool inlier mask of pose 0"""
    lib = _lib.load()
    _lib.require_gpu()
    f, cx, cy = _camera3(K_query)
    pp, xp, m, keep = _corr_args(points, pixels, stream)
    if isinstance(poses, (DeviceArray, DeviceView)):
        sp, sshape, k3 = as_device(poses, np.float64, stream)
    else:
        poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float64))
        sp, sshape, k3 = as_device(poses.reshape(-1, 3, 4), np.float64, stream)
    P = int(np.prod(sshape, dtype=np.int64)) // 12
    counts = DeviceArray((P,), np.int32)
    mask = DeviceArray((max(m, 1),), np.uint8) if want_mask else None
    _lib.check(lib.avl_pnp_score(pp, xp, m, sp, P, f, cx, cy, float(max_error), counts.ptr, mask.ptr if want_mask else None, stream),
               "avl_pnp_score")
    c = counts.numpy(stream)
    if want_mask:
        return c, mask.numpy(stream)[:m].astype(bool)
    return c


class PnpRefineResult:
    """pose (3, 4), cost (sum of squared pixel residuals over the correspondences refined on), iterations, mask (M,) bool and count:
    the inliers of the refined pose, n_used: the inliers of the given pose, which the refinement ran on"""
    __slots__ = ("pose", "cost", "iterations", "mask", "count", "n_used")

    def __init__(self, pose, cost, iterations, mask, count, n_used):
        self.pose, self.cost, self.iterations, self.mask, self.count, self.n_used = pose, float(cost), int(iterations), mask, int(count), int(n_used)


def pnp_refine(points, pixels, pose, K_query, max_error=PNP_MAX_ERROR, max_iter=PNP_MAX_ITERATIONS, step_tol=PNP_STEP_TOLERANCE,
               stream=None) -> PnpRefineResult:
    """Levenberg-Marquardt on the inliers of `pose` ((3, 4), host or the device pose of pnp_ransac), focal length fixed, in one
    launch that iterates on the device; the refined pose is returned even if its inlier count dropped (upstream does not re-check)."""
    lib = _lib.load()
    _lib.require_gpu()
    f, cx, cy = _camera3(K_query)
    pp, xp, m, keep = _corr_args(points, pixels, stream)
    if m < 1:
        raise ValueError("pnp_refine needs at least one correspondence")
    if not isinstance(pose, (DeviceArray, DeviceView)):
        pose = np.ascontiguousarray(np.asarray(pose, dtype=np.float64).reshape(3, 4))
    sp, _, k3 = as_device(pose, np.float64, stream)
    o13, o3, mask = DeviceArray((13,), np.float64), DeviceArray((3,), np.int32), DeviceArray((m,), np.uint8)
    _lib.check(lib.avl_pnp_refine(pp, xp, m, sp, f, cx, cy, float(max_error), int(max_iter), float(step_tol), o13.ptr, o3.ptr, mask.ptr, stream),
               "avl_pnp_refine")
    a, b = o13.numpy(stream), o3.numpy(stream)
    return PnpRefineResult(a[:12].reshape(3, 4).copy(), a[12], b[0], mask.numpy(stream).astype(bool), b[1], b[2])


def retrieve_frame(ref_desc, query_desc, stream=None):
    """localization_utils.py:432-447: the reference frame most similar to each query, (indices (Q,) int64, scores (Q,) float32), from
    the two existing calls: sim_scores in its exact float32 mode and argmax_f32 (the first maximum over the frames).  ref_desc (N, D)
    float32: pass a resident DeviceArray to upload a scene's descriptors once.  query_desc (D,) or (Q, D); a (D,) query returns
    scalars."""
    _lib.load()
    _lib.require_gpu()
    q = query_desc
    single = False
    if not (isinstance(q, (DeviceArray, DeviceView)) or _is_torch(q)):
        q = np.ascontiguousarray(np.asarray(q, dtype=np.float32))
        single = q.ndim == 1
        q = q.reshape(1, -1) if single else q
    if not (isinstance(ref_desc, (DeviceArray, DeviceView)) or _is_torch(ref_desc)):
        ref_desc = DeviceArray.from_numpy(np.ascontiguousarray(np.asarray(ref_desc, dtype=np.float32)), stream)
    qp, qshape, qk = as_device(q, np.float32, stream)
    if len(qshape) != 2 or len(ref_desc.shape) != 2 or qshape[1] != ref_desc.shape[1]:
        raise ValueError(f"shape mismatch: reference descriptors {tuple(ref_desc.shape)}, queries {tuple(qshape)}")
    N, D = int(ref_desc.shape[0]), int(qshape[1])
    if N < 1:
        raise ValueError("no reference frames")
    idx, val = np.zeros(qshape[0], np.int64), np.zeros(qshape[0], np.float32)
    scores = DeviceArray((N, 1), np.float32)
    for j in range(int(qshape[0])):      # one (N, 1) score column per query: argmax_f32 takes a contiguous vector
        sim_scores(ref_desc, DeviceView(qp + j * D * 4, (1, D), np.float32), want_argmax=False, precision="exact", stream=stream,
                   out_scores=scores, col_support=None)
        idx[j], val[j] = argmax_f32(DeviceView(scores.ptr, (N,), np.float32), stream)
    return (int(idx[0]), float(val[0])) if single else (idx, val)


# ---------------------------------------------------------------------------------------- sound map audio (csrc/avl_audio.hip)
AUDIO_MAX_SAMPLES = 2 ** 31 - 1
AUDIO_MAX_CHANNELS = 8


def _audio_f32(audio, stream):
    """a mono float32 recording, host or device -> (ptr, n, DeviceArray / view that keeps it alive)"""
    if isinstance(audio, (DeviceArray, DeviceView)) or _is_torch(audio):
        ptr, shape, keep = as_device(audio, np.float32, stream)
        if len(shape) != 1:
            raise ValueError(f"expected a mono recording of shape (n,), got {tuple(shape)}")
        return ptr, int(shape[0]), keep
    a = np.asarray(audio)
    if a.ndim != 1:
        raise ValueError(f"expected a mono recording of shape (n,), got {a.shape}")
    if a.dtype != np.float32:
        raise TypeError(f"expected float32 samples, got {a.dtype} (decode_pcm16 converts int16 PCM)")
    if not 1 <= a.shape[0] <= AUDIO_MAX_SAMPLES:
        raise ValueError(f"a recording of {a.shape[0]} samples is outside 1 .. 2^31 - 1")
    _lib.require_gpu()
    d = DeviceArray.from_numpy(a, stream)
    return d.ptr, int(a.shape[0]), d


def decode_pcm16(pcm, device=True, stream=None):
    """Interleaved int16 PCM, (n,) or (n, channels) with channels <= 8, host or int16 DeviceArray -> the mono float32 recording
    np.mean(pcm.astype(np.float32) / 32768, axis=1), the documented meaning of librosa.load(..., mono=True) for PCM16 input
    (never compared with librosa or libsndfile, which this project does not have).  A DeviceArray (n,) with device=True."""
    lib = _lib.load()
    if isinstance(pcm, (DeviceArray, DeviceView)):
        ptr, shape, keep = as_device(pcm, np.int16, stream)
    else:
        a = np.asarray(pcm)
        if a.dtype != np.int16:
            raise TypeError(f"expected int16 PCM, got {a.dtype}")
        shape, ptr, keep = a.shape, None, a
    if len(shape) not in (1, 2):
        raise ValueError(f"expected PCM of shape (n,) or (n, channels), got {tuple(shape)}")
    n, ch = int(shape[0]), int(shape[1]) if len(shape) == 2 else 1
    if not 1 <= n <= AUDIO_MAX_SAMPLES or not 1 <= ch <= AUDIO_MAX_CHANNELS:
        raise ValueError(f"{n} frames of {ch} channels: outside 1 .. 2^31 - 1 frames, 1 .. {AUDIO_MAX_CHANNELS} channels")
    _lib.require_gpu()
    if ptr is None:
        keep = DeviceArray.from_numpy(np.ascontiguousarray(keep), stream)
        ptr = keep.ptr
    out = DeviceArray((n,), np.float32)
    _lib.check(lib.avl_audio_decode_pcm16(ptr, n, ch, out.ptr, stream), "avl_audio_decode_pcm16")
    return _result(out, device, stream, keep=(keep,))


class AudioSegments:
    """segment_audio's result.  segments: (S, 2) int64 (l, r) per segment, host array (a DeviceArray with device=True;
    segments_host always holds the host copy); time_ranges: (S, 2) float64 = segments / float(sample_rate), librosa's samples_to_time;
    audio: the recording on the device, (n,) float32, alive as long as this object."""

    def __init__(self, segments_dev, segments_host, sample_rate, audio, n, device):
        self.segments_dev, self.segments_host = segments_dev, segments_host
        self.segments = segments_dev if device else segments_host
        self.sample_rate, self.audio, self.n = sample_rate, audio, n
        self.time_ranges = segments_host / float(sample_rate)

    def __len__(self):
        return len(self.segments_host)


def segment_audio(audio, sample_rate, silence_duration_s=1.0, silence_thres=0.0, device=False, stream=None) -> AudioSegments:
    """audio_utils.py:515-546 segment_audio_with_silence on a mono float32 recording (host array or DeviceArray): sample i is loud
    iff audio[i] > silence_thres; a loud sample starts a segment iff it is the first one or follows the previous loud sample by
    gap = int(silence_duration_s * sample_rate) samples or more; a segment is (l, r), the track upstream cuts audio[l:r].
    Departures: a recording without a loud sample returns zero segments (upstream: IndexError); gap must be at least 1 (upstream's
    loop then emits an extra leading (l, l)); a threshold that float32 cannot hold exactly raises ValueError, because the compare
    runs in float32."""
    lib = _lib.load()
    thr = float(silence_thres)
    if thr != thr or float(np.float32(thr)) != thr:
        raise ValueError(f"silence_thres={silence_thres!r} is not exactly representable in float32")
    gap = int(silence_duration_s * sample_rate)
    if gap < 1:
        raise ValueError(f"silence_duration_s * sample_rate = {silence_duration_s * sample_rate}: the gap must be at least one sample")
    ap, n, keep = _audio_f32(audio, stream)
    nws = C.c_size_t(0)
    _lib.check(lib.avl_audio_segment_work_bytes(n, C.byref(nws)), "avl_audio_segment_work_bytes")
    _lib.require_gpu()
    cap = (n - 1) // gap + 1                      # two starts are at least gap samples apart
    ws, cnt = DeviceArray((nws.value,), np.uint8), DeviceArray((1,), np.int64)
    seg = DeviceArray((cap, 2), np.int64)
    _lib.check(lib.avl_audio_segment(ap, n, thr, gap, seg.ptr, cap, cnt.ptr, ws.ptr, nws.value, stream), "avl_audio_segment")
    S = int(cnt.numpy(stream)[0])
    if S > cap:
        raise _lib.AvlError(f"avl_audio_segment: {S} segments for a capacity of {cap}")
    host = seg.numpy(stream)[:S].copy() if S else np.zeros((0, 2), np.int64)
    dev = None
    if device:                                    # an exact-size copy: the capacity buffer goes back to the pool
        dev = DeviceArray((S, 2), np.int64)
        if S:
            _lib.check(lib.avl_memcpy_d2d(dev.ptr, seg.ptr, S * 16, stream), "avl_memcpy_d2d")
            _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")
    res = AudioSegments(dev, host, sample_rate, keep if isinstance(keep, (DeviceArray, DeviceView)) else DeviceView(ap, (n,), np.float32),
                        n, device)
    res._keep = keep
    return res


def _check_ranges(ranges, n):
    r = np.asarray(ranges)
    if r.size == 0:
        return np.zeros((0, 2), np.int64)
    if r.ndim != 2 or r.shape[1] != 2 or r.dtype.kind not in "iu":
        raise ValueError(f"expected (S, 2) integer (start, stop) ranges, got shape {r.shape} of {r.dtype}")
    r = np.ascontiguousarray(r, dtype=np.int64)
    if (r[:, 0] < 0).any() or (r[:, 0] > r[:, 1]).any() or (r[:, 1] > n).any():
        raise ValueError(f"ranges must satisfy 0 <= start <= stop <= {n}")
    return r


def pack_tracks(audio, ranges, length, scale=32768.0, device=False, stream=None):
    """(S, length) float32: row k is audio[start_k:stop_k] * scale cut or zero-padded to `length` samples.  With scale = 32768 and
    length = 5 * sample_rate this is audio_mapping_utils.py:85 followed by get_five_second_contexts_audio(track, [2.5], sr) for all
    segments at once (the same numbers as upstream's float64 buffers: the scale is a power of two).  ranges: (S, 2) host integers,
    0 <= start <= stop <= n, checked here."""
    lib = _lib.load()
    length, scale = int(length), float(scale)
    if not 1 <= length <= AUDIO_MAX_SAMPLES:
        raise ValueError(f"length={length} outside 1 .. 2^31 - 1")
    if float(np.float32(scale)) != scale:
        raise ValueError(f"scale={scale!r} is not exactly representable in float32")
    ap, n, keep = _audio_f32(audio, stream)
    r = _check_ranges(ranges, n)
    S = len(r)
    _lib.require_gpu()
    out = DeviceArray((S, length), np.float32)
    if S:
        rd = DeviceArray.from_numpy(r, stream)
        _lib.check(lib.avl_audio_pack(ap, n, rd.ptr, S, length, scale, out.ptr, stream), "avl_audio_pack")
        keep = (keep, rd)
    return _result(out, device, stream, keep=(keep,))


def context_ranges(n, times, sample_rate, seconds=5.0):
    """Host code: the (start, stop) slices audio_utils.py:569-583 get_five_second_contexts_audio takes of an n-sample recording,
    one per kept time, as (S, 2) int64 with 0 <= start <= stop <= n, ready for pack_tracks.  A time is skipped when
    t - seconds / 2 > (n - 1) / sample_rate; the bounds are (np.asarray([t - 2.5, t + 2.5]) * sr).astype(int) (librosa's
    time_to_samples); Python's slice rules then apply: a negative bound counts from the end, both are clipped to [0, n], and
    start >= stop is an empty slice (stop = start here)."""
    n, half = int(n), seconds / 2
    out = []
    for t in times:
        if t - half > (n - 1) / sample_rate:
            continue
        b = (np.asarray([t - half, t + half]) * sample_rate).astype(int)
        start, stop, _ = slice(int(b[0]), int(b[1])).indices(n)
        out.append((start, max(start, stop)))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


# ---------------------------------------------------------------------------------------- any rate, any PCM width (csrc/avl_resample.hip)
RESAMPLE_MAX_RATIO = 4096       # 1 <= up, down; every pair of the rates 8 000 .. 192 000 Hz needs at most 2 560 (11 025 <-> 192 000)
RESAMPLE_TILE = 1024            # outputs per tile of the kernel
RESAMPLE_LDS_TAPS = 9216        # the tap table is staged in LDS up to this many taps, read from global memory beyond
RESAMPLE_LDS_WINDOW = 8192      # a tile's input window is staged in LDS up to this many samples
_RESAMPLE_TAPS_KEPT = 8
_RESAMPLE_TAPS = {}             # (device, up, down) -> the taps' DeviceArray, most recent last


def resample_limits():
    """(tile, lds_taps, lds_window) as the library was compiled; RESAMPLE_TILE, RESAMPLE_LDS_TAPS and RESAMPLE_LDS_WINDOW state them"""
    t, a, w = C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.check(_lib.load().avl_audio_resample_limits(C.byref(t), C.byref(a), C.byref(w)), "avl_audio_resample_limits")
    return t.value, a.value, w.value


def resample_ratio(sr_in, sr_out):
    """(up, down) = (sr_out, sr_in) / gcd; ValueError unless both rates are positive integers and 1 <= up, down <= 4096"""
    import math
    if int(sr_in) != sr_in or int(sr_out) != sr_out or sr_in < 1 or sr_out < 1:
        raise ValueError(f"sample rates must be positive integers, got {sr_in!r} and {sr_out!r}")
    sr_in, sr_out = int(sr_in), int(sr_out)
    g = math.gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g
    if max(up, down) > RESAMPLE_MAX_RATIO:
        raise ValueError(f"{sr_in} Hz -> {sr_out} Hz is the ratio {up} / {down}: both terms must be at most {RESAMPLE_MAX_RATIO}")
    return up, down


def resample_taps(up, down) -> np.ndarray:
    """Host code: the float64 taps of scipy.signal.resample_poly(x, up, down)'s default filter,
    firwin(2 * half + 1, 1 / M, window=("kaiser", 5.0)) * up with M = max(up, down) and half = 10 * M, from NumPy alone: the
    windowed sinc, normalised to unit gain at 0 Hz, times up.  Within 5.6e-16 of SciPy's for the ratios the tests list."""
    up, down = int(up), int(down)
    if not (1 <= up <= RESAMPLE_MAX_RATIO and 1 <= down <= RESAMPLE_MAX_RATIO):
        raise ValueError(f"ratio {up} / {down}: both terms must lie in 1 .. {RESAMPLE_MAX_RATIO}")
    M = max(up, down)
    half = 10 * M
    L = 2 * half + 1
    i = np.arange(L) - half
    t = np.sinc(i / M) / M * np.kaiser(L, 5.0)
    return t / t.sum() * up


def _device_taps(up, down, stream):
    key = (_lib.current_device(), up, down)
    d = _RESAMPLE_TAPS.pop(key, None)
    if d is None:
        d = DeviceArray.from_numpy(resample_taps(up, down), stream)
    _RESAMPLE_TAPS[key] = d
    while len(_RESAMPLE_TAPS) > _RESAMPLE_TAPS_KEPT:
        del _RESAMPLE_TAPS[next(iter(_RESAMPLE_TAPS))]
    return d


def _audio_len(audio):
    """the length of a mono float32 recording, host or device, checked without any device work"""
    if isinstance(audio, (DeviceArray, DeviceView)):
        shape, dt = audio.shape, audio.dtype
    elif _is_torch(audio):
        shape, dt = tuple(audio.shape), np.dtype(np.float32) if str(audio.dtype) == "torch.float32" else str(audio.dtype)
    else:
        a = np.asarray(audio)
        shape, dt = a.shape, a.dtype
    if len(shape) != 1:
        raise ValueError(f"expected a mono recording of shape (n,), got {tuple(shape)}")
    if dt != np.float32:
        raise TypeError(f"expected float32 samples, got {dt} (decode_pcm converts PCM)")
    if not 1 <= int(shape[0]) <= AUDIO_MAX_SAMPLES:
        raise ValueError(f"a recording of {shape[0]} samples is outside 1 .. 2^31 - 1")
    return int(shape[0])


def resample_audio(audio, sr_in, sr_out, device=False, stream=None):
    """scipy.signal.resample_poly(audio, up, down) with its default filter, a float64 accumulator and one rounding to float32, where
    up / down is sr_out / sr_in reduced: stands in for the resampling of librosa.load(path, sr=sr_out) (audio_mapping_utils.py:238),
    whose own filter (soxr_hq) this is NOT.  audio: a mono float32 host array, DeviceArray or DeviceView; the result has
    ceil(n * up / down) samples, a host array or (device=True) a DeviceArray.  sr_in == sr_out returns `audio` itself.  The taps
    (resample_taps) are kept on the device per (up, down)."""
    up, down = resample_ratio(sr_in, sr_out)
    n = _audio_len(audio)
    if up == down:
        return audio
    n_out = -(-n * up // down)
    if n_out > AUDIO_MAX_SAMPLES:
        raise ValueError(f"{n} samples at {up} / {down} are {n_out} samples, more than 2^31 - 1")
    lib = _lib.load()
    ap, n, keep = _audio_f32(audio, stream)
    taps = _device_taps(up, down, stream)
    out = DeviceArray((n_out,), np.float32)
    _lib.check(lib.avl_audio_resample(ap, n, up, down, taps.ptr, taps.shape[0], out.ptr, n_out, stream), "avl_audio_resample")
    return _result(out, device, stream, keep=(keep, taps))


def decode_pcm(data, width=None, channels=None, device=True, stream=None):
    """Interleaved PCM of any of the widths a WAV file has -> the mono float32 recording (a DeviceArray (n,) with device=True):
      int16  (n,) or (n, channels)   decode_pcm16, unchanged
      int32  (n,) or (n, channels)   32-bit PCM, or 24-bit left-justified in 32 bits (scipy.io.wavfile's convention): width 4
      uint8  with width=3            the raw little-endian 3-byte samples of a 24-bit file, any shape of n * channels * 3 bytes
                                     (channels defaults to 1, or to shape[1] of an (n, channels, 3) array)
    host arrays, DeviceArrays or DeviceViews.  Widths 3 and 4: float32((sum_c float64(s[i, c]) / 2^(8 width - 1)) / channels), the
    NumPy expression ((s.astype(np.float64) / 2.0 ** (8 * width - 1)).sum(axis=1) / channels).astype(np.float32)."""
    dev = isinstance(data, (DeviceArray, DeviceView))
    a = data if dev else np.asarray(data)
    dt, shape = np.dtype(a.dtype), tuple(a.shape)
    if dt == np.int16 and width in (None, 2):
        if channels not in (None, shape[1] if len(shape) == 2 else 1):
            raise ValueError(f"channels={channels} does not match PCM of shape {shape}")
        return decode_pcm16(data, device=device, stream=stream)
    if dt == np.int32 and width in (None, 4):
        width = 4
        if len(shape) not in (1, 2):
            raise ValueError(f"expected PCM of shape (n,) or (n, channels), got {shape}")
        n, ch = shape[0], shape[1] if len(shape) == 2 else 1
        if channels not in (None, ch):
            raise ValueError(f"channels={channels} does not match PCM of shape {shape}")
    elif dt == np.uint8 and width == 3:
        ch = int(channels) if channels is not None else (shape[1] if len(shape) == 3 and shape[2] == 3 else 1)
        size = int(np.prod(shape, dtype=np.int64))
        if ch < 1 or size % (3 * ch):
            raise ValueError(f"{size} bytes are not whole frames of {ch} channels of 3 bytes")
        n = size // (3 * ch)
    else:
        raise ValueError(f"{dt} samples with width={width}: int16, int32, or uint8 bytes with width=3 are decoded")
    if not 1 <= n <= AUDIO_MAX_SAMPLES or not 1 <= ch <= AUDIO_MAX_CHANNELS:
        raise ValueError(f"{n} frames of {ch} channels: outside 1 .. 2^31 - 1 frames, 1 .. {AUDIO_MAX_CHANNELS} channels")
    lib = _lib.load()
    _lib.require_gpu()
    keep = a if dev else DeviceArray.from_numpy(np.ascontiguousarray(a), stream)
    out = DeviceArray((n,), np.float32)
    _lib.check(lib.avl_audio_decode_pcm(keep.ptr, n, ch, width, out.ptr, stream), "avl_audio_decode_pcm")
    return _result(out, device, stream, keep=(keep,))


# ---------------------------------------------------------------------------------------- observed free space (csrc/avl_explore.hip)
EXPLORE_MAX_SIDE = 16384
NEVER_SEEN = -1             # first_seen of a cell no sight ray crossed


def _mask_dtype_check(x, what):
    """bool / uint8 masks only (host array, DeviceArray / DeviceView or torch tensor): anything else would be cast quietly"""
    if _is_torch(x):
        ok = str(x.dtype) in ("torch.bool", "torch.uint8")
    else:
        ok = hasattr(x, "dtype") and np.dtype(x.dtype) in (np.dtype(bool), np.dtype(np.uint8))
    if not ok:
        raise TypeError(f"{what} must be a bool or uint8 mask, got {getattr(x, 'dtype', type(x).__name__)}")


def carve_free_space(first_seen, depth, calib, transforms, frame_ids, gs, cs, stride=4, h_min=0.0, h_max=1.5, min_depth=0.1,
                     max_depth=6.0, depth_div=1000.0, device=False, stream=None):
    """Fold the sight rays of F depth frames into first_seen (gs, gs) int32: the smallest frame id whose rays crossed a cell inside
    the height band [h_min, h_max], NEVER_SEEN (-1) where none did (avl_carve_free_space; the ray is defined at the top of
    csrc/avl_explore.hip).  first_seen: None (a new map), a host int32 array (updated in place and returned), or an int32
    DeviceArray / GPU tensor (updated in place; returned as it is with device=True, else copied back).  depth: (F, H, W) or (H, W),
    uint16 (value / depth_div metres) or float32 metres, host or device; calib: the 3 x 3 camera matrix; transforms: (F, 4, 4)
    camera -> map (VLMapBuilder.frame_transforms); frame_ids: (F,) ids >= 0.  The fold is a minimum: calls may come in any order
    and continue each other.  TypeError on other dtypes, ValueError on bad shapes or parameters, before any device work."""
    gs, stride = int(gs), int(stride)
    if not 1 <= gs <= EXPLORE_MAX_SIDE:
        raise ValueError(f"carve_free_space: grid size {gs} (1 .. {EXPLORE_MAX_SIDE})")
    if stride < 1:
        raise ValueError(f"carve_free_space: stride {stride} < 1")
    if not (np.isfinite(h_min) and np.isfinite(h_max) and h_min <= h_max):
        raise ValueError(f"carve_free_space: height band [{h_min}, {h_max}]")
    if not (np.isfinite(cs) and cs > 0):
        raise ValueError(f"carve_free_space: cell size {cs}")
    if not (np.isfinite(min_depth) and np.isfinite(max_depth) and 0 <= min_depth < max_depth):
        raise ValueError(f"carve_free_space: depth range ({min_depth}, {max_depth})")
    ddt = str(depth.dtype) if _is_torch(depth) else np.dtype(getattr(depth, "dtype", object))
    if ddt not in ("torch.uint16", "torch.int16", "torch.float32", np.dtype(np.uint16), np.dtype(np.float32)):
        raise TypeError(f"depth must be uint16 (value / depth_div metres) or float32 metres, got {ddt}")
    dshape = tuple(int(s) for s in depth.shape)
    if len(dshape) == 2:
        dshape = (1,) + dshape
    if len(dshape) != 3 or dshape[1] < 1 or dshape[2] < 1:
        raise ValueError(f"carve_free_space: depth must be (F, H, W) or (H, W), got shape {tuple(depth.shape)}")
    F, H, W = dshape
    K = np.asarray(calib, dtype=np.float64)
    if K.size != 9:
        raise ValueError(f"carve_free_space: calib must be 3 x 3, got shape {K.shape}")
    T = np.ascontiguousarray(transforms, dtype=np.float64)
    if T.shape not in ((F, 4, 4), (4, 4)) or T.size != F * 16:
        raise ValueError(f"carve_free_space: {F} frames but transforms of shape {T.shape}")
    ids = np.ascontiguousarray(np.asarray(frame_ids).reshape(-1))
    if ids.shape[0] != F:
        raise ValueError(f"carve_free_space: {F} frames but {ids.shape[0]} frame ids")
    if F and (ids.dtype.kind not in "iu" or ids.min() < 0 or ids.max() > 2 ** 31 - 2):
        raise ValueError("carve_free_space: frame ids are integers in [0, 2^31 - 2]")
    ids = ids.astype(np.int32)
    host_map = None
    if first_seen is not None:
        fdt = str(first_seen.dtype) if _is_torch(first_seen) else np.dtype(getattr(first_seen, "dtype", object))
        if fdt not in ("torch.int32", np.dtype(np.int32)):
            raise TypeError(f"first_seen must be int32, got {fdt}")
        if tuple(first_seen.shape) != (gs, gs):
            raise ValueError(f"carve_free_space: first_seen must be ({gs}, {gs}), got shape {tuple(first_seen.shape)}")
        if isinstance(first_seen, np.ndarray):
            host_map = first_seen
    lib = _lib.load()
    _lib.require_gpu()
    if first_seen is None:
        fs = DeviceArray((gs, gs), np.int32)
        _lib.check(lib.avl_memset(fs.ptr, 0xFF, fs.nbytes, stream), "avl_memset")       # every cell NEVER_SEEN
        fp = fs.ptr
    elif host_map is not None:
        fs = DeviceArray.from_numpy(host_map, stream)
        fp = fs.ptr
    else:
        fp, fs = as_device(first_seen, np.int32, stream)[0], first_seen
    Kinv = np.ascontiguousarray(np.linalg.inv(K.reshape(3, 3)))
    keep_d = None
    if F:
        dp, _, keep_d, is_u16 = _global_depth(depth, stream)
        _lib.check(lib.avl_carve_free_space(dp, int(is_u16), float(depth_div), F, H, W, Kinv.ctypes.data, T.ctypes.data, ids.ctypes.data,
                                            gs, float(cs), stride, float(h_min), float(h_max), float(min_depth), float(max_depth), fp,
                                            stream), "avl_carve_free_space")
    if device:
        if isinstance(fs, DeviceArray):
            fs._keep = (keep_d,)
        else:
            _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")          # the staged depth may be released on return
        return fs
    out = host_map if host_map is not None and host_map.flags["C_CONTIGUOUS"] else np.empty((gs, gs), np.int32)
    _lib.check(lib.avl_memcpy_d2h(out.ctypes.data, fp, out.nbytes, stream), "avl_memcpy_d2h")       # (synchronous: the staged depth may go)
    if host_map is not None and out is not host_map:
        np.copyto(host_map, out)
    return out if host_map is None else host_map


def frontier_mask(free, explored, device=False, stream=None):
    """(H, W) uint8: 1 where a cell is explored and free and at least one of its 4 neighbours inside the image is unknown, i.e. not
    explored and free (avl_frontier_mask).  A cell that holds an obstacle is known whether or not a ray crossed it.  free, explored:
    bool / uint8 masks of one shape, host or device; any other dtype raises TypeError."""
    _mask_dtype_check(free, "free")
    _mask_dtype_check(explored, "explored")
    shape = _image_shape(free)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1 or _image_shape(explored) != shape:
        raise ValueError(f"frontier_mask: expected two non-empty 2-D masks of one shape, got {shape} and {_image_shape(explored)}")
    if max(shape) > EXPLORE_MAX_SIDE:
        raise ValueError(f"frontier_mask: sides up to {EXPLORE_MAX_SIDE}, got {shape}")
    lib = _lib.load()
    _lib.require_gpu()
    fp, (H, W), k1 = _image_u8(free, stream)
    ep, _, k2 = _image_u8(explored, stream)
    out = DeviceArray((H, W), np.uint8)
    _lib.check(lib.avl_frontier_mask(fp, ep, H, W, out.ptr, stream), "avl_frontier_mask")
    return _result(out, device, stream, keep=(k1, k2))


# ---------------------------------------------------------------------------------------- ground-truth label map (csrc/avl_gtmap.hip)
GT_MAX_CLASSES = 4096
GT_MAX_VOTES = 1 << 40        # n_voxels * n_classes
CONFUSION_MAX_CLASSES = 65536
CONFUSION_MAX_COUNTERS = 1 << 28
UNLABELLED = -1               # label of a voxel / cell no vote reached


def _is_dev(x):
    return isinstance(x, (DeviceArray, DeviceView)) or _is_torch(x)


def _dtype_of(x):
    return str(x.dtype) if _is_torch(x) else np.dtype(getattr(x, "dtype", object))


def _ids_i32(x, what):
    """object / class ids of any integer dtype -> int32 on the host (a device array must be int32 already); ids that do not fit raise"""
    if _is_dev(x):
        if _dtype_of(x) not in ("torch.int32", np.dtype(np.int32)):
            raise TypeError(f"{what} on the device must be int32, got {_dtype_of(x)}")
        return x
    a = np.asarray(x)
    if a.dtype.kind not in "iu":
        raise TypeError(f"{what} must hold integers, got {a.dtype}")
    if a.size and (int(a.max()) >= 2 ** 31 or int(a.min()) < -2 ** 31):
        raise ValueError(f"{what}: ids must fit int32 (largest {int(a.max())}, smallest {int(a.min())})")
    return np.ascontiguousarray(a, dtype=np.int32)


def obj2cls_table(obj2cls):
    """-> int32 table (n_obj,) object id -> class id (-1 = no class), or None.  obj2cls: None, an integer array, a dict
    {object id: class id | (class id, name)} (the values of dataset/README.md:80-90's obj2cls, keys int or str) or a path to a .npy
    (array) or .json (dict or list) file.  Ids that do not fit int32 and negative object ids raise ValueError."""
    if obj2cls is None:
        return None
    if isinstance(obj2cls, (str, Path)):
        path = Path(obj2cls)
        if path.suffix == ".npy":
            obj2cls = np.load(path, allow_pickle=False)
        elif path.suffix == ".json":
            import json
            obj2cls = json.loads(path.read_text())
        else:
            raise ValueError(f"obj2cls: {path} is neither .npy nor .json")
    if isinstance(obj2cls, dict):
        items = []
        for k, v in obj2cls.items():
            v = v[0] if isinstance(v, (tuple, list)) else v
            items.append((int(k), int(v)))
        if any(k < 0 for k, _ in items):
            raise ValueError("obj2cls: negative object id")
        if any(k >= 2 ** 31 or not -2 ** 31 <= v < 2 ** 31 for k, v in items):
            raise ValueError("obj2cls: ids must fit int32")
        table = np.full((max((k for k, _ in items), default=-1) + 1,), -1, np.int32)
        for k, v in items:
            table[k] = v
        return table
    table = _ids_i32(np.asarray(obj2cls), "obj2cls")
    if table.ndim != 1:
        raise ValueError(f"obj2cls: expected a 1-D table, got shape {table.shape}")
    return table


def check_label_flag(err_flag, what, stream=None):
    """raise AvlError when a label kernel found data out of range (bit 0 of its device error flag)"""
    if int(err_flag.numpy(stream)[0]) != 0:
        raise _lib.AvlError(f"{what}: an id on the device is out of range (a voxel id >= n_voxels, or a label >= the number of classes)")


def _counter_check(x, shape, dtype, what):
    """the host-side checks of an in-place counter array (None, a host array or a DeviceArray), before any device work"""
    if x is None:
        return
    if not isinstance(x, (np.ndarray, DeviceArray)) or np.dtype(x.dtype) != np.dtype(dtype):
        raise TypeError(f"{what} must be a host array or DeviceArray of {np.dtype(dtype)}, got {getattr(x, 'dtype', type(x).__name__)}")
    if tuple(int(s) for s in x.shape) != tuple(shape):
        raise ValueError(f"{what} must have shape {tuple(shape)}, got {tuple(x.shape)}")


def _counter_arg(x, shape, dtype, stream):
    """an in-place counter array that passed _counter_check: None (new, zero), a host array (updated in place) or a DeviceArray
    -> (ptr, owner, host)"""
    if x is None:
        d = DeviceArray(shape, dtype).zero_(stream)
        return d.ptr, d, None
    if isinstance(x, np.ndarray):
        d = DeviceArray.from_numpy(x, stream)
        return d.ptr, d, x
    return x.ptr, x, None


def _counter_result(owner, host, device, stream):
    if device:
        return owner
    out = owner.numpy(stream)
    if host is not None:
        np.copyto(host, out)
        return host
    return out


def gt_vote(votes, depth, semantic, calib, transforms, occupied_ids, n_voxels, n_classes, cs, stride=1, min_depth=0.1, max_depth=6.0,
            obj2cls=None, depth_div=1000.0, stats=None, err_flag=None, device=False, stream=None):
    """Fold the semantic frames of F views into per-voxel class counts (avl_gt_vote; the vote is defined at the top of
    csrc/avl_gtmap.hip).  -> (votes (n_voxels, n_classes) uint32, stats (4,) uint64: pixels dropped by depth or grid, by class,
    for want of a voxel, and votes cast).  votes / stats: None (new, zero), a host array (updated in place and returned) or a
    DeviceArray (updated in place; returned as it is with device=True).  depth: (F, H, W) or (H, W), uint16 (value / depth_div
    metres) or float32 metres; semantic: the same shape, object ids of any integer dtype (converted to int32 on the host; a device
    array must be int32), or class ids when obj2cls is None; obj2cls: an int table object id -> class id (see obj2cls_table), host
    or device; calib: the 3 x 3 camera matrix; transforms: (F, 4, 4) camera -> map (VLMapBuilder.frame_transforms); occupied_ids:
    the map's (gs, gs, vh) int32 voxel index, host or device.  err_flag: a zeroed (1,) int32 DeviceArray to collect the error bit
    of several calls (check it with check_label_flag); None: this call checks its own, which waits for the launch.  TypeError on
    other dtypes, ValueError on bad shapes or parameters, before any device work."""
    stride, n_voxels, n_classes = int(stride), int(n_voxels), int(n_classes)
    if stride < 1:
        raise ValueError(f"gt_vote: stride {stride} < 1")
    if not 1 <= n_classes <= GT_MAX_CLASSES:
        raise ValueError(f"gt_vote: {n_classes} classes (1 .. {GT_MAX_CLASSES})")
    if n_voxels < 0 or n_voxels * n_classes >= GT_MAX_VOTES:
        raise ValueError(f"gt_vote: {n_voxels} voxels x {n_classes} classes (N * C < 2^40)")
    if not (np.isfinite(cs) and cs > 0):
        raise ValueError(f"gt_vote: cell size {cs}")
    if not (np.isfinite(min_depth) and np.isfinite(max_depth) and 0 <= min_depth < max_depth):
        raise ValueError(f"gt_vote: depth range ({min_depth}, {max_depth})")
    ddt = _dtype_of(depth)
    if ddt not in ("torch.uint16", "torch.int16", "torch.float32", np.dtype(np.uint16), np.dtype(np.float32)):
        raise TypeError(f"depth must be uint16 (value / depth_div metres) or float32 metres, got {ddt}")
    dshape = tuple(int(s) for s in depth.shape)
    if len(dshape) == 2:
        dshape = (1,) + dshape
    if len(dshape) != 3 or dshape[1] < 1 or dshape[2] < 1:
        raise ValueError(f"gt_vote: depth must be (F, H, W) or (H, W), got shape {tuple(depth.shape)}")
    F, H, W = dshape
    semantic = _ids_i32(semantic, "semantic")
    sshape = tuple(int(s) for s in semantic.shape)
    if (sshape if len(sshape) == 3 else (1,) + sshape) != dshape:
        raise ValueError(f"gt_vote: depth frames of shape {dshape} but semantic frames of shape {sshape}")
    K = np.asarray(calib, dtype=np.float64)
    if K.size != 9:
        raise ValueError(f"gt_vote: calib must be 3 x 3, got shape {K.shape}")
    T = np.ascontiguousarray(transforms, dtype=np.float64)
    if T.shape not in ((F, 4, 4), (4, 4)) or T.size != F * 16:
        raise ValueError(f"gt_vote: {F} frames but transforms of shape {T.shape}")
    if _dtype_of(occupied_ids) not in ("torch.int32", np.dtype(np.int32)):
        raise TypeError(f"occupied_ids must be int32, got {_dtype_of(occupied_ids)}")
    oshape = tuple(int(s) for s in occupied_ids.shape)
    if len(oshape) != 3 or oshape[0] != oshape[1] or not 1 <= oshape[0] <= EXPLORE_MAX_SIDE or oshape[2] < 1:
        raise ValueError(f"gt_vote: occupied_ids must be (gs, gs, vh) with gs <= {EXPLORE_MAX_SIDE}, got shape {oshape}")
    gs, vh = oshape[0], oshape[2]
    if obj2cls is not None:
        obj2cls = _ids_i32(obj2cls, "obj2cls")
        if len(obj2cls.shape) != 1 or int(obj2cls.shape[0]) < 1:
            raise ValueError(f"gt_vote: obj2cls must be a non-empty 1-D table, got shape {tuple(obj2cls.shape)}")
    _counter_check(votes, (n_voxels, n_classes), np.uint32, "votes")
    _counter_check(stats, (4,), np.uint64, "stats")
    lib = _lib.load()
    _lib.require_gpu()
    vp, vown, vhost = _counter_arg(votes, (n_voxels, n_classes), np.uint32, stream)
    sp, sown, shost = _counter_arg(stats, (4,), np.uint64, stream)
    own_flag = err_flag is None
    if own_flag:
        err_flag = DeviceArray((1,), np.int32).zero_(stream)
    keep = []
    if F:
        Kinv = np.ascontiguousarray(np.linalg.inv(K.reshape(3, 3)))
        dp, _, k1, is_u16 = _global_depth(depth, stream)
        mp, _, k2 = as_device(semantic, np.int32, stream)
        op, _, k3 = as_device(occupied_ids, np.int32, stream)
        tp, n_obj, k4 = None, 0, None
        if obj2cls is not None:
            tp, _, k4 = as_device(obj2cls, np.int32, stream)
            n_obj = int(obj2cls.shape[0])
        keep = [k1, k2, k3, k4]
        _lib.check(lib.avl_gt_vote(dp, int(is_u16), float(depth_div), mp, F, H, W, Kinv.ctypes.data, T.ctypes.data, gs, float(cs), vh, stride,
                                   float(min_depth), float(max_depth), tp, n_obj, n_classes, op, n_voxels, vp, sp, err_flag.ptr, stream),
                   "avl_gt_vote")
    if own_flag:
        check_label_flag(err_flag, "gt_vote", stream)
    elif device:
        _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")              # the staged frames may be released on return
    del keep
    return _counter_result(vown, vhost, device, stream), _counter_result(sown, shost, device, stream)


def gt_labels(votes, device=False, stream=None):
    """-> (label (N,) int32, support (N,) uint32) of a (N, C) uint32 vote array, host or device (avl_gt_labels): the lowest class
    whose count is the row's maximum, UNLABELLED (-1) for an all-zero row, and the row's sum (wrapping at 2^32)."""
    if not isinstance(votes, (np.ndarray, DeviceArray, DeviceView)) or np.dtype(votes.dtype) != np.dtype(np.uint32):
        raise TypeError(f"votes must be a host array or DeviceArray of uint32, got {getattr(votes, 'dtype', type(votes).__name__)}")
    shape = tuple(int(s) for s in votes.shape)
    if len(shape) != 2 or not 1 <= shape[1] <= GT_MAX_CLASSES or shape[0] * shape[1] >= GT_MAX_VOTES:
        raise ValueError(f"gt_labels: votes must be (N, C) with 1 <= C <= {GT_MAX_CLASSES} and N * C < 2^40, got shape {shape}")
    lib = _lib.load()
    _lib.require_gpu()
    N, C_ = shape
    if isinstance(votes, np.ndarray):
        keep = DeviceArray.from_numpy(votes, stream)
        vp = keep.ptr
    else:
        vp, keep = votes.ptr, votes
    label, support = DeviceArray((N,), np.int32), DeviceArray((N,), np.uint32)
    _lib.check(lib.avl_gt_labels(vp, N, C_, label.ptr, support.ptr, stream), "avl_gt_labels")
    if device:
        label._keep = support._keep = (keep,)
        return label, support
    return label.numpy(stream), support.numpy(stream)


def pool_labels_2d(labels, occupied_ids, window=None, err_flag=None, device=False, stream=None):
    """The label-valued top-down pool (avl_pool_labels_2d): (r1 - r0 + 1, c1 - c0 + 1) int32 over window = (r0, r1, c0, c1), both
    ends included (None: the whole grid); a cell holds the label of the highest voxel of its column that has one (label >= 0),
    UNLABELLED (-1) when none has.  labels: (N,) int32; occupied_ids: (gs, gs, vh) int32; host or device."""
    labels = _ids_i32(labels, "labels")
    if _dtype_of(occupied_ids) not in ("torch.int32", np.dtype(np.int32)):
        raise TypeError(f"occupied_ids must be int32, got {_dtype_of(occupied_ids)}")
    oshape = tuple(int(s) for s in occupied_ids.shape)
    if len(oshape) != 3 or oshape[0] != oshape[1] or not 1 <= oshape[0] <= EXPLORE_MAX_SIDE or oshape[2] < 1:
        raise ValueError(f"pool_labels_2d: occupied_ids must be (gs, gs, vh) with gs <= {EXPLORE_MAX_SIDE}, got shape {oshape}")
    if len(labels.shape) != 1:
        raise ValueError(f"pool_labels_2d: labels must be (N,), got shape {tuple(labels.shape)}")
    gs, vh = oshape[0], oshape[2]
    r0, r1, c0, c1 = (0, gs - 1, 0, gs - 1) if window is None else (int(w) for w in window)
    if not (0 <= r0 <= r1 < gs and 0 <= c0 <= c1 < gs):
        raise ValueError(f"pool_labels_2d: window rows {r0} .. {r1}, columns {c0} .. {c1} of a grid of {gs}")
    lib = _lib.load()
    _lib.require_gpu()
    lp, _, k1 = as_device(labels, np.int32, stream)
    op, _, k2 = as_device(occupied_ids, np.int32, stream)
    own_flag = err_flag is None
    if own_flag:
        err_flag = DeviceArray((1,), np.int32).zero_(stream)
    out = DeviceArray((r1 - r0 + 1, c1 - c0 + 1), np.int32)
    _lib.check(lib.avl_pool_labels_2d(lp, int(labels.shape[0]), op, gs, vh, r0, r1, c0, c1, out.ptr, err_flag.ptr, stream),
               "avl_pool_labels_2d")
    if own_flag:
        check_label_flag(err_flag, "pool_labels_2d", stream)
    return _result(out, device, stream, keep=(k1, k2))


def label_confusion_limits() -> int:
    """the largest n_gt_classes * n_pred_classes label_confusion counts in LDS; larger matrices take global atomics"""
    n = C.c_int(0)
    _lib.check(_lib.load().avl_label_confusion_limits(C.byref(n)), "avl_label_confusion_limits")
    return n.value


def label_confusion(gt, pred, n_gt_classes, n_pred_classes, conf=None, skipped=None, err_flag=None, device=False, stream=None):
    """-> (conf (n_gt_classes, n_pred_classes) uint64, skipped (2,) uint64) of two label arrays of one length (avl_label_confusion):
    gt < 0 counts in skipped[0]; otherwise pred < 0 counts in skipped[1]; otherwise conf[gt, pred] += 1.  A label at or above its
    number of classes raises AvlError.  conf / skipped: None (new, zero), a host array (updated in place and returned) or a
    DeviceArray (updated in place).  gt, pred: int32 on the device, any integer dtype on the host."""
    Cg, Cp = int(n_gt_classes), int(n_pred_classes)
    if not (1 <= Cg <= CONFUSION_MAX_CLASSES and 1 <= Cp <= CONFUSION_MAX_CLASSES and Cg * Cp <= CONFUSION_MAX_COUNTERS):
        raise ValueError(f"label_confusion: a {Cg} x {Cp} matrix (sides 1 .. {CONFUSION_MAX_CLASSES}, at most 2^28 counters)")
    gt, pred = _ids_i32(gt, "gt"), _ids_i32(pred, "pred")
    gshape, pshape = tuple(int(s) for s in gt.shape), tuple(int(s) for s in pred.shape)
    if gshape != pshape:
        raise ValueError(f"label_confusion: gt of shape {gshape} but pred of shape {pshape}")
    n = int(np.prod(gshape, dtype=np.int64))
    _counter_check(conf, (Cg, Cp), np.uint64, "conf")
    _counter_check(skipped, (2,), np.uint64, "skipped")
    lib = _lib.load()
    _lib.require_gpu()
    cp_, cown, chost = _counter_arg(conf, (Cg, Cp), np.uint64, stream)
    sp, sown, shost = _counter_arg(skipped, (2,), np.uint64, stream)
    own_flag = err_flag is None
    if own_flag:
        err_flag = DeviceArray((1,), np.int32).zero_(stream)
    k1 = k2 = None
    if n:
        gp, _, k1 = as_device(gt, np.int32, stream)
        pp, _, k2 = as_device(pred, np.int32, stream)
        _lib.check(lib.avl_label_confusion(gp, pp, n, Cg, Cp, cp_, sp, err_flag.ptr, stream), "avl_label_confusion")
    if own_flag:
        check_label_flag(err_flag, "label_confusion", stream)
    elif device:
        _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")
    del k1, k2
    return _counter_result(cown, chost, device, stream), _counter_result(sown, shost, device, stream)


class MapScores:
    """the scores of a predicted label map against the ground truth (map_scores): pixel_acc, mean_acc, miou, fwiou (float64), the
    per-class acc and iou ((Cg,) float64, NaN for a class without ground truth), support ((Cg,) int64, the row sums), the integer
    matrix conf they come from and, when known, skipped = (entries without ground truth, entries without a prediction)"""

    def __init__(self, pixel_acc, mean_acc, miou, fwiou, acc, iou, support, conf, skipped=None, categories=None):
        self.pixel_acc, self.mean_acc, self.miou, self.fwiou = pixel_acc, mean_acc, miou, fwiou
        self.acc, self.iou, self.support, self.conf, self.skipped, self.categories = acc, iou, support, conf, skipped, categories

    def as_dict(self) -> dict:
        names = list(self.categories) if self.categories is not None else [str(k) for k in range(len(self.acc))]
        nan = lambda x: None if np.isnan(x) else float(x)      # noqa: E731
        return dict(pixel_acc=nan(self.pixel_acc), mean_acc=nan(self.mean_acc), miou=nan(self.miou), fwiou=nan(self.fwiou),
                    total=int(self.support.sum()), skipped=None if self.skipped is None else [int(s) for s in self.skipped],
                    classes=[dict(id=k, name=names[k] if k < len(names) else str(k), support=int(self.support[k]), acc=nan(self.acc[k]),
                                  iou=nan(self.iou[k])) for k in range(len(self.acc))])

    def __repr__(self):
        return (f"MapScores(pixel_acc={self.pixel_acc:.4f}, mean_acc={self.mean_acc:.4f}, miou={self.miou:.4f}, fwiou={self.fwiou:.4f}, "
                f"total={int(self.support.sum())})")


def map_scores(conf, skipped=None, categories=None) -> MapScores:
    """Pixel accuracy, mean accuracy, mIoU and frequency-weighted IoU of a (Cg, Cp) integer confusion matrix (rows = ground truth),
    host-side in float64:  pixel_acc = trace / total;  acc[k] = conf[k, k] / row_sum[k];  iou[k] = conf[k, k] / (row_sum[k] +
    col_sum[k] - conf[k, k]) with col_sum[k] = conf[k, k] = 0 for k >= Cp;  mean_acc, miou = np.mean over the classes with
    row_sum > 0 in class order;  fwiou = (sum of row_sum[k] * iou[k] over those classes, added in class order) / total.  Cp may
    exceed Cg (init_categories appends "other": a voxel predicted "other" is simply wrong).  An empty matrix gives NaN scores."""
    m = np.asarray(conf)
    if m.ndim != 2 or m.dtype.kind not in "iu":
        raise ValueError(f"map_scores: expected a 2-D integer matrix, got {m.dtype}{m.shape}")
    m = m.astype(np.int64)
    Cg, Cp = m.shape
    row_sum = m.sum(axis=1)
    col_sum, diag = np.zeros(Cg, np.int64), np.zeros(Cg, np.int64)
    k = min(Cg, Cp)
    col_sum[:k] = m.sum(axis=0)[:k]
    diag[:k] = np.diagonal(m)[:k]
    total = int(row_sum.sum())
    valid = row_sum > 0
    acc, iou = np.full(Cg, np.nan), np.full(Cg, np.nan)
    acc[valid] = diag[valid] / row_sum[valid]
    iou[valid] = diag[valid] / (row_sum[valid] + col_sum[valid] - diag[valid])
    if total == 0:
        return MapScores(np.nan, np.nan, np.nan, np.nan, acc, iou, row_sum, m, skipped, categories)
    weighted = 0.0
    for c in np.flatnonzero(valid):
        weighted += float(row_sum[c]) * float(iou[c])
    return MapScores(int(diag.sum()) / total, float(np.mean(acc[valid])), float(np.mean(iou[valid])), weighted / total, acc, iou, row_sum,
                     m, skipped, categories)
