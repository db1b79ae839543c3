"""Similarity scores, their prepared maps, and the selections over a score vector (csrc/avl_sim.hip, csrc/avl_rows.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from ..device import DeviceArray, as_device, _is_torch

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
        from ..device import torch_stream_ptr
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
        from ..device import torch_stream_ptr
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
        from ..device import torch_stream_ptr
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


def topk_f32(vals, k, stream=None):
    """(indices (k,) int64, values (k,) float32) of the k largest entries, descending, ties by ascending index."""
    lib = _lib.load()
    vp, vshape, vk = as_device(vals, np.float32, stream)
    idx = np.empty((k,), dtype=np.int64)
    val = np.empty((k,), dtype=np.float32)
    _lib.check(lib.avl_topk_f32(vp, int(np.prod(vshape)), int(k), idx.ctypes.data, val.ctypes.data, stream), "avl_topk_f32")
    return idx, val
