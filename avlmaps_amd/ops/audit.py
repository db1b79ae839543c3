"""The visibility audit of a voxel map: a device cell index of the voxel list and the 3-D sight-ray pass over it
(csrc/avl_audit.hip).  Upstream has no counterpart: its maps are static."""
from __future__ import annotations

import numpy as np

from .. import _lib
from ..device import DeviceArray, DeviceView, as_device, _is_torch
from ._args import _image_shape, _workspace
from ._rays import frame_args
from .builder import _global_depth

AUDIT_MAX_SIDE = 16384
NEVER_HIT = -1              # last_hit of a voxel no depth ray ended in; `after` of a voxel every frame counts for


def _check_grid(who, gs, vh):
    gs, vh = int(gs), int(vh)
    if not (1 <= gs <= AUDIT_MAX_SIDE and vh >= 1 and gs * gs * vh < 2 ** 31 - 1):
        raise ValueError(f"{who}: grid {gs} x {gs} x {vh} (gs 1 .. {AUDIT_MAX_SIDE}, vh >= 1, gs * gs * vh < 2^31)")
    return gs, vh


class CellIndex:
    """cell_index's result: the lookup cell (row, col, h) -> voxel row of an N-voxel list on a gs x gs x vh grid, one device buffer
    (an occupancy bitmap, the prefix of its words' popcounts, a rank -> row permutation).  Lives until close()."""

    def __init__(self, buf, nbytes, N, gs, vh, keep=None):
        self.buf, self.nbytes, self.N, self.gs, self.vh, self._keep = buf, int(nbytes), int(N), int(gs), int(vh), keep

    @property
    def ptr(self):
        if self.buf is None:
            raise ValueError("the cell index has been closed")
        return self.buf.ptr

    def close(self):
        if self.buf is not None:
            self.buf.free()
        self.buf = self._keep = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _cells_i32(x, what):
    """(N, 3) integer cells, host or device -> (the argument ready for as_device, N)"""
    shape = _image_shape(x)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"{what}: expected (N, 3) cells, got shape {shape}")
    if not (isinstance(x, (DeviceArray, DeviceView)) or _is_torch(x)):
        x = np.asarray(x)
        if x.dtype.kind not in "iu" or (x.size and not (-2 ** 31 <= int(x.min()) and int(x.max()) <= 2 ** 31 - 1)):
            raise TypeError(f"{what}: cells are int32 values, got {x.dtype}")
    return x, shape[0]


def cell_index(grid_pos, gs, vh, stream=None) -> CellIndex:
    """Build the CellIndex of grid_pos (N, 3) int32 cells (row, col, h), a host array, a DeviceArray / DeviceView or a GPU tensor
    (avl_cell_index_build).  Rows outside the grid are ignored: no probe finds them.  Of several rows in one cell the largest row
    index owns it.  N = 0 is valid.  gs * gs * vh < 2^31."""
    gs, vh = _check_grid("cell_index", gs, vh)
    grid_pos, N = _cells_i32(grid_pos, "cell_index")
    lib = _lib.load()
    buf, nbytes = _workspace(lib.avl_cell_index_work_bytes, "avl_cell_index_work_bytes", N, gs, vh)
    pp, _, keep = as_device(grid_pos, np.int32, stream)
    _lib.check(lib.avl_cell_index_build(pp, N, gs, vh, buf.ptr, nbytes, stream), "avl_cell_index_build")
    return CellIndex(buf, nbytes, N, gs, vh, keep)


def lookup_cells(index: CellIndex, cells, device=False, stream=None):
    """(M,) int32: the voxel row that owns each of the M cells (M, 3) (row, col, h), -1 where the cell is empty or outside the grid
    (avl_cell_index_lookup)."""
    if not isinstance(index, CellIndex):
        raise TypeError(f"lookup_cells: expected a CellIndex, got {type(index).__name__}")
    cells, M = _cells_i32(cells, "lookup_cells")
    lib = _lib.load()
    _lib.require_gpu()
    out = DeviceArray((M,), np.int32)
    keep = None
    if M:
        cp, _, keep = as_device(cells, np.int32, stream)
        _lib.check(lib.avl_cell_index_lookup(index.ptr, index.nbytes, index.N, index.gs, index.vh, cp, M, out.ptr, stream),
                   "avl_cell_index_lookup")
    if device:
        out._keep = (keep, index)
        return out
    return out.numpy(stream)


def _per_voxel(x, name, dtype, N):
    """an optional per-voxel array of the audit: None, a host array of `dtype` or a DeviceArray / DeviceView / GPU tensor of it"""
    if x is None:
        return None
    if _is_torch(x):
        dt = {"torch.int32": np.dtype(np.int32), "torch.uint32": np.dtype(np.uint32)}.get(str(x.dtype))
    else:
        dt = getattr(x, "dtype", None)
        dt = None if dt is None else np.dtype(dt)
    if dt != np.dtype(dtype):
        raise TypeError(f"{name} must be {np.dtype(dtype)}, got {getattr(x, 'dtype', type(x).__name__)}")
    if tuple(int(s) for s in x.shape) != (N,):
        raise ValueError(f"audit_rays: {name} must be ({N},), got shape {tuple(x.shape)}")
    return x


def _stage(x, dtype, stream):
    """-> (device pointer, the device array that holds the bytes, the host array to copy back into or None)"""
    if x is None:
        return None, None, None
    if isinstance(x, np.ndarray):
        d = DeviceArray.from_numpy(x, stream)
        return d.ptr, d, x
    if _is_torch(x):
        if not x.is_cuda or not x.is_contiguous():
            raise TypeError("torch tensors passed to avlmaps_amd must be contiguous and live on the GPU")
        return x.data_ptr(), x, None
    return x.ptr, x, None


def audit_rays(index: CellIndex, depth, calib, transforms, frame_ids, cs, stride=4, h_min=None, h_max=None, min_depth=0.1,
               max_depth=6.0, depth_div=1000.0, end_margin=2, last_hit=None, through=None, after=None, device=False, stream=None):
    """Fold the sight rays of F depth frames into last_hit (N,) int32 -- the largest frame id whose depth ray ended in a voxel,
    NEVER_HIT (-1) where none did -- and through (N,) uint32 -- the rays that passed through a voxel's cell on their way to
    something further away (avl_audit_rays; the ray and the walk are defined at the top of csrc/avl_audit.hip).  A cell counts as
    passed through when it lies more than end_margin steps before the surface the ray ends on, or anywhere on a ray without a
    surface at its end (a far ray, or one cut by the height band [h_min, h_max], default [-cs, vh * cs]); with `after` (N,) int32
    only for frames with id > after[voxel].  depth, calib, transforms, frame_ids as carve_free_space takes them.  last_hit,
    through, after: None, a host array (last_hit and through are updated in place) or a device array (updated in place).  Returns
    (last_hit, through), each None where it was not given; with device=True a host array is not written back and its updated
    device copy (a DeviceArray) is returned in its place.  Both folds
    commute: calls may come in any order and continue each other.  through does not saturate: it wraps after 2^32 rays through one
    voxel.  TypeError on other dtypes, ValueError on bad shapes or parameters, before any device work."""
    if not isinstance(index, CellIndex):
        raise TypeError(f"audit_rays: expected a CellIndex, got {type(index).__name__}")
    gs, vh, N = index.gs, index.vh, index.N
    stride, end_margin = int(stride), int(end_margin)
    if end_margin < 0:
        raise ValueError(f"audit_rays: end_margin {end_margin} < 0")
    if np.isfinite(cs):                                 # (any other cell size is refused below, before the band is looked at)
        h_min = -float(cs) if h_min is None else h_min
        h_max = vh * float(cs) if h_max is None else h_max
    F, H, W, Kinv, T, ids = frame_args("audit_rays", depth, calib, transforms, frame_ids, stride, cs, min_depth, max_depth,
                                       h_band=(h_min, h_max), depth_div=depth_div)
    last_hit = _per_voxel(last_hit, "last_hit", np.int32, N)
    through = _per_voxel(through, "through", np.uint32, N)
    after = _per_voxel(after, "after", np.int32, N)
    lib = _lib.load()
    _lib.require_gpu()
    ip = index.ptr                                      # a closed index raises here
    lp, ld, lhost = _stage(last_hit, np.int32, stream)
    tp, td, thost = _stage(through, np.uint32, stream)
    ap, ad, _ = _stage(after, np.int32, stream)
    if F and (lp or tp):
        dp, _, keep_d, is_u16 = _global_depth(depth, stream)
        _lib.check(lib.avl_audit_rays(ip, index.nbytes, N, gs, vh, dp, int(is_u16), float(depth_div), F, H, W, Kinv.ctypes.data,
                                      T.ctypes.data, ids.ctypes.data, float(cs), stride, float(h_min), float(h_max), float(min_depth),
                                      float(max_depth), end_margin, lp, tp, ap, stream), "avl_audit_rays")
    out = []
    for dev, host in ((ld, lhost), (td, thost)):
        if host is not None and not device:
            back = dev.numpy(stream)                    # (synchronous: the staged arrays may go)
            np.copyto(host, back)
            dev.free()
            out.append(host)
        else:
            out.append(dev)
    _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")          # the staged depth and `after` may be released on return
    if isinstance(after, np.ndarray) and ad is not None:
        ad.free()
    return tuple(out)
