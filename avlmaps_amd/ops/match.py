"""Registration of depth frames to a voxel map: correlative scan matching on the CellIndex of ops/audit.py (csrc/avl_match.hip,
DESIGN.md 4.23).  Upstream has no counterpart: it takes the poses of a recording on trust.

The search is planar -- a table of rotations about z and whole-cell shifts in row and col; pitch, roll and height are not searched --
and it counts occupied cells only: free space that a frame saw through does not speak against a pose."""
from __future__ import annotations

import math

import numpy as np

from .. import _lib
from ..device import DeviceArray
from ._args import _workspace
from ._rays import frame_args
from .audit import CellIndex
from .builder import _global_depth

MATCH_MAX_ANGLES = 1024
MATCH_MAX_RADIUS = 64
MATCH_MAX_SPLIT = 65536


def match_angles(max_deg, step_deg) -> np.ndarray:
    """(K, 2) float64 (cos, sin) of the angles -n * step .. n * step degrees, n = floor(max_deg / step_deg): K = 2n + 1 entries,
    the middle one exactly (1, 0), and entry n + j the mirror image of entry n - j (the same cos, the negated sin)."""
    max_deg, step_deg = float(max_deg), float(step_deg)
    if not (math.isfinite(max_deg) and max_deg >= 0.0 and math.isfinite(step_deg) and step_deg > 0.0):
        raise ValueError(f"match_angles: max_deg {max_deg} (>= 0), step_deg {step_deg} (> 0)")
    n = int(math.floor(max_deg / step_deg + 1e-9))
    if 2 * n + 1 > MATCH_MAX_ANGLES:
        raise ValueError(f"match_angles: {2 * n + 1} angles (at most {MATCH_MAX_ANGLES})")
    out = np.zeros((2 * n + 1, 2), np.float64)
    out[n] = (1.0, 0.0)
    for j in range(1, n + 1):
        a = math.radians(j * step_deg)
        out[n + j] = (math.cos(a), math.sin(a))
        out[n - j] = (math.cos(a), -math.sin(a))
    return out


def _angle_table(angles, k0):
    """-> ((K, 2) float64, k0): the table checked, and the prior index -- the caller's, or the table's first (1, 0) entry"""
    a = np.ascontiguousarray(angles, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 2 or not 1 <= a.shape[0] <= MATCH_MAX_ANGLES:
        raise ValueError(f"match_frames: angles must be (K, 2) (cos, sin) with 1 <= K <= {MATCH_MAX_ANGLES}, got shape {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError("match_frames: an angle's cos or sin is not finite")
    if k0 is None:
        zero = np.flatnonzero((a[:, 0] == 1.0) & (a[:, 1] == 0.0))
        if len(zero) == 0:
            raise ValueError("match_frames: the angle table has no (1, 0) entry: pass k0, the index of the prior's angle")
        return a, int(zero[0])
    k0 = int(k0)
    if not 0 <= k0 < a.shape[0]:
        raise ValueError(f"match_frames: k0 {k0} (0 .. {a.shape[0] - 1})")
    return a, k0


class MatchResult:
    """match_frames's result.  scores (V, K, S, S) uint32, S = 2 * radius + 1: scores[v, k, di + radius, dj + radius] = the points of
    volume v that land on an occupied cell when rotated by angle k and shifted by (di, dj) cells.  best (V, 4) int32 = (k, di, dj,
    score) of each volume's winner.  valid (V,) uint32 = the volume's points inside the depth range and the height band.  With
    device=True the three are DeviceArrays (read fraction and corrections from their .numpy())."""

    def __init__(self, scores, best, valid, radius, keep=(), workspace=None):
        self.scores, self.best, self.valid, self.radius, self._keep, self._workspace = scores, best, valid, int(radius), keep, workspace

    def free(self) -> None:
        """release the three device arrays of a device=True result and the call's workspace (a host result holds none); the
        caller's own inputs are left alone.  Synchronise the call's stream first"""
        for x in (self.scores, self.best, self.valid, self._workspace):
            if isinstance(x, DeviceArray):
                x.free()
        self._keep, self._workspace = (), None

    @property
    def fraction(self) -> np.ndarray:
        """(V,) float64: the winner's score over valid, 0 where a volume has no valid point"""
        best, valid = _host(self.best), _host(self.valid).astype(np.float64)
        return np.divide(best[:, 3].astype(np.float64), valid, out=np.zeros(len(valid)), where=valid > 0)

    def corrections(self, cs, angles, pivots) -> np.ndarray:
        """(V, 4, 4) float64: C = Trans(-di * cs, -dj * cs, 0) @ Trans(pivot) @ Rz(cos_k, sin_k) @ Trans(-pivot) of every volume's
        winner, to be left-multiplied onto the prior transforms (corrected = C @ T).  angles: the table the call was made with;
        pivots: (V, 2), or one (2,) pivot for all volumes.  The shift is a whole number of cells: the translation is accurate to one
        cell, cs metres, and no better."""
        best = _host(self.best)
        a = np.asarray(angles, dtype=np.float64).reshape(-1, 2)
        piv = np.broadcast_to(np.asarray(pivots, dtype=np.float64).reshape(-1, 2), (len(best), 2))
        out = np.zeros((len(best), 4, 4), np.float64)
        for v, (k, di, dj, _) in enumerate(best.tolist()):
            c, s = a[k]
            px, py = piv[v]
            to, rot, back, shift = np.eye(4), np.eye(4), np.eye(4), np.eye(4)
            to[:2, 3] = (-px, -py)
            rot[:2, :2] = ((c, -s), (s, c))
            back[:2, 3] = (px, py)
            shift[:2, 3] = (-di * float(cs), -dj * float(cs))
            out[v] = shift @ back @ rot @ to
        return out


def _host(x):
    return x.numpy() if isinstance(x, DeviceArray) else np.asarray(x)


def match_frames(index: CellIndex, depth, calib, transforms, cs, angles, radius, stride=4, min_depth=0.1, max_depth=6.0, h_band=(2, None),
                 joint=False, pivot=None, k0=None, device=False, stream=None, depth_div=1000.0, split=None) -> MatchResult:
    """Score the F depth frames against the map of `index` over every angle of `angles` ((K, 2) float64 (cos, sin), match_angles) and
    every shift of [-radius, radius]^2 cells (avl_match_frames; the definition is at the top of csrc/avl_match.hip).  depth, calib
    and transforms (the priors) as audit_rays takes them; only points with min_depth < z < max_depth whose height cell lies in
    h_band = (lo, hi), inclusive, None = the grid's last cell, take part.  joint=False: a volume per frame (V = F), rotated about
    the frame's own origin.  joint=True: one volume (V = 1) of all frames, rotated about `pivot` (x, y), default the first
    frame's origin.  k0: the index of the prior's angle, which ties fall to; default the table's (1, 0) entry.  The winner of a
    volume is the largest score, then the smallest di^2 + dj^2, then the smallest |k - k0|, then the smallest k, di, dj.  The search
    is planar and a shift is a whole number of cells: MatchResult.corrections is accurate to one cell.  split: over how many blocks
    at most a volume's list of points is spread in the scoring kernel (1 .. MATCH_MAX_SPLIT), None to have the library choose; it
    changes the launch, never the results.  With device=True free the result with MatchResult.free().  TypeError on a
    non-CellIndex or another depth dtype, ValueError on bad shapes or parameters, before any device work."""
    if not isinstance(index, CellIndex):
        raise TypeError(f"match_frames: expected a CellIndex, got {type(index).__name__}")
    gs, vh, N = index.gs, index.vh, index.N
    stride, radius, joint = int(stride), int(radius), bool(joint)
    if not 0 <= radius <= MATCH_MAX_RADIUS:
        raise ValueError(f"match_frames: radius {radius} (0 .. {MATCH_MAX_RADIUS} cells)")
    if split is not None and not 1 <= int(split) <= MATCH_MAX_SPLIT:
        raise ValueError(f"match_frames: split {split} (None, or 1 .. {MATCH_MAX_SPLIT} blocks per list)")
    angles, k0 = _angle_table(angles, k0)
    K, S = angles.shape[0], 2 * radius + 1
    h_lo = 0 if h_band[0] is None else int(h_band[0])
    h_hi = vh - 1 if h_band[1] is None else int(h_band[1])
    if not 0 <= h_lo <= h_hi < vh:
        raise ValueError(f"match_frames: height band [{h_lo}, {h_hi}] (0 <= lo <= hi < {vh} cells)")
    F, H, W, Kinv, T, _ = frame_args("match_frames", depth, calib, transforms, None, stride, cs, min_depth, max_depth, depth_div=depth_div)
    T = T.reshape(F, 4, 4)
    V = 1 if joint else F
    if V * K * S * S >= 2 ** 31:
        raise ValueError(f"match_frames: {V} volumes x {K} angles x {S}^2 shifts (fewer than 2^31 scores)")
    if (gs + 2 * radius) ** 2 * vh >= 2 ** 32:
        raise ValueError(f"match_frames: grid {gs} + 2 * {radius} cells a side x {vh}: (gs + 2R)^2 * vh must stay below 2^32")
    if pivot is None:
        pivot = (T[0, 0, 3], T[0, 1, 3]) if F else (0.0, 0.0)
    px, py = (float(x) for x in np.asarray(pivot, dtype=np.float64).reshape(2))
    if joint and not (math.isfinite(px) and math.isfinite(py)):
        raise ValueError(f"match_frames: the pivot ({px}, {py}) is not finite")
    if not joint and not np.all(np.isfinite(T[:, :2, 3])):
        raise ValueError("match_frames: a frame's origin, its pivot, is not finite")
    lib = _lib.load()
    ip = index.ptr                                      # a closed index raises here
    ws, ws_bytes = _workspace(lib.avl_match_ws_bytes, "avl_match_ws_bytes", F, H, W, stride, K, radius, int(joint))
    scores, best, valid = DeviceArray((V, K, S, S), np.uint32), DeviceArray((V, 4), np.int32), DeviceArray((V,), np.uint32)
    keep = (index,)
    if F:
        dp, _, keep_d, is_u16 = _global_depth(depth, stream)
        _lib.check(lib.avl_match_frames(ip, index.nbytes, N, gs, vh, dp, int(is_u16), float(depth_div), F, H, W, Kinv.ctypes.data, T.ctypes.data,
                                        float(cs), stride, float(min_depth), float(max_depth), angles.ctypes.data, K, radius, h_lo, h_hi,
                                        int(joint), px, py, k0, 0 if split is None else int(split), scores.ptr, best.ptr, valid.ptr, ws.ptr, ws_bytes, stream), "avl_match_frames")
        keep += (keep_d,)
    elif V:                                             # joint mode without a frame: the empty volume's answer, no kernel
        scores.zero_(stream)
        valid.zero_(stream)
        best.free()
        best = DeviceArray.from_numpy(np.array([[k0, 0, 0, 0]], np.int32), stream)
    if device:
        return MatchResult(scores, best, valid, radius, keep, ws)
    out = MatchResult(scores.numpy(stream), best.numpy(stream), valid.numpy(stream), radius)       # (synchronous: the staged arrays may go)
    for d in (scores, best, valid, ws):
        d.free()
    return out
