"""Raw-map similarity calls that consist of ONE resident launch recompute the rows their range guard flags inside that launch
(csrc/avl_sim.hip: split_epilogue -> fixup_row) instead of publishing guard words for sim_fixup_rows_kernel.  Through the C ABI:

  * rows inside the guard's range: bit-identical to avl_sim_scores_prepared on an avl_sim_prepare_map copy made without row
    scales (the identity the project guarantees: the same split8 operands);
  * flagged rows: bit-identical to the first Q columns of a call that still ends in the stand-alone fix-up kernel (the same map
    against 128 queries whose first Q rows are the same: several launches), argmax / best with np.argmax semantics (first NaN
    wins, else the first maximum);
  * every subset of the outputs, ld_feat > D, no workspace, and a column-block call against the dense call on each window.

Small shapes only: every N at which the tile / tail-round split of the kernel changes, the run-time and the unrolled k loop."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = (1, 31, 32, 33, 255, 257, 70_001)      # 70 001: more than one full round of 256-row tiles on 256 CUs + a ragged tail
DS = (64, 128, 512)                         # run-time k loop (64, 128) and the unrolled NSTEPS = 8 path (512)
QS = (1, 2, 33, 64, 65, 78)
QREF = 128                                  # > 96 resident rows: query chunks or the streamed kernel, then sim_fixup_rows_kernel
GUARD_LO, GUARD_HI = 2.0 ** -7, 2.0 ** 15   # kGuardLo / kGuardHi
COL_POS, COL_ONE, COL_SEVERAL = 5, 3, 7     # columns of the planted +inf elements (see _queries)


@pytest.fixture(scope="module")
def env():
    import torch
    from avlmaps_amd import _lib
    lib = _lib.load()
    _lib.require_gpu()
    return lib, _lib, torch


def _planted_rows(N):
    """first / interior / last position of a 32-row unit, in the first tile, in a later tile and in the tail round"""
    rows = [0, 13, 31, 32, 64 + 17, 255, 256, 65_536, 65_536 + 31, 69_984 + 13, N - 2, N - 1]
    return sorted({r for r in rows if 0 <= r < N})


KINDS = ("zero", "tiny", "huge", "inf", "nan_one", "nan_several", "nan_all")


def _map(N, D, seed):
    """LSeg-scale rows with flagged rows planted; returns the map and {row: kind}"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((N, D)).astype(np.float32)
    kinds = {}
    for i, r in enumerate(_planted_rows(N)):
        k = KINDS[(i + seed) % len(KINDS)]
        kinds[r] = k
        if k == "zero":
            f[r] = 0                                     # in range by definition (largest |element| == 0): scores are exact zeros
        elif k == "tiny":
            f[r] *= np.float32(1e-9)
        elif k == "huge":
            f[r] *= np.float32(1e6)
        elif k == "inf":
            f[r, COL_POS] = np.inf                       # every query is non-zero there: +-inf scores, no NaN
        elif k == "nan_one":
            f[r, COL_ONE] = np.inf                       # inf * 0 = NaN in ONE query product
        elif k == "nan_several":
            f[r, COL_SEVERAL] = np.inf                   # ... in every other query product
        else:
            f[r, 11] = np.nan                            # NaN against every query
    return f, kinds


def _queries(D, seed):
    rng = np.random.default_rng(1000 + seed)
    q = (rng.standard_normal((QREF, D)) / np.sqrt(D)).astype(np.float32)
    q[:, COL_POS] = np.abs(q[:, COL_POS]) + np.float32(0.01)
    return q


def _zero_columns(q, Q):
    """the zeros that turn a planted +inf into NaN: in ONE of the first Q query rows, and in every other query row"""
    q = q.copy()
    q[Q // 2, COL_ONE] = 0
    q[0:QREF:2, COL_SEVERAL] = 0
    return q


def _flagged(f):
    with np.errstate(invalid="ignore"):
        m = np.abs(f).max(axis=1)
    return ~((m == 0) | ((m >= GUARD_LO) & (m < GUARD_HI)))      # NaN / inf compare false: flagged


class _Call:
    """one avl_sim_scores_ws / _prepared / _blocks call on device tensors, outputs back as numpy (None when not requested)"""

    def __init__(self, env):
        self.lib, self._lib, self.torch = env

    def __call__(self, feat_t, N, D, ld, q_t, Q, ldq, outs="sab", workspace=True, prepared_scale=None, prepared=False, blocks=None):
        lib, _lib, torch = self.lib, self._lib, self.torch
        sc = torch.full((N, Q), -7.0, device="cuda") if "s" in outs else None
        am = torch.full((N,), -7, dtype=torch.int32, device="cuda") if "a" in outs else None
        be = torch.full((N,), -7.0, device="cuda") if "b" in outs else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        wsp, wsb = None, 0
        if workspace:
            need = C.c_size_t()
            _lib.check(lib.avl_sim_workspace_bytes_n(N, D, Q, C.byref(need)))
            ws = torch.empty((max(need.value, 256),), dtype=torch.uint8, device="cuda")
            wsp, wsb = ws.data_ptr(), need.value
        if blocks is not None:
            cb, ce = blocks
            rc = lib.avl_sim_scores_blocks(feat_t.data_ptr(), None, N, D, ld, q_t.data_ptr(), Q, ldq, cb.ctypes.data, ce.ctypes.data,
                                           ptr(sc), ptr(am), ptr(be), _lib.SIM_AUTO, wsp, wsb, None)
        elif prepared:
            rc = lib.avl_sim_scores_prepared(feat_t.data_ptr(), ptr(prepared_scale), N, D, ld, q_t.data_ptr(), Q, ldq, ptr(sc), ptr(am),
                                             ptr(be), wsp, wsb, None)
        else:
            rc = lib.avl_sim_scores_ws(feat_t.data_ptr(), N, D, ld, q_t.data_ptr(), Q, ldq, ptr(sc), ptr(am), ptr(be), _lib.SIM_SPLIT_F16,
                                       wsp, wsb, None)
        _lib.check(rc, "avl_sim_scores")
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() if t is not None else None for t in (sc, am, be))


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _np_argmax_rows(sc):
    """np.argmax per row: the first NaN wins, else the first maximum"""
    return np.argmax(sc, axis=1).astype(np.int32)


_CACHE = {}


def _world(env, N, D):
    """per (N, D), computed once and shared by the Q cases (which run back to back): the map on the device, its unscaled
    prepared copy, and per Q the 128-query reference call that ends in the stand-alone fix-up kernel"""
    key = (N, D)
    if key not in _CACHE:
        _CACHE.clear()
        lib, _lib, torch = env
        call = _Call(env)
        f, kinds = _map(N, D, seed=N % 7 + D)
        q = _queries(D, seed=D)
        ft = torch.from_numpy(f).cuda()
        prep = ft.clone()
        _lib.check(lib.avl_sim_prepare_map(prep.data_ptr(), N, D, D, None, None))
        torch.cuda.synchronize()
        _CACHE[key] = dict(f=f, kinds=kinds, ft=ft, prep=prep, q=q, flagged=_flagged(f), call=call, ref={})
    return _CACHE[key]


def _reference(w, N, D, Q):
    """the QREF queries whose first Q rows are this case's, and the scores of the several-launch call on all of them"""
    if Q not in w["ref"]:
        torch = w["call"].torch
        q = _zero_columns(w["q"], Q)
        qt = torch.from_numpy(q).cuda()
        sc, _, _ = w["call"](w["ft"], N, D, D, qt, QREF, D, outs="s")
        w["ref"][Q] = (q, qt, sc)
    return w["ref"][Q]


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("N", NS)
def test_one_launch_call(env, N, D, Q):
    w = _world(env, N, D)
    call, flagged = w["call"], w["flagged"]
    q, qt, ref_sc = _reference(w, N, D, Q)
    sc, am, be = call(w["ft"], N, D, D, qt, Q, D)
    # rows the guard leaves alone: the prepared map's bits.  The identity holds between launches of the same accumulator layout.
    # At 512 columns a prepared map sends the 33rd query row to the extra-row kernel (one tile, three accumulator sets) while a
    # raw map keeps two tiles with two sets each (run_split: use_xr), so there the prepared call takes 37 queries -- two plain
    # tiles like the raw call -- whose first 33 are this case's: a column's bits do not depend on the other columns
    Qp = 37 if Q == 33 else Q
    psc, pam, pbe = call(w["prep"], N, D, D, qt, Qp, D, prepared=True)
    ok = ~flagged
    assert _same_bits(sc[ok], np.ascontiguousarray(psc[ok, :Q]))
    if Qp == Q:                                                  # (argmax and best of every row are checked against the row below)
        assert np.array_equal(am[ok], pam[ok]) and _same_bits(be[ok], pbe[ok])
    for r, k in w["kinds"].items():
        if k == "zero":
            assert not flagged[r] and not sc[r].any() and am[r] == 0 and be[r] == 0
    # flagged rows: the stand-alone fix-up kernel's bits, np.argmax semantics
    assert flagged.sum() == sum(k != "zero" for k in w["kinds"].values())
    assert _same_bits(sc[flagged], np.ascontiguousarray(ref_sc[flagged, :Q]))
    with np.errstate(invalid="ignore"):
        assert np.array_equal(am, _np_argmax_rows(sc))
    assert _same_bits(be, sc[np.arange(N), am])
    for r, k in w["kinds"].items():
        if k == "nan_all":
            assert np.isnan(sc[r]).all() and am[r] == 0
        elif k == "nan_one":
            assert np.isnan(sc[r]).sum() == 1 and am[r] == Q // 2
        elif k == "nan_several":
            assert np.isnan(sc[r, 0::2]).all() and not np.isnan(sc[r, 1::2]).any() and am[r] == 0
        elif k == "inf":
            assert np.isinf(sc[r]).all() and am[r] == 0
        elif k in ("tiny", "huge"):
            # float32 chain of D / 64 <= 8 fused multiply-adds and 6 adds per lane: 14 roundings of 2^-24 = 8.4e-7 of sum |a| |q|
            want = w["f"][r].astype(np.float64) @ q[:Q].astype(np.float64).T
            bound = 1e-6 * (np.abs(w["f"][r]).astype(np.float64) @ np.abs(q[:Q]).astype(np.float64).T)
            assert np.all(np.abs(sc[r] - want) <= bound)
    # every subset of the outputs returns the same bits; so does a call without a workspace
    subset = ("a", "s", "b", "ab", "sa", "sb")[(N + D // 64 + Q) % 6]
    for outs, workspace in ((subset, True), ("sab", False)):
        sc2, am2, be2 = call(w["ft"], N, D, D, qt, Q, D, outs=outs, workspace=workspace)
        assert sc2 is None or _same_bits(sc2, sc)
        assert am2 is None or np.array_equal(am2, am)
        assert be2 is None or _same_bits(be2, be)


def test_row_strides_wider_than_the_rows(env):
    """ld_feat > D and ld_q > D: the recomputed rows read the caller's strides"""
    lib, _lib, torch = env
    call = _Call(env)
    N, D, Q, ld, ldq = 257, 128, 33, 192, 160
    f, kinds = _map(N, D, seed=3)
    q = _zero_columns(_queries(D, seed=4), Q)
    wide = torch.full((N, ld), 3.0e38, device="cuda")            # what lies beyond column D must never be read into a score
    wide[:, :D] = torch.from_numpy(f).cuda()
    qwide = torch.full((QREF, ldq), 3.0e38, device="cuda")
    qwide[:, :D] = torch.from_numpy(q).cuda()
    dense_f, dense_q = wide[:, :D].contiguous(), qwide[:, :D].contiguous()
    got = call(wide, N, D, ld, qwide, Q, ldq)
    want = call(dense_f, N, D, D, dense_q, Q, D)
    assert _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and _same_bits(got[2], want[2])
    flagged = _flagged(f)
    ref_sc, _, _ = call(wide, N, D, ld, qwide, QREF, ldq, outs="s")
    assert flagged.any() and _same_bits(got[0][flagged], np.ascontiguousarray(ref_sc[flagged, :Q]))


def test_column_block_call_equals_the_dense_call_on_each_window(env):
    """avl_sim_scores_blocks with two support groups (256 + 128 columns): every query's scores are the bits of a dense call on
    its window alone (same operands, same order), argmax and best are np.argmax over the returned row"""
    lib, _lib, torch = env
    call = _Call(env)
    N, D = 4099, 256 + 128
    rng = np.random.default_rng(17)
    f = rng.standard_normal((N, D)).astype(np.float32)
    windows = ((0, 256), (256, 384))
    owner = np.array([0, 1, 0, 0, 1, 1, 0, 1, 1, 0] * 4)                       # 40 queries, the groups interleaved
    Q = len(owner)
    q = np.zeros((Q, D), np.float32)
    for i, g in enumerate(owner):
        lo, hi = windows[g]
        q[i, lo:hi] = rng.standard_normal(hi - lo) / 16
    q[6] = q[2]                                                                  # an exact tie inside a group
    cb = np.array([windows[g][0] for g in owner], np.int32)
    ce = np.array([windows[g][1] for g in owner], np.int32)
    ft, qt = torch.from_numpy(f).cuda(), torch.from_numpy(q).cuda()
    sc, am, be = call(ft, N, D, D, qt, Q, D, blocks=(cb, ce))
    for g, (lo, hi) in enumerate(windows):
        idx = np.flatnonzero(owner == g)
        fw = ft[:, lo:hi].contiguous()
        qw = qt[torch.from_numpy(idx).cuda()][:, lo:hi].contiguous()
        wsc, _, _ = call(fw, N, hi - lo, hi - lo, qw, len(idx), hi - lo, outs="s")
        assert _same_bits(np.ascontiguousarray(sc[:, idx]), wsc), g
    assert np.array_equal(am, _np_argmax_rows(sc)) and _same_bits(be, sc[np.arange(N), am])
    assert not np.any(am == 6)
    for outs in ("a", "ab"):
        _, am2, be2 = call(ft, N, D, D, qt, Q, D, outs=outs, blocks=(cb, ce), workspace=(outs == "a"))
        assert np.array_equal(am2, am) and (be2 is None or _same_bits(be2, be))
