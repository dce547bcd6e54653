"""Host-side mirror of the last subdivision stage of the reference's RepeatResolver (RepeatResolver.c, "RR:") over the C ABI
of include/pgr.h: Kmeans_Subdivision (RR:3382-3403), which gives every part with more than 2 * (cov // 2) rows its variables
(Relative_Vars, RR:2424-2493) and clusters it on them (Kmeans, RR:2604-2821), and whose labels the reference writes as
`KmeansSubdivisionOf_*` (RR:4064-4075): the tool's result.  The relative significance of the pairs, the centroids, the
assignment and the scores run in libpwr.so's HIP kernels (pgr_km_device.hip); there is no CPU path for them."""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from .group_refinement import RefinedGroups, _check, _copy
from .subdivision import Subdivision, _ptr, _result_struct


@dataclass
class KmeansSubdivision:
    labels: np.ndarray           # [rows] int32 part of every input row, -1: row left out of the window
    parts_before: int            # parts of the input after renumbering
    parts: int
    part: list                   # per eligible part: its label before the stage
    rows: list                   # per eligible part: the kept-row indices of its rows, ascending
    vars: list                   # per eligible part: its variables (variation indices, ascending)
    cluster_before: list         # per eligible part: Clusternumber after the assignment
    cluster_after: list          # per eligible part: Clusternumber after the reassignment chain
    pairs: int                   # pairs of variations evaluated
    pair_z: dict                 # debug_pairs=True: {(eligible part, i, j): Z}, else empty

    @property
    def eligible(self):
        return len(self.part)


def kmeans_subdivide(rows, refined: RefinedGroups, subdivision, von=None, bis=None, cov: int = 30, device: int = 0,
                     debug_pairs: bool = False) -> KmeansSubdivision:
    """rows, von, bis: as given to refine_groups; refined: its result (kept, maxcorrs and cutoff are used); subdivision: what
    subdivide returned, or its reldrop_labels ([rows], -1 for the rows left out); cov: the reference's -c."""
    lib = _lib.load()
    T, W = len(rows), len(rows[0])
    if any(len(r) != W for r in rows):
        raise ValueError("rows of unequal length")
    if (von is None) != (bis is None):
        raise ValueError("von and bis go together")
    lab = np.ascontiguousarray(subdivision.reldrop_labels if isinstance(subdivision, Subdivision) else subdivision, dtype=np.int32)
    if lab.shape != (T,):
        raise ValueError("one label per input row")
    res, _keep = _result_struct(refined, T)
    win = _lib.PgrWindow()
    _check(lib, lib.pgr_read_window(T, W, b"".join(rows), -1 if von is None else von, -1 if bis is None else bis, ctypes.byref(win)))
    out = _lib.PgrKmeans()
    call = lib.pgr_kmeans_subdivide_pairs if debug_pairs else lib.pgr_kmeans_subdivide
    try:
        _check(lib, call(ctypes.byref(win), ctypes.byref(res), _ptr(lab, ctypes.c_int), cov, device, ctypes.byref(out)))
        try:
            E = out.eligible
            ro, vo = _copy(out.row_offset, (E + 1,), np.int32), _copy(out.var_offset, (E + 1,), np.int32)
            row, before, after = (_copy(p, (int(ro[E]),), np.int32) for p in (out.row, out.cluster_before, out.cluster_after))
            var = _copy(out.vars, (int(vo[E]),), np.int32)
            cut = lambda a, o: [a[o[e]:o[e + 1]].copy() for e in range(E)]   # noqa: E731
            n = out.debug_pairs
            pz = dict(zip(zip(_copy(out.pair_part, (n,), np.int32).tolist(), _copy(out.pair_i, (n,), np.int32).tolist(),
                              _copy(out.pair_j, (n,), np.int32).tolist()), _copy(out.pair_z, (n,), np.float64).tolist()))
            return KmeansSubdivision(labels=_copy(out.labels, (T,), np.int32), parts_before=out.parts_before, parts=out.parts,
                                     part=_copy(out.part, (E,), np.int32).tolist(), rows=cut(row, ro), vars=cut(var, vo),
                                     cluster_before=cut(before, ro), cluster_after=cut(after, ro), pairs=out.pairs, pair_z=pz)
        finally:
            lib.pgr_kmeans_free(ctypes.byref(out))
    finally:
        lib.pgr_window_free(ctypes.byref(win))


def reassign(scores, clusternumber, mingroup):
    """The reassignment chain of Kmeans alone (RR:2726-2755, host only): scores[i, j] = GrMatch(Centroids[j], VarSigs[i]);
    returns Clusternumber after it."""
    lib = _lib.load()
    s = np.ascontiguousarray(scores, dtype=np.uint16)
    cl = np.array(clusternumber, dtype=np.int32)
    if s.shape != (len(cl), len(cl)):
        raise ValueError("scores must be square, one row per entry of clusternumber")
    _check(lib, lib.pgr_kmeans_reassign(len(cl), _ptr(s, ctypes.c_ushort), mingroup, _ptr(cl, ctypes.c_int)))
    return cl


def last_timing():
    lib = _lib.load()
    t = (ctypes.c_double * 6)()
    lib.pgr_last_kmeans_timing(t)
    return {"total_ms": t[0], "counts_ms": t[1], "pairs_ms": t[2], "kmeans_ms": t[3], "chain_ms": t[4], "pairs": int(t[5])}
