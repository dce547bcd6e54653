"""Host-side mirror of the first two subdivision stages of the reference's RepeatResolver (RepeatResolver.c, "RR:") over the
C ABI of include/pgr.h: DropOff_Subdivision (RR:3180-3271) and RelativeDropoff_Subdivision (RR:3274-3378), which partition
the rows of the window into repeat copies from the arrays of the group refinement, and the writer of the reference's
`DropoffSubdivisionOf_*` / `RelDropSubdivisionOf_*` files (RR:568-585, RR:4040-4062).  Stage 1 is sequential host code in
libpwr.so; the votes of stage 2 run in its HIP kernel k_gr_reldrop; there is no CPU path for stage 2."""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from .group_refinement import MAXCLIQUE, RefinedGroups, _check, _copy


@dataclass
class Subdivision:
    dropoff_labels: np.ndarray   # [rows] int32 part of every input row after DropOff_Subdivision, -1: row left out of the window
    reldrop_labels: np.ndarray   # [rows] after RelativeDropoff_Subdivision
    dropoff_parts: int
    reldrop_parts: int
    selected: int                # variations over the cutoff (with Sizes > 5)
    eligible: int                # parts of stage 1 with more than 2 * (cov // 2) rows
    winner: np.ndarray           # [dropoff_parts] the variation that split the part in stage 2, -1: none
    winner_cutoff: np.ndarray    # [dropoff_parts] its relative cutoff, -1: none


def _ptr(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _result_struct(refined: RefinedGroups, rows: int):
    """a PgrResult over numpy arrays (returned too: they must outlive the struct)"""
    S = len(refined.significant)
    sc = int(refined.kept.sum()) // 64 + 1
    a = {"kept": np.ascontiguousarray(refined.kept, dtype=np.uint8), "maxcorrs": np.ascontiguousarray(refined.maxcorrs, dtype=np.float64),
         "significant": np.ascontiguousarray(refined.significant, dtype=np.int32), "sizes": np.ascontiguousarray(refined.sizes, dtype=np.int32),
         "cliques": np.ascontiguousarray(refined.cliques, dtype=np.int32), "cutoffs": np.ascontiguousarray(refined.cutoffs, dtype=np.int32),
         "drop_off": np.ascontiguousarray(refined.drop_off, dtype=np.float64), "c_groups": np.ascontiguousarray(refined.c_groups, dtype=np.uint64),
         "c_coverage": np.ascontiguousarray(refined.c_coverage, dtype=np.uint64)}
    if len(a["kept"]) != rows or a["maxcorrs"].shape != (refined.width * 5,) or a["cliques"].shape != (S, MAXCLIQUE + 1) or \
            a["sizes"].shape != (S,) or a["drop_off"].shape != (S,) or a["c_groups"].shape != (S, sc):
        raise ValueError("refined: arrays of inconsistent shapes")
    res = _lib.PgrResult(rows=rows, kept_rows=int(refined.kept.sum()), width=refined.width, sc=sc, nsig=S, cutoff=refined.cutoff,
                         kept=_ptr(a["kept"], ctypes.c_ubyte), maxcorrs=_ptr(a["maxcorrs"], ctypes.c_double),
                         significant=_ptr(a["significant"], ctypes.c_int), sizes=_ptr(a["sizes"], ctypes.c_int),
                         cliques=_ptr(a["cliques"], ctypes.c_int), cutoffs=_ptr(a["cutoffs"], ctypes.c_int),
                         drop_off=_ptr(a["drop_off"], ctypes.c_double), c_groups=_ptr(a["c_groups"], ctypes.c_uint64),
                         c_coverage=_ptr(a["c_coverage"], ctypes.c_uint64))
    return res, a


def subdivide(rows, refined: RefinedGroups, von=None, bis=None, cov: int = 30, device: int = 0) -> Subdivision:
    """rows, von, bis: as given to refine_groups (the window is read again: the refinement's result does not carry its
    Groups); refined: its result, or any RefinedGroups over the same window; cov: the reference's -c (mingroup = cov // 2)."""
    lib = _lib.load()
    T, W = len(rows), len(rows[0])
    if any(len(r) != W for r in rows):
        raise ValueError("rows of unequal length")
    if (von is None) != (bis is None):
        raise ValueError("von and bis go together")
    res, _keep = _result_struct(refined, T)
    win = _lib.PgrWindow()
    _check(lib, lib.pgr_read_window(T, W, b"".join(rows), -1 if von is None else von, -1 if bis is None else bis, ctypes.byref(win)))
    out = _lib.PgrSubdivision()
    try:
        _check(lib, lib.pgr_subdivide(ctypes.byref(win), ctypes.byref(res), cov, device, ctypes.byref(out)))
        try:
            n1 = out.dropoff_parts
            return Subdivision(dropoff_labels=_copy(out.dropoff_labels, (T,), np.int32), reldrop_labels=_copy(out.reldrop_labels, (T,), np.int32),
                               dropoff_parts=n1, reldrop_parts=out.reldrop_parts, selected=out.selected, eligible=out.eligible,
                               winner=_copy(out.winner, (n1,), np.int32), winner_cutoff=_copy(out.winner_cutoff, (n1,), np.int32))
        finally:
            lib.pgr_subdivision_free(ctypes.byref(out))
    finally:
        lib.pgr_window_free(ctypes.byref(win))


def dropoff_subdivision(refined: RefinedGroups, cov: int = 30):
    """Stage 1 alone (host only, no device): (labels of the KEPT rows, number of parts)."""
    lib = _lib.load()
    res, _keep = _result_struct(refined, len(refined.kept))
    labels = np.zeros(max(1, res.kept_rows), dtype=np.int32)
    parts = ctypes.c_int()
    _check(lib, lib.pgr_dropoff_subdivision(ctypes.byref(res), cov // 2, _ptr(labels, ctypes.c_int), ctypes.byref(parts), None))
    return labels[:res.kept_rows], parts.value


def write_subdivision(path, labels):
    """Unterteilung_Rausschreiben (RR:568-585): one decimal label per input row, newline separated, none at the end"""
    lib = _lib.load()
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    _check(lib, lib.pgr_write_subdivision(str(path).encode(), _ptr(lab, ctypes.c_int), len(lab)))


def subdivision_name(stage, von, bis, msa):
    """"<stage>SubdivisionOf_<von>_<bis>_<msa>" (RR:4041-4046), stage "Dropoff" or "RelDrop"; von = bis = None: the whole width,
    which the reference names 0 and 1500000"""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(400)
    _check(lib, lib.pgr_subdivision_name(buf, len(buf), stage.encode(), -1 if von is None else von, -1 if bis is None else bis, msa.encode()))
    return buf.value.decode()


def last_timing():
    lib = _lib.load()
    t = (ctypes.c_double * 5)()
    lib.pgr_last_subdivision_timing(t)
    return {"sort_ms": t[0], "stage1_ms": t[1], "upload_ms": t[2], "kernel_ms": t[3], "apply_ms": t[4]}
