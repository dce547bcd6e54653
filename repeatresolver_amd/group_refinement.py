"""Host-side mirror of the group refinement of the reference's RepeatResolver (RepeatResolver.c, "RR:") over the C ABI of
include/pgr.h: main() up to and including Group_Refinement (RR:3948-4024).  For every variation of the window whose
MaxCorrs exceed the cutoff: its clique (RR:1179-1240), Sizes, the cutoff of the smallest drop (RR:1460-1522), the refined
group and its coverage (RR:976-1008, RR:1064-1096).  The cliques and the votes run in libpwr.so's HIP kernels; there is no
CPU path."""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from .realigner import PwrError

MAXCLIQUE = 30


@dataclass
class RefinedGroups:
    kept: np.ndarray          # bool per input row: covers both ends of the window (RR:330)
    width: int                # of the window
    cutoff: float             # the one used (RR:3977)
    maxcorrs: np.ndarray      # [width * 5] after the coverage restriction (RR:4011-4014) and the zeroing of RR:1686
    significant: np.ndarray   # [S] variation index of each entry below
    sizes: np.ndarray         # [S] Sizes
    cliques: np.ndarray       # [S, 31] int32, -1 padded
    cutoffs: np.ndarray       # [S] Cutoffs
    drop_off: np.ndarray      # [S] Drop_Off
    c_groups: np.ndarray      # [S, sc] uint64: bit r = the r-th kept row
    c_coverage: np.ndarray    # [S, sc] uint64


def _check(lib, rc):
    if rc:
        raise PwrError(rc, lib.pwr_strerror(rc).decode())


def _copy(ptr, shape, dtype):
    n = int(np.prod(shape))
    if n == 0:
        return np.zeros(shape, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True).reshape(shape)


def refine_groups(rows, maxcorrs, von=None, bis=None, cov: int = 30, cutoff: float = 0.0, device: int = 0) -> RefinedGroups:
    """rows: equally long byte strings (the lines of the realigned MSA); maxcorrs: MaxCorrelation's vector for the whole
    MSA (width * 5).  von / bis: first and last column of the window (the reference's -f; None: the whole width), cov its
    -c, cutoff its -t (below 0.1: -log10(1 / (5 * window width)))."""
    lib = _lib.load()
    T, W = len(rows), len(rows[0])
    if any(len(r) != W for r in rows):
        raise ValueError("rows of unequal length")
    mc = np.ascontiguousarray(maxcorrs, dtype=np.float64)
    if mc.shape != (W * 5,):
        raise ValueError("maxcorrs must hold width * 5 values")
    if (von is None) != (bis is None):
        raise ValueError("von and bis go together")
    res = _lib.PgrResult()
    rc = lib.pgr_refine(T, W, b"".join(rows), mc.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), -1 if von is None else von,
                        -1 if bis is None else bis, cov, cutoff, device, ctypes.byref(res))
    _check(lib, rc)
    try:
        S, sc, w = res.nsig, res.sc, res.width
        return RefinedGroups(kept=_copy(res.kept, (T,), np.uint8).astype(bool), width=w, cutoff=res.cutoff,
                             maxcorrs=_copy(res.maxcorrs, (w * 5,), np.float64), significant=_copy(res.significant, (S,), np.int32),
                             sizes=_copy(res.sizes, (S,), np.int32), cliques=_copy(res.cliques, (S, MAXCLIQUE + 1), np.int32),
                             cutoffs=_copy(res.cutoffs, (S,), np.int32), drop_off=_copy(res.drop_off, (S,), np.float64),
                             c_groups=_copy(res.c_groups, (S, sc), np.uint64), c_coverage=_copy(res.c_coverage, (S, sc), np.uint64))
    finally:
        lib.pgr_free(ctypes.byref(res))


def last_timing():
    lib = _lib.load()
    t = (ctypes.c_double * 5)()
    lib.pgr_last_timing(t)
    return {"total_ms": t[0], "bits_ms": t[1], "cliques_ms": t[2], "votes_ms": t[3], "pairs": int(t[4])}


def read_window(rows, von=None, bis=None):
    """Einlesen (RR:293-429), host only: (kept, von, bis, groups[width * 5, sc], local_coverage[width, sc], coverage[width])."""
    lib = _lib.load()
    T, W = len(rows), len(rows[0])
    win = _lib.PgrWindow()
    _check(lib, lib.pgr_read_window(T, W, b"".join(rows), -1 if von is None else von, -1 if bis is None else bis, ctypes.byref(win)))
    try:
        w, sc = win.width, win.sc
        return (_copy(win.kept, (T,), np.uint8).astype(bool), win.von, win.bis, _copy(win.groups, (w * 5, sc), np.uint64),
                _copy(win.local_coverage, (w, sc), np.uint64), _copy(win.coverage, (w,), np.int32))
    finally:
        lib.pgr_window_free(ctypes.byref(win))
