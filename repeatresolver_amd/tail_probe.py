"""Test hooks over the C ABI (pmc_tail_probe of include/pmc.h, pgr_tail_probe / pgr_km_tail_probe of include/pgr.h): the
device's hypergeometric tail (csrc/hyper_tail.h) and the three stages' significances on chosen counts, each as its stage's
own file compiles it.  One launch per call, one thread per tuple.  Not part of the product path."""
import ctypes

import numpy as np

from . import _lib
from .realigner import PwrError

# columns of the arrays returned
MC_Q, MC_TAIL0, MC_TAIL, MC_SIG = 0, 1, 2, 3        # pmc_tail_probe
GR_TAIL, GR_SIG = 0, 1                              # pgr_tail_probe
KM_P, KM_Q, KM_SIG = 0, 1, 2                        # pgr_km_tail_probe

_ENTRIES = {"mc": ("pmc_tail_probe", 4), "gr": ("pgr_tail_probe", 2), "km": ("pgr_km_tail_probe", 3)}


def tail_probe(stage, counts, floor=None, device=0):
    """stage: "mc", "gr" or "km"; counts[n][6] = (schnitt, cov, gr1, gr2, size1, size2); floor[n] or None.  Returns
    float64 [n][4 | 2 | 3].  PwrError(PWR_ERR_ARG) for counts the stage's kernel could not produce (nothing is launched)."""
    name, nout = _ENTRIES[stage]
    lib = _lib.load()
    c = np.ascontiguousarray(counts, dtype=np.int32)
    if c.ndim != 2 or c.shape[1] != 6:
        raise ValueError("counts must be [n][6]")
    n = c.shape[0]
    f = None
    if floor is not None:
        f = np.ascontiguousarray(floor, dtype=np.float64)
        if f.shape != (n,):
            raise ValueError("floor must be [n]")
    out = np.zeros((max(n, 1), nout), dtype=np.float64)
    pd = ctypes.POINTER(ctypes.c_double)
    rc = getattr(lib, name)(n, c.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), f.ctypes.data_as(pd) if f is not None else None,
                            device, out.ctypes.data_as(pd))
    if rc:
        raise PwrError(rc, lib.pwr_strerror(rc).decode())
    return out[:n]
