"""The whole repeat over the C ABI of include/pgr.h (pgr_msa_*, pgr_connect): the MSA goes to the device once, every window
[sites[p], sites[p + 1]] is read there by the HIP window reader (pgr_win_device.hip) and runs through RepeatResolver's three
stages (RepeatResolver.c main(), RR:3948-4075, once per window as the reference README's `-f x y`, `-f y z`, ...), and the
windows' final labellings are chained into the connection matrix of SimDataAssessment.py ("SDA:") MultiStepResolution
(SDA:359-391).  There is no CPU path for the reader or the stages; the connection is host code in libpwr.so."""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from .group_refinement import _check, _copy


class Msa:
    """an MSA resident on the device; close() it (or use it as a context manager)"""

    def __init__(self, handle, rows, width, device, keep):
        self.handle, self.rows, self.width, self.device, self._keep = handle, rows, width, device, keep

    def close(self):
        if self.handle is not None:
            _lib.load().pgr_msa_close(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


@dataclass
class ResolvedWindow:
    von: int
    bis: int
    kept_rows: int
    cutoff: float                # the one used (RR:3977)
    dropoff_labels: np.ndarray   # [rows] int32, -1: the row does not span the window
    reldrop_labels: np.ndarray
    kmeans_labels: np.ndarray    # the final partition of the window's rows into repeat copies
    dropoff_parts: int
    reldrop_parts: int
    kmeans_parts: int


@dataclass
class Connection:
    matrix: np.ndarray           # [parts of the first labelling, parts of the last] rows sum to 1 or are zero
    best: np.ndarray             # [parts of the first] the first column with the largest value above 0; -1: a zero row
    confidence: np.ndarray       # the value there
    mutual: np.ndarray           # bool: that value is also the largest of its column


def open_msa(rows, device: int = 0) -> Msa:
    """rows: a list of equally long bytes, or a C-contiguous 2-D uint8 array (passed by pointer, not copied)."""
    lib = _lib.load()
    if isinstance(rows, np.ndarray):
        if rows.dtype != np.uint8 or rows.ndim != 2 or not rows.flags["C_CONTIGUOUS"]:
            raise ValueError("rows: a C-contiguous 2-D uint8 array")
        text = rows
    else:
        W = len(rows[0])
        if any(len(r) != W for r in rows):
            raise ValueError("rows of unequal length")
        text = np.empty((len(rows), W), dtype=np.uint8)
        for i, r in enumerate(rows):
            text[i] = np.frombuffer(r, dtype=np.uint8)
    T, W = text.shape
    h = ctypes.c_void_p()
    _check(lib, lib.pgr_msa_open(T, W, text.ctypes.data_as(ctypes.c_void_p), device, ctypes.byref(h)))
    return Msa(h, T, W, device, None)


def window(msa: Msa, von=None, bis=None):
    """Einlesen (RR:293-429) on the device copy: the tuple group_refinement.read_window returns, bit for bit."""
    lib = _lib.load()
    if (von is None) != (bis is None):
        raise ValueError("von and bis go together")
    win = _lib.PgrWindow()
    _check(lib, lib.pgr_msa_window(msa.handle, -1 if von is None else von, -1 if bis is None else bis, ctypes.byref(win)))
    try:
        w, sc = win.width, win.sc
        return (_copy(win.kept, (msa.rows,), np.uint8).astype(bool), win.von, win.bis, _copy(win.groups, (w * 5, sc), np.uint64),
                _copy(win.local_coverage, (w, sc), np.uint64), _copy(win.coverage, (w,), np.int32))
    finally:
        lib.pgr_window_free(ctypes.byref(win))


def resolve(msa: Msa, maxcorrs, sites, cov: int = 30, cutoff: float = 0.0):
    """maxcorrs: MaxCorrelation's vector of the whole MSA (width * 5); sites: strictly increasing columns, window p =
    [sites[p], sites[p + 1]]; cov the reference's -c, cutoff its -t.  Returns a list of ResolvedWindow."""
    lib = _lib.load()
    mc = np.ascontiguousarray(maxcorrs, dtype=np.float64)
    if mc.shape != (msa.width * 5,):
        raise ValueError("maxcorrs must hold width * 5 values")
    st = np.ascontiguousarray(sites, dtype=np.int32)
    if st.ndim != 1:
        raise ValueError("sites: a list of columns")
    out = _lib.PgrResolution()
    _check(lib, lib.pgr_msa_resolve(msa.handle, mc.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(st),
                                    st.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), cov, cutoff, ctypes.byref(out)))
    try:
        T = out.rows
        res = []
        for p in range(out.nwindows):
            w = out.windows[p]
            res.append(ResolvedWindow(von=w.von, bis=w.bis, kept_rows=w.kept_rows, cutoff=w.cutoff,
                                      dropoff_labels=_copy(w.dropoff_labels, (T,), np.int32), reldrop_labels=_copy(w.reldrop_labels, (T,), np.int32),
                                      kmeans_labels=_copy(w.kmeans_labels, (T,), np.int32), dropoff_parts=w.dropoff_parts,
                                      reldrop_parts=w.reldrop_parts, kmeans_parts=w.kmeans_parts))
        return res
    finally:
        lib.pgr_resolution_free(ctypes.byref(out))


def connect(label_vectors) -> Connection:
    """label_vectors: two or more labellings of the same rows (-1: the row is not in it), in the order of the windows; flank
    labellings may stand in front and behind, as SDA:375 puts them.  Host only."""
    lib = _lib.load()
    lab = np.ascontiguousarray(label_vectors, dtype=np.int32)
    if lab.ndim != 2:
        raise ValueError("label_vectors: equally long vectors")
    out = _lib.PgrConnection()
    _check(lib, lib.pgr_connect(lab.shape[0], lab.shape[1], lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(out)))
    try:
        k1, k2 = out.k_first, out.k_last
        return Connection(matrix=_copy(out.matrix, (k1, k2), np.float64), best=_copy(out.best, (k1,), np.int32),
                          confidence=_copy(out.confidence, (k1,), np.float64), mutual=_copy(out.mutual, (k1,), np.int32).astype(bool))
    finally:
        lib.pgr_connection_free(ctypes.byref(out))


def last_timing():
    lib = _lib.load()
    t = (ctypes.c_double * 7)()
    lib.pgr_last_resolve_timing(t)
    return {"upload_ms": t[0], "resolve_ms": t[1], "reader_ms": t[2], "download_ms": t[3], "refine_ms": t[4], "subdivide_ms": t[5],
            "kmeans_ms": t[6]}


def resolution_quality(truth, labels):
    """ResolutionQuality (SDA:269-351) in numpy: truth[rows] = the copy every row comes from (datagen's copy ids), labels[rows]
    = a labelling (-1: row not in it).  Returns (true positives, false positives, [resolved copies with confidence > 0.0,
    0.1, ... 0.9])."""
    truth, labels = np.asarray(truth), np.asarray(labels)
    if truth.shape != labels.shape or truth.ndim != 1:
        raise ValueError("one truth and one label per row")
    inside = labels > -1
    if not inside.any():
        raise ValueError("no row is labelled")
    copies = np.unique(truth[inside & (truth > -1)])                  # GroupMaker: the ground-truth groups that occur (SDA:272-279)
    G, K = len(copies), int(labels.max()) + 1
    counts = np.zeros((G, K))
    for g, c in enumerate(copies):
        counts[g] = np.bincount(labels[inside & (truth == c)], minlength=K)
    m1 = counts / counts.sum(axis=1, keepdims=True)                   # SDA:291-294
    size = np.bincount(labels[inside], minlength=K).astype(float)     # Resolution.count(ttt), SDA:297
    m2 = np.divide(counts.T, size[:, None], out=np.zeros((K, G)), where=size[:, None] > 0)   # SDA:296-300
    m3 = m1 @ m2                                                      # SDA:302
    s = m3.sum(axis=1, keepdims=True)
    m3 = np.divide(m3, s, out=m3.copy(), where=s > 0)                 # SDA:305-309
    tp = fp = 0
    by_conf = [0] * 10
    for t in range(G):                                                # SDA:325-344
        maxi, maxtt = 0.0, 0
        for tt in range(G):
            if m3[t, tt] > maxi:
                maxi, maxtt = m3[t, tt], tt
        if maxi == m3[maxtt].max():
            if maxtt != t:
                fp += 1
            else:
                tp += 1
                for c in range(10):
                    if maxi > c / 10.0:
                        by_conf[c] += 1
    return tp, fp, by_conf
