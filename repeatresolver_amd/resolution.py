"""The whole repeat over the C ABI of include/pgr.h (pgr_msa_*, pgr_connect): the MSA goes to the device once, every window
[sites[p], sites[p + 1]] is read there by the HIP window reader (pgr_win_device.hip) and runs through RepeatResolver's three
stages (RepeatResolver.c main(), RR:3948-4075, once per window as the reference README's `-f x y`, `-f y z`, ...), and the
windows' final labellings are chained into the connection matrix of SimDataAssessment.py ("SDA:") MultiStepResolution
(SDA:359-391).  There is no CPU path for the reader or the stages; the connection is host code in libpwr.so.  `consensus`
gives, for a labelling, every part's consensus in a window and the differences between them (pgr_cons_device.hip), on which
`resolvability` restates TransposonAssessment.py ("TA:").  `assign` is the way back: every row of the MSA, also those that do not
span the window, against every part's consensus (pgr_assign_device.hip); the reference has no counterpart for it."""
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


@dataclass
class Consensus:
    """pgr_consensus (include/pgr.h): the parts of a labelling in one window [von, bis] of the MSA"""
    von: int
    bis: int
    part_label: np.ndarray       # [parts] int32, the labels that occur, ascending (GroupMaker, TA:159-160)
    part_rows: np.ndarray        # [parts] rows of each
    consensus: np.ndarray        # [parts, width] uint8 codes 0..4 = a c g t -; the first of the most frequent (np.argmax, TA:91)
    depth: np.ndarray            # [parts, width] int32 rows of the part with a symbol there; 0: the code 0 stands for nothing
    counts: object               # [parts, width, 5] int32, or None unless asked for
    selected: np.ndarray         # absolute columns whose MaxCorrs exceed the cutoff (TA:157), ascending
    diff: np.ndarray             # [parts, parts] int32 selected columns where two consensus differ (Diff, TA:94-95)
    diff_all: np.ndarray         # the same over every column of the window

    @property
    def parts(self):
        return len(self.part_label)

    def sequences(self):
        """one bytes per part: the consensus without its '-' columns, in ACGT as MMA_Auslesen writes bases"""
        acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
        return [acgt[row[row < 4]].tobytes() for row in self.consensus]


def _labels(msa, labels):
    lab = np.array([-1 if x is None else x for x in labels] if not isinstance(labels, np.ndarray) else labels, dtype=np.int64)
    if lab.shape != (msa.rows,):
        raise ValueError("one label per row of the MSA")
    if lab.size and (lab.max() > 2 ** 31 - 1 or lab.min() < -2 ** 31):
        raise ValueError("labels do not fit 32 bits")
    return np.ascontiguousarray(lab, dtype=np.int32)


def consensus(msa: Msa, labels, von=None, bis=None, maxcorrs=None, cutoff: float = 1.0, counts: bool = False) -> Consensus:
    """The per-part consensus of the window [von, bis] (both inclusive; None, None: the whole width) for labels[rows] (-1 or
    None: the row is in no part; None is the empty line of a label file, TA:74-75), computed on the device copy of the MSA
    (pgr_cons_device.hip).  maxcorrs: MaxCorrelation's vector of the whole MSA (width * 5) or None: every column is selected."""
    lib = _lib.load()
    if (von is None) != (bis is None):
        raise ValueError("von and bis go together")
    lab = _labels(msa, labels)
    mc = None
    if maxcorrs is not None:
        mc = np.ascontiguousarray(maxcorrs, dtype=np.float64)
        if mc.shape != (msa.width * 5,):
            raise ValueError("maxcorrs must hold width * 5 values")
    out = _lib.PgrConsensus()
    _check(lib, lib.pgr_msa_consensus(msa.handle, lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), -1 if von is None else von,
                                      -1 if bis is None else bis, None if mc is None else mc.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                      cutoff, 1 if counts else 0, ctypes.byref(out)))
    try:
        P, W = out.parts, out.width
        return Consensus(von=out.von, bis=out.bis, part_label=_copy(out.part_label, (P,), np.int32), part_rows=_copy(out.part_rows, (P,), np.int32),
                         consensus=_copy(out.consensus, (P, W), np.uint8), depth=_copy(out.depth, (P, W), np.int32),
                         counts=_copy(out.counts, (P, W, 5), np.int32) if counts else None,
                         selected=_copy(out.selected, (out.nselected,), np.int32), diff=_copy(out.diff, (P, P), np.int32),
                         diff_all=_copy(out.diff_all, (P, P), np.int32))
    finally:
        lib.pgr_consensus_free(ctypes.byref(out))


def last_consensus_timing():
    lib = _lib.load()
    t = (ctypes.c_double * 5)()
    lib.pgr_last_consensus_timing(t)
    return {"all_ms": t[0], "order_ms": t[1], "counts_ms": t[2], "consensus_diff_ms": t[3], "download_ms": t[4]}


@dataclass
class Assignment:
    """pgr_assignment (include/pgr.h): every row of the MSA against the consensus of every part, over `columns`.  The
    semantics are this project's own; the reference has no counterpart."""
    von: int
    bis: int
    part_label: np.ndarray       # [parts] int32: the label that part index p stands for
    columns: np.ndarray          # [ncolumns] int32 the compared columns, absolute, ascending
    compared: np.ndarray         # [rows] int32 compared columns in which the row has a symbol
    best: np.ndarray             # [rows] int32 the part INDEX with the fewest mismatches, the lowest among equals; -1: nothing compared
    second: np.ndarray           # [rows] the same over the other parts; -1: nothing compared, or a single part
    best_mismatches: np.ndarray  # [rows] int32
    second_mismatches: np.ndarray
    mismatches: object           # [rows, parts] int32, or None unless asked for

    def labels(self, min_compared, min_margin, keep=None):
        """int32 [rows]: part_label[best] where compared >= min_compared and (second == -1 or second_mismatches -
        best_mismatches >= min_margin), -1 elsewhere; where keep (an existing labelling of the rows) is >= 0, that label stays.
        The two thresholds depend on the read error rate and on the number of compared columns: there is no default."""
        sure = (self.best >= 0) & (self.compared >= min_compared) & \
            ((self.second == -1) | (self.second_mismatches - self.best_mismatches >= min_margin))
        out = np.where(sure, self.part_label[np.maximum(self.best, 0)], -1).astype(np.int32)
        if keep is not None:
            keep = np.asarray(keep)
            if keep.shape != out.shape:
                raise ValueError("keep: one label per row")
            out = np.where(keep >= 0, keep, out).astype(np.int32)
        return out


def assign_sequences(msa: Msa, von: int, codes, columns, part_label=None, matrix: bool = False) -> Assignment:
    """pgr_msa_assign (pgr_assign_device.hip): codes [parts, width] uint8, 0 .. 4, is every part's sequence over the window
    [von, von + width - 1]; columns: the absolute columns compared, strictly ascending; part_label: the label of every part
    (default: its index)."""
    lib = _lib.load()
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    if codes.ndim != 2:
        raise ValueError("codes: [parts, width]")
    parts, width = codes.shape
    cols = np.ascontiguousarray(columns, dtype=np.int32)
    if cols.ndim != 1:
        raise ValueError("columns: a list of columns")
    part_label = np.arange(parts, dtype=np.int32) if part_label is None else np.array(part_label, dtype=np.int32)
    if part_label.shape != (parts,):
        raise ValueError("one label per part")
    out = _lib.PgrAssignment()
    _check(lib, lib.pgr_msa_assign(msa.handle, parts, von, width, codes.ctypes.data_as(ctypes.c_void_p), len(cols),
                                   cols.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 1 if matrix else 0, ctypes.byref(out)))
    try:
        T = out.rows
        return Assignment(von=von, bis=von + width - 1, part_label=part_label, columns=cols.copy(), compared=_copy(out.compared, (T,), np.int32),
                          best=_copy(out.best, (T,), np.int32), second=_copy(out.second, (T,), np.int32),
                          best_mismatches=_copy(out.best_mismatches, (T,), np.int32),
                          second_mismatches=_copy(out.second_mismatches, (T,), np.int32),
                          mismatches=_copy(out.mismatches, (T, parts), np.int32) if matrix else None)
    finally:
        lib.pgr_assignment_free(ctypes.byref(out))


def assign(msa: Msa, con: Consensus, min_depth: int = 1, all_columns: bool = False, matrix: bool = False) -> Assignment:
    """Every row of the MSA against the consensus of every part of `con`, over con.selected (all_columns: over every column of
    the window), of which only the columns are kept at which EVERY part has depth >= min_depth: that makes the mismatch counts
    of two parts comparable (min_depth = 1: every part has a consensus there).  ValueError when no column is left."""
    cols = np.arange(con.von, con.bis + 1, dtype=np.int32) if all_columns else np.asarray(con.selected, dtype=np.int32)
    cols = cols[(con.depth[:, cols - con.von] >= min_depth).all(axis=0)]
    if len(cols) == 0:
        raise ValueError("no column at which every part has the depth asked for")
    return assign_sequences(msa, con.von, con.consensus, cols, con.part_label, matrix)


def last_assign_timing():
    lib = _lib.load()
    t = (ctypes.c_double * 5)()
    lib.pgr_last_assign_timing(t)
    return {"all_ms": t[0], "prepare_ms": t[1], "planes_ms": t[2], "dist_best_ms": t[3], "download_ms": t[4]}


@dataclass
class Settlement:
    """pgr_settlement (include/pgr.h): a labelling settled by iterating consensus, assign and Assignment.labels on the device.
    The per-row arrays, part_label and columns are those of the last iteration -- the assignment the labels were made from (with
    stop == "EMPTY": the one that emptied the labelling) --, None when there was none ("NO_COLUMN" in iteration 0)."""
    labels: np.ndarray           # [rows] int32 the settled labelling
    stop: str                    # "CONVERGED", "MAX_ITER", "EMPTY" or "NO_COLUMN"
    iterations: int              # entries of the three histories
    changed: np.ndarray          # [iterations] int32 rows whose label moved
    parts_at: np.ndarray         # [iterations] the parts (labels that occur) the iteration started from
    ncolumns_at: np.ndarray      # [iterations] its compared columns
    part_label: object           # [parts] int32 the label of every part index of the last iteration
    columns: object              # int32 the compared columns of the last iteration, absolute, ascending
    compared: object             # [rows] int32, as Assignment
    best: object
    second: object
    best_mismatches: object
    second_mismatches: object


def settle(msa: Msa, labels, von=None, bis=None, maxcorrs=None, cutoff: float = 1.0, *, min_compared, min_margin, max_iter,
           min_depth: int = 1, all_columns: bool = False, hold: bool = False) -> Settlement:
    """consensus(msa, lab, von, bis, maxcorrs, cutoff), assign(msa, con, min_depth, all_columns) and
    a.labels(min_compared, min_margin, keep=labels if hold else None) iterated from lab = labels until no row moves
    ("CONVERGED"), for max_iter iterations ("MAX_ITER"), until an iteration labels no row ("EMPTY": the labelling before it is
    returned) or no column is left at which every part has the depth ("NO_COLUMN"), on the device (pgr_settle_device.hip): the
    rows' bit planes stay resident and nothing but one small record per iteration crosses the bus.  A label that no row holds any
    more is no part from then on; with hold the rows labelled at the start keep their label throughout.  The thresholds and
    max_iter have no default, as in Assignment.labels."""
    lib = _lib.load()
    if (von is None) != (bis is None):
        raise ValueError("von and bis go together")
    lab = _labels(msa, labels)
    mc = None
    if maxcorrs is not None:
        mc = np.ascontiguousarray(maxcorrs, dtype=np.float64)
        if mc.shape != (msa.width * 5,):
            raise ValueError("maxcorrs must hold width * 5 values")
    out = _lib.PgrSettlement()
    pi = ctypes.POINTER(ctypes.c_int)
    _check(lib, lib.pgr_msa_settle(msa.handle, lab.ctypes.data_as(pi), -1 if von is None else von, -1 if bis is None else bis,
                                   None if mc is None else mc.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), cutoff, min_depth,
                                   1 if all_columns else 0, min_compared, min_margin, 1 if hold else 0, max_iter, ctypes.byref(out)))
    try:
        T, n = out.rows, out.iterations
        per_row = [_copy(getattr(out, name), (T,), np.int32) if getattr(out, name) else None
                   for name in ("compared", "best", "second", "best_mismatches", "second_mismatches")]
        return Settlement(labels=_copy(out.labels, (T,), np.int32), stop=_lib.PGR_ST_NAMES[out.stop], iterations=n,
                          changed=_copy(out.changed, (n,), np.int32) if n else np.zeros(0, np.int32),
                          parts_at=_copy(out.parts_at, (n,), np.int32) if n else np.zeros(0, np.int32),
                          ncolumns_at=_copy(out.ncolumns_at, (n,), np.int32) if n else np.zeros(0, np.int32),
                          part_label=_copy(out.part_label, (out.parts,), np.int32) if out.part_label else None,
                          columns=_copy(out.columns, (out.ncolumns,), np.int32) if out.columns else None,
                          compared=per_row[0], best=per_row[1], second=per_row[2], best_mismatches=per_row[3], second_mismatches=per_row[4])
    finally:
        lib.pgr_settlement_free(ctypes.byref(out))


def last_settle_timing():
    lib = _lib.load()
    t = (ctypes.c_double * 5)()
    lib.pgr_last_settle_timing(t)
    return {"all_ms": t[0], "prepare_ms": t[1], "planes_ms": t[2], "iterations_ms": t[3], "download_ms": t[4]}


@dataclass
class Crossovers:
    """pgr_crossovers (include/pgr.h): every row of the MSA against every part per segment of the compared columns, and per row
    the best explanation by two different parts joined at a segment boundary.  The semantics are this project's own."""
    von: int
    bis: int
    part_label: np.ndarray       # [parts] int32: the label that part index p stands for
    columns: np.ndarray          # [ncolumns] int32 the compared columns, absolute, ascending
    seg_end: np.ndarray          # [nseg] int32: segment s is columns[seg_end[s - 1]:seg_end[s]]
    compared: np.ndarray         # [rows] the five fields of Assignment for the same codes and columns: the one-copy explanation
    best: np.ndarray
    second: np.ndarray
    best_mismatches: np.ndarray
    second_mismatches: np.ndarray
    seg_compared: np.ndarray     # [rows, nseg] int32 compared columns of the segment in which the row has a symbol
    seg_best: np.ndarray         # [rows, nseg] the part INDEX with the fewest mismatches in the segment; -1: nothing compared there
    cross_split: np.ndarray      # [rows] k in 1 .. nseg - 1: part cross_left in the segments < k, cross_right from k on; -1: none
    cross_left: np.ndarray       # [rows] part INDEX, or -1
    cross_right: np.ndarray
    cross_mismatches: np.ndarray     # [rows] the mismatches of that explanation
    cross_left_compared: np.ndarray  # [rows] the row's compared columns in the segments < k
    seg_mismatches: object       # [rows, nseg, parts] int32, or None unless asked for

    @property
    def segment_columns(self):
        """one int32 array per segment: its compared columns"""
        return np.split(self.columns, self.seg_end[:-1])

    def rows(self, min_gain):
        """the rows with a crossover that explains at least min_gain mismatches more than the best single part.  min_gain
        depends on the read error rate, like Assignment.labels' thresholds: there is no default."""
        return np.nonzero((self.cross_split >= 0) & (self.best_mismatches - self.cross_mismatches >= min_gain))[0]


def _segment_ends(cols, segments, segment_sites):
    if (segments is None) == (segment_sites is None):
        raise ValueError("either segments or segment_sites")
    n = len(cols)
    if segments is not None:
        if segments < 1 or segments > n:
            raise ValueError("a segment would be empty")
        return np.array([(s + 1) * n // segments for s in range(segments)], dtype=np.int32)
    sites = np.asarray(segment_sites, dtype=np.int64)
    if sites.ndim != 1 or len(sites) < 1 or (np.diff(sites) <= 0).any():
        raise ValueError("segment_sites: ascending columns")
    at = np.searchsorted(sites, cols, side="right") - 1            # the last site <= the column
    count = np.bincount(at[at >= 0], minlength=len(sites))
    if (at < 0).any() or (count == 0).any():
        raise ValueError("a segment would be empty, or a compared column lies before the first site")
    return np.cumsum(count).astype(np.int32)


def crossover_sequences(msa: Msa, von: int, codes, columns, seg_end, *, min_side, part_label=None, matrix: bool = False) -> Crossovers:
    """pgr_msa_crossovers (pgr_cross_device.hip): codes, columns and part_label as assign_sequences; seg_end: ascending ends of the
    segments as indices into columns, the last one len(columns)."""
    lib = _lib.load()
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    if codes.ndim != 2:
        raise ValueError("codes: [parts, width]")
    parts, width = codes.shape
    cols = np.ascontiguousarray(columns, dtype=np.int32)
    ends = np.ascontiguousarray(seg_end, dtype=np.int32)
    if cols.ndim != 1 or ends.ndim != 1:
        raise ValueError("columns and seg_end: lists")
    part_label = np.arange(parts, dtype=np.int32) if part_label is None else np.array(part_label, dtype=np.int32)
    if part_label.shape != (parts,):
        raise ValueError("one label per part")
    out = _lib.PgrCrossovers()
    pi = ctypes.POINTER(ctypes.c_int)
    _check(lib, lib.pgr_msa_crossovers(msa.handle, parts, von, width, codes.ctypes.data_as(ctypes.c_void_p), len(cols), cols.ctypes.data_as(pi),
                                       len(ends), ends.ctypes.data_as(pi), min_side, 1 if matrix else 0, ctypes.byref(out)))
    try:
        T, S = out.rows, out.nseg
        per_row = {name: _copy(getattr(out, name), (T,), np.int32)
                   for name in ("compared", "best", "second", "best_mismatches", "second_mismatches", "cross_split", "cross_left",
                                "cross_right", "cross_mismatches", "cross_left_compared")}
        return Crossovers(von=von, bis=von + width - 1, part_label=part_label, columns=cols.copy(), seg_end=ends.copy(),
                          seg_compared=_copy(out.seg_compared, (T, S), np.int32), seg_best=_copy(out.seg_best, (T, S), np.int32),
                          seg_mismatches=_copy(out.seg_mismatches, (T, S, parts), np.int32) if matrix else None, **per_row)
    finally:
        lib.pgr_crossovers_free(ctypes.byref(out))


def crossovers(msa: Msa, con: Consensus, *, segments=None, segment_sites=None, min_side, min_depth: int = 1, all_columns: bool = False,
               matrix: bool = False) -> Crossovers:
    """Every row of the MSA against the consensus of every part of `con` per segment, over the columns `assign` compares (same
    min_depth and all_columns).  Either `segments`: that many segments of as equal a number of compared columns as possible, or
    `segment_sites`: ascending absolute columns, a compared column c belonging to the segment of the last site <= c.  ValueError
    when no column is left or a segment would be empty.  min_side has no default: it depends on the read error rate."""
    cols = np.arange(con.von, con.bis + 1, dtype=np.int32) if all_columns else np.asarray(con.selected, dtype=np.int32)
    cols = cols[(con.depth[:, cols - con.von] >= min_depth).all(axis=0)]
    if len(cols) == 0:
        raise ValueError("no column at which every part has the depth asked for")
    return crossover_sequences(msa, con.von, con.consensus, cols, _segment_ends(cols, segments, segment_sites), min_side=min_side,
                               part_label=con.part_label, matrix=matrix)


def last_crossover_timing():
    lib = _lib.load()
    t = (ctypes.c_double * 6)()
    lib.pgr_last_crossover_timing(t)
    return {"all_ms": t[0], "prepare_ms": t[1], "planes_ms": t[2], "dist_ms": t[3], "cross_best_ms": t[4], "download_ms": t[5]}


@dataclass
class Threads:
    """pgr_threads (include/pgr.h): the labellings of neighbouring windows threaded into whole copies.  Host only."""
    nres: int
    first: np.ndarray            # [threads] int32 the labelling in which the thread begins
    last: np.ndarray             # [threads] and ends
    offset: np.ndarray           # [nres + 1] into thread_of: labelling i's labels are thread_of[offset[i]:offset[i + 1]]
    thread_of: np.ndarray        # the thread of every (labelling, label); -1: the label does not occur
    row_thread: np.ndarray       # [rows] the thread common to all of the row's labels >= 0; -1: none, or they disagree
    row_conflict: np.ndarray     # [rows] bool: they disagree

    @property
    def nthreads(self):
        return len(self.first)

    def labels(self, complete_only: bool = True):
        """int32 [rows]: row_thread; with complete_only the rows of threads that do not span all labellings are -1"""
        if not complete_only:
            return self.row_thread.copy()
        whole = (self.first == 0) & (self.last == self.nres - 1)
        return np.where((self.row_thread >= 0) & whole[np.maximum(self.row_thread, 0)], self.row_thread, -1).astype(np.int32)


def thread(label_vectors) -> Threads:
    """label_vectors as `connect` takes them.  Labels of neighbouring labellings are linked where each is the other's first
    largest partner by shared rows; a thread is a maximal chain of links (pgr_thread, include/pgr.h).  Host only."""
    lib = _lib.load()
    lab = np.ascontiguousarray(label_vectors, dtype=np.int32)
    if lab.ndim != 2:
        raise ValueError("label_vectors: equally long vectors")
    out = _lib.PgrThreads()
    _check(lib, lib.pgr_thread(lab.shape[0], lab.shape[1], lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(out)))
    try:
        n, N, T = out.nthreads, out.nres, out.rows
        offset = _copy(out.offset, (N + 1,), np.int32)
        return Threads(nres=N, first=_copy(out.first, (n,), np.int32), last=_copy(out.last, (n,), np.int32), offset=offset,
                       thread_of=_copy(out.thread_of, (int(offset[-1]),), np.int32), row_thread=_copy(out.row_thread, (T,), np.int32),
                       row_conflict=_copy(out.row_conflict, (T,), np.int32).astype(bool))
    finally:
        lib.pgr_threads_free(ctypes.byref(out))


def write_copies(path, consensus: Consensus, name: str):
    """One FASTA record per part, `>name_<von>_<bis>_copy<label> rows=<n>` and the sequence on one line.  The format is this
    project's own: the reference writes no consensus."""
    with open(path, "wb") as f:
        for label, n, seq in zip(consensus.part_label, consensus.part_rows, consensus.sequences()):
            f.write(f">{name}_{consensus.von}_{consensus.bis}_copy{int(label)} rows={int(n)}\n".encode() + seq + b"\n")


@dataclass
class Locus:
    """A whole copy between its unique flanks: what an assembly is patched with.  Host only."""
    thread: int                  # the thread of Threads, and the label of its part in the whole Consensus
    left_label: int              # the flank cluster in the first labelling
    right_label: int             # and in the last
    rows: int                    # rows of the part
    left_len: int                # bases of the three pieces of `sequence`
    copy_len: int
    right_len: int
    sequence: str                # left flank + copy + right flank, ACGT in template orientation


def join_loci(threads: Threads, whole: Consensus, left_fc, right_fc, min_depth: int = 1):
    """threads = thread([left, *labellings, right]) with the flank labellings at both ends, whole = the Consensus of
    threads.labels(), left_fc / right_fc = the flanks.FlankConsensus of the two sides.  Every thread that spans all labellings
    and has a part in `whole` gives a Locus: left_fc.oriented("left")[L] + copy + right_fc.oriented("right")[R], L and R being
    the thread's labels in the first and the last labelling (a label the FlankConsensus does not hold adds nothing).  The copy
    is the part's consensus over the columns with a base (code < 4) and depth >= min_depth: Consensus.sequences() would emit
    an A for a column that no row of the part covers."""
    if min_depth < 1:
        raise ValueError("min_depth >= 1")
    lefts, rights = left_fc.oriented("left"), right_fc.oriented("right")
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ends = []
    for i in (0, threads.nres - 1):
        of = threads.thread_of[threads.offset[i]:threads.offset[i + 1]]
        ends.append({int(t): label for label, t in enumerate(of) if t >= 0})
    loci = []
    for p, t in enumerate(whole.part_label):
        t = int(t)
        if not (0 <= t < threads.nthreads and threads.first[t] == 0 and threads.last[t] == threads.nres - 1):
            continue
        row, depth = whole.consensus[p], whole.depth[p]
        copy = acgt[row[(row < 4) & (depth >= min_depth)]].tobytes().decode()
        L, R = ends[0][t], ends[1][t]
        left, right = lefts.get(L, ""), rights.get(R, "")
        loci.append(Locus(thread=t, left_label=L, right_label=R, rows=int(whole.part_rows[p]), left_len=len(left), copy_len=len(copy),
                          right_len=len(right), sequence=left + copy + right))
    return loci


def write_loci(path, loci, name: str):
    """One FASTA record per Locus, `>name_locus<thread> left=<L>:<bases> copy=<bases> right=<R>:<bases> rows=<n>` and the sequence
    on one line.  The format is this project's own."""
    with open(path, "w") as f:
        for l in loci:
            f.write(f">{name}_locus{l.thread} left={l.left_label}:{l.left_len} copy={l.copy_len} right={l.right_label}:{l.right_len} "
                    f"rows={l.rows}\n{l.sequence}\n")


def unique_parts(diff):
    """Resolvability (TA:97-119) on a diff matrix: (unique[11], min_diff[parts], last_diff[parts]).  unique[t] = the parts whose
    smallest diff to any other part is > t; last_diff is what the reference itself returns -- the diff to the last other part
    visited, since TA:112 appends `diff`, not `mindiff`."""
    lib = _lib.load()
    d = np.ascontiguousarray(diff, dtype=np.int32)
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        raise ValueError("diff: a square matrix")
    P = d.shape[0]
    pi = ctypes.POINTER(ctypes.c_int)
    unique, mind, last = np.zeros(11, dtype=np.int32), np.zeros(max(P, 1), dtype=np.int32), np.zeros(max(P, 1), dtype=np.int32)
    _check(lib, lib.pgr_resolvability(P, d.ctypes.data_as(pi), unique.ctypes.data_as(pi), mind.ctypes.data_as(pi), last.ctypes.data_as(pi)))
    return unique.tolist(), mind, last


def resolvability(msa: Msa, truth, maxcorrs, start: int, ende: int, cutoff: float = 1.0):
    """TA:262-283: how many ground-truth copies (truth[rows], -1 / None: none) have a consensus that differs from every other
    copy's in more than 0 .. 10 of the significant columns.  start and ende are variation indices as in the name of a label
    file: the columns are range(start / 5, ende / 5) (TA:157) -- the script is Python 2, where / on ints is floor division --,
    so von = start // 5 and bis = ende // 5 - 1.  Returns (unique[11], parts, min_diff, last_diff)."""
    von, bis = start // 5, ende // 5 - 1
    if von < 0 or bis < von:
        raise ValueError("start and ende leave no column")
    con = consensus(msa, truth, von, bis, maxcorrs, cutoff)
    unique, mind, last = unique_parts(con.diff)
    return unique, con.parts, mind, last


def transposon_resolution_quality(truth, labels):
    """ResolutionQuality of TransposonAssessment.py (TA:162-255) in numpy.  It differs from resolution_quality (SDA:269-351)
    in one place: a truth group is all rows of the copy, also those the labelling leaves at -1 (TA:165, TA:178; the SDA
    script first restricts the truth to the labelled rows).  While some rows of a copy are labelled the normalisation of
    TA:191-195 divides the size out again; a copy left out altogether keeps a zero row here, which the scan of TA:229-242
    counts as a true positive (at no confidence level) when it is the first copy and as a false positive otherwise.  Returns
    (true positives, false positives, [resolved copies with confidence > 0.0, 0.1, ... 0.9])."""
    truth = np.array([-1 if x is None else x for x in truth])
    labels = np.array([-1 if x is None else x for x in labels])
    if truth.shape != labels.shape or truth.ndim != 1:
        raise ValueError("one truth and one label per row")
    if not (labels > -1).any() or not (truth > -1).any():
        raise ValueError("no row is labelled")
    copies = np.unique(truth[truth > -1])                             # GroupMaker (TA:159-160, TA:165)
    G, K = len(copies), int(labels.max()) + 1
    counts = np.zeros((G, K))
    for g, c in enumerate(copies):
        counts[g] = np.bincount(labels[(truth == c) & (labels > -1)], minlength=K)
    size1 = np.array([(truth == c).sum() for c in copies], dtype=float)
    m1 = counts / size1[:, None]                                      # TA:177-180
    size = np.bincount(labels[labels > -1], minlength=K).astype(float)     # Resolution.count(ttt), TA:183
    m2 = np.divide(counts.T, size[:, None], out=np.zeros((K, G)), where=size[:, None] > 0)   # TA:182-186
    m3 = m1 @ m2                                                      # TA:188
    s = m3.sum(axis=1, keepdims=True)
    m3 = np.divide(m3, s, out=m3.copy(), where=s > 0)                 # TA:191-195
    tp = fp = 0
    by_conf = [0] * 10
    for t in range(G):                                                # TA:229-248
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
