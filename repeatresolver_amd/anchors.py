"""The locus anchorer (include/pla.h): where in an assembly the copies of a resolved repeat belong.

`pipeline.loci` ends with left flank + copy + right flank per whole copy.  Here the `reach` bases of every flank nearest to the
repeat boundary are searched in every contig of an assembly, in both orientations (`LocusAnchorer.search`, libpwr.so's HIP
kernel k_la_search; there is no CPU path), the hits of a locus's two flanks decide its placement (`place`, host C), and the
PLACED intervals are replaced by the copies (`patch`).  `place_loci` chains the three for resolution.Locus objects; `run_files`
is the drop-in binary."""
import ctypes
import dataclasses
import os
import subprocess

import numpy as np

from . import _lib
from .read_cutter import _offsets
from .realigner import PwrError
from .strands import reverse_complement

CLI_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "LocusAnchorer")

_PI = ctypes.POINTER(ctypes.c_int)
_PLL = ctypes.POINTER(ctypes.c_longlong)
STATUS_NAMES = _lib.PLA_STATUS_NAMES


def _check(lib, rc):
    if rc:
        raise PwrError(rc, lib.pwr_strerror(rc).decode())


def _ints(a):
    return a.ctypes.data_as(_PI)


@dataclasses.dataclass
class Hits:
    """The hits of one search, sorted by (pattern, orientation, contig, boundary): int32 arrays of equal length.  orientation 0
    is +, 1 is -; boundary, lo and hi count the contig's bases in front of the repeat boundary."""
    pattern: np.ndarray
    orientation: np.ndarray
    contig: np.ndarray
    boundary: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    distance: np.ndarray

    FIELDS = ("pattern", "orientation", "contig", "boundary", "lo", "hi", "distance")

    def __len__(self):
        return len(self.pattern)

    def rows(self):
        """the hits as a list of 7-tuples in the order of FIELDS"""
        return list(zip(*(getattr(self, f).tolist() for f in self.FIELDS)))

    @classmethod
    def of(cls, rows):
        a = np.array(list(rows), dtype=np.int32).reshape(-1, 7)
        return cls(*(np.ascontiguousarray(a[:, f]) for f in range(7)))

    def _c(self):
        cols = [np.ascontiguousarray(getattr(self, f), dtype=np.int32) for f in self.FIELDS]
        pad = [np.concatenate((c, np.zeros(1, np.int32))) for c in cols]            # (never a null pointer)
        return _lib.PlaHits(len(cols[0]), *[_ints(c) for c in pad]), pad


@dataclasses.dataclass
class Placement:
    """pla_placement: status is an index into STATUS_NAMES; a side with exactly one hit has its contig, orientation, boundary
    and distance, any other -1; lo, hi where both lie on one contig; span where they also share the orientation, else None."""
    status: int
    left_hits: int
    right_hits: int
    left_contig: int
    left_orientation: int
    left_boundary: int
    left_distance: int
    right_contig: int
    right_orientation: int
    right_boundary: int
    right_distance: int
    lo: int
    hi: int
    span: object

    @property
    def name(self):
        return STATUS_NAMES[self.status]

    def _c(self):
        return _lib.PlaPlacement(self.status, self.left_hits, self.right_hits, self.left_contig, self.left_orientation, self.left_boundary,
                                 self.left_distance, self.right_contig, self.right_orientation, self.right_boundary, self.right_distance,
                                 self.lo, self.hi, 0 if self.span is None else 1, 0 if self.span is None else self.span)


def _contig_pairs(contigs):
    """[(name, bytes)] from pairs or from plain sequences (named contig0, contig1, ...)"""
    out = []
    for j, c in enumerate(contigs):
        name, seq = (f"contig{j}", c) if isinstance(c, (bytes, bytearray, memoryview)) else c
        out.append((name.decode() if isinstance(name, bytes) else str(name), bytes(seq)))
    return out


class _CContigs:
    """a pla_contigs over Python-owned memory, for the writers"""
    def __init__(self, contigs):
        pairs = _contig_pairs(contigs)
        self.names = (ctypes.c_char_p * (len(pairs) + 1))(*[n.encode() for n, _ in pairs])
        self.off = _offsets([s for _, s in pairs])
        self.bases = ctypes.create_string_buffer(b"".join(s for _, s in pairs))
        self.c = _lib.PlaContigs(len(pairs), ctypes.cast(self.names, ctypes.POINTER(ctypes.c_char_p)), self.off.ctypes.data_as(_PLL),
                                 ctypes.cast(self.bases, ctypes.c_void_p))


def read_contigs(path):
    """pla_read_contigs: [(name, sequence)] of a FASTA, the name being the first word after '>'; every sequence byte is kept,
    acgtACGT as it is and anything else as b'n'."""
    lib = _lib.load()
    c = _lib.PlaContigs()
    _check(lib, lib.pla_read_contigs(os.fsencode(path), ctypes.byref(c)))
    try:
        total = c.off[c.nc] if c.nc else 0
        bases = ctypes.string_at(c.bases, total) if total else b""
        return [(c.name[j].decode(), bases[c.off[j]:c.off[j + 1]]) for j in range(c.nc)]
    finally:
        lib.pla_contigs_free(ctypes.byref(c))


def read_loci(path):
    """pla_read_loci: what resolution.write_loci wrote, as a list of dicts with name, left_len, copy_len, right_len, sequence
    and the two anchored sequences left and right (the left part reversed, the right part as it is)."""
    lib = _lib.load()
    l = _lib.PlaLoci()
    _check(lib, lib.pla_read_loci(os.fsencode(path), ctypes.byref(l)))
    try:
        seq = ctypes.string_at(l.seq, l.off[l.n]) if l.n and l.off[l.n] else b""
        anc = ctypes.string_at(l.anchored, l.aoff[2 * l.n]) if l.n and l.aoff[2 * l.n] else b""
        return [dict(name=l.name[i].decode(), left_len=l.left_len[i], copy_len=l.copy_len[i], right_len=l.right_len[i],
                     sequence=seq[l.off[i]:l.off[i + 1]], left=anc[l.aoff[2 * i]:l.aoff[2 * i + 1]],
                     right=anc[l.aoff[2 * i + 1]:l.aoff[2 * i + 2]], sides=(l.side[2 * i], l.side[2 * i + 1])) for i in range(l.n)]
    finally:
        lib.pla_loci_free(ctypes.byref(l))


class LocusAnchorer:
    """A context with the contigs of an assembly on the device: uploaded once, searched any number of times."""

    def __init__(self, contigs, device: int = 0):
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        _check(self._lib, self._lib.pla_create(ctypes.byref(self._h), device))
        try:
            self.open(contigs)
        except Exception:
            self.close()
            raise

    def open(self, contigs):
        """pla_open_text: replaces the text of the context"""
        self.contigs = _contig_pairs(contigs)
        seqs = [s for _, s in self.contigs]
        off = _offsets(seqs)
        _check(self._lib, self._lib.pla_open_text(self._h, len(seqs), b"".join(seqs), off.ctypes.data_as(_PLL)))

    def close(self):
        if self._h:
            self._lib.pla_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_chunk(self, n):
        """the walk columns a lane owns: a multiple of 4 in 32 .. 65536 (a test hook and a tuning knob)"""
        _check(self._lib, self._lib.pla_set_option(self._h, b"chunk", int(n)))

    def search(self, anchored, side, *, max_permille, reach=256, min_len=100):
        """pla_search: anchored[p] (bytes of acgt, first base at the repeat boundary) with side[p] (0 left, 1 right), the
        min(len, reach) bases nearest to the boundary, in both orientations.  max_permille has no default."""
        anchored = [bytes(a) for a in anchored]
        sd = np.ascontiguousarray(list(side) + [0], dtype=np.int32)
        if len(sd) != len(anchored) + 1:
            raise ValueError("one side per pattern")
        return _search(self._lib, self._h, anchored, sd, reach, min_len, max_permille)

    def stats(self):
        cells, ms = ctypes.c_uint64(), ctypes.c_double()
        self._lib.pla_get_stats(self._h, ctypes.byref(cells), ctypes.byref(ms))
        return {"cells": cells.value, "kernel_ms": ms.value}


def _search(lib, handle, anchored, sd, reach, min_len, max_permille):
    off = _offsets(anchored)
    res = _lib.PlaHits()
    _check(lib, lib.pla_search(handle, len(anchored), b"".join(anchored), off.ctypes.data_as(_PLL), _ints(sd), int(reach), int(min_len),
                               int(max_permille), ctypes.byref(res)))
    try:
        take = lambda p: np.ctypeslib.as_array(p, shape=(res.n,)).copy() if res.n else np.zeros(0, np.int32)
        return Hits(*(take(getattr(res, f)) for f in Hits.FIELDS))
    finally:
        lib.pla_hits_free(ctypes.byref(res))


def place(hits: Hits, left_pattern, right_pattern, *, max_span):
    """pla_place, host only: locus i has the patterns left_pattern[i] and right_pattern[i] of `hits` (-1: none).  Returns a list
    of Placement.  max_span has no default."""
    lib = _lib.load()
    lp = np.ascontiguousarray(list(left_pattern) + [0], dtype=np.int32)
    rp = np.ascontiguousarray(list(right_pattern) + [0], dtype=np.int32)
    if len(lp) != len(rp):
        raise ValueError("one left and one right pattern per locus")
    n = len(lp) - 1
    out = (_lib.PlaPlacement * (n + 1))()
    ch, _keep = hits._c()
    _check(lib, lib.pla_place(n, _ints(lp), _ints(rp), ctypes.byref(ch), int(max_span), out))
    return [Placement(p.status, p.left_hits, p.right_hits, p.left_contig, p.left_orientation, p.left_boundary, p.left_distance,
                      p.right_contig, p.right_orientation, p.right_boundary, p.right_distance, p.lo, p.hi, p.span if p.has_span else None)
            for p in out[:n]]


def locus_patterns(loci):
    """The 2 n anchored sequences of resolution.Locus objects as pla_read_loci derives them from the file: pattern 2 i is locus
    i's left flank reversed (side 0), 2 i + 1 its right flank (side 1), lower case.  Returns (anchored, side, left_pattern,
    right_pattern); a side of 0 bases is an empty pattern and has index -1 in left_pattern / right_pattern."""
    anchored, side, lp, rp = [], [], [], []
    for i, l in enumerate(loci):
        s = l.sequence.encode() if isinstance(l.sequence, str) else bytes(l.sequence)
        anchored += [s[:l.left_len][::-1], s[l.left_len + l.copy_len:]]
        side += [0, 1]
        lp.append(2 * i if l.left_len else -1)
        rp.append(2 * i + 1 if l.right_len else -1)
    return anchored, side, lp, rp


def place_loci(loci, contigs, *, max_permille, max_span, reach=256, min_len=100, device=0):
    """Straight from resolution.Locus objects: (Hits, [Placement]) of the loci in the contigs."""
    anchored, side, lp, rp = locus_patterns(loci)
    with LocusAnchorer(contigs, device) as g:
        hits = g.search(anchored, side, max_permille=max_permille, reach=reach, min_len=min_len)
    return hits, place(hits, lp, rp, max_span=max_span)


def patch(contigs, placements, copies):
    """The contigs with every PLACED interval replaced by that locus's copy (copies[i], bytes or str), reverse-complemented
    where the orientation is -; the intervals of a contig are taken by (lo, hi, locus).  Returns [(name, sequence, patched)].
    Plain Python: what pla_write_patched writes."""
    out = []
    for c, (name, seq) in enumerate(_contig_pairs(contigs)):
        mine = sorted((p.lo, p.hi, i) for i, p in enumerate(placements) if p.status == _lib.PLA_PLACED and p.left_contig == c)
        parts, pos = [], 0
        for lo, hi, i in mine:
            copy = copies[i].encode() if isinstance(copies[i], str) else bytes(copies[i])
            parts += [seq[pos:max(lo, pos)], reverse_complement(copy) if placements[i].left_orientation else copy]
            pos = max(pos, hi)
        out.append((name, b"".join(parts) + seq[pos:], len(mine)))
    return out


def write_placements(path, names, placements, contigs):
    """pla_write_placements: one tab-separated line per locus"""
    lib = _lib.load()
    n = len(placements)
    if len(names) != n:
        raise ValueError("one name per locus")
    cn = (ctypes.c_char_p * (n + 1))(*[str(x).encode() for x in names])
    arr = (_lib.PlaPlacement * (n + 1))(*[p._c() for p in placements])
    cc = _CContigs(contigs)
    _check(lib, lib.pla_write_placements(os.fsencode(path), n, ctypes.cast(cn, ctypes.POINTER(ctypes.c_char_p)), arr, ctypes.byref(cc.c)))


def write_patched(path, contigs, placements, copies):
    """pla_write_patched: every contig as `>name patched=<n>` and its patched sequence on one line"""
    lib = _lib.load()
    n = len(placements)
    if len(copies) != n:
        raise ValueError("one copy per locus")
    cps = [c.encode() if isinstance(c, str) else bytes(c) for c in copies]
    off = _offsets(cps)
    arr = (_lib.PlaPlacement * (n + 1))(*[p._c() for p in placements])
    cc = _CContigs(contigs)
    _check(lib, lib.pla_write_patched(os.fsencode(path), ctypes.byref(cc.c), n, arr, b"".join(cps), off.ctypes.data_as(_PLL)))


def anchor_lines(hits: Hits, names, contigs):
    """the text of the drop-in's <prefix>_Anchors for hits of locus_patterns' numbering"""
    cn = [n for n, _ in _contig_pairs(contigs)]
    return "".join(f"{names[p // 2]}\t{'right' if p % 2 else 'left'}\t{'-' if o else '+'}\t{cn[c]}\t{b}\t{lo}\t{hi}\t{d}\n"
                   for p, o, c, b, lo, hi, d in hits.rows())


def run_files(loci_path, assembly_path, max_permille, max_span, reach=None, min_len=None, prefix=None, device=None, cwd=None):
    """The drop-in binary; returns (exit code, stdout).  It writes <prefix>_Anchors, <prefix>_Placements and
    <prefix>_Patched.fasta."""
    if not os.path.exists(CLI_PATH):
        raise RuntimeError(f"{CLI_PATH} is missing: build it with `make -C repeatresolver_amd/csrc`")
    cmd = [CLI_PATH, str(loci_path), str(assembly_path), "-e", str(max_permille), "-s", str(max_span)]
    for flag, v in (("-r", reach), ("-m", min_len), ("-o", prefix), ("-g", device)):
        if v is not None:
            cmd += [flag, str(v)]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=cwd)
    return p.returncode, p.stdout
