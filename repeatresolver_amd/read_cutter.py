"""Host-side mirror of the reference's ReadCutter (ReadCutter.c, "RC:") over the C ABI of include/prc.h.

The reference is a process (`./ReadCutter template.fasta reads.fasta -p parts -l overlap -e error_cutoff -w wiggleroom -o Seq
-r ReadSeqInfo`, RC:939-1112) around FullAnalysis (RC:581-757), which maps the first and the last template piece into each
read (Occurrence, RC:491-568) and picks the cut points.  `ReadCutter` below exposes both halves; `run_files` is the drop-in
binary.  The edit-distance rows run in libpwr.so's HIP kernel; there is no CPU path."""
import ctypes
import os
import subprocess

import numpy as np

from . import _lib
from .initial_aligner import _clean
from .realigner import PwrError

CLI_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "ReadCutter")


def _offsets(reads):
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return off


def _take(lib, ptr, n):
    """copy n ints out of a buffer the library malloc'ed, then free it"""
    try:
        return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_int)), shape=(n,)).copy() if n else np.zeros(0, np.int32)
    finally:
        lib.prc_free(ptr)


class ReadCutter:
    def __init__(self, template: bytes, device: int = 0):
        self._lib = _lib.load()
        self.template = _clean(template)
        self._h = ctypes.c_void_p()
        rc = self._lib.prc_create(ctypes.byref(self._h), self.template, len(self.template), device)
        if rc:
            raise PwrError(rc, self._lib.pwr_strerror(rc).decode())

    def close(self):
        if self._h:
            self._lib.prc_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def occurrences(self, reads, parts=60, overlap=0, error_cutoff=0.30, both_strands=False):
        """Occurrence (RC:491-568) of piece 0 and piece parts-1 (piece 0 alone when parts == 1) in every read: a list per
        read of one or two position arrays, in the reference's order.  both_strands: a list per read of two such lists, the
        read's own and its reverse complement's, each in the coordinates of that orientation (prc_occurrences_strands)."""
        reads = [bytes(r) for r in reads]
        nq = 2 if parts > 1 else 1
        off = _offsets(reads)
        ns = 2 if both_strands else 1
        pos_off = np.zeros(len(reads) * ns * nq + 1, dtype=np.int64)
        p = ctypes.c_void_p()
        entry = self._lib.prc_occurrences_strands if both_strands else self._lib.prc_occurrences
        rc = entry(self._h, len(reads), b"".join(reads), off.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
                                       int(parts), int(overlap), float(error_cutoff),
                                       pos_off.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), ctypes.byref(p))
        if rc:
            raise PwrError(rc, self._lib.pwr_strerror(rc).decode())
        pos = _take(self._lib, p, int(pos_off[-1]))
        job = lambda k: [pos[pos_off[k * nq + q]:pos_off[k * nq + q + 1]] for q in range(nq)]
        if both_strands:
            return [[job(2 * j), job(2 * j + 1)] for j in range(len(reads))]
        return [job(j) for j in range(len(reads))]

    def cut(self, reads, parts=60, overlap=0, error_cutoff=0.30, both_strands=False):
        """FullAnalysis (RC:581-757) of each read on its own: a list of cut-point arrays.  both_strands (prc_cut_strands):
        FullAnalysis of the read and of its reverse complement, a cut at c of the latter being a cut at len(read) - c; returns
        (the merged ascending cut-point arrays, the number of cut points each read's own orientation gave, the number its
        reverse complement gave)."""
        reads = [bytes(r) for r in reads]
        n = len(reads)
        off = _offsets(reads)
        pi = ctypes.POINTER(ctypes.c_int)
        ncut = np.zeros(max(n, 1), dtype=np.int32)
        nfwd, nrev = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        p = ctypes.c_void_p()
        args = (self._h, n, b"".join(reads), off.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), int(parts), int(overlap),
                float(error_cutoff), ncut.ctypes.data_as(pi), ctypes.byref(p))
        if both_strands:
            rc = self._lib.prc_cut_strands(*args, nfwd.ctypes.data_as(pi), nrev.ctypes.data_as(pi))
        else:
            rc = self._lib.prc_cut(*args)
        if rc:
            raise PwrError(rc, self._lib.pwr_strerror(rc).decode())
        cuts = _take(self._lib, p, int(ncut[:n].sum()))
        ends = np.cumsum(ncut[:n])
        per_read = [cuts[e - k:e] for e, k in zip(ends, ncut[:n])]
        return (per_read, nfwd[:n].copy(), nrev[:n].copy()) if both_strands else per_read

    def stats(self):
        cells, ms = ctypes.c_uint64(), ctypes.c_double()
        self._lib.prc_get_stats(self._h, ctypes.byref(cells), ctypes.byref(ms))
        return {"cells": cells.value, "kernel_ms": ms.value}


def run_files(template_path, reads_path, seq_path=None, info_path=None, parts=None, overlap=None, error_cutoff=None,
              wiggleroom=None, device=None, cwd=None, both_strands=False):
    """The drop-in binary with the reference's argv (RC:939-1030); returns (exit code, stdout).  both_strands: `-b 1`."""
    if not os.path.exists(CLI_PATH):
        raise RuntimeError(f"{CLI_PATH} is missing: build it with `make -C repeatresolver_amd/csrc`")
    cmd = [CLI_PATH, str(template_path), str(reads_path)]
    for flag, v in (("-o", seq_path), ("-r", info_path), ("-p", parts), ("-l", overlap), ("-e", error_cutoff),
                    ("-w", wiggleroom), ("-g", device), ("-b", 1 if both_strands else None)):
        if v is not None:
            cmd += [flag, str(v)]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=cwd)
    return p.returncode, p.stdout
