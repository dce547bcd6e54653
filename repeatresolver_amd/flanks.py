"""Flank labellings from the reads (include/pfl.h): which unique sequence lies left and right of every MSA row.

The reference takes FlankingLeft / FlankingRight from the simulator's ground truth (SimDataAssessment.py:226-245); here they
come from the pieces ReadCutter wrote: a row's flank is the unique piece beside it in its read, two flanks are compared by an
edit distance anchored at the repeat boundary (`FlankClusterer.distances`, libpwr.so's HIP kernel; there is no CPU path),
and the labels are the single-linkage components at `max_permille` (`cluster`, host C).  `flank_labels` chains the three and
returns what `resolution.connect` takes in front of and behind the windows' labellings; `run_files` is the drop-in binary.

What sequence a cluster is comes from `FlankClusterer.consensus`: every flank of a cluster is aligned block by block, with
traceback, against a backbone (`place`, libpwr.so's second HIP kernel), the alignments vote position by position, and the
call is the backbone of the next round.  `flank_sequences` does this for both sides of the MSA rows."""
import ctypes
import dataclasses
import os
import subprocess

import numpy as np

from . import _lib
from .read_cutter import _offsets
from .realigner import PwrError

CLI_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "FlankClusterer")

_PI = ctypes.POINTER(ctypes.c_int)


def _ints(a):
    return a.ctypes.data_as(_PI)


def _check(lib, rc):
    if rc:
        raise PwrError(rc, lib.pwr_strerror(rc).decode())


def _classes(classes) -> bytes:
    """SeqClass letters as one byte each: a str or bytes of letters, or a sequence of 'r' / 'l' strings"""
    if isinstance(classes, (bytes, bytearray)):
        return bytes(classes)
    return "".join(classes).encode()


def neighbours(piece_read, classes, strands=None):
    """pfl_neighbours, host only.  piece_read[k]: the read of piece k; classes[k]: its SeqClass letter; strands[k]: 1 where
    InitialAligner turned the piece (None: all forward).  Returns five int32 arrays over the MSA rows: the row's piece, its
    left flank's piece (-1: none) and mode, its right flank's piece and mode."""
    lib = _lib.load()
    pr = np.ascontiguousarray(piece_read, dtype=np.int32)
    n = len(pr)
    cls = _classes(classes)
    if len(cls) != n or (strands is not None and len(strands) != n):
        raise ValueError("one class and one strand per piece")
    st = None if strands is None else np.ascontiguousarray(list(strands) + [0], dtype=np.uint8)
    out = [np.zeros(max(n, 1), dtype=np.int32) for _ in range(5)]
    nrows = ctypes.c_int()
    _check(lib, lib.pfl_neighbours(n, _ints(pr), cls, None if st is None else st.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)),
                                   ctypes.byref(nrows), *[_ints(o) for o in out]))
    return tuple(o[:nrows.value].copy() for o in out)


def cluster(a, dist, max_permille, min_size=1):
    """pfl_cluster, host only: a[k] = min(len_k, reach), dist the matrix of FlankClusterer.distances.  Returns int32 labels."""
    lib = _lib.load()
    a = np.ascontiguousarray(a, dtype=np.int32)
    d = np.ascontiguousarray(dist, dtype=np.int32)
    n = len(a)
    if d.shape != (n, n):
        raise ValueError("dist must be n x n")
    label = np.full(max(n, 1), -1, dtype=np.int32)
    _check(lib, lib.pfl_cluster(n, _ints(a), _ints(d), int(max_permille), int(min_size), _ints(label)))
    return label[:n].copy()


class FlankClusterer:
    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        _check(self._lib, self._lib.pfl_create(ctypes.byref(self._h), device))

    def close(self):
        if self._h:
            self._lib.pfl_destroy(self._h)
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

    def distances(self, pieces, piece, mode, reach=256, min_len=100):
        """pfl_distances: flank k is pieces[piece[k]] read in mode[k].  Returns (lengths, dist): the flank pieces' lengths and
        the n x n int32 matrix of anchored distances (-1 in the rows and columns of flanks shorter than min_len)."""
        pieces = [bytes(p) for p in pieces]
        pc, md = np.ascontiguousarray(piece, dtype=np.int32), np.ascontiguousarray(mode, dtype=np.int32)
        n = len(pc)
        if len(md) != n or (n and int(pc.max()) >= len(pieces)):
            raise ValueError("one mode per flank, and every flank a piece")
        off = _offsets(pieces)
        lens = np.zeros(max(n, 1), dtype=np.int32)
        dist = np.zeros((max(n, 1), max(n, 1)), dtype=np.int32)
        _check(self._lib, self._lib.pfl_distances(self._h, n, b"".join(pieces), off.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
                                                  _ints(pc), _ints(md), int(reach), int(min_len), _ints(lens), _ints(dist)))
        return lens[:n].copy(), dist[:n, :n].copy()

    def labels(self, pieces, piece_read, classes, strands=None, *, max_permille, reach=256, min_len=100, min_size=1):
        """pfl_labels: (left, right) over the MSA rows."""
        pieces = [bytes(p) for p in pieces]
        pr = np.ascontiguousarray(piece_read, dtype=np.int32)
        n = len(pieces)
        cls = _classes(classes)
        if len(pr) != n or len(cls) != n or (strands is not None and len(strands) != n):
            raise ValueError("one read, one class and one strand per piece")
        st = None if strands is None else np.ascontiguousarray(list(strands) + [0], dtype=np.uint8)
        off = _offsets(pieces)
        left, right = np.full(max(n, 1), -1, dtype=np.int32), np.full(max(n, 1), -1, dtype=np.int32)
        nrows = ctypes.c_int()
        _check(self._lib, self._lib.pfl_labels(self._h, n, b"".join(pieces), off.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), _ints(pr),
                                               cls, None if st is None else st.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)),
                                               int(max_permille), int(reach), int(min_len), int(min_size), ctypes.byref(nrows),
                                               _ints(left), _ints(right)))
        return left[:nrows.value].copy(), right[:nrows.value].copy()

    def stats(self):
        cells, ms = ctypes.c_uint64(), ctypes.c_double()
        self._lib.pfl_get_stats(self._h, ctypes.byref(cells), ctypes.byref(ms))
        return {"cells": cells.value, "kernel_ms": ms.value}

    def _flanks(self, pieces, piece, mode, group):
        pieces = [bytes(p) for p in pieces]
        pc, md = np.ascontiguousarray(piece, dtype=np.int32), np.ascontiguousarray(mode, dtype=np.int32)
        gr = np.ascontiguousarray(group, dtype=np.int32)
        n = len(pc)
        if len(md) != n or len(gr) != n or (n and int(pc.max()) >= len(pieces)):
            raise ValueError("one mode and one cluster per flank, and every flank a piece")
        return n, b"".join(pieces), _offsets(pieces), pc, md, gr

    def place(self, pieces, piece, mode, cluster, backbones, *, block=256, extent, max_permille):
        """pfl_place: flank k (pieces[piece[k]] read in mode[k]) against backbones[cluster[k]] (bytes of acgt; -1: not placed).
        Returns (ops, blocks, used, dist): ops[k, i] the vote byte of member k at backbone position i (15: none), a row as
        long as the longest backbone's used blocks, and per member the blocks voted, the bases consumed, the summed distance."""
        n, joined, off, pc, md, cl = self._flanks(pieces, piece, mode, cluster)
        backbones = [bytes(b) for b in backbones]
        if n and (int(cl.max()) >= len(backbones) or int(cl.min()) < -1):
            raise ValueError("every cluster a backbone, or -1")
        if int(block) < 1:
            raise ValueError("block must be positive")
        boff = _offsets(backbones)
        stride = max([min(len(b), int(extent)) // int(block) * int(block) for b in backbones] + [0])
        ops = np.full((max(n, 1), max(stride, 1)), 15, dtype=np.uint8)
        out = [np.zeros(max(n, 1), dtype=np.int32) for _ in range(3)]
        pll = ctypes.POINTER(ctypes.c_longlong)
        _check(self._lib, self._lib.pfl_place(self._h, n, joined, off.ctypes.data_as(pll), _ints(pc), _ints(md), _ints(cl), len(backbones),
                                              b"".join(backbones), boff.ctypes.data_as(pll), int(block), int(extent), int(max_permille),
                                              ops.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), ops.shape[1], *[_ints(o) for o in out]))
        return (ops[:n, :stride].copy(),) + tuple(o[:n].copy() for o in out)

    def consensus(self, pieces, piece, mode, labels, *, block=256, extent, max_permille, min_depth, rounds=2):
        """pfl_consensus: the consensus sequence of the flanks of every label >= 0, as a FlankConsensus."""
        n, joined, off, pc, md, lb = self._flanks(pieces, piece, mode, labels)
        res = _lib.PflConsensusResult()
        _check(self._lib, self._lib.pfl_consensus(self._h, n, joined, off.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), _ints(pc),
                                                  _ints(md), _ints(lb), int(block), int(extent), int(max_permille), int(min_depth),
                                                  int(rounds), ctypes.byref(res)))
        try:
            k = res.nclusters
            take = lambda p, m: np.ctypeslib.as_array(p, shape=(m,)).copy() if m else np.zeros(0, np.int32)
            offs = [res.off[j] for j in range(k + 1)] if k else [0]
            seq = ctypes.string_at(res.seq, offs[-1]) if offs[-1] else b""
            depth = take(res.depth, offs[-1])
            return FlankConsensus(take(res.label, k), take(res.members, k), take(res.backbone, k),
                                  [seq[offs[j]:offs[j + 1]] for j in range(k)], [depth[offs[j]:offs[j + 1]] for j in range(k)])
        finally:
            self._lib.pfl_consensus_free(ctypes.byref(res))

    def set_scratch_limit(self, nbytes):
        """the bytes of traceback scratch a placement may take (0: the default); the members go in ranges beyond it"""
        _check(self._lib, self._lib.pfl_set_scratch_limit(self._h, int(nbytes)))

    def place_stats(self):
        cells, pm, vm = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_double()
        self._lib.pfl_get_place_stats(self._h, ctypes.byref(cells), ctypes.byref(pm), ctypes.byref(vm))
        return {"cells": cells.value, "place_ms": pm.value, "votes_ms": vm.value}


@dataclasses.dataclass
class FlankConsensus:
    """The flank clusters of one side: per cluster its label, the number of member flanks, the flank index of round 1's
    backbone (-1: no member), the consensus as lower-case acgt bytes, anchored (first base at the repeat boundary), and the
    depth of every base."""
    labels: np.ndarray
    members: np.ndarray
    backbone: np.ndarray
    sequences: list
    depths: list

    def oriented(self, side):
        """{label: upper-case ACGT in template orientation}: a left flank is the anchored consensus reversed (not
        complemented: the modes have done that), a right flank stays as it is"""
        if side not in ("left", "right"):
            raise ValueError("side is 'left' or 'right'")
        return {int(l): (s[::-1] if side == "left" else s).upper().decode() for l, s in zip(self.labels, self.sequences)}


def flank_sequences(pieces, piece_read, classes, strands, left, right, *, block=256, extent, max_permille, min_depth, rounds=2,
                    device=0):
    """(left_fc, right_fc): the consensus of every flank cluster on either side of the MSA rows.  left / right: the rows'
    labels there (flank_labels, or any labelling of the rows); a side's flanks are the pieces `neighbours` names, each
    labelled by its row's label."""
    _row, lp, lm, rp, rm = neighbours(piece_read, classes, strands)
    left, right = np.asarray(left), np.asarray(right)
    if len(left) != len(lp) or len(right) != len(rp):
        raise ValueError("one left and one right label per MSA row")
    out = []
    with FlankClusterer(device) as g:
        for fp, fm, lab in ((lp, lm, left), (rp, rm, right)):
            has = fp >= 0
            out.append(g.consensus(pieces, fp[has], fm[has], lab[has], block=block, extent=extent, max_permille=max_permille,
                                   min_depth=min_depth, rounds=rounds))
    return tuple(out)


def flank_labels(pieces, piece_read, classes, strands=None, *, max_permille, reach=256, min_len=100, min_size=1, device=0):
    """FlankingLeft and FlankingRight of the MSA rows, as int32 arrays: the label of the row's flank on that side or -1.
    max_permille has no default: it depends on the reads' error rate (DESIGN 23 has the table to choose it by)."""
    with FlankClusterer(device) as g:
        return g.labels(pieces, piece_read, classes, strands, max_permille=max_permille, reach=reach, min_len=min_len,
                        min_size=min_size)


def read_info(path, npieces=None):
    """pfl_read_info: the read of every piece, from ReadCutter's ReadSeqInfo.  npieces: the number of pieces Seq.fasta holds;
    ReadCutter never sets the cut count of the last record it writes, so the file may list fewer pieces, and the pieces past
    the listed ones are then taken as the last listed read's, as pfl_run_files takes them.  More listed pieces than npieces
    is an error."""
    lib = _lib.load()
    n, p = ctypes.c_int(), ctypes.c_void_p()
    _check(lib, lib.pfl_read_info(os.fsencode(path), ctypes.byref(n), ctypes.byref(p)))
    try:
        got = np.ctypeslib.as_array(ctypes.cast(p, _PI), shape=(n.value,)).copy() if n.value else np.zeros(0, np.int32)
    finally:
        lib.pfl_free(p)
    if npieces is None or npieces == len(got):
        return got
    if npieces < len(got):
        raise ValueError(f"{path} lists {len(got)} pieces, Seq.fasta holds {npieces}")
    return np.concatenate((got, np.full(npieces - len(got), got[-1] if len(got) else 0, dtype=np.int32)))


def run_files(seq_path, info_path, class_path, max_permille, strands_path=None, reach=None, min_len=None, min_size=None,
              prefix=None, device=None, cwd=None, extent=None, block=None, min_depth=None, rounds=None):
    """The drop-in binary; returns (exit code, stdout).  It writes <prefix>_FlankingLeft and <prefix>_FlankingRight, and with
    extent (-c) also <prefix>_FlankLeft.fasta and <prefix>_FlankRight.fasta."""
    if not os.path.exists(CLI_PATH):
        raise RuntimeError(f"{CLI_PATH} is missing: build it with `make -C repeatresolver_amd/csrc`")
    cmd = [CLI_PATH, str(seq_path), str(info_path), str(class_path), "-e", str(max_permille)]
    for flag, v in (("-b", strands_path), ("-l", reach), ("-m", min_len), ("-s", min_size), ("-o", prefix), ("-g", device),
                    ("-c", extent), ("-k", block), ("-d", min_depth), ("-n", rounds)):
        if v is not None:
            cmd += [flag, str(v)]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=cwd)
    return p.returncode, p.stdout
