"""Checker for the flank labellings (include/pfl.h): a literal restatement of its semantics in numpy.  The edit distance is the
full DP table, one row of it at a time, over integers; there is no bit vector here and nothing is shared with the C code.

  anchored(piece, mode)                       the flank's anchored sequence as codes 0..3 (a c g t)
  anchored_distance(P, T)                     min over 0 <= y <= |T| of D(|P|, y), D(0, y) = y, D(x, 0) = x, unit costs
  distances(pieces, piece, mode, reach, min_len) -> (a, dist)
  neighbours(piece_read, classes, strands)    per MSA row: piece, left piece, left mode, right piece, right mode
  cluster(a, dist, max_permille, min_size)    single linkage, labels numbered by lowest flank index
  truth_case(config, side)                    the flanks of datagen.simulate_dataset's true cut and their distances, made once
"""
import functools

import numpy as np

_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"acgt"):
    _CODE[_c] = _i
    _CODE[_c - 32] = _i
_COMP = np.array([3, 2, 1, 0], dtype=np.uint8)          # a<->t, c<->g
_PAD = 200                                              # a text code that matches no base


def anchored(piece: bytes, mode: int) -> np.ndarray:
    """mode bit 0: walk the piece from its last base to its first; bit 1: complement every base"""
    s = _CODE[np.frombuffer(bytes(piece), dtype=np.uint8)]
    assert (s < 4).all(), "a byte outside acgtACGT"
    if mode & 1:
        s = s[::-1]
    if mode & 2:
        s = _COMP[s]
    return np.ascontiguousarray(s)


def _last_rows(P: np.ndarray, T: np.ndarray) -> np.ndarray:
    """T: (k, w) texts, padded with _PAD.  Returns D(|P|, 0 .. w) of every text: the DP one row at a time.  Row x from row
    x - 1: first the cells' vertical and diagonal predecessors, then the horizontal one as a running minimum of
    (value - column) + column."""
    k, w = T.shape
    idx = np.arange(w + 1, dtype=np.int64)
    row = np.broadcast_to(idx, (k, w + 1)).copy()                       # D(0, y) = y
    for x in range(1, len(P) + 1):
        tmp = np.empty_like(row)
        tmp[:, 0] = x                                                   # D(x, 0) = x
        tmp[:, 1:] = np.minimum(row[:, 1:] + 1, row[:, :-1] + (T != P[x - 1]))
        row = np.minimum.accumulate(tmp - idx, axis=1) + idx
    return row


def anchored_distance(P, T) -> int:
    P, T = np.asarray(P, dtype=np.uint8), np.asarray(T, dtype=np.uint8)
    return int(_last_rows(P, T.reshape(1, -1))[0].min())


def distances(pieces, piece, mode, reach=256, min_len=100):
    """pfl_distances: a[k] = min(len_k, reach) (what pfl_cluster takes; the C entry returns len_k), dist the n x n matrix."""
    n = len(piece)
    lens = np.array([len(pieces[p]) for p in piece], dtype=np.int64)
    a = np.minimum(lens, reach)
    dist = np.full((n, n), -1, dtype=np.int32)
    keep = [k for k in range(n) if lens[k] >= min_len]
    order = sorted(keep, key=lambda k: (a[k], k))
    seqs = {k: anchored(pieces[piece[k]], mode[k]) for k in keep}
    for pos, i in enumerate(order):
        dist[i, i] = 0
        rest = order[pos + 1:]
        if not rest:
            continue
        m = int(a[i])
        if m == 0:                                                      # (min_len <= 0: an empty pattern is at distance 0)
            for j in rest:
                dist[i, j] = dist[j, i] = 0
            continue
        tl = [min(int(lens[j]), m + m // 4) for j in rest]
        T = np.full((len(rest), max(tl)), _PAD, dtype=np.uint8)
        for r, j in enumerate(rest):
            T[r, :tl[r]] = seqs[j][:tl[r]]
        last = _last_rows(seqs[i][:m], T)
        for r, j in enumerate(rest):
            assert tl[r] >= m
            dist[i, j] = dist[j, i] = int(last[r, :tl[r] + 1].min())
    return a.astype(np.int32), dist


def neighbours(piece_read, classes, strands=None):
    """Per MSA row t (the t-th piece of class 'r', piece k): (k, left piece or -1, left mode, right piece or -1, right mode)."""
    n = len(piece_read)
    strands = [0] * n if strands is None else strands
    out = []

    def unique_beside(k, q):
        return q if 0 <= q < n and piece_read[q] == piece_read[k] and classes[q] != "r" else -1
    for k in range(n):
        if classes[k] != "r":
            continue
        if strands[k]:
            out.append((k, unique_beside(k, k + 1), 2, unique_beside(k, k - 1), 3))
        else:
            out.append((k, unique_beside(k, k - 1), 1, unique_beside(k, k + 1), 0))
    return out


def cluster(a, dist, max_permille, min_size=1):
    n = len(a)
    label = [-1] * n
    seen = [False] * n
    comps = []
    for s in range(n):
        if seen[s] or dist[s][s] < 0:
            continue
        comp, todo = [], [s]
        seen[s] = True
        while todo:
            i = todo.pop()
            comp.append(i)
            for j in range(n):
                if not seen[j] and dist[i][j] >= 0 and 1000 * int(dist[i][j]) <= max_permille * int(min(a[i], a[j])):
                    seen[j] = True
                    todo.append(j)
        comps.append(comp)
    nxt = 0
    for comp in comps:                                                  # (found in the order of their lowest index)
        if len(comp) >= min_size:
            for i in comp:
                label[i] = nxt
            nxt += 1
    return np.array(label, dtype=np.int32)


def true_flanks(cfg):
    """The flanks of datagen.simulate_dataset's true cut: (pieces, piece_read, classes, copy_of_piece).  Every read with a
    repeat part gives its left rest, the repeat part and its right rest (empty rests left out), as ReadCutter would."""
    from repeatresolver_amd import datagen as dg
    _seq, full, _starts, cids, cut, _ = dg.simulate_dataset(cfg)
    pieces, piece_read, classes, copy = [], [], [], []
    for r, (rb, cb) in enumerate(zip(full, cut)):
        fb = dg.ASCII[rb].tobytes()
        if cb is None:
            parts = [(fb, "l")]
        else:
            c = dg.ASCII[cb].tobytes()
            at = fb.find(c)
            assert at >= 0
            parts = [(fb[:at], "l"), (c, "r" if len(c) >= cfg.min_aligned else "l"), (fb[at + len(c):], "l")]
        for s, cl in parts:
            if len(s):
                pieces.append(s); piece_read.append(r); classes.append(cl); copy.append(cids[r])
    return pieces, piece_read, classes, copy


@functools.lru_cache(maxsize=None)
def truth_case(name, side, reach=256, min_len=100):
    """The flanks on one side ("left" / "right") of the rows of datagen.CONFIGS[name]'s true cut, with the checker's distances:
    (pieces, piece, mode, copy, a, dist).  Computed once per process and shared: nobody changes what it returns."""
    from repeatresolver_amd import datagen as dg
    pieces, piece_read, classes, copy = true_flanks(dg.CONFIGS[name])
    col = 1 if side == "left" else 3
    rows = [r for r in neighbours(piece_read, classes) if r[col] >= 0]
    piece, mode = [r[col] for r in rows], [r[col + 1] for r in rows]
    a, dist = distances(pieces, piece, mode, reach, min_len)
    dist.setflags(write=False)
    return pieces, piece, mode, [copy[r[0]] for r in rows], a, dist
