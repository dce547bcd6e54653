"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  include/pla.h restated in numpy: the last row of the semi-global table, the four
walks, the runs, y* and the coordinates.  Device results must equal this exactly.

The last row is computed by rows over the pattern, vectorised over the text: with prev = D(x-1, .) and the row's match vector,
t[y] = min(prev[y-1] + (no match), prev[y] + 1) is the cell without its left neighbour, and D(x, y) = min over y' <= y of
t[y'] + (y - y') is `np.minimum.accumulate(t - arange) + arange` (D(x, 0) = x takes part as t[0]).  `last_row_loops` is the
cell-by-cell double loop it is tested against."""
import numpy as np

_CODE = np.full(256, 4, dtype=np.int64)
for _i, _ch in enumerate(b"acgt"):
    _CODE[_ch] = _i
    _CODE[_ch - 32] = _i


def codes(seq) -> np.ndarray:
    """a c g t in either case -> 0 .. 3, every other byte -> 4"""
    return _CODE[np.frombuffer(bytes(seq), dtype=np.uint8)]


def last_row(q: np.ndarray, w: np.ndarray) -> np.ndarray:
    """D(m, 0 .. len(w)) of rows q (codes 0 .. 3) against the walk w (codes 0 .. 4; 4 matches nothing) with D(0, y) = 0 and
    D(x, 0) = x"""
    n = len(w)
    ar = np.arange(n + 1, dtype=np.int64)
    prev = np.zeros(n + 1, dtype=np.int64)
    for x in range(1, len(q) + 1):
        t = np.empty(n + 1, dtype=np.int64)
        t[0] = x
        t[1:] = np.minimum(prev[:-1] + (w != q[x - 1]), prev[1:] + 1)
        prev = np.minimum.accumulate(t - ar) + ar
    return prev


def last_row_loops(q, w):
    m, n = len(q), len(w)
    D = [[0] * (n + 1) for _ in range(m + 1)]
    for x in range(1, m + 1):
        D[x][0] = x
        for y in range(1, n + 1):
            D[x][y] = min(D[x - 1][y - 1] + (0 if q[x - 1] == w[y - 1] and w[y - 1] < 4 else 1), D[x - 1][y] + 1, D[x][y - 1] + 1)
    return np.array(D[m], dtype=np.int64)


def rows_of(anchored, reach):
    """Q[x] = A[m - 1 - x], m = min(|A|, reach)"""
    a = codes(anchored)
    m = min(len(a), reach)
    return a[:m][::-1]


def walk(t: np.ndarray, side: int, o: int) -> np.ndarray:
    """the contig as job (side, o) walks it: backwards iff side != o, complemented (codes below 4) iff o == 1"""
    w = t[::-1] if side != o else t
    return np.where(w < 4, 3 - w, w) if o else w


def runs(last: np.ndarray, k: int):
    """the maximal runs of columns 1 .. n with last[y] <= k as (y1, y2, minimum, y*)"""
    out, y, n = [], 1, len(last) - 1
    while y <= n:
        if last[y] > k:
            y += 1
            continue
        y2 = y
        while y2 + 1 <= n and last[y2 + 1] <= k:
            y2 += 1
        seg = last[y:y2 + 1]
        out.append((y, y2, int(seg.min()), y + int(np.argmin(seg))))                # (argmin: the first)
        y = y2 + 1
    return out


def search(contigs, anchored, side, reach, min_len, max_permille):
    """pla_search: the sorted list of (pattern, orientation, contig, boundary, lo, hi, distance)"""
    texts = [codes(c) for c in contigs]
    hits = []
    for p, (a, s) in enumerate(zip(anchored, side)):
        if len(a) < min_len:
            continue
        q = rows_of(a, reach)
        m = len(q)
        k = max_permille * m // 1000
        for o in (0, 1):
            for c, t in enumerate(texts):
                L = len(t)
                b = (lambda y: L - y) if s != o else (lambda y: y)
                for y1, y2, d, ys in runs(last_row(q, walk(t, s, o)), k):
                    hits.append((p, o, c, b(ys), min(b(y1), b(y2)), max(b(y1), b(y2)), d))
    return sorted(hits, key=lambda h: h[:4])


def chunked_last_row(q, w, k, chunk):
    """min(D(m, y), k + 1) for y = 1 .. len(w) as the device computes it: chunks of `chunk` owned columns, each started m + k
    columns earlier (or at the walk's start) from D(x, .) = x"""
    m, n = len(q), len(w)
    out = np.zeros(n + 1, dtype=np.int64)
    for y0 in range(0, n, chunk):
        start = max(0, y0 - (m + k))
        end = min(n, y0 + chunk)
        part = last_row(q, w[start:end])
        out[y0 + 1:end + 1] = part[y0 - start + 1:]
    return np.minimum(out, k + 1)


# ---- pla_place ----
NONE, AMBIGUOUS, LEFT_ONLY, RIGHT_ONLY, PLACED, BRIDGE, INCONSISTENT, CONFLICT = range(8)


def place(hits, left_pattern, right_pattern, max_span):
    """per locus (status, left hit or None, right hit or None, lo, hi, span or None) by the rules of the header"""
    out = []
    for lp, rp in zip(left_pattern, right_pattern):
        lh = [h for h in hits if lp >= 0 and h[0] == lp]
        rh = [h for h in hits if rp >= 0 and h[0] == rp]
        l = lh[0] if len(lh) == 1 else None
        r = rh[0] if len(rh) == 1 else None
        lo = hi = -1
        span = None
        if not lh and not rh:
            st = NONE
        elif len(lh) > 1 or len(rh) > 1:
            st = AMBIGUOUS
        elif not rh:
            st = LEFT_ONLY
        elif not lh:
            st = RIGHT_ONLY
        elif l[2] != r[2]:
            st = BRIDGE
        else:
            lo, hi = min(l[3], r[3]), max(l[3], r[3])
            st = INCONSISTENT
            if l[1] == r[1]:
                span = l[3] - r[3] if l[1] else r[3] - l[3]
                if 0 <= span <= max_span:
                    st = PLACED
        out.append([st, l, r, lo, hi, span])
    placed = [i for i, e in enumerate(out) if e[0] == PLACED]
    clash = set()
    for a in placed:
        for b in placed:
            if a < b and out[a][1][2] == out[b][1][2] and out[a][3] < out[b][4] and out[b][3] < out[a][4]:
                clash |= {a, b}
    for i in clash:
        out[i][0] = CONFLICT
    return [tuple(e) for e in out]
