"""CPU model of one strip-row update of k_fill_v3 in both forms: the row kept as the true score M (the form
k_fill_v2 still has) and as N = M - G.  int32 arithmetic as on the device, every intermediate also in int64 so that a wrap
would show.  Asserted cell by cell over chained rows: N + G == M, the same A and C bits, the same P_end."""
import numpy as np
import pytest

INF = 1 << 30            # PWR_INF
BIG = 0x7fffffff         # PWR_BIG
FBIG = 0x3fffffff        # neutral element of the fast path's scan
NCOL = 256               # one macro-strip of 64 lanes x 4 columns


def _i32(a):
    """int64 -> int32 as the device would hold it; the value must fit (nothing wraps)"""
    a = np.asarray(a, dtype=np.int64)
    assert a.min() >= -(1 << 31) and a.max() < (1 << 31), "an intermediate leaves the 32-bit range"
    return a


class Strip:
    """the constants of one macro-strip as the gather leaves them: {S_b - G}, {up - G, G, INF - G}; GL = G of the column before"""

    def __init__(self, rng, g_total, max_tally, up_inf_frac):
        w4 = rng.integers(0, max_tally + 1, NCOL + 1)
        room = g_total - int(w4.sum())
        assert room >= 0
        G = room + np.cumsum(w4)                                   # absolute prefix sums: the last one is g_total (< 2^29)
        self.GL, self.G = int(G[0]), G[1:].astype(np.int64)
        S = rng.integers(0, max_tally + 1, (4, NCOL)).astype(np.int64)
        up = rng.integers(0, max_tally + 1, NCOL).astype(np.int64)
        up[rng.random(NCOL) < up_inf_frac] = INF - 1               # "up = INF" columns (INF - 1: pm + up stays below 2^31)
        self.Sg = _i32(S - self.G)
        self.ugm = _i32(up - self.G)
        self.ig = _i32(INF - self.G)
        # the tilted constants, built once at strip take-over
        Gprev = np.concatenate(([self.GL], self.G[:-1]))
        self.tab = _i32(self.Sg + Gprev)
        self.ugt = _i32(self.ugm + self.G)


def row_true(s, M, Mleft, P_in, b, inb, left_of_band, fast):
    """the row with Mprev = M.  fast: the straight-line groups (scan seeded with FBIG, result clamped); else the one-row path"""
    pm1 = np.concatenate(([Mleft], M[:-1]))
    d = _i32(pm1 + s.Sg[b])
    u = _i32(M + s.ugm)
    C = d <= u
    t3 = np.minimum(np.minimum(d, u), s.ig)
    tg = np.where(inb, t3, FBIG if fast else BIG)
    pq = min(P_in, FBIG) if fast else P_in
    pb = np.minimum.accumulate(np.concatenate(([pq], tg)))          # pb[i]: the running minimum before cell i
    A = tg >= pb[:-1]
    p = pb[1:]
    if fast:
        Mn = np.minimum(_i32(s.G + p), INF)
    else:
        Mn = np.where(left_of_band, INF, _i32(s.G + np.where(left_of_band, 0, p)))
    return Mn, A, C, min(P_in, int(tg.min())), (d, u, t3, p)


def row_tilted(s, N, Nleft, P_in, b, inb, left_of_band, fast, interior):
    """the row with Mprev = N = M - G"""
    pm1 = np.concatenate(([Nleft], N[:-1]))
    d = _i32(pm1 + s.tab[b])
    u = _i32(N + s.ugt)
    C = d <= u
    t3 = np.minimum(np.minimum(d, u), s.ig)
    tg = np.where(inb, t3, FBIG if fast else BIG)
    pq = min(P_in, FBIG) if fast else P_in
    pb = np.minimum.accumulate(np.concatenate(([pq], tg)))
    A = tg >= pb[:-1]
    p = pb[1:]
    if fast:
        if interior:
            assert (p <= s.ig).all(), "without a band guard p <= INF - G must hold by construction"
            Nn = p
        else:
            Nn = np.minimum(p, s.ig)
    else:
        Nn = np.where(left_of_band, s.ig, p)
    return Nn, A, C, min(P_in, int(tg.min())), (d, u, t3, p)


def _start_vector(rng, s, kind, g_total):
    """(M, N) above the first row: the free start, the one-cell start, a random mix of finite and unreachable cells, or the
    virtual extension G + Ptot a strip starts from (not clamped: it may pass INF)"""
    if kind == "free":
        M = np.zeros(NCOL, dtype=np.int64)
        return M, _i32(-s.G)
    if kind == "one_cell":
        c = int(rng.integers(0, NCOL))
        M = np.full(NCOL, INF, dtype=np.int64)
        M[c] = 0
        return M, np.where(np.arange(NCOL) == c, -s.G, s.ig)
    if kind == "extension":
        eT = int(rng.integers(-s.GL, INF - g_total + 1))           # a P word: some t3 <= INF - G of a column further left
        return _i32(s.G + eT), np.full(NCOL, eT, dtype=np.int64)
    M = rng.integers(0, INF, NCOL).astype(np.int64)
    M[rng.random(NCOL) < 0.3] = INF
    return M, _i32(M - s.G)


CASES = [  # g_total (just under 2^29 at the top), largest tally, share of up = INF columns
    (10000, 30, 0.0), (1 << 20, 3000, 0.1), ((1 << 29) - 1, 170000, 0.2), ((1 << 29) - 1, 5, 1.0), ((NCOL + 1) * 7, 7, 0.05)]


@pytest.mark.parametrize("start", ["free", "one_cell", "random", "extension"])
@pytest.mark.parametrize("g_total,max_tally,up_inf", CASES)
def test_tilted_row_is_the_true_row_minus_g(g_total, max_tally, up_inf, start):
    rng = np.random.default_rng(g_total % 9973 + max_tally)
    for trial in range(6):
        s = Strip(rng, g_total, max_tally, up_inf)
        M, N = _start_vector(rng, s, start, g_total)
        assert (N + s.G == M).all()
        for x in range(24):
            # the role of the row: INTERIOR (no guard), RIGHT (band ends in the strip), LEFT (band starts in it), both guards
            # (run-time flags), and the one-row path with either guard
            role = ["interior", "right", "left", "flags", "general"][int(rng.integers(0, 5))]
            af = int(rng.integers(1, NCOL - 1)) if role in ("left", "flags", "general") and rng.random() < 0.8 else 0
            be = int(rng.integers(af + 1, NCOL + 1)) if role in ("right", "flags", "general") else NCOL
            if role == "interior":
                af, be = 0, NCOL
            y = np.arange(NCOL)
            inb, left_of_band = (y >= af) & (y < be), y < af
            # what the left neighbour hands over: nothing (the band starts here, or the neighbour is past the band: INF as
            # PW:276 has it), or its last cell and its running minimum
            has_left = role in ("interior", "right") or (role in ("flags", "general") and af == 0 and rng.random() < 0.7)
            if has_left and rng.random() < 0.8:
                Mleft = INF if rng.random() < 0.25 else int(rng.integers(0, INF))
                P_in = int(rng.integers(-s.GL, INF + 1))            # some t3 - it contains INF - G - of a column further left
            else:
                Mleft, P_in = INF, BIG
            Nleft = Mleft - s.GL                                    # unreachable is exactly INF - G(y) as N
            b = int(rng.integers(0, 4))
            fast = role != "general"
            Mn, A0, C0, Pe0, q0 = row_true(s, M, Mleft, P_in, b, inb, left_of_band, fast)
            Nn, A1, C1, Pe1, q1 = row_tilted(s, N, Nleft, P_in, b, inb, left_of_band, fast, role == "interior")
            for a0, a1, name in zip(q0, q1, "d u t3 p".split()):
                assert (a0 == a1).all(), (trial, x, role, name)
            assert (A0 == A1).all() and (C0 == C1).all() and Pe0 == Pe1, (trial, x, role)
            assert (_i32(Nn + s.G) == Mn).all(), (trial, x, role)
            unreachable = Mn == INF
            assert (Nn[unreachable] == s.ig[unreachable]).all(), (trial, x, role)
            M, N = Mn, Nn


def test_the_three_identities_on_their_own():
    """min(G + p, INF) = G + min(p, INF - G);  p <= INF - G where a cell's own candidate is in the minimum;  hence every compared
    quantity is the same number"""
    rng = np.random.default_rng(11)
    G = rng.integers(0, 1 << 29, 100000).astype(np.int64)
    p = rng.integers(-(1 << 29), FBIG + 1, 100000).astype(np.int64)
    p[:1000] = FBIG
    G[:10] = 0
    assert (np.minimum(_i32(G + p), INF) == _i32(G + np.minimum(p, INF - G))).all()
    t3 = np.minimum(p, INF - G)                                     # a candidate always contains ig
    run = np.minimum.accumulate(t3[::-1])[::-1]                     # any minimum that includes the cell's own candidate
    assert (np.minimum(run, t3) <= INF - G).all()
