"""CPU model of k_fill_v3's RIGHT rows with and without their clamp ("the band's last strip").

A RIGHT row is a row of the fast path whose band ENDS in the wave's macro-strip (or left of it: the rows a wave runs ahead of
its strip's first row with work, every cell masked).  Its cells past the band's end are masked to FBIG, so the running minimum
p they carry is the minimum of the whole DP row, Ptot, and the row stores min(p, INF - G(y)).  The clamp is a no-op exactly
where G(y) + Ptot stays below INF.  That follows from the gather's admission rule U + (2B + 4096) * maxS < 2^30 (U: the cost
of the row's present placement, maxS: the largest tally) WHEREVER the placement's cost as the DP counts it is at most U: the
cell (x, Way[x]) lies in the band and is reachable at that cost, from the free start, from the one-cell start (two tallies
more) and across a tear through the extension.  The kernel keeps the clamp all the same: for rows with blank runs between
their bases the gather's U leaves out what the DP charges for the columns of a run, and nothing separates those rows from the
others in the row's code.  This file pins the arithmetic for the case that is proved, so that the step can be taken up again.

The model is the int32 strip-row of test_fill_tilted_model.py (constants, ranges and the class imported from there and from
test_fill_handover_model.py), extended by the RIGHT role's choice, over a DP of three macro-strips whose band moves along a
placement whose cost -- every column it skips included -- is counted into U.  Two chains of rows run side by side, each on its
own results and its own hand-over words: one clamps every row behind a guard (the kernel), one stores p in RIGHT rows; LEFT rows
and rows with both guards clamp in both, INTERIOR rows in neither.  Every strip from the band's first one to the last of the
three is run in every row -- more rows ahead of a strip's first row with work than the kernel runs.  Asserted row by row and
strip by strip: the same Mprev, the same P_end, the same A and C bits; and the lemma itself, G(y) + Ptot < INF.  One case
violates the admission rule on purpose: there the two chains part, so the comparison can see a difference."""
import functools

import numpy as np
import pytest

from test_fill_handover_model import StripAt
from test_fill_tilted_model import BIG, FBIG, INF, NCOL, _i32

NS = 3                   # macro-strips of the model
SLACK = 4096             # the admission rule's slack, in columns


def _row(s, N, Nleft, P_in, b, inb, clamp):
    """one strip-row of the straight-line groups, Mprev = N = M - G; clamp: what a row behind a guard stores is min(p, INF - G)"""
    pm1 = np.concatenate(([Nleft], N[:-1]))
    d = _i32(pm1 + s.tab[b])
    u = _i32(N + s.ugt)
    C = d <= u
    t3 = np.minimum(np.minimum(d, u), s.ig)
    tg = np.where(inb, t3, FBIG)
    pb = np.minimum.accumulate(np.concatenate(([min(P_in, FBIG)], tg)))   # pb[i]: the running minimum before cell i
    A = tg >= pb[:-1]
    p = pb[1:]
    return (np.minimum(p, s.ig) if clamp else p), A, C, min(P_in, int(tg.min()))


class Dp:
    """three strips on common prefix sums; the columns from W on lie past the interval's end and keep the sentinels V4_LOADS
    gives them (scores, up and INF - G all FBIG, nothing added to them)"""

    def __init__(self, rng, g_total, max_tally, up_inf, W):
        ncol = NS * NCOL
        w = rng.integers(0, max_tally + 1, ncol + 1)
        w[rng.integers(1, ncol, 8)] = max_tally                       # (the largest tally does occur)
        room = g_total - int(w.sum())
        assert room >= 0
        G = room + np.cumsum(w)                                        # absolute prefix sums: the last one is g_total
        self.G, self.w, self.W, self.max_tally = G, w, W, max_tally
        self.strips = [StripAt(rng, G[k * NCOL:(k + 1) * NCOL + 1], max_tally, up_inf) for k in range(NS)]
        for k, s in enumerate(self.strips):
            past = k * NCOL + np.arange(NCOL) >= W
            s.tab[:, past] = FBIG
            s.ugt[past] = FBIG
            s.ig[past] = FBIG
            s.G = np.where(past, 0, s.G)
        self.S = [np.where(s.ig == FBIG, 0, s.tab + s.G - np.concatenate(([s.GL], s.G[:-1]))) for s in self.strips]   # S_b(y) again

    def score(self, b, y):
        return int(self.S[y // NCOL][b, y % NCOL])

    def gaps(self, y0, y1):
        """what the columns (y0, y1) cost a row that has no base in them"""
        return int(self.G[y1 - 1 + 1] - self.G[y0 + 1]) if y1 - 1 > y0 else 0


def _chains(dp, way, bases, B, start, K):
    """both chains over the rows of one placement; returns (rows compared, RIGHT strip-rows, of them wholly masked, first
    difference or None, the largest G(y) + Ptot seen in a masked cell)"""
    H, W = B // 2, dp.W
    c0 = way[0] - 1                                                    # the column of the base before the first row
    N = {}
    for form in ("clamped", "plain"):
        N[form] = []
        for k, s in enumerate(dp.strips):
            y = k * NCOL + np.arange(NCOL)
            free = np.where(s.ig == FBIG, FBIG, _i32(K - s.G))
            N[form].append(free if start == "free" else np.where(y == c0, free, s.ig))
    prev = None                                                        # (a, be, {form: Ptot}, {form: [P_end per strip]}) of row x - 1
    rows = rights = masked_rows = 0
    first_diff, worst = None, -1
    for x, (wy, b) in enumerate(zip(way, bases)):
        a = max(0, wy - H)
        be = min(a + B, W)
        assert a <= wy < be
        pend = {"clamped": [None] * NS, "plain": [None] * NS}
        out = {}
        for k, s in enumerate(dp.strips):
            y0 = k * NCOL
            if a >= y0 + NCOL:
                continue                                               # the band has left this strip behind: no work
            y = y0 + np.arange(NCOL)
            inb = (y >= a) & (y < be)
            left_guard, right_guard = a > y0, be < y0 + NCOL
            role = "interior" if not (left_guard or right_guard) else ("right" if not left_guard else "left_or_both")
            for form in ("clamped", "plain"):
                yq = y0 - 1
                if x == 0:
                    Nleft = (K - s.GL) if (start == "free" or yq == c0) else INF - s.GL
                elif yq < prev[0]:
                    Nleft = INF - s.GL                                 # PW:276
                elif yq < prev[1]:
                    Nleft = prev[3][form][k - 1]                       # M_last(x-1) = P_end(x-1) of the left neighbour
                else:
                    Nleft = prev[2][form]                              # the extension Ptot(x-1), PW:285-295
                P_in = pend[form][k - 1] if (k > 0 and a < y0) else BIG
                clamp = role == "left_or_both" or (role == "right" and form == "clamped")
                out[form] = _row(s, N[form][k], Nleft, P_in, b, inb, clamp)
                pend[form][k] = out[form][3]
            rows += 1
            if role == "right":
                rights += 1
                masked_rows += 0 if inb.any() else 1
                p = out["plain"][0]
                msk = ~inb & (s.ig != FBIG)
                if msk.any():
                    worst = max(worst, int((s.G[msk] + p[msk]).max()))
            same = all((out["clamped"][i] == out["plain"][i]).all() for i in range(3)) and out["clamped"][3] == out["plain"][3]
            if not same and first_diff is None:
                first_diff = (x, k, role)
            for form in ("clamped", "plain"):
                N[form][k] = out[form][0]
        last = (be - 1) // NCOL                                        # the strip that ends the band publishes the row's minimum
        prev = (a, be, {f: pend[f][last] for f in pend}, pend)
    return rows, rights, masked_rows, first_diff, worst


def _placement(kind, rng):
    """(B, W, Way): the band is [Way - B/2, Way + B/2), clamped to [0, W)"""
    if kind == "sweep":                                                # the band's end passes 250..273: every offset of a lane,
        return 200, NS * NCOL, list(range(150, 174))                   # strip 1's first column (257) and strip 0's last (256)
    if kind == "gaps":
        return 200, NS * NCOL, list(np.cumsum(rng.integers(1, 4, 60)) + 120)
    if kind == "right_edge":                                           # W = 700: the band's end stops there while its start moves on
        return 200, 700, list(range(520, 640))
    if kind == "tear":                                                 # the band jumps further than its width
        return 200, NS * NCOL, list(range(60, 80)) + list(range(430, 452))
    assert kind == "wide"                                              # wider than a strip: RIGHT in the third strip
    return 400, NS * NCOL, list(np.cumsum(rng.integers(1, 3, 50)) + 205)


KINDS = ["sweep", "gaps", "right_edge", "tear", "wide"]
# g_total (G up to 2^29 - 1), share of up = INF columns, and where the admission bound's room goes: "tallies" -- the largest tally
# the rule admits, "scores" -- tallies up to 3 000 and a start score that puts the placement's cost at the bound (every finite
# score then lies within 2 % of INF), None -- small numbers
TALLIES = [((1 << 29) - 1, 0.2, "tallies"), ((1 << 29) - 1, 0.2, "scores"), ((1 << 29) - 1, 1.0, "scores"), (NS * NCOL * 40, 0.05, None)]


@functools.lru_cache(maxsize=None)
def _case(kind, start, g_total, up_inf, at_bound, over=0):
    rng = np.random.default_rng(len(kind) * 131 + (start == "free") + int(up_inf * 10) + (g_total % 977))
    B, W, way = _placement(kind, rng)
    way = [int(v) for v in way]
    # the largest tally the rule admits next to a sum of G below 2^29: (2B + 4096) maxS + U < 2^30 with U >= what the rows cost
    max_tally = {"tallies": min(g_total // (NS * NCOL + 1), ((1 << 30) - 1) // (2 * B + SLACK + 2 * (way[-1] - way[0] + len(way)))), "scores": 3000, None: 30}[at_bound]
    dp = Dp(rng, g_total, max_tally, up_inf, W)
    bases = [int(v) for v in rng.integers(0, 4, len(way))]
    cost = sum(dp.score(b, y) for b, y in zip(bases, way)) + sum(dp.gaps(y0, y1) for y0, y1 in zip([way[0] - 1] + way[:-1], way))
    maxS = dp.max_tally                                                # (every tally of the model is drawn up to it, and it occurs)
    assert maxS == int(dp.w[1:].max()) and max(int(S.max()) for S in dp.S) <= maxS
    # K: what the rows before the first one have cost (a segment's rows start from 0; the model starts from the score at which the
    # whole placement sits exactly at the admission bound) -- `over` columns' worth of the largest tally beyond it violates the rule
    K = ((1 << 30) - 1 - (2 * B + SLACK) * maxS - cost + over * maxS) if at_bound else 0
    assert K >= 0
    U = K + cost
    admitted = U + (2 * B + SLACK) * maxS < (1 << 30) and g_total < (1 << 29)
    return _chains(dp, way, bases, B, start, K) + (admitted, U, maxS, B)


@pytest.mark.parametrize("g_total,up_inf,at_bound", TALLIES)
@pytest.mark.parametrize("start", ["free", "one_cell"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_right_row_stores_the_same_with_and_without_its_clamp(kind, start, g_total, up_inf, at_bound):
    rows, rights, masked_rows, first_diff, worst, admitted, U, maxS, B = _case(kind, start, g_total, up_inf, at_bound)
    print("%s/%s: %d strip-rows, %d RIGHT (%d wholly masked); U = %d, maxS = %d, bound %d; largest G + Ptot in a masked cell %d"
          % (kind, start, rows, rights, masked_rows, U, maxS, U + (2 * B + SLACK) * maxS, worst))
    assert admitted
    assert rights >= 20 and (masked_rows >= 10 or kind == "right_edge")   # (at the right edge no strip lies beyond the band)
    assert first_diff is None, first_diff
    assert 0 <= worst < INF                                            # the lemma: the extension is a finite score in every masked cell


def test_every_offset_of_the_band_end_occurs():
    """the sweep's band ends at 250..273: each of a lane's four offsets six times, the last column of strip 0 (the band ends at
    256: strip 1 wholly masked) and the first column of strip 1 (257)"""
    B, W, way = _placement("sweep", None)
    ends = [min(max(0, w - B // 2) + B, W) for w in way]
    assert {e % 4 for e in ends} == {0, 1, 2, 3} and NCOL in ends and NCOL + 1 in ends and ends == list(range(250, 274))
    B, W, way = _placement("right_edge", None)
    ends = [min(max(0, w - B // 2) + B, W) for w in way]
    assert ends.count(W) > 30 and W % NCOL != 0                        # the band's end stops moving, inside a strip


@pytest.mark.parametrize("kind", ["sweep", "wide"])
def test_beyond_the_admission_rule_the_two_forms_part(kind):
    """the same rows with the start score raised by 6 000 columns' worth of the largest tally -- more than the rule's whole
    allowance of 2B + 4096: G + Ptot passes INF in masked cells, the clamped row stores INF - G there and the plain one Ptot"""
    rows, rights, masked_rows, first_diff, worst, admitted, U, maxS, B = _case(kind, "free", (1 << 29) - 1, 0.2, "scores", over=6000)
    assert not admitted
    assert worst >= INF
    assert first_diff is not None and first_diff[2] == "right"
