"""CPU model of the hand-over between two neighbouring macro-strips of k_fill_v3: a wave publishes ONE tagged
word per DP row, P_end, and its right neighbour takes the score left of its first column, M_last(x-1), from that word.  The
strip-row itself is the int32 model of test_fill_tilted_model.py (imported, not restated); here a producer strip and a consumer
strip run side by side over chained rows whose band moves over both, and the consumer's row is computed from two words
({P_end, M_last}, as k_fill_v2 has them) and from one.

The consumer's rule for the score left of its strip (yq = the producer's last column; [ap, bp) = the band of row x - 1):
    yq <  ap        INF - G(yq)   PW:276      never reads a word
    ap <= yq < bp   M_last(x-1)               the ONLY case that reads it
    yq >= bp        Ptot(x-1)     PW:285-295  the P_end word of the strip that ends the band
Asserted: wherever the rule reads M_last it equals P_end of that row bit for bit, and the consumer's row (scores, P_end, A and C
bits) is identical either way.  Rows the kernel runs AHEAD of a strip's first row with work (every cell masked) read the word
whatever the rule says; there it can only reach the C bit of one masked cell, and the first row with work after them takes it
as the extension, which it is whenever G(yq) + Ptot stays finite -- what the gather proves before a job may use this kernel."""
import functools

import numpy as np
import pytest

from test_fill_tilted_model import BIG, FBIG, INF, NCOL, Strip, _i32, row_tilted

YQ = NCOL - 1            # the producer's last column; the producer owns [0, NCOL), the consumer [NCOL, 2 * NCOL)


class StripAt(Strip):
    """a macro-strip on given prefix sums (G[0] belongs to the column before it), with the constants Strip derives"""

    def __init__(self, rng, G, max_tally, up_inf_frac):
        self.GL, self.G = int(G[0]), G[1:].astype(np.int64)
        S = rng.integers(0, max_tally + 1, (4, NCOL)).astype(np.int64)
        up = rng.integers(0, max_tally + 1, NCOL).astype(np.int64)
        up[rng.random(NCOL) < up_inf_frac] = INF - 1
        self.Sg = _i32(S - self.G)
        self.ugm = _i32(up - self.G)
        self.ig = _i32(INF - self.G)
        Gprev = np.concatenate(([self.GL], self.G[:-1]))
        self.tab = _i32(self.Sg + Gprev)
        self.ugt = _i32(self.ugm + self.G)


def _two_strips(rng, g_total, max_tally, up_inf):
    w = rng.integers(0, max_tally + 1, 2 * NCOL + 1)
    room = g_total - int(w.sum())
    assert room >= 0
    G = room + np.cumsum(w)                                         # absolute prefix sums, the last one g_total (< 2^29)
    return StripAt(rng, G[:NCOL + 1], max_tally, up_inf), StripAt(rng, G[NCOL:], max_tally, up_inf)


def _band(rng, kind):
    """[af, be) in the columns of the two strips (it may reach beyond them on either side)"""
    if kind == "over_both":
        return -50, 2 * NCOL + 50
    if kind == "starts_in_producer":
        return int(rng.integers(1, NCOL)), 2 * NCOL + 50
    if kind == "ends_in_consumer":
        return -50, int(rng.integers(NCOL + 1, 2 * NCOL))
    if kind == "starts_and_ends_inside":
        return int(rng.integers(1, NCOL)), int(rng.integers(NCOL + 1, 2 * NCOL))
    if kind == "ends_at_the_boundary":                              # the producer's last column is the band's last
        return int(rng.integers(-50, NCOL - 1)), NCOL
    if kind == "narrow_across":                                     # narrower than one strip, over the boundary
        af = int(rng.integers(NCOL - 40, NCOL))
        return af, int(rng.integers(NCOL + 1, af + 60))
    if kind == "narrow_in_producer":
        af = int(rng.integers(0, NCOL - 60))
        return af, af + int(rng.integers(1, 60))
    if kind == "ends_in_producer":
        return -50, int(rng.integers(1, NCOL))
    if kind == "producer_left_of_band":
        return int(rng.integers(NCOL, 2 * NCOL - 1)), 2 * NCOL + 50
    assert kind == "producer_right_of_band"
    return -400, int(rng.integers(-300, 1))


READS = ["over_both", "starts_in_producer", "ends_in_consumer", "starts_and_ends_inside", "ends_at_the_boundary", "narrow_across"]
OTHERS = ["narrow_in_producer", "ends_in_producer", "producer_left_of_band", "producer_right_of_band"]

CASES = [  # g_total (just under 2^29 at the top), largest tally, share of up = INF columns
    (20000, 30, 0.0), (1 << 21, 3000, 0.1), ((1 << 29) - 1, 170000, 0.2), ((1 << 29) - 1, 5, 1.0), ((2 * NCOL + 1) * 7, 7, 0.05)]

ALL_CASES = [(g, t, u, s) for (g, t, u) in CASES for s in ("free", "one_cell")]


def _start(rng, s, kind):
    """N above the first row: the free start, or the one-cell start (an unreachable prefix: every other column INF - G)"""
    if kind == "free":
        return _i32(-s.G)
    c = int(rng.integers(0, NCOL))
    return np.where(np.arange(NCOL) == c, -s.G, s.ig)


def _role(rng, af, be, y0):
    """(inb, left_of_band, fast, interior) of a strip whose first column is y0, for the band [af, be)"""
    y = y0 + np.arange(NCOL)
    inb, left = (y >= af) & (y < be), y < af
    guards = not inb.all()
    fast = rng.random() < 0.75                                      # the straight-line groups, or the one-row loop
    return inb, left, fast, fast and not guards


@functools.lru_cache(maxsize=None)
def _run_case(g_total, max_tally, up_inf, start):
    """the chained rows of one case, every assertion on the way; returns what was seen (computed once, shared by the tests)"""
    TALLY = {"rows": 0, "reads": 0, "ahead": 0, "ahead_differs": 0, "kinds": set()}
    rng = np.random.default_rng(g_total % 9973 + max_tally + (start == "free"))
    for trial in range(8):
        sp, sc = _two_strips(rng, g_total, max_tally, up_inf)
        Np, Nc = _start(rng, sp, start), _start(rng, sc, start)
        if start == "one_cell":
            Nc = sc.ig.copy()                                       # the one cell lies in the producer's strip
        prev = None                                                 # (ap, bp, P_end, M_last) of the producer's row x - 1
        ahead_before = False
        for x in range(28):
            kind = READS[int(rng.integers(0, len(READS)))] if rng.random() < 0.72 else OTHERS[int(rng.integers(0, len(OTHERS)))]
            af, be = _band(rng, kind)
            TALLY["kinds"].add(kind)
            b = int(rng.integers(0, 4))
            # ---- the producer's row x
            pub = None
            if af <= YQ:                                            # (a strip wholly left of the band has no work and publishes nothing)
                inb, left, fast, interior = _role(rng, af, be, 0)
                if not inb.any():
                    fast = True                                     # rows past the band run in the groups, masked by the right-hand guard
                if af < 0:                                          # the band starts further left: its own neighbour hands over
                    Nleft = (INF if rng.random() < 0.25 else int(rng.integers(0, INF))) - sp.GL
                    P_in = int(rng.integers(-sp.GL, INF - sp.GL + 1))
                else:
                    Nleft, P_in = INF - sp.GL, BIG
                Np, _, _, Pe, _ = row_tilted(sp, Np, Nleft, P_in, b, inb, left, fast, interior)
                pub = (int(Pe), int(Np[-1]))
            # ---- the consumer's row x, from the words of the producer's rows x - 1 and x
            if af < 2 * NCOL:
                inb, left, fast, interior = _role(rng, af, be, NCOL)
                all_masked = not inb.any()
                if all_masked:
                    fast = True
                reads = prev is not None and prev[0] <= YQ < prev[1]
                if prev is None or YQ < prev[0]:
                    left2 = left1 = (-sc.GL if (prev is None and start == "free") else INF - sc.GL)
                elif reads:
                    left2, left1 = prev[3], prev[2]                 # M_last(x-1) / the P_end word in its place
                    assert left2 == left1, (trial, x, kind, "the rule reads M_last and it is not P_end")
                else:
                    left2 = left1 = prev[2]                         # Ptot(x-1): the band ended in the producer's strip or left of it
                forced = prev is not None and not reads and YQ >= prev[1] and fast and (all_masked or ahead_before)
                if forced:
                    # a row run ahead of the strip's first row with work, or that first row itself: the kernel takes the word of
                    # row x - 1 whatever the rule says -- two words: min(Ptot, INF - G(yq)) from a producer's group, one word: Ptot
                    left2, left1 = prev[3], prev[2]
                    assert left2 in (left1, min(left1, int(sp.ig[-1])))   # (the one-row loop clamps nothing: the same word)
                P_in = pub[0] if (pub is not None and af < NCOL) else BIG
                r2 = row_tilted(sc, Nc, left2, P_in, b, inb, left, fast, interior)
                r1 = row_tilted(sc, Nc, left1, P_in, b, inb, left, fast, interior)
                same_c = (r2[2] == r1[2]).all()
                assert (r2[0] == r1[0]).all() and (r2[1] == r1[1]).all() and r2[3] == r1[3], (trial, x, kind)
                if forced and all_masked:
                    TALLY["ahead"] += 1
                    TALLY["ahead_differs"] += 0 if same_c else 1
                    assert (r2[2][1:] == r1[2][1:]).all()           # only the C bit of the masked first cell can tell them apart,
                    assert same_c or left1 + int(sp.G[-1]) >= INF   # and only past what the gather admits
                elif forced:
                    assert same_c or left1 + int(sp.G[-1]) >= INF, (trial, x, kind)   # the extension: finite, so not clamped
                else:
                    assert same_c, (trial, x, kind)
                    TALLY["rows"] += 1
                    TALLY["reads"] += 1 if reads else 0
                ahead_before = all_masked and YQ >= be
                Nc = r2[0]
            prev = (af, be, pub[0], pub[1]) if pub is not None else (af, be, None, None)
    return TALLY


@pytest.mark.parametrize("g_total,max_tally,up_inf,start", ALL_CASES)
def test_one_word_hands_over_what_two_did(g_total, max_tally, up_inf, start):
    t = _run_case(g_total, max_tally, up_inf, start)
    assert t["rows"] > 100 and t["reads"] > 50


def test_the_dangerous_case_is_not_rare_in_the_sample():
    """The share of generated consumer rows in which the rule reads M_last: 0.83 of the 1 849 rows these seeds generate (bands
    that cover the boundary are drawn 72 % of the time; rows run ahead of a strip's first row are counted apart), required: at
    least half.
    Every kind of band is drawn, and rows run ahead of a strip's first row with work occur."""
    ts = [_run_case(*c) for c in ALL_CASES]
    rows, reads = sum(t["rows"] for t in ts), sum(t["reads"] for t in ts)
    ahead, differs = sum(t["ahead"] for t in ts), sum(t["ahead_differs"] for t in ts)
    print("rows %d, the rule reads M_last in %d (%.2f); rows run ahead %d, of them with another C bit in the masked cell %d"
          % (rows, reads, reads / rows, ahead, differs))
    assert reads / rows >= 0.5
    assert set().union(*(t["kinds"] for t in ts)) == set(READS + OTHERS)
    assert ahead > 0


def test_p_end_is_the_last_column_in_both_paths():
    """lane 63's running minimum after the strip's last cell is min(P_in, every tg) = P_end: the fast path caps P_in at FBIG
    first, which changes nothing because the scan is seeded with FBIG; the one-row path caps nothing"""
    rng = np.random.default_rng(3)
    tg = rng.integers(-(1 << 29), FBIG + 1, (2000, 16)).astype(np.int64)
    tg[rng.random(tg.shape) < 0.3] = FBIG
    P_in = rng.integers(-(1 << 29), BIG, 2000).astype(np.int64)
    P_in[:200] = BIG
    incl = np.minimum(tg.min(axis=1), FBIG)
    assert (np.minimum(np.minimum(P_in, FBIG), incl) == np.minimum(P_in, incl)).all()
