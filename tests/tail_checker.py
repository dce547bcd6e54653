"""Exact yardstick for the device's hypergeometric tail (repeatresolver_amd/csrc/hyper_tail.h) and the three stage formulas on
top of it, and the grid of counts the tail tests evaluate (tests/test_tail_checker.py without a GPU, tests/test_gpu_tail.py
on one).  Python integers and `decimal` at 60 digits only: no numpy float, no scipy, no lgamma on the exact side.

Counts are the stages' own: (schnitt, cov, gr1, gr2, size1, size2) -> the tail of X ~ Hypergeometric(n1 = gr2 successes,
n2 = cov - gr2 failures, t = gr1 draws) at k = schnitt - 1 (MC:415, RR:451, RR:492-493).

The error model.  The scheme (GSL's, restated in oracle/mc_oracle.c and on the device) takes one pdf term as exp of three
lnchoose, each a difference of lgamma values as large as lgamma(cov + 1), and sums ratio-recurrence terms away from k.  The
table's rounding, a few 2^-53 * lgamma(cov + 1), therefore is the RELATIVE error of the sum, and 2^-53 * lgamma(cov + 1) *
log10(e) its error in -log10 units.  Below the midpoint t * n1 / (n1 + n2) the scheme sums the OTHER tail and returns
1 - sum: the absolute error of the sum becomes the absolute error of the value returned, which is (1 - q) / q times larger
relative to a small q.  bound() below is that model; C_HOST is what the host restatement needs of it, measured."""
import math
import random
from collections import namedtuple
from decimal import Decimal, localcontext
from functools import lru_cache

PREC = 60
MAX_ROWS = 30000                    # PMC_MAX_ROWS = PGR_MAX_ROWS
LOG10E = math.log10(math.e)
CAP = Decimal(99)

# Largest |mco_hyper_Q / mco_hyper_P - exact| / bound(cov, amp, 1) in -log10 units over grid(), on the CPU
# (tests/test_tail_checker.py::test_host_oracle_against_exact_measures_c_host measures it and holds it against this record).
C_HOST = 6.6                        # measured 6.543 on 2026-10-20, at (schnitt, cov, gr1, gr2) = (2, 30000, 3, 3), direct sum
C_DEV = 2.0 * C_HOST                # the device reads the same table; exp, log10 and the multiply chain add a few ulp


@lru_cache(maxsize=None)
def _comb(n, m):
    return math.comb(n, m)                                             # (0.2 s at 30 000 over 15 000: the grid repeats them)


def _iter_terms(n1, n2, t):
    """(i, C(n1, i) C(n2, t - i)) over the support, ascending: one comb at the low end, then the integer ratio recurrence"""
    lo, hi = max(0, t - n2), min(n1, t)
    c = _comb(n1, min(lo, n1 - lo)) * _comb(n2, min(t - lo, n2 - t + lo))
    yield lo, c
    for i in range(lo, hi):
        c, r = divmod(c * ((n1 - i) * (t - i)), (i + 1) * (n2 - t + i + 1))
        assert r == 0
        yield i + 1, c


def terms(n1, n2, t):
    """(lo, hi, [C(n1, i) C(n2, t - i) for i in lo .. hi]); the terms sum to C(n1 + n2, t)"""
    lo, hi = max(0, t - n2), min(n1, t)
    out = [c for _, c in _iter_terms(n1, n2, t)]
    assert len(out) == hi - lo + 1 and sum(out) == _comb(n1 + n2, min(t, n1 + n2 - t))
    return lo, hi, out


def tails(n1, n2, t, ks):
    """One pass over the support for several k: ({k: (#{X <= k}, term at k)}, denominator C(n1 + n2, t))"""
    want = set(ks)
    got = {}
    cum = 0
    lo = max(0, t - n2)
    for i, c in _iter_terms(n1, n2, t):
        cum += c
        if i in want:
            got[i] = (cum, c)
    assert cum == _comb(n1 + n2, min(t, n1 + n2 - t))
    for k in want:
        if k not in got:
            got[k] = (0, 0) if k < lo else (cum, 0)
    return got, cum


def exact_P(k, n1, n2, t):
    """P(X <= k) as (numerator, denominator)"""
    got, den = tails(n1, n2, t, [k])
    return got[k][0], den


def exact_Q(k, n1, n2, t):
    """P(X > k) as (numerator, denominator)"""
    num, den = exact_P(k, n1, n2, t)
    return den - num, den


def _log10_int(x):
    sh = max(0, x.bit_length() - 256)                                  # (the bits dropped are 2^-255 of x)
    return Decimal(x >> sh).log10() + sh * Decimal(2).log10()


def neglog10(num, den):
    """-log10(num / den) as a Decimal of 60 digits, uncapped; None for num == 0 (infinite)"""
    if num == 0:
        return None
    if num == den:
        return Decimal(0)
    with localcontext() as ctx:
        ctx.prec = PREC
        return _log10_int(den) - _log10_int(num)


def capped(z):
    """`if (isinf(Z) || Z > 99) Z = 99` (MC:417, RR:453, RR:503)"""
    return CAP if z is None or z > CAP else z


def exact_Z(schnitt, cov, gr1, gr2):
    """-log10 P(X > schnitt - 1), capped at 99"""
    return capped(neglog10(*exact_Q(schnitt - 1, gr2, cov - gr2, gr1)))


def branch(k, n1, n2, t):
    """True where the scheme sums downward from k and returns the complement for Q (k < t * n1 / (n1 + n2)).  In integers:
    the double quotient of two integers below 2^31 cannot round across an integer k unless it equals it."""
    return k * (n1 + n2) < t * n1


def amp(complement, num, den):
    """(1 - q) / q for the exact value q = num / den the scheme returns as a complement (1 - sum), else 1"""
    if not complement:
        return 1.0
    return math.inf if num == 0 else (den - num) / num


def bound(cov, amp, C):
    """the error model in -log10 units (the + 1 keeps it positive at cov = 1)"""
    return C * 2.0 ** -53 * (math.lgamma(cov + 1) + 1.0) * LOG10E * max(1.0, amp)


# ---- the three stage formulas from an exact tail ----
def mc_significance(z_raw, s, gr1, gr2, size1, size2):
    """MC:413-434.  z_raw: the uncapped exact -log10 Q (None: infinite).  Returns (value, saturated)."""
    if gr1 == 0 or gr2 == 0 or s < 1:
        return Decimal(0), False
    if z_raw is None or z_raw > 98:
        return 98.0 + 2.0 * s / (2.0 * s + (size1 - s) + (size2 - s)), True
    return z_raw, False


def gr_significance(z_raw, s, gr1, gr2, size_i, size_a):
    """RR:472-488.  Returns (value, saturated)."""
    if gr1 == 0 or gr2 == 0 or s < 1:
        return Decimal(0), False
    if z_raw is None or z_raw > 98:
        return 97.90 + float(2 * s) / float(size_i + size_a), True
    return z_raw, False


def km_choice(s, pnum, qnum):
    """RR:495-503: True where the relative significance takes P(X <= s), False where it takes Q = P(X >= s) (0 at s = 0, where
    the unsigned s - 1 wraps and the tail of RR:493 is empty)"""
    return pnum < qnum or s == 0


# ---- a tuple of the grid with everything exact about it ----
Rec = namedtuple("Rec", "counts tag den pnum qnum tnum lower_q lower_p amp_q amp_p zq_raw zp_raw zb_raw")
# counts = (schnitt, cov, gr1, gr2, size1, size2); pnum = #{X <= s}, qnum = #{X >= s}, tnum = #{X = s};
# lower_q / lower_p: the scheme's branch for Q(s - 1) / P(s) (None: answered before the sum);
# amp_*: (1 - q) / q where the value returned is a complement, else 1;  z*_raw: uncapped -log10 (None: infinite)


def annotate(tuples):
    """tuples: [(counts, tag)] -> [Rec], one pass over the support per distinct (gr2, cov - gr2, gr1)"""
    by = {}
    for idx, (c, _) in enumerate(tuples):
        by.setdefault((c[3], c[1] - c[3], c[2]), []).append(idx)
    out = [None] * len(tuples)
    for (n1, n2, t), idxs in by.items():
        ks = set()
        for i in idxs:
            s = tuples[i][0][0]
            ks.update((s - 1, s))
        got, den = tails(n1, n2, t, ks)
        for i in idxs:
            c, tag = tuples[i]
            s = c[0]
            below = got[s - 1][0]                                      # #{X <= s - 1}
            pnum, tnum = got[s]
            qnum = den - below
            lower_q = None if (s < 1 or s - 1 >= n1 or s - 1 >= t) else branch(s - 1, n1, n2, t)
            lower_p = None if (s >= n1 or s >= t) else branch(s, n1, n2, t)
            amp_q = amp(lower_q is True, qnum, den)                    # Q is the complement below the midpoint,
            amp_p = amp(lower_p is False, pnum, den)                   # P at and above it
            out[i] = Rec(c, tag, den, pnum, qnum, tnum, lower_q, lower_p, amp_q, amp_p,
                         neglog10(qnum, den), neglog10(pnum, den), neglog10(tnum, den))
    return out


# ---- the grid ----
COVS = (1, 2, 63, 64, 65, 600, 2049, 13594, 30000)
SEED = 20261020


def _sizes(rng, g1, g2):
    pick = rng.randrange(4)
    if pick == 0:
        return g1, g2
    if pick == 1:
        return min(MAX_ROWS, g1 + 5), min(MAX_ROWS, g2 + 7)
    if pick == 2:
        return rng.randint(g1, MAX_ROWS), rng.randint(g2, MAX_ROWS)
    return MAX_ROWS, g2


def _main_tuples(rng):
    out = []
    for cov in COVS:
        grs = {g for g in (1, 2, 3, cov // 2, cov - 1, cov) if 1 <= g <= cov}
        grs.update(rng.randint(1, cov) for _ in range(4 if cov <= 2049 else 2))   # (a deep pair costs 0.2 s of binomials)
        grs = sorted(grs)
        for g1 in grs:
            for g2 in grs:
                lo, hi = max(0, g1 + g2 - cov), min(g1, g2)
                m = g1 * g2 / cov
                cand = {lo, lo + 1, math.floor(m), math.ceil(m), hi - 1, hi, 0, 1, rng.randint(lo, hi), rng.randint(lo, hi)}
                for s in sorted(x for x in cand if lo <= x <= hi):
                    out.append(((s, cov, g1, g2) + _sizes(rng, g1, g2), "main"))
        # an empty group: every stage answers 0 before any lookup
        out.append(((0, cov, 0, min(cov, 3), 0, 5), "main"))
        out.append(((0, cov, min(cov, 2), 0, 4, 0), "main"))
    return out


def _corner_tuples(rng):
    """small groups in deep coverage sharing one row: k = 0 lies below a midpoint far below 1, the scheme returns 1 - P(X = 0)
    and the table's rounding is amplified by about cov / (gr1 * gr2)"""
    out = []
    for cov in (600, 2049, 13594, 30000):
        for g1 in range(1, 11):
            for g2 in range(1, 11, 2 if cov > 2049 else 1):
                if g1 * g2 * 150 < cov:
                    out.append(((1, cov, g1, g2) + _sizes(rng, g1, g2), "corner"))
    return out


def _sat_tuples(rng):
    """the k whose exact -log10 tail lies in (96, 101), around the two saturation thresholds: for n up to 900 (as
    tests/test_mc_oracle.py does), and with cov near 2049 and near 13 594"""
    triples = []
    for _ in range(45):
        n1, n2 = rng.randrange(150, 900), rng.randrange(150, 900)
        triples.append((n1, n2, rng.randrange(120, n1 + n2 - 50)))
    for _ in range(40):
        cov = rng.randint(2040, 2058)
        n1 = rng.randint(100, 1000)
        triples.append((n1, cov - n1, rng.randint(100, 1000)))
    for _ in range(40):
        cov = rng.randint(13580, 13594)
        n1 = rng.randint(80, 3000)
        triples.append((n1, cov - n1, rng.randint(80, 3000)))
    out = []
    for n1, n2, t in triples:
        lo, hi, tm = terms(n1, n2, t)
        den = sum(tm)
        dbits = den.bit_length()
        tail = 0
        for i in range(hi, lo, -1):                                    # tail = #{X > k}, k = i - 1
            tail += tm[i - lo]
            rough = (dbits - tail.bit_length()) * 0.30103             # within 0.31 of -log10(tail / den)
            if rough < 94.5:
                break
            if rough > 102.5:
                continue
            z = neglog10(tail, den)
            if Decimal(96) < z < Decimal(101):
                k, cov = i - 1, n1 + n2
                out.append(((k + 1, cov, t, n1, min(MAX_ROWS, t + 5), min(MAX_ROWS, n1 + 7)), "sat"))
    return out


def _lnc(n, m):
    return math.lgamma(n + 1) - math.lgamma(m + 1) - math.lgamma(n - m + 1)


def _median_tuples(rng):
    """counts at which the k-means rule's two candidates P(X <= s) and P(X >= s) nearly tie: the s nearest the median of a
    wide distribution.  Floating point only proposes them here; the exact P and Q decide what the tests count."""
    out = []
    for cov, wanted in ((2049, 36), (13594, 26), (30000, 12)):
        have = 0
        while have < wanted:
            n1, t = rng.randint(cov // 4, 3 * cov // 4), rng.randint(cov // 4, 3 * cov // 4)
            n2 = cov - n1
            mean = t * n1 / cov
            sd = math.sqrt(t * (n1 / cov) * (n2 / cov) * (cov - t) / (cov - 1))
            a, b = max(0, t - n2, int(mean - 9 * sd)), min(n1, t, int(mean + 9 * sd) + 1)
            base = _lnc(cov, t)
            p = [math.exp(_lnc(n1, i) + _lnc(n2, t - i) - base) for i in range(a, b + 1)]
            best = None
            below = 0.0
            for j, pj in enumerate(p):
                P, Q = below + pj, 1.0 - below                         # P(X <= s), P(X >= s), s = a + j
                rel = abs(P - Q) / max(P, Q)
                if best is None or rel < best[0]:
                    best = (rel, a + j)
                below += pj
            if 2e-4 < best[0] < 8e-3:
                out.append(((best[1], cov, t, n1, t, n1), "median"))
                have += 1
    return out


@lru_cache(maxsize=1)
def grid():
    """[Rec]: a few thousand tuples, fixed seed, each inside what the probes accept"""
    rng = random.Random(SEED)
    tuples = _main_tuples(rng) + _corner_tuples(rng) + _sat_tuples(rng) + _median_tuples(rng)
    seen = set()
    uniq = []
    for c, tag in tuples:
        assert counts_ok(c), c
        if c[:4] not in seen:
            seen.add(c[:4])
            uniq.append((c, tag))
    return tuple(annotate(uniq))


def counts_ok(c):
    """what the callers can produce, as the probes' host side checks it"""
    s, cov, g1, g2, z1, z2 = c
    return (0 <= s <= min(g1, g2) and max(g1, g2) <= cov <= MAX_ROWS and s >= g1 + g2 - cov
            and g1 <= z1 <= MAX_ROWS and g2 <= z2 <= MAX_ROWS)


def near_threshold(z_raw, half_width=Decimal("0.5")):
    return z_raw is not None and any(abs(z_raw - Decimal(x)) < half_width for x in ("97.9", "98", "99"))


# ---- what a set of probe outputs must satisfy (tests/test_gpu_tail.py with the device's, tests/test_tail_checker.py with a
# ---- Python copy of the header's logic, sound and deliberately broken) ----
# Every tuple goes through the mc and gr probes once per floor, tuple-major: row i * NF + f.  Z is the exact capped tail.
# The issue's list is {0, Z - 1e-3, Z + 2e-6, Z + 1, 97.95, 200}; Z - 5e-7 and Z itself are added because the early-out's
# margin exists for them: a floor that IS a value computed elsewhere (the running maximum, the 29th of the list) must not
# drop an equal value whose first-term bound rounds a hair below it.
FLOORS = ("0", "Z-1e-3", "Z-5e-7", "Z", "Z+2e-6", "Z+1", "97.95", "200")
NF = len(FLOORS)
F_ZERO, F_PLUS1 = 0, 5
MC_Q, MC_TAIL0, MC_TAIL, MC_SIG = 0, 1, 2, 3
GR_TAIL, GR_SIG = 0, 1
KM_P, KM_Q, KM_SIG = 0, 1, 2


def live(r):
    """the stage formulas reach the tail at all (else they answer 0)"""
    return r.counts[0] >= 1 and r.counts[2] > 0 and r.counts[3] > 0


def zq_float(r):
    return float(capped(r.zq_raw)) if live(r) else 0.0


def floors_of(r):
    z = zq_float(r)
    return [0.0, z - 1e-3, z - 5e-7, z, z + 2e-6, z + 1.0, 97.95, 200.0]


def probe_inputs(recs):
    """(counts [n * NF][6], floors [n * NF]) for the mc and gr probes; the km probe takes [r.counts for r in recs]"""
    counts, floors = [], []
    for r in recs:
        for f in floors_of(r):
            counts.append(r.counts)
            floors.append(f)
    return counts, floors


def z_of_prob(p):
    """a probability as the stages use it: -log10, capped at 99"""
    if p != p or p < 0.0:
        return math.nan
    if p == 0.0:
        return 99.0
    return min(99.0, -math.log10(p))


def err(got, exact):
    """|got - exact| for a float and a Decimal (or float); NaN is infinitely wrong"""
    got = float(got)
    if got != got:
        return math.inf
    return abs(float(Decimal(got) - Decimal(exact)))


class Worst:
    """the largest error / bound(cov, amp, 1) seen per output, and where"""

    def __init__(self):
        self.w = {}

    def see(self, name, e, unit, r):
        ratio = e / unit
        if name not in self.w or ratio > self.w[name][0]:
            self.w[name] = (ratio, e, r.counts)

    def lines(self):
        return ["%-12s worst |error| / bound(cov, amp, 1) = %.3f  (|error| %.3e at %s)" % (k, v[0], v[1], v[2]) for k, v in sorted(self.w.items())]

    def max(self):
        return max(v[0] for v in self.w.values())


def _near(z_raw, x, b):
    return z_raw is not None and abs(float(z_raw - Decimal(x))) < b


def check_values(recs, mc, gr, km, C):
    """assertion 1: every tail and every unsaturated significance within bound(cov, amp, C) of the exact value; floor 0"""
    worst = Worst()
    for i, r in enumerate(recs):
        s, cov, g1, g2, z1, z2 = r.counts
        j = i * NF + F_ZERO
        bq, uq = bound(cov, r.amp_q, C), bound(cov, r.amp_q, 1.0)
        if not live(r):
            assert mc[j][MC_TAIL0] == 0 and mc[j][MC_SIG] == 0 and gr[j][GR_TAIL] == 0 and gr[j][GR_SIG] == 0, r.counts
            if s < 1:
                assert mc[j][MC_Q] == 0 and km[i][KM_Q] == 0, r.counts             # k = 2^32 - 1: answered before the sum
        else:
            zq = capped(r.zq_raw)
            for name, got in (("mc Q", z_of_prob(mc[j][MC_Q])), ("mc tail", mc[j][MC_TAIL0]), ("gr tail", gr[j][GR_TAIL]), ("km Q", z_of_prob(km[i][KM_Q]))):
                e = err(got, zq)
                worst.see(name, e, uq, r)
                assert e <= bq, (name, r.counts, float(got), float(zq), e, bq)
            if not (r.zq_raw is None or r.zq_raw > 98 or _near(r.zq_raw, 98, bq)):
                for name, got in (("mc sig", mc[j][MC_SIG]), ("gr sig", gr[j][GR_SIG])):
                    e = err(got, zq)
                    worst.see(name, e, uq, r)
                    assert e <= bq, (name, r.counts, float(got), float(zq), e, bq)
        zp = capped(r.zp_raw)
        bp, up = bound(cov, r.amp_p, C), bound(cov, r.amp_p, 1.0)
        e = err(z_of_prob(km[i][KM_P]), zp)
        worst.see("km P", e, up, r)
        assert e <= bp, ("km P", r.counts, km[i][KM_P], float(zp), e, bp)
        if g1 == 0 or g2 == 0:
            assert km[i][KM_SIG] == 0, r.counts
            continue
        use_p = km_choice(s, r.pnum, r.qnum)
        want, b, u = (zp, bp, up) if use_p else (capped(r.zq_raw), bq, uq)
        e = err(km[i][KM_SIG], want)
        if e > b and s >= 1:                                           # a tie the bound cannot resolve: either candidate
            other, bo = (capped(r.zq_raw), bq) if use_p else (zp, bp)
            if abs(float(zp - capped(r.zq_raw))) <= bp + bq and err(km[i][KM_SIG], other) <= bo:
                continue
        worst.see("km sig", e, u, r)
        assert e <= b, ("km sig", r.counts, km[i][KM_SIG], float(want), e, b)
    return worst


def check_branches(recs, mc, gr, C):
    """assertion 3: Z > 99 and Z > 98 go the way the exact Z goes, a saturated value is the stage's formula to 1e-12; tuples
    whose exact Z lies within the bound of a threshold are left out, at most 1 % of the saturation tuples"""
    nsat = sum(r.tag == "sat" for r in recs)
    left_out = saturated = capped99 = 0
    for i, r in enumerate(recs):
        if not live(r):
            continue
        s, cov, g1, g2, z1, z2 = r.counts
        j = i * NF + F_ZERO
        b = bound(cov, r.amp_q, C)
        if _near(r.zq_raw, 98, b) or _near(r.zq_raw, 99, b):
            left_out += r.tag == "sat"
            continue
        over99 = r.zq_raw is None or r.zq_raw > 99
        over98 = r.zq_raw is None or r.zq_raw > 98
        assert (mc[j][MC_TAIL0] == 99.0) == over99 and (gr[j][GR_TAIL] == 99.0) == over99, (r.counts, mc[j][MC_TAIL0], gr[j][GR_TAIL], r.zq_raw)
        capped99 += over99
        m, m_sat = mc_significance(r.zq_raw, s, g1, g2, z1, z2)
        g, g_sat = gr_significance(r.zq_raw, s, g1, g2, z1, z2)
        assert m_sat == g_sat == over98
        if over98:
            saturated += 1
            assert abs(mc[j][MC_SIG] - m) <= 1e-12, (r.counts, mc[j][MC_SIG], m)
            assert abs(gr[j][GR_SIG] - g) <= 1e-12, (r.counts, gr[j][GR_SIG], g)
        else:
            assert mc[j][MC_SIG] <= 98.0 and gr[j][GR_SIG] <= 98.0, (r.counts, mc[j][MC_SIG], gr[j][GR_SIG])
    assert left_out <= 0.01 * nsat, (left_out, nsat)
    assert saturated >= 100 and capped99 >= 50, (saturated, capped99)
    return {"saturation tuples": nsat, "left out": left_out, "saturated": saturated, "capped at 99": capped99}


def check_floors(recs, mc, gr, C):
    """assertion 4: the early-out never hides a value that matters"""
    fired = kept_high = 0
    for i, r in enumerate(recs):
        if not live(r):
            continue
        s, cov, g1, g2, z1, z2 = r.counts
        b = bound(cov, r.amp_q, C)
        zq = capped(r.zq_raw)
        zf = float(zq)
        m = mc_significance(r.zq_raw, s, g1, g2, z1, z2)[0]
        g = gr_significance(r.zq_raw, s, g1, g2, z1, z2)[0]
        unresolved = _near(r.zq_raw, 98, b)                            # (the significance's own branch, assertion 3)
        high = r.zb_raw is None or float(r.zb_raw) >= 97.9 + b        # the first term does not bound what the callers put there
        kept_high += high
        for f, floor in enumerate(floors_of(r)):
            j = i * NF + f
            outs = [("mc tail", mc[j][MC_TAIL], zq), ("gr tail", gr[j][GR_TAIL], zq)]
            if not unresolved:
                outs += [("mc sig", mc[j][MC_SIG], m), ("gr sig", gr[j][GR_SIG], g)]
            for name, got, want in outs:
                where = (name, FLOORS[f], floor, r.counts, float(got), zf)
                if zf <= b:                                            # the value itself is 0 within the bound: nothing to hide
                    assert err(got, want) <= b, where
                elif got == 0:
                    assert zq < Decimal(floor), where                  # 0 only if exact Z < floor
                    assert not high, where
                else:
                    assert err(got, want) <= b, where                  # (non-zero whenever exact Z >= floor: 0 fails above)
            if f == F_PLUS1 and zf < 97.9 and zf > b:
                fired += mc[j][MC_TAIL] == 0 and gr[j][GR_TAIL] == 0 and mc[j][MC_SIG] == 0 and gr[j][GR_SIG] == 0
    assert fired >= 100 and kept_high >= 100, (fired, kept_high)
    return {"early-out fired at floor Z + 1": fired, "tuples whose first term is at 97.9 or beyond (never dropped)": kept_high}


def check_compiles(recs, mc, gr, km, C):
    """assertion 5: the three compiles of the header agree within the bound"""
    worst = {"mc tail - gr tail": (0.0, None), "mc Q - km Q": (0.0, None)}
    for i, r in enumerate(recs):
        if not live(r):
            continue
        j = i * NF + F_ZERO
        b = bound(r.counts[1], r.amp_q, C)
        for name, d in (("mc tail - gr tail", abs(mc[j][MC_TAIL0] - gr[j][GR_TAIL])), ("mc Q - km Q", abs(z_of_prob(mc[j][MC_Q]) - z_of_prob(km[i][KM_Q])))):
            assert d <= b, (name, r.counts, d, b)
            if d > worst[name][0]:
                worst[name] = (d, r.counts)
    return worst


def km_near_ties(recs, C):
    """indices of the tuples whose exact P(X <= s) and P(X >= s) lie within 1 % of each other but further apart than the bound"""
    out = []
    for i, r in enumerate(recs):
        if not live(r) or r.pnum == 0 or r.qnum == 0 or r.pnum == r.qnum:
            continue
        if abs(r.pnum - r.qnum) * 100 > max(r.pnum, r.qnum):
            continue
        if abs(float(r.zp_raw - r.zq_raw)) > 4.0 * (bound(r.counts[1], r.amp_p, C) + bound(r.counts[1], r.amp_q, C)):
            out.append(i)
    return out


def check_km_rule(recs, km, C):
    """assertion 6: the P / Q choice and the schnitt == 0 path"""
    ties = km_near_ties(recs, C)
    assert len(ties) >= 50, len(ties)
    took_p = 0
    for i in ties:
        r = recs[i]
        use_p = km_choice(r.counts[0], r.pnum, r.qnum)
        took_p += use_p
        want, other = (r.zp_raw, r.zq_raw) if use_p else (r.zq_raw, r.zp_raw)
        assert err(km[i][KM_SIG], want) < err(km[i][KM_SIG], other), (r.counts, km[i][KM_SIG], float(want), float(other))
    assert 10 <= took_p <= len(ties) - 10, (took_p, len(ties))          # both ways round
    zero = 0
    for i, r in enumerate(recs):
        if r.counts[0] == 0 and r.counts[2] > 0 and r.counts[3] > 0:
            zero += 1
            assert km[i][KM_Q] == 0.0, r.counts
            assert err(km[i][KM_SIG], capped(r.zp_raw)) <= bound(r.counts[1], r.amp_p, C), (r.counts, km[i][KM_SIG], r.zp_raw)
    assert zero >= 50, zero
    return {"near ties": len(ties), "of them P": took_p, "schnitt == 0": zero}
