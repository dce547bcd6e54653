"""The exact checker of the hypergeometric tail (tests/tail_checker.py) without a GPU: against brute-force rationals, the host
restatement oracle/mc_oracle.c against it over the grid of tests/test_gpu_tail.py -- which is where C_HOST, the constant of
the error model, is measured --, the grid's own claims, and the GPU test's assertions run on a Python copy of the logic of
repeatresolver_amd/csrc/hyper_tail.h: they pass on the copy and fail on it with either of two deliberate breaks."""
import ctypes
import ctypes.util
import math
import os
import subprocess
from decimal import Decimal
from fractions import Fraction

import numpy as np
import pytest

import tail_checker as tc
from conftest import ROOT


@pytest.fixture(scope="module")
def mco():
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "port"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "libmcoracle.so"))
    for n in ("mco_hyper_Q", "mco_hyper_P"):
        getattr(lib, n).restype = ctypes.c_double
        getattr(lib, n).argtypes = [ctypes.c_uint] * 4
    lib.mco_significance.restype = ctypes.c_double
    lib.mco_significance.argtypes = [ctypes.c_int] * 6
    return lib


def test_checker_against_brute_force_fractions():
    """every (k, n1, n2, t) with n1 + n2 <= 12: the tails, the support, the branch, the logarithm"""
    n = 0
    for n1 in range(0, 13):
        for n2 in range(0, 13 - n1):
            for t in range(0, n1 + n2 + 1):
                den = math.comb(n1 + n2, t)
                pmf = {i: Fraction(math.comb(n1, i) * math.comb(n2, t - i), den) for i in range(0, t + 1) if t - i <= n2 and i <= n1}
                assert sum(pmf.values()) == 1
                lo, hi, tm = tc.terms(n1, n2, t)
                assert (lo, hi) == (min(pmf), max(pmf)) and [Fraction(c, den) for c in tm] == [pmf[i] for i in range(lo, hi + 1)]
                for k in range(-1, n1 + n2 + 2):
                    P = sum((p for i, p in pmf.items() if i <= k), Fraction(0))
                    assert Fraction(*tc.exact_P(k, n1, n2, t)) == P and Fraction(*tc.exact_Q(k, n1, n2, t)) == 1 - P
                    if n1 + n2 > 0 and k >= 0:
                        assert tc.branch(k, n1, n2, t) == (k < Fraction(t * n1, n1 + n2))
                    z = tc.neglog10(*tc.exact_Q(k, n1, n2, t))
                    if P == 1:
                        assert z is None
                    else:
                        assert abs(float(z) + math.log10(float(1 - P))) < 1e-13
                    n += 1
    assert n > 5000
    # the logarithm beyond what a double holds, the cap, the stage formulas' thresholds
    assert abs(tc.neglog10(3, 3 * 10 ** 400) - 400) < Decimal("1e-55")
    assert tc.capped(None) == 99 and tc.capped(Decimal("99.5")) == 99 and tc.capped(Decimal("98.5")) == Decimal("98.5")
    assert tc.mc_significance(Decimal("98.0000001"), 3, 5, 6, 8, 9) == (98.0 + 6.0 / (6.0 + 5 + 6), True)
    assert tc.mc_significance(Decimal("98"), 3, 5, 6, 8, 9) == (Decimal("98"), False)
    assert tc.gr_significance(None, 3, 5, 6, 8, 9) == (97.90 + 6.0 / 17.0, True)
    assert tc.mc_significance(None, 0, 5, 6, 8, 9)[0] == 0 and tc.gr_significance(None, 3, 0, 6, 8, 9)[0] == 0
    assert tc.km_choice(0, 5, 1) and tc.km_choice(2, 1, 5) and not tc.km_choice(2, 5, 5)


def test_grid_has_what_it_claims():
    """so that tests/test_gpu_tail.py cannot be vacuous: by the exact checker alone"""
    g = tc.grid()
    assert 2000 <= len(g) <= 6000 and all(tc.counts_ok(r.counts) for r in g)
    assert {r.counts[1] for r in g if r.tag == "main"} == set(tc.COVS)
    assert sum(r.lower_q is True for r in g) >= 200 and sum(r.lower_q is False for r in g) >= 200       # each branch
    assert sum(r.amp_q > 100 for r in g) >= 100
    assert sum(tc.near_threshold(r.zq_raw) for r in g if tc.live(r)) >= 100
    assert sum(r.counts[0] == max(0, r.counts[2] + r.counts[3] - r.counts[1]) for r in g) >= 50         # the support's ends
    assert sum(r.counts[0] == min(r.counts[2], r.counts[3]) for r in g) >= 50
    sat = [r for r in g if r.tag == "sat"]
    assert len(sat) >= 300 and all(96 < r.zq_raw < 101 for r in sat)
    assert {c for c in (2049, 13594) if any(abs(r.counts[1] - c) < 15 for r in sat)} == {2049, 13594}
    assert any(r.counts[1] <= 1800 for r in sat)
    assert len(tc.km_near_ties(g, tc.C_DEV)) >= 50
    # the amplified corner of the coverage the benchmark has, and of the deepest the stages accept
    amp = {r.counts[:4]: r.amp_q for r in g}
    assert 3.3e3 < amp[(1, 13594, 2, 2)] < 3.5e3 and 7.4e3 < amp[(1, 30000, 2, 2)] < 7.6e3


def _host_errors(mco, g):
    worst = tc.Worst()
    for r in g:
        s, cov, g1, g2, z1, z2 = r.counts
        n1, n2, t = g2, cov - g2, g1
        if s >= 1:
            e = tc.err(tc.z_of_prob(mco.mco_hyper_Q(s - 1, n1, n2, t)), tc.capped(r.zq_raw))
            worst.see("lower Q" if r.lower_q else "upper Q", e, tc.bound(cov, r.amp_q, 1.0), r)
        e = tc.err(tc.z_of_prob(mco.mco_hyper_P(s, n1, n2, t)), tc.capped(r.zp_raw))
        worst.see("P", e, tc.bound(cov, r.amp_p, 1.0), r)
    return worst


def test_host_oracle_against_exact_measures_c_host(mco):
    """mco_hyper_Q / mco_hyper_P against exact tails over the whole grid, in -log10 units: the largest error in units of
    bound(cov, amp, 1) is C_HOST.  The recorded constant must cover what is measured and not be more than twice it."""
    g = tc.grid()
    worst = _host_errors(mco, g)
    print()
    print("\n".join(worst.lines()))
    for cov in (13594, 30000):
        r = next(r for r in g if r.counts[:4] == (1, cov, 2, 2))
        e = tc.err(tc.z_of_prob(mco.mco_hyper_Q(0, 2, cov - 2, 2)), r.zq_raw)
        print("complement branch at cov %d, groups 2 and 2 sharing one row: Z %.4f, amp %.0f, |oracle - exact| %.2e" % (cov, float(r.zq_raw), r.amp_q, e))
    print("C_host measured %.3f, recorded %.3f" % (worst.max(), tc.C_HOST))
    assert tc.C_HOST / 2 < worst.max() <= tc.C_HOST
    # the whole function, both saturation branches included, within the same bound
    for r in g:
        if not tc.live(r):
            continue
        s, cov, g1, g2, z1, z2 = r.counts
        b = tc.bound(cov, r.amp_q, tc.C_HOST)
        if tc._near(r.zq_raw, 98, b):
            continue
        want, sat = tc.mc_significance(r.zq_raw, s, g1, g2, z1, z2)
        got = mco.mco_significance(s, cov, g1, g2, z1, z2)
        assert abs(got - want) <= 1e-12 if sat else tc.err(got, want) <= b, (r.counts, got, want)


# ---- a Python copy of the logic of hyper_tail.h and of the three callers, to try the GPU test's assertions on ----
M32 = 0xFFFFFFFF
EPS = 2.2204460492503131e-16


class HeaderCopy:
    """doubles and the host's lgamma as on the device; `plus_one` and `margin` are the two places the breaks touch"""

    def __init__(self, maxcov, plus_one=1.0, margin=-1e-6):
        libm = ctypes.CDLL(ctypes.util.find_library("m"))
        libm.lgamma.restype = ctypes.c_double
        libm.lgamma.argtypes = [ctypes.c_double]
        self.lnf = [libm.lgamma(n + 1.0) for n in range(maxcov + 2)]
        self.plus_one, self.margin = plus_one, margin

    def lnchoose(self, n, m):
        return 0.0 if m == n or m == 0 else self.lnf[n] - self.lnf[m] - self.lnf[n - m]

    def ln_pdf(self, k, n1, n2, t):
        return self.lnchoose(n1, k) + self.lnchoose(n2, t - k) - self.lnchoose(n1 + n2, t)

    def pdf(self, k, n1, n2, t):
        t = min(t, n1 + n2)
        if k > n1 or k > t or (t > n2 and k + n2 < t):
            return 0.0
        return math.exp(self.ln_pdf(k, n1, n2, t))

    def hyper_sum(self, k, n1, n2, t):
        lower = k < (float(t) * n1) / (float(n1) + n2)
        if lower:
            i = k
            s = P = self.pdf(i, n1, n2, t)
            while i > 0:
                s *= (i / (n1 - i + 1.0)) * (((n2 + i - t) & M32) / (t - i + 1.0))
                P += s
                if P > 0 and s / P < EPS:
                    break
                i -= 1
            return P, True
        i = k + 1
        s = Q = self.pdf(i, n1, n2, t)
        while i < t:
            s *= ((n1 - i) / (i + self.plus_one)) * ((t - i) / (n2 + i + 1.0 - t))
            Q += s
            if Q > 0 and s / Q < EPS:
                break
            i += 1
        return Q, False

    def Q(self, k, n1, n2, t):
        if k >= n1 or k >= t:
            return 0.0
        s, lower = self.hyper_sum(k, n1, n2, t)
        return 1.0 - s if lower else s

    def P(self, k, n1, n2, t):
        if k >= n1 or k >= t:
            return 1.0
        s, lower = self.hyper_sum(k, n1, n2, t)
        return s if lower else 1.0 - s

    @staticmethod
    def _z(p):
        if p < 0:
            return math.nan
        z = math.inf if p == 0 else -1.0 * math.log10(p)
        return 99.0 if z > 99 else z

    def tail_z(self, s, cov, g1, g2, floor, q):
        if g1 == 0 or g2 == 0 or s < 1:
            return 0.0
        if s <= g2 and s <= g1 and g1 - s <= cov - g2:
            zb = self.ln_pdf(s, g2, cov - g2, g1) * -0.43429448190325182
            if zb < floor + self.margin and zb < 97.9:
                return 0.0
        return self._z(q)

    def outputs(self, recs):
        mc, gr, km = [], [], []
        for r in recs:
            s, cov, g1, g2, z1, z2 = r.counts
            n1, n2, t = g2, cov - g2, g1
            q = self.Q((s - 1) & M32, n1, n2, t)
            p = self.P(s, n1, n2, t)
            z0 = self.tail_z(s, cov, g1, g2, 0.0, q)
            for floor in tc.floors_of(r):
                z = self.tail_z(s, cov, g1, g2, floor, q)
                mc.append((q, z0, z, 98.0 + 2.0 * s / (2.0 * s + (z1 - s) + (z2 - s)) if z > 98.0 else z))
                gr.append((z, 97.90 + float(2 * s) / float(z1 + z2) if z > 98.0 else z))
            km.append((p, q, 0.0 if g1 == 0 or g2 == 0 else self._z(p if (p < q or s == 0) else q)))
        return mc, gr, km


def _run_all(recs, mc, gr, km):
    worst = tc.check_values(recs, mc, gr, km, tc.C_DEV)
    tc.check_branches(recs, mc, gr, tc.C_DEV)
    tc.check_floors(recs, mc, gr, tc.C_DEV)
    tc.check_compiles(recs, mc, gr, km, tc.C_DEV)
    tc.check_km_rule(recs, km, tc.C_DEV)
    return worst


def test_assertions_hold_on_a_copy_of_the_header_and_catch_two_breaks():
    g = tc.grid()
    worst = _run_all(g, *HeaderCopy(tc.MAX_ROWS).outputs(g))
    print()
    print("\n".join(worst.lines()))
    # break 1: the + 1.0 of one recurrence ratio dropped (the upward sum's (n1 - i) / (i + 1.0)): the values
    mc, gr, km = HeaderCopy(tc.MAX_ROWS, plus_one=0.0).outputs(g)
    with pytest.raises(AssertionError):
        tc.check_values(g, mc, gr, km, tc.C_DEV)
    # break 2: the early-out's margin + 1e-6 instead of - 1e-6: a value equal to the floor is dropped
    mc, gr, km = HeaderCopy(tc.MAX_ROWS, margin=1e-6).outputs(g)
    tc.check_values(g, mc, gr, km, tc.C_DEV)                           # (floor 0 does not see it)
    with pytest.raises(AssertionError):
        tc.check_floors(g, mc, gr, tc.C_DEV)


def test_probes_refuse_counts_no_caller_can_produce():
    """The lnf lookups have no bounds check of their own, so the probes' host side turns away, before it touches a device
    (this test runs where there is none), every tuple outside what the three kernels can hand over."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "repeatresolver_amd", "csrc"), "all"], check=True, stdout=subprocess.DEVNULL)
    from repeatresolver_amd.realigner import PwrError
    from repeatresolver_amd.tail_probe import tail_probe
    good = (2, 100, 5, 7, 9, 11)
    assert tc.counts_ok(good)
    bad = [(-1, 100, 5, 7, 9, 11), (6, 100, 5, 7, 9, 11), (6, 100, 7, 5, 9, 11),      # schnitt outside 0 .. min(gr1, gr2)
           (2, 6, 5, 7, 9, 11), (2, 6, 7, 5, 9, 11), (2, tc.MAX_ROWS + 1, 5, 7, 9, 11), (0, -1, 0, 0, 0, 0),   # cov
           (1, 10, 5, 7, 9, 11),                                                        # schnitt < gr1 + gr2 - cov
           (2, 100, 5, 7, 4, 11), (2, 100, 5, 7, 9, 6), (2, 100, 5, 7, tc.MAX_ROWS + 1, 11), (2, 100, 5, 7, 9, tc.MAX_ROWS + 1),   # sizes
           (2, 100, -5, 7, 9, 11), (2, 2 ** 31 - 1, 5, 7, 9, 11), (-2 ** 31, 100, 5, 7, 9, 11)]
    for stage in ("mc", "gr", "km"):
        for c in bad:
            assert not tc.counts_ok(c)
            for counts in ([c], [good, c], [c, good]):                 # one bad tuple anywhere refuses the call
                with pytest.raises(PwrError) as e:
                    tail_probe(stage, counts, [0.0] * len(counts))
                assert e.value.code == -1, (stage, c)                  # PWR_ERR_ARG
        with pytest.raises(PwrError) as e:
            tail_probe(stage, np.zeros((0, 6), dtype=np.int32))
        assert e.value.code == -1                                      # no tuple at all
