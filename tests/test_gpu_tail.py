"""-m gpu: the device's hypergeometric tail (repeatresolver_amd/csrc/hyper_tail.h) evaluated count by count through the test
hooks of its three translation units -- pmc_device.hip (hipcc's default contraction), pgr_device.hip and pgr_km_device.hip
(-ffp-contract=off) -- against EXACT tails (tests/tail_checker.py: Python integers, 60 digits), one launch per probe.  The
stage tests see the tail only behind a maximum per variation, behind the order of the best 29, or against the host
restatement oracle/mc_oracle.c, which implements the same scheme and reads the same lgamma table.

The bound is tail_checker.bound(cov, amp, C_DEV) with C_DEV = 2 * C_HOST, C_HOST measured on the host restatement in
tests/test_tail_checker.py; the 1e-9 against the oracle and the 1e-12 of the saturated formulas are the suite's own.  The
assertions themselves live in tail_checker (check_*): tests/test_tail_checker.py shows on a Python copy of the header that
they hold, and that they fail when the copy is broken.  Every test prints what it measured."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import tail_checker as tc
from conftest import ROOT
from test_mc_oracle import literal_maxcorrs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mco():
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "port"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "libmcoracle.so"))
    for n in ("mco_hyper_Q", "mco_hyper_P"):
        getattr(lib, n).restype = ctypes.c_double
        getattr(lib, n).argtypes = [ctypes.c_uint] * 4
    lib.mco_significance.restype = ctypes.c_double
    lib.mco_significance.argtypes = [ctypes.c_int] * 6
    lib.mco_maxcorrs.restype = ctypes.c_int
    lib.mco_maxcorrs.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    return lib


@pytest.fixture(scope="module")
def probed():
    """the grid through the three probes: one launch each"""
    from repeatresolver_amd.tail_probe import tail_probe
    recs = tc.grid()
    counts, floors = tc.probe_inputs(recs)
    mc = tail_probe("mc", counts, floors)
    gr = tail_probe("gr", counts, floors)
    km = tail_probe("km", [r.counts for r in recs])
    assert mc.shape == (len(recs) * tc.NF, 4) and gr.shape == (len(recs) * tc.NF, 2) and km.shape == (len(recs), 3)
    return recs, mc, gr, km


def test_values_against_exact(probed):
    """1: every tail and every unsaturated significance within bound(cov, amp, C_DEV) of the exact value"""
    recs, mc, gr, km = probed
    worst = tc.check_values(recs, mc, gr, km, tc.C_DEV)
    print()
    print("\n".join(worst.lines()))
    print("C_dev = %.1f allows; the device needs %.3f (C_host %.1f)" % (tc.C_DEV, worst.max(), tc.C_HOST))


def test_device_against_oracle(probed, mco):
    """2: the same outputs against the host restatement at the suite's 1e-9, over the whole grid, the amplified corner included"""
    recs, mc, gr, km = probed
    worst = {}

    def see(name, got, exp, r):
        d = abs(got - exp) if not (math.isnan(got) and math.isnan(exp)) else 0.0
        if name not in worst or d > worst[name][0]:
            worst[name] = (d, r.counts, r.amp_q)

    for i, r in enumerate(recs):
        s, cov, g1, g2, z1, z2 = r.counts
        j = i * tc.NF + tc.F_ZERO
        n1, n2, t = g2, cov - g2, g1
        q = mco.mco_hyper_Q((s - 1) & 0xFFFFFFFF, n1, n2, t)
        p = mco.mco_hyper_P(s, n1, n2, t)
        zq = tc.z_of_prob(q)
        tail = zq if tc.live(r) else 0.0
        see("mc Q", tc.z_of_prob(mc[j][tc.MC_Q]), zq, r)
        see("km Q", tc.z_of_prob(km[i][tc.KM_Q]), zq, r)
        see("km P", tc.z_of_prob(km[i][tc.KM_P]), tc.z_of_prob(p), r)
        see("mc tail", mc[j][tc.MC_TAIL0], tail, r)
        see("gr tail", gr[j][tc.GR_TAIL], tail, r)
        see("mc sig", mc[j][tc.MC_SIG], mco.mco_significance(s, cov, g1, g2, z1, z2), r)
        see("gr sig", gr[j][tc.GR_SIG], 97.90 + float(2 * s) / float(z1 + z2) if tail > 98.0 else tail, r)      # RR:472-488 on the oracle's tail
        km_exp = 0.0 if g1 == 0 or g2 == 0 else tc.z_of_prob(p if (p < q or s == 0) else q)                      # RR:490-504
        see("km sig", km[i][tc.KM_SIG], km_exp, r)
    print()
    for name, (d, c, amp) in sorted(worst.items()):
        print("%-8s largest |device - oracle| = %.3e at %s (amp %.3g)" % (name, d, c, amp))
    for name, (d, c, amp) in worst.items():
        assert d <= 1e-9, (name, d, c, amp)


def test_branches_are_the_exact_ones(probed):
    """3: Z > 99 and Z > 98 go the way the exact Z goes; a saturated value is the stage's formula to 1e-12"""
    recs, mc, gr, _ = probed
    print()
    print(tc.check_branches(recs, mc, gr, tc.C_DEV))


def test_early_out_never_hides_a_value_that_matters(probed):
    """4: per tuple and floor the result is 0 or right, 0 only below the floor; the early-out does fire, and never at 97.9 or beyond"""
    recs, mc, gr, _ = probed
    print()
    print(tc.check_floors(recs, mc, gr, tc.C_DEV))


def test_three_compiles_agree(probed):
    """5: pmc_device.hip (contracted) against pgr_device.hip on the tail, pgr_km_device.hip's Q against pmc_device.hip's"""
    recs, mc, gr, km = probed
    worst = tc.check_compiles(recs, mc, gr, km, tc.C_DEV)
    print()
    for name, (d, c) in sorted(worst.items()):
        print("%-18s largest difference %.3e at %s" % (name, d, c))


def test_kmeans_rule(probed):
    """6: the P / Q choice where the two nearly tie, and the schnitt == 0 path"""
    recs, _, _, km = probed
    print()
    print(tc.check_km_rule(recs, km, tc.C_DEV))


# ---- through the real kernel: planted pairs whose every output is a maximum over at most two known tuples ----
def planted_msa(T, sizes, shared, W=100):
    """all rows `a`; column 10 carries `c` in sizes[0] rows, column 70 `g` in sizes[1] rows, `shared` rows carry both"""
    rows = [bytearray(b"a" * W) for _ in range(T)]
    first = list(range(5, 5 + sizes[0]))
    second = list(range(5 + sizes[0] - shared, 5 + sizes[0] - shared + sizes[1]))
    for r in first:
        rows[r][10] = ord("c")
    for r in second:
        rows[r][70] = ord("g")
    return [bytes(r) for r in rows]


@pytest.mark.parametrize("planting", [((2, 2), 1), ((3, 5), 2)])
@pytest.mark.parametrize("T", [600, 2049, 13594])
def test_planted_pairs_through_max_correlations(T, planting, mco):
    from repeatresolver_amd.max_correlation import max_correlations
    sizes, shared = planting
    rows = planted_msa(T, sizes, shared)
    bounds, seen = {}, []

    def exact_sig(s, cov, g1, g2, z1, z2):
        r = tc.annotate([((s, cov, g1, g2, z1, z2), "planted")])[0]
        v = float(tc.mc_significance(r.zq_raw, s, g1, g2, z1, z2)[0])
        bounds[v] = max(bounds.get(v, 0.0), tc.bound(cov, r.amp_q, tc.C_DEV))
        seen.append((s, cov, g1, g2, v, r.amp_q))
        return v

    exp = literal_maxcorrs(rows, 4, exact_sig)
    assert sorted(set(x[:4] for x in seen)) == sorted({(shared, T, sizes[0], sizes[1]), (sizes[0] - shared, T, sizes[0], T - sizes[1]),
                                                        (sizes[1] - shared, T, T - sizes[0], sizes[1]),
                                                        (T - sizes[0] - sizes[1] + shared, T, T - sizes[0], T - sizes[1])})
    assert (exp > 0).sum() == 4
    got = max_correlations(rows, 4)
    assert np.array_equal(got == 0, exp == 0)
    print()
    for v in np.flatnonzero(exp):
        b = bounds[exp[v]]
        print("T %5d, variation (%d, %s): exact %.12f, device %.12f, |difference| %.2e, bound %.2e" % (T, v // 5, "acgt-"[v % 5], exp[v], got[v], abs(got[v] - exp[v]), b))
        assert abs(got[v] - exp[v]) <= b
    if shared == 1:                                                    # k = 0 below the midpoint: the amplified corner is among them
        assert max(x[5] for x in seen) > T / 5                         # (1 - Q) / Q is about T / (2 * 2); sharing 2 rows sums directly
    ora = np.zeros(len(rows[0]) * 5)
    assert mco.mco_maxcorrs(T, len(rows[0]), b"".join(rows), 4, ora.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
    assert np.array_equal(got == 0, ora == 0)
    print("largest |device - oracle| %.3e" % float(np.abs(got - ora).max()))
    assert np.allclose(got, ora, rtol=0, atol=1e-9), float(np.abs(got - ora).max())
