"""-m gpu: the HIP group refinement (include/pgr.h) against the literal restatement tests/gr_checker.py, for the arrays
the reference never writes.  What it does write -- the label files that depend on these arrays -- is compared with the
REFERENCE (the unmodified program text linked with a stand-in for its three GSL functions, not a GSL-linked binary) in
tests/test_gpu_rr_reference.py: see the checker's header.

Compared exactly: kept, sizes, cutoffs, c_groups, c_coverage, cliques and the zero pattern of maxcorrs; drop_off to 1e-12.
The device's tail differs from the host's by rounding (the MaxCorrelation tests allow 1e-9 for it), so a variation whose
ranked candidates hold two unequal values closer than 1e-8 among the first 30 or at the greedy threshold is *undecided*:
there every device member must have a checker value within 1e-8 of the checker's 29th or better, and its groups are not
compared.  Undecided variations are at most 2 % of the significant ones in every input and none in the cut-at-30, index-0
and saturation cases; tests/test_group_refinement.py confirms that on the CPU for the same inputs.

The inputs (generated here, shared with tests/test_group_refinement.py through CASES / checked()): k planted copy groups,
each with d distinguishing columns, about 10 % substitution and indel noise, rows blank at their ends."""
import functools
import os

import numpy as np
import pytest

import gr_checker as gc
from conftest import GOLDEN, golden_output, split_rows

ACGT = np.frombuffer(b"acgt", dtype=np.uint8)


def planted_msa(seed, kept, W, d, noise=0.10, extra=6, minority_a_at_0=False, spread=False, inner_blanks=True):
    """`kept` rows that span the whole width plus `extra` rows blank at one or both ends; copy group g (rows r % len(d) == g)
    carries its own base in d[g] distinguishing columns (at least 20 columns apart from most of the others, so that
    MaxCorrelation pairs them).  Returns the rows in a shuffled order."""
    rng = np.random.default_rng(seed)
    k = len(d)
    cons = rng.integers(0, 4, W)
    cols = rng.permutation(np.arange(1, W - 1))[:sum(d)] if not spread else np.linspace(2, W - 3, sum(d)).astype(int)
    owner = np.repeat(np.arange(k), d)
    if spread:
        owner = rng.permutation(owner)                               # every group's columns lie all over the width
    rows = []
    for r in range(kept + extra):
        g = r % k
        seq = cons.copy()
        mine = cols[owner == g]
        seq[mine] = (cons[mine] + 1 + g % 3) % 4
        sub = rng.random(W) < noise / 2
        seq[sub] = rng.integers(0, 4, int(sub.sum()))
        row = ACGT[seq].copy()
        row[rng.random(W) < noise / 2] = ord("-")
        if inner_blanks and r % 7 == 3:
            p = int(rng.integers(5, W - 15))
            row[p:p + 6] = ord(" ")                                  # a hole inside a kept row: not covered there
        if r % 11 == 5:
            row = np.frombuffer(bytes(row).upper().replace(b"-", b"_"), dtype=np.uint8).copy()
        if minority_a_at_0:
            row[0] = ord("a") if g == 0 else ord("g")               # 'a' at column 0 is group 0's mark: variation 0
        if r >= kept:                                                # left out: blank at the left, the right or both ends
            e = r - kept
            if e % 3 != 1:
                row[:int(rng.integers(1, W // 6))] = ord(" ")
            if e % 3 != 0:
                row[W - int(rng.integers(1, W // 6)):] = ord(" ")
        elif row[0] == ord(" ") or row[-1] == ord(" "):
            raise AssertionError("generator: a kept row lost an end")
        rows.append(row.tobytes())
    order = rng.permutation(len(rows))
    return [rows[i] for i in order]


def saturated_msa(T=960, W=140):
    """no noise: group A (every second row) marks 34 columns, group B (every third) marks 8, their overlap C (every sixth)
    marks 5 -- the tails underflow 1e-99, identical groups give F = 1 (ordered by index), nested ones smaller equal F"""
    rows = []
    colsA = list(range(3, 3 + 34 * 3, 3))
    colsB = list(range(4, 4 + 8 * 12, 12))
    colsC = list(range(5, 5 + 5 * 21, 21))
    for r in range(T):
        row = bytearray(b"a" * W)
        if r % 2 == 0:
            for c in colsA:
                row[c] = ord("c")
        if r % 3 == 0:
            for c in colsB:
                row[c] = ord("g")
        if r % 6 == 0:
            for c in colsC:
                row[c] = ord("t")
        rows.append(bytes(row))
    return rows


def windowed_msa(seed=21, T=110, W=420):
    """a wider MSA whose rows start and end at scattered columns: a window inside it keeps those that cover both its ends"""
    rng = np.random.default_rng(seed)
    base = planted_msa(seed, T, W, [9, 9, 9], extra=0, inner_blanks=False)
    rows = []
    for r, line in enumerate(base):
        row = bytearray(line)
        a, b = int(rng.integers(0, W // 2)), int(W - rng.integers(0, W // 2))
        if r % 3 == 0:
            a, b = 0, W
        row[:a] = b" " * a
        row[b:] = b" " * (W - b)
        rows.append(bytes(row))
    return rows


# name -> (rows, von, bis, cov)
CASES = {
    "kept63": lambda: (planted_msa(63, 63, 300, [8, 8, 8]), None, None, 12),
    "kept64": lambda: (planted_msa(64, 64, 300, [8, 8, 8]), None, None, 12),
    "kept65": lambda: (planted_msa(65, 65, 300, [8, 8, 8]), None, None, 12),
    "kept129": lambda: (planted_msa(129, 129, 300, [8, 8, 8]), None, None, 12),
    "cut30": lambda: (planted_msa(45, 90, 400, [40, 0], extra=4, inner_blanks=False), None, None, 12),
    "tiles": lambda: (planted_msa(5, 96, 900, [40, 12], extra=4, spread=True), None, None, 12),
    "index0": lambda: (planted_msa(10, 90, 300, [12, 8, 8], minority_a_at_0=True), None, None, 12),
    "saturation": lambda: (saturated_msa(), None, None, 30),
    "drop": lambda: (planted_msa(17, 100, 300, [3, 10, 10]), None, None, 12),
    "window": lambda: (windowed_msa(), 120, 330, 12),
    "bis_beyond": lambda: (windowed_msa(seed=22, T=80, W=300), 60, 5000, 12),
}
# inputs that other test files send through checked() / compare() and that no test here is parametrised over: the layout of
# CASES, filled by the file that owns them (tests/deep_cases.py)
EXTRA_CASES = {}


def fixture_cases():
    out = []
    for name in sorted(os.listdir(GOLDEN)):
        if name.endswith(".out.gz"):
            rows = split_rows(golden_output(name[:-7]))
            if len(rows) >= 12 and len(rows[0]) >= 60:
                out.append(name[:-7])
    return out


@functools.lru_cache(maxsize=None)
def checked(name):
    """(rows, maxcorrs of the whole MSA, von, bis, cov, the checker's result): computed once per process"""
    if name in CASES or name in EXTRA_CASES:
        rows, von, bis, cov = (CASES.get(name) or EXTRA_CASES[name])()
    else:
        rows = split_rows(golden_output(name))                       # their middle 600 columns, the window in the middle of those
        c0 = max(0, len(rows[0]) // 2 - 300)
        rows = [r[c0:c0 + 600] for r in rows]
        von, bis, cov = len(rows[0]) // 4, len(rows[0]) * 3 // 4, max(4, len(rows) // 3)
    mc = gc.mco_maxcorrs(rows, cov)
    exp = gc.Window(rows, mc, von, bis, cov).refine()
    return rows, mc, von, bis, cov, exp


def compare(name, max_undecided=0.02):
    from repeatresolver_amd.group_refinement import refine_groups
    rows, mc, von, bis, cov, exp = checked(name)
    got = refine_groups(rows, mc, von, bis, cov)
    assert np.array_equal(got.kept, exp["kept"]) and got.width == exp["width"] and got.cutoff == exp["cutoff"]
    assert np.array_equal(got.significant, exp["significant"])
    S = len(exp["significant"])
    und = [s for s in range(S) if gc.undecided(exp["candidates"][s], exp["cutoff"])]
    print(f"{name}: {got.kept.sum()} kept rows x {got.width} columns, {S} significant, {len(und)} undecided, "
          f"{int((exp['sizes'] > 5).sum())} refined, max |drop_off difference| "
          f"{float(np.abs(got.drop_off - exp['drop_off']).max()) if S else 0.0:.3g}")
    assert len(und) <= max_undecided * S
    ok = np.ones(S, dtype=bool)
    ok[und] = False
    for s in und:
        z = dict((i, v) for v, i in exp["candidates"][s])
        r = gc.ranked(exp["candidates"][s], exp["cutoff"])
        floor = r[gc.MAXCLIQUE - 2][0] if len(r) >= gc.MAXCLIQUE - 1 else exp["cutoff"]
        members = [int(i) for i in got.cliques[s, 1:] if i >= 0]
        assert got.cliques[s, 0] == exp["significant"][s] and len(set(members)) == len(members)
        assert all(i in z and z[i] >= floor - 1e-8 for i in members)
    assert np.array_equal(got.cliques[ok], exp["cliques"][ok])
    assert np.array_equal(got.sizes[ok], exp["sizes"][ok])
    assert np.array_equal(got.cutoffs[ok], exp["cutoffs"][ok])
    assert np.array_equal(got.c_groups[ok], exp["c_groups"][ok])
    assert np.array_equal(got.c_coverage[ok], exp["c_coverage"][ok])
    assert np.allclose(got.drop_off[ok], exp["drop_off"][ok], rtol=0, atol=1e-12)
    keep = np.ones(len(exp["maxcorrs"]), dtype=bool)
    keep[exp["significant"][und]] = False
    assert np.array_equal(got.maxcorrs[keep] == 0, exp["maxcorrs"][keep] == 0)
    assert np.array_equal(got.maxcorrs[keep & (exp["maxcorrs"] != 0)], exp["maxcorrs"][keep & (exp["maxcorrs"] != 0)])
    return got, exp


@pytest.mark.gpu
@pytest.mark.parametrize("kept", [63, 64, 65, 129])
def test_word_boundaries(kept):
    """sc = kept / 64 + 1 steps at 64 and 128 (64 kept rows: an empty second word); bit 63 and bit 0 of the last word"""
    got, exp = compare(f"kept{kept}")
    assert got.kept.sum() == kept and got.c_groups.shape[1] == kept // 64 + 1
    assert (exp["sizes"] > 5).sum() >= 10
    last = np.bitwise_or.reduce(exp["c_groups"][:, (kept - 1) // 64])
    assert (int(last) >> ((kept - 1) % 64)) & 1                   # the last kept row is in some refined group


@pytest.mark.gpu
def test_clique_cut_at_30():
    """one copy group with 40 distinguishing columns: more than 29 partners pass greedy and the cut decides"""
    got, exp = compare("cut30", max_undecided=0.0)
    over = [s for s in range(len(exp["significant"])) if len(gc.ranked(exp["candidates"][s], exp["cutoff"])) > 29]
    assert len(over) >= 30
    assert all(got.cliques[s, gc.MAXCLIQUE - 1] >= 0 and got.cliques[s, gc.MAXCLIQUE] == -1 for s in over)


@pytest.mark.gpu
def test_several_tiles_and_chunks():
    """4 500 variations = 18 chunks of 256 for the kernel's threads, walked in 9 slices of 2; the partners of the big copy
    group's cliques lie every 17 columns over the whole width, so every clique is merged from all slices' lists"""
    got, exp = compare("tiles")
    assert got.width == 900 and len(exp["significant"]) > 32       # more than two tiles of 16
    wide = [s for s in range(len(exp["significant"])) if exp["sizes"][s] == 30 and
            len({int(i) // 512 for i in exp["cliques"][s, :30]}) >= 7]
    assert len(wide) >= 10


@pytest.mark.gpu
def test_index_0_rule():
    """variation 0 (column 0, 'a') is a copy group's mark: as a clique member it ends Sizes (RR:1650) while C_Groups still
    counts it (RR:982-989), and as a significant variation itself it has Sizes = 0 and is dropped"""
    got, exp = compare("index0", max_undecided=0.0)
    assert exp["significant"][0] == 0 and exp["sizes"][0] == 0 and got.maxcorrs[0] == 0
    inside = [s for s in range(1, len(exp["significant"])) if 0 in list(exp["cliques"][s, 1:])]
    assert len(inside) >= 5
    for s in inside:
        assert exp["sizes"][s] == list(exp["cliques"][s]).index(0) < (exp["cliques"][s] >= 0).sum()
    assert any(exp["sizes"][s] > 5 for s in inside)                # ... and some of them are refined with it


@pytest.mark.gpu
def test_saturation():
    """960 rows, perfectly linked columns: the 97.90 + F branch; equal F across different partners, ordered by index"""
    got, exp = compare("saturation", max_undecided=0.0)
    nsat = 0
    for s in range(len(exp["significant"])):
        r = gc.ranked(exp["candidates"][s], exp["cutoff"])
        top = [z for z, _ in r[:29]]
        nsat += sum(z > 97.9 for z in top)
        if len(r) > 29 and r[28][0] == r[29][0]:
            assert r[28][1] < r[29][1] and got.cliques[s, 29] == r[28][1]      # a tie at the cut: the lower index stays
    assert nsat > 500
    assert any(len(r) > 29 and r[28][0] == r[29][0] for r in (gc.ranked(c, exp["cutoff"]) for c in exp["candidates"]))


@pytest.mark.gpu
def test_drop():
    """a copy group with three distinguishing columns: its variations have fewer than 5 partners -> MaxCorrs zeroed, no groups"""
    got, exp = compare("drop")
    small = exp["sizes"] <= 5
    assert small.sum() >= 3 and (~small).sum() >= 10
    assert (got.maxcorrs[exp["significant"][small]] == 0).all() and (got.maxcorrs[exp["significant"][~small]] > 0).all()
    assert not got.c_groups[small].any() and not got.c_coverage[small].any()
    assert (got.cutoffs[small] == 0).all() and (got.drop_off[small] == 1000.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["window", "bis_beyond"])
def test_window(name):
    """von / bis inside a wider MSA (bis beyond the width is clipped): rows not covering an end are left out"""
    got, exp = compare(name)
    rows = checked(name)[0]
    assert 12 < got.kept.sum() < len(rows) and got.width < len(rows[0])
    assert (exp["sizes"] > 5).sum() >= 5


@pytest.mark.gpu
def test_realigner_fixtures():
    """what the pipeline feeds it: MSAreal files (the golden outputs of the realigner fixtures)"""
    names = fixture_cases()
    assert len(names) >= 5
    for name in names:
        compare(name)


@pytest.mark.gpu
def test_pipeline_chain_and_errors():
    """pipeline.refined_groups chains the GPU MaxCorrelation into the refinement; -t above 100 is an argument error"""
    from repeatresolver_amd.group_refinement import last_timing, refine_groups
    from repeatresolver_amd.pipeline import refined_groups
    from repeatresolver_amd.realigner import PwrError
    rows, mc, von, bis, cov, exp = checked("kept65")
    got = refined_groups(rows, von, bis, cov)
    assert np.array_equal(got.significant, exp["significant"]) and np.array_equal(got.sizes, exp["sizes"])
    t = last_timing()
    assert t["pairs"] == len(exp["significant"]) * (got.width * 5 - 1) and t["cliques_ms"] > 0
    with pytest.raises(PwrError) as e:
        refine_groups(rows, mc, cov=cov, cutoff=100.5)
    assert e.value.code == -1
    none = refine_groups(rows, mc, cov=cov, cutoff=99.5)           # nothing is significant: empty arrays, no device work
    assert none.significant.shape == (0,) and none.cliques.shape == (0, 31) and none.c_groups.shape == (0, 2)
