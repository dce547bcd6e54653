"""-m gpu: every compiled width of the three kernels that keep a bit-vector DP row in a lane's registers, each against its
checker, integers only and exact.

  k_ia_bits<WPL, STORE, BOTH>   pia_device.hip   WPL 1 .. 35, pass 1 / pass 2, forward / both strands    oracle/libiaoracle.so
  k_rc_rows<WPL, BOTH>          prc_device.hip   WPL 1 .. 20, forward / both strands, G 1 .. 64          rc_checker.py
  k_fl_tiles<NW>                pfl_device.hip   NW 1 .. 16                                              fl_checker.py

The host picks the instance from a length; tests/width_cases.py restates the three rules and holds, for every width, an
input at its first and at its last length, and test_width_cases.py checks without a GPU that those tables reach every
instance and that their inputs are not trivial.  One case per width, so that a failure names it.  The checkers' results are
made once per input and shared between the forward and the both-strands test."""
import pytest

import rc_checker as ck
import strand_checker as sc
import width_cases as wc

pytestmark = pytest.mark.gpu


# ---- InitialAligner --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle():
    return sc.ia_oracle()


_ia_expected = {}


def ia_expected(oracle, wpl, L2):
    """(placements, distance) of the case's six reads and of their six reverse complements, in that order"""
    if (wpl, L2) not in _ia_expected:
        templ, reads = wc.ia_case(wpl, L2)
        _ia_expected[wpl, L2] = [oracle(r, templ) for r in reads + [sc.rc(r) for r in reads]]
    return _ia_expected[wpl, L2]


def _align(templ, reads, expected, mem_budget=None):
    from repeatresolver_amd.initial_aligner import InitialAligner
    g = InitialAligner(templ)
    try:
        if mem_budget is not None:
            g.set_option("mem_budget", mem_budget)
        got, dist = g.align(reads)
        st = g.stats()
    finally:
        g.close()
    assert st["cells"] == sum(len(r) for r in reads) * len(templ)
    for j, (r, (place, d)) in enumerate(zip(reads, expected)):
        assert int(dist[j]) == d, (len(templ), mem_budget, wc.IA_READ_NAMES[j])
        assert list(got[j]) == place, (len(templ), mem_budget, wc.IA_READ_NAMES[j])


@pytest.mark.parametrize("wpl", range(1, wc.IA_MAXWPL + 1))
def test_initial_aligner_every_width(wpl, oracle):
    """k_ia_bits<wpl, *, false> at the width's first and last template length: every placement, every distance, the cells.
    All reads in one batch of pass 2 (every band but the first starts at a non-zero multiple of 16 uint2 of the buffer), and
    at the last length also one read per batch (every band starts at 0, through the IA_NBUF buffers and streams)."""
    first, last = wc.ia_lengths(wpl)
    for L2 in (first, last):
        templ, reads = wc.ia_case(wpl, L2)
        _align(templ, reads, ia_expected(oracle, wpl, L2)[:6])
    _align(templ, reads, ia_expected(oracle, wpl, last)[:6], mem_budget=1)


@pytest.mark.parametrize("wpl", range(1, wc.IA_MAXWPL + 1))
def test_initial_aligner_every_width_both_strands(wpl, oracle):
    """k_ia_bits<wpl, *, true>: the six reads and their reverse complements in one call: strand, both distances, the
    placements, the turned reads.  Reads 0 to 3 come back forward and their reverse complements reverse, so pass 2 has run
    reverse jobs at this width."""
    from repeatresolver_amd.initial_aligner import InitialAligner
    from repeatresolver_amd.strands import reverse_complement
    for L2 in wc.ia_lengths(wpl):
        templ, reads = wc.ia_case(wpl, L2)
        reads = reads + [sc.rc(r) for r in reads]
        exp = ia_expected(oracle, wpl, L2)
        g = InitialAligner(templ)
        try:
            place, dist, strand, other = g.align_strands(reads)
            turned = g.turned(reads, strand)
            st = g.stats()
        finally:
            g.close()
        assert st["cells"] == 2 * sum(len(r) for r in reads) * L2
        for j, r in enumerate(reads):
            (pf, df), (pr, dr) = exp[j], exp[(j + 6) % 12]              # the read as given, and turned
            s, p, d, o = (1, pr, dr, df) if dr < df else (0, pf, df, dr)
            assert (int(strand[j]), int(dist[j]), int(other[j])) == (s, d, o), (L2, j)
            assert list(place[j]) == p, (L2, j)
            assert turned[j] == (reverse_complement(r) if s else r)
        assert [int(s) for s in strand[0:4]] == [0] * 4 and [int(s) for s in strand[6:10]] == [1] * 4, L2


# ---- ReadCutter ------------------------------------------------------------------------------------------------------

RC_CUTOFFS = (0.30, 0.05)
_rc_rows = {}


def rc_rows(ln, j):
    """the last DP rows of piece 0 and piece 2 in read j of wc.rc_reads_both(ln) (j >= n: the reverse complement of j - n)"""
    if (ln, j) not in _rc_rows:
        templ, overlap, _ = wc.rc_case(ln)
        read = wc.rc_reads_both(ln)[j]
        _rc_rows[ln, j] = [ck.last_row_myers(ck.piece(templ, wc.RC_PARTS, overlap, q), read) for q in (0, wc.RC_PARTS - 1)]
    return _rc_rows[ln, j]


def rc_positions(ln, j, e):
    return [ck.scan(row, ln, int(ln * e)) for row in rc_rows(ln, j)]


def rc_cuts(ln, j):
    """rc_checker.cut on the rows made already"""
    templ, _overlap, _ = wc.rc_case(ln)
    occ = rc_positions(ln, j, 0.30)
    return ck.select_cuts(wc.RC_PARTS, ln, len(templ), len(wc.rc_reads_both(ln)[j]), occ[0], occ[-1])


def ints(arrays):
    return [list(map(int, a)) for a in arrays]


@pytest.mark.parametrize("ln", wc.RC_LENGTHS)
def test_read_cutter_every_width(ln):
    """k_rc_rows<WPL, false> for pieces of ln rows: the positions at both cutoffs and the cut points of every read"""
    from repeatresolver_amd import read_cutter
    templ, overlap, reads = wc.rc_case(ln)
    g = read_cutter.ReadCutter(templ.encode())
    try:
        got = {e: g.occurrences([r.encode() for r in reads], wc.RC_PARTS, overlap, e) for e in RC_CUTOFFS}
        cuts = g.cut([r.encode() for r in reads], wc.RC_PARTS, overlap, 0.30)
        st = g.stats()
    finally:
        g.close()
    assert st["cells"] == 3 * sum(len(r) for r in reads) * ln * 2      # three calls, two pieces
    for j, r in enumerate(reads):
        for e in RC_CUTOFFS:
            assert ints(got[e][j]) == rc_positions(ln, j, e), (ln, wc.rc_geometry(ln), e, j, len(r))
        assert list(map(int, cuts[j])) == rc_cuts(ln, j), (ln, wc.rc_geometry(ln), j, len(r))


@pytest.mark.parametrize("ln", wc.RC_LENGTHS)
def test_read_cutter_every_width_both_strands(ln):
    """k_rc_rows<WPL, true>: every read and every read's reverse complement in one call; each orientation of each against
    the checker on that sequence, the forward half equal to the forward-only call, the merged cut points"""
    from repeatresolver_amd import read_cutter
    templ, overlap, _ = wc.rc_case(ln)
    reads = wc.rc_reads_both(ln)
    n = len(reads)
    raw = [r.encode() for r in reads]
    g = read_cutter.ReadCutter(templ.encode())
    try:
        got = {e: g.occurrences(raw, wc.RC_PARTS, overlap, e, both_strands=True) for e in RC_CUTOFFS}
        fwd = g.occurrences(raw, wc.RC_PARTS, overlap, 0.30)
        cuts, nfwd, nrev = g.cut(raw, wc.RC_PARTS, overlap, 0.30, both_strands=True)
    finally:
        g.close()
    for j, r in enumerate(reads):
        turned = (j + n // 2) % n                                       # where rc(r) stands in the list
        assert reads[turned] == sc.rc(r)
        for s, k in enumerate((j, turned)):
            for e in RC_CUTOFFS:
                assert ints(got[e][j][s]) == rc_positions(ln, k, e), (ln, wc.rc_geometry(ln), e, j, s, len(r))
        assert ints(fwd[j]) == ints(got[0.30][j][0]), (ln, j)
        f, b = rc_cuts(ln, j), rc_cuts(ln, turned)
        assert (list(map(int, cuts[j])), int(nfwd[j]), int(nrev[j])) == (sc.merge_cuts(len(r), f, b), len(f), len(b)), (ln, j)
    if ln >= 20:                                                        # both kinds of job have found something
        assert got[0.30][0][0][0].size and got[0.30][n // 2][1][0].size


def test_read_cutter_refuses_a_piece_above_the_widest_kernel():
    """a piece of PRC_MAX_PART + 1 rows: PWR_ERR_RANGE from every entry, and the context answers the next call"""
    import random
    from repeatresolver_amd import read_cutter
    from repeatresolver_amd.realigner import PwrError
    rng = random.Random(40961)
    templ = "".join(rng.choice("acgt") for _ in range(wc.RC_MAX_PART + 1))
    read = "".join(rng.choice("acgt") for _ in range(60)) + templ[:999] + "".join(rng.choice("acgt") for _ in range(45))
    g = read_cutter.ReadCutter(templ.encode())
    try:
        for both in (False, True):
            for entry in (g.occurrences, g.cut):
                with pytest.raises(PwrError) as e:
                    entry([read.encode()], 1, 0, 0.30, both_strands=both)
                assert e.value.code == -5
        with pytest.raises(PwrError) as e:
            g.occurrences([read.encode()], 3, wc.RC_MAX_PART + 1 - len(templ) // 3, 0.30)      # the overlap makes it too long
        assert e.value.code == -5
        got = g.occurrences([read.encode()], 41, 0, 0.30)[0]            # 41 pieces of 999 rows
        both = g.occurrences([read.encode()], 41, 0, 0.30, both_strands=True)[0]
    finally:
        g.close()
    exp = ck.occurrences(templ, read, 41, 0, 0.30)
    assert exp[0] == [60 + 998] and ints(got) == exp
    assert [ints(s) for s in both] == sc.occurrences_strands(templ, read, 41, 0, 0.30)


# ---- flank distances -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reach", [wc.FL_REACH, 511, 33])
def test_flank_distances_every_word_count(reach):
    """k_fl_tiles<1 .. 16> in one call at reach 512: patterns at the first and the last row count of every word count, texts
    without slack, with the whole slack, one base beyond it and far beyond, all four modes; then the same flanks at two
    shorter reaches, which cut the long ones to an m that is not their length (511: every width again; 33: widths 1 and 2)"""
    from repeatresolver_amd.flanks import FlankClusterer
    from test_gpu_flanks import compare
    pieces, piece, mode = wc.fl_case()
    with FlankClusterer() as g:
        dist = compare(g, pieces, piece, mode, reach, wc.FL_MIN_LEN)
    assert (dist >= 0).all()
