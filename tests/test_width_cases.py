"""What tests/width_cases.py claims, checked without a GPU: through the restated host rules its tables reach every compiled
instance of k_ia_bits, k_rc_rows and k_fl_tiles, each at its first and its last length, and -- by the checkers alone -- the
inputs are not trivial: the exact reads are exact, the noisy ones are found but not exact, the unrelated ones are not found,
and a read is nearer on its own strand than turned.  test_gpu_kernel_widths.py runs the same tables on the GPU."""
import pytest

import rc_checker as ck
import strand_checker as sc
import width_cases as wc


# ---- coverage ---------------------------------------------------------------------------------------------------------

def test_initial_aligner_cases_reach_every_width_at_both_ends():
    assert {wc.ia_wpl(L2) for _w, L2 in wc.IA_CASES} == set(range(1, 36))
    assert all(wc.ia_wpl(L2) == w for w, L2 in wc.IA_CASES) and len(set(wc.IA_CASES)) == 70
    for w in range(1, 36):
        first, last = wc.ia_lengths(w)
        assert (w, first) in wc.IA_CASES and (w, last) in wc.IA_CASES
        assert wc.ia_wpl(last) == w and (last == 70000 or wc.ia_wpl(last + 1) == w + 1)        # the last length of the width
        assert w == 1 or wc.ia_wpl(first - 1) == w - 1                                           # and the first
    assert wc.ia_lengths(1) == (300, 2048) and wc.ia_lengths(35) == (69633, 70000)
    assert {w for w in range(1, 36) if w > 2 and w % 2 == 0} <= {w for w, _ in wc.IA_CASES}    # pass 2's 16-byte stores, no odd word


def test_read_cutter_cases_reach_every_width_and_group_size():
    geo = {ln: wc.rc_geometry(ln) for ln in wc.RC_LENGTHS}
    assert {w for w, _g in geo.values()} == set(range(1, 21))
    assert {g for _w, g in geo.values()} >= {1, 2, 4, 8, 16, 32, 64}
    for w in range(1, 21):
        first, last = 2048 * (w - 1) + 1, 2048 * w
        assert geo[first][0] == w and geo[last][0] == w
        assert w == 1 or wc.rc_geometry(first - 1)[0] == w - 1
        assert last == wc.RC_MAX_PART or wc.rc_geometry(last + 1)[0] == w + 1
    assert wc.RC_MAX_PART in geo and {65, 128, 129, 256, 257} <= set(geo)
    assert [geo[ln][1] for ln in (65, 128, 129, 256, 257)] == [4, 4, 8, 8, 16]
    # where the last piece row sits (prc_device.hip:68-70): (word within its lane, bit, lane)
    def top(ln):
        w = geo[ln][0]
        wt = (ln - 1) >> 5
        return wt - wt // w * w, (ln - 1) & 31, wt // w
    for w in range(1, 21):
        assert top(2048 * w) == (w - 1, 31, 63)                         # the last length: the lane's last word, bit 31, lane 63
        assert top(2048 * (w - 1) + 1)[1] == 0                          # the first: bit 0 of the word behind the width below
    tws = {(geo[ln][0], top(ln)[0]) for ln in geo}
    assert {(w, 0) for w in (2, 4, 8, 16)} <= tws                       # that word is the lane's first where WPL divides 64 ...
    assert {(3, 2), (5, 1), (20, 16)} <= tws                            # ... and lies inside the lane elsewhere
    for ln in wc.RC_LENGTHS:
        templ, overlap, reads = wc.rc_case(ln)
        assert len(templ) // wc.RC_PARTS + overlap == ln and overlap == (40 if ln > 41 else 0)
        assert len(reads) == (10 if ln in wc.RC_SHORT_LENGTHS else 2) and len(reads[1]) == ln // 2 + 3
        if ln in wc.RC_SHORT_LENGTHS:
            assert len({len(r) for r in reads}) > 5 and all(1 <= len(r) <= 4 * ln for r in reads[2:])


def test_flank_cases_reach_every_word_count_at_both_ends():
    lengths = wc.fl_lengths()
    assert len(lengths) < 130
    assert {wc.fl_nw(n, wc.FL_REACH) for n in lengths} == set(range(1, 17))
    for nw in range(1, 17):
        first, mid, last = wc.fl_pattern_lengths(nw)
        assert (first, mid, last) == (32 * (nw - 1) + 1, 32 * nw - 1, 32 * nw)
        assert {wc.fl_nw(first, 512), wc.fl_nw(mid, 512), wc.fl_nw(last, 512)} == {nw}
        assert wc.fl_nw(first - 1, 512) == nw - 1 and (nw == 16 or wc.fl_nw(last + 1, 512) == nw + 1)
        for m in (first, mid, last):                                   # a pattern: some flank follows it in the order (a, index)
            k = lengths.index(m)
            assert any((min(n, 512), j) > (m, k) for j, n in enumerate(lengths))
        assert lengths.count(first) >= 2 and lengths.count(last) >= 2   # a text without slack
        assert {last + last // 4, last + last // 4 + 1, 2 * last + 7} <= set(lengths)
    pieces, piece, mode = wc.fl_case()
    assert [len(p) for p in pieces] == lengths and piece == list(range(len(lengths)))
    assert all({mode[k] for k, n in enumerate(lengths) if wc.fl_nw(n, 512) == nw} == {0, 1, 2, 3} for nw in range(1, 17))
    # the two shorter reaches cut long flanks to an m that is not their length
    assert {wc.fl_nw(n, 511) for n in lengths} == set(range(1, 17)) and sum(n > 511 for n in lengths) > 3
    assert {wc.fl_nw(n, 33) for n in lengths} == {1, 2} and sum(n > 33 for n in lengths) > 100


# ---- the inputs mean something ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle():
    return sc.ia_oracle()


@pytest.mark.parametrize("wpl", range(1, 36))
def test_initial_aligner_reads_are_what_they_are_called(wpl, oracle):
    for L2 in wc.ia_lengths(wpl):
        templ, reads = wc.ia_case(wpl, L2)
        assert len(templ) == L2 and len(reads) == 6
        d = [oracle(r, templ)[1] for r in reads]
        d_rc = [oracle(sc.rc(r), templ)[1] for r in reads]
        n = [len(r) for r in reads]
        assert d[0] == 0 and d[1] == 0, (wpl, L2, d)
        assert 0 < d[2] < 0.30 * n[2] and 0 < d[3] < 0.30 * n[3], (wpl, L2, d, n)
        assert d[4] > 0.30 * n[4], (wpl, L2, d, n)
        assert all(d[j] < d_rc[j] for j in range(4)), (wpl, L2, d, d_rc)
        place = oracle(reads[0], templ)[0]
        assert place == list(range(L2 - 200, L2))                       # the entry is the last column
        b = wc.ia_boundary(wpl, L2)
        place = oracle(reads[1], templ)[0]
        assert b % (32 * wpl) == 0 and place[0] < b <= place[-1] < L2  # read 1 lies on both sides of a lane boundary
        assert min(p for p in oracle(reads[3], templ)[0] if p >= 0) < 8    # read 3 starts at the template's first columns


RC_FULL_WIDTHS = (1, 2, 3, 8, 13, 20)           # the CPU suite pays for these; the GPU test checks every length anyway


@pytest.mark.parametrize("ln", [ln for ln in wc.RC_LENGTHS if wc.rc_geometry(ln)[0] in RC_FULL_WIDTHS])
def test_read_cutter_reads_are_what_they_are_called(ln):
    """Read 0 holds piece 0 at 5 % errors and piece 2 at 20 %; read 1 holds neither.  Piece 0 has one position at both
    cutoffs from 20 rows on (a piece of one row has a cutoff of 0, and nothing is ever below that).  Piece 2 has one at 0.30
    and none at 0.05 where that can be: its last 40 rows lie past the template's end and match nothing, which alone is above
    30 % of a piece of up to 133 rows, and with 18 % of the other rows in edits above 30 % of one of some 300; asserted
    from 1024 rows on."""
    templ, overlap, reads = wc.rc_case(ln)
    rows = [[ck.last_row_myers(ck.piece(templ, wc.RC_PARTS, overlap, q), r) for q in (0, wc.RC_PARTS - 1)] for r in reads[:2]]
    found = {e: [[ck.scan(row, ln, int(ln * e)) for row in rr] for rr in rows] for e in (0.30, 0.05)}
    assert found[0.30][1] == [[], []] and found[0.05][1] == [[], []]
    if ln >= 20:
        assert len(found[0.30][0][0]) == 1 and len(found[0.05][0][0]) == 1
    else:
        assert found[0.30][0] == [[], []]
    if ln >= 1024:
        assert len(found[0.30][0][1]) == 1 and found[0.05][0][1] == []
        assert found[0.30][0][0][0] < found[0.30][0][1][0]              # piece 0 ends before piece 2 does
    if ln in wc.RC_SHORT_LENGTHS:                                       # the eight further reads: not all of them are empty of hits
        hits = [len(ck.scan(ck.last_row_myers(ck.piece(templ, wc.RC_PARTS, overlap, 0), r), ln, int(ln * 0.30))) for r in reads[2:]]
        assert sum(h > 0 for h in hits) >= 2
