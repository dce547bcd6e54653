"""-m gpu: the band's last strip in k_fill_v3 (the RIGHT role sets the fill's pace; the rows of every role fill the
scan's wait states with their own work, and RIGHT and LEFT rows take their band guard from masks made a row ahead).  What matters is
how often a wave is RIGHT and in how many ways: rows of 2 500 to 3 600 columns on 256-column strips, so every wave takes the
band's last strip over several times per realignment, runs ahead of its first row with work (every cell masked), and meets
band ends at every column of a strip; bands that tear, bands clamped at both edges of the MSA, a band narrower than a strip
(LEFT and RIGHT at once: run-time flags), short segments from both starts with their check, and one deep stack at the edge of
the 32-bit admission rule.  The checker is the CPU oracle, realignment by realignment (test_gpu_parity._row_by_row: Way, entry
column, placement, MSA); every case also runs in k_fill_v2 (fill=3), which keeps the true score and every clamp."""
import ctypes

import numpy as np
import pytest

from test_gpu_fill_handover import _long_rows
from test_gpu_parity import _row_by_row

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"acgt", dtype=np.uint8)

FILLS = pytest.mark.parametrize("fill", [4, 3], ids=["v3", "v2"])


@FILLS
@pytest.mark.parametrize("bw", [400, 600])
def test_every_wave_is_the_last_strip_several_times(bw, fill, oracle):
    """26 rows of 3 100 columns: twelve strips, a band of two to four of them"""
    _row_by_row(_long_rows(26, 3100, 81), bw, 1, oracle, fill=fill)


@FILLS
@pytest.mark.parametrize("bw", [400, 600])
def test_blank_runs_that_tear_the_band(bw, fill, oracle):
    """Blank runs of 150 to 900 columns: the longer ones tear the band (no strip is taken over across a tear, the first row
    behind one starts from the extension Ptot), the shorter ones move its end over a strip or more in one row"""
    _row_by_row(_long_rows(28, 3600, 82, holes=(150, 900)), bw, 1, oracle, fill=fill)


@FILLS
def test_band_ends_clamped_at_both_edges(fill, oracle):
    """every row starts at column 0 or ends at the last column: the band's end stops at the MSA's right edge, inside a strip"""
    rows = _long_rows(24, 2500, 83)
    W = len(rows[0])
    edge = [r for r in rows if r[0] != ord("-") or r[W - 1] != ord("-")]
    rng = np.random.default_rng(84)
    out = []
    for r in (edge * 6)[:24]:                                # (copies of the four edge rows, each with blanks of its own)
        a = np.frombuffer(r, dtype=np.uint8).copy()
        a[1:-1][rng.random(W - 2) < 0.03] = ord("-")
        out.append(bytes(a))
    _row_by_row(out, 400, 1, oracle, fill=fill)


@FILLS
def test_band_narrower_than_a_strip(fill, oracle):
    """Bandwidth 100: a strip is LEFT and RIGHT at once (run-time flags, which keep their clamp) and changes hands every few rows"""
    _row_by_row(_long_rows(24, 2500, 85, holes=(30, 160)), 100, 1, oracle, fill=fill)


@FILLS
@pytest.mark.parametrize("src_start", [0, 1])
def test_short_segments_from_both_starts(src_start, fill, oracle):
    """64 own rows per segment behind a warm-up of 1.5 bandwidths (most rows of the launch are warm-up rows, the form without the
    record), from the free start and from the one-cell start with its unreachable prefix; k_seg_check passes or the job is repeated"""
    _row_by_row(_long_rows(24, 2600, 86, holes=(120, 500)), 300, 1, oracle, fill=fill, seg_rows=64, seg_max=64, warm_pct=150, src_start=src_start)


@FILLS
def test_narrow_and_deep_near_the_admission_bound(fill, oracle):
    """A stack of 36 columns, a base at both ends of every row, as in test_gpu_fill_tilted -- at the smallest depth at which the
    gather's bound U + (2B + 4096) * maxS comes within a factor two of 2^30: the end columns' tally is T - 1 (the row under
    realignment is taken out), so (T - 1) * (2B + 4096) >= 2^29 gives T = 88 071 for B = 1000.  The oracle's own tallies show
    it; and the job still runs in the 32-bit kernels (rows_wide 0)."""
    from repeatresolver_amd.realigner import PWReAligner
    B, W = 1000, 36
    T = -(-(1 << 29) // (2 * B + 4096)) + 1
    assert T == 88071 and (T - 2) * (2 * B + 4096) < 1 << 29 <= (T - 1) * (2 * B + 4096)
    rng = np.random.default_rng(87)
    tmpl = rng.integers(0, 4, W)
    m = np.tile(tmpl, (T, 1))
    sub = rng.random((T, W)) < 0.05
    m[sub] = rng.integers(0, 4, int(sub.sum()))
    txt = ACGT[m]
    txt[rng.random((T, W)) < 0.06] = ord("-")
    txt[:, 0] = ACGT[tmpl[0]]
    txt[:, -1] = ACGT[tmpl[-1]]
    rows = [bytes(r) for r in txt]
    g = PWReAligner(rows, bandwidth=B, window=4, fill=fill)
    g.trim_ends()
    lib = oracle.lib
    h = oracle.create(rows, B)
    lib.pwo_trim(h)
    assert g.total_score() == lib.pwo_total_score(h)
    for k in range(4):                                       # one at a time: Way, entry, placement
        assert lib.pwo_realign_row(h, k) == 0
        if k == 0:
            # the oracle's tallies as the fill saw them: the largest one is the end columns' T - 1, and with it alone the bound is past 2^29
            n = lib.pwo_dbg_W_at_fill(h) * 6
            mx = int(np.ctypeslib.as_array(ctypes.cast(lib.pwo_dbg_tallies(h), ctypes.POINTER(ctypes.c_uint64)), shape=(n,)).max())
            print("largest tally %d of %d rows: (2B + 4096) * maxS = %d = %.3f * 2^30" % (mx, T, (2 * B + 4096) * mx, (2 * B + 4096) * mx / (1 << 30)))
            assert mx == T - 1 and (1 << 29) <= (2 * B + 4096) * mx < (1 << 30)
        g.realign_row(k)
        L = lib.pwo_dbg_L(h)
        d = g.debug_last_job()
        assert d["L"] == L and d["entry"] == lib.pwo_dbg_entry(h), k
        assert d["newcol"] == [(lib.pwo_dbg_newcol(h)[x] << 1) | lib.pwo_dbg_newins(h)[x] for x in range(L)], k
    g.realign_rows(4, 20)                                    # a batch of 20
    for k in range(4, 24):
        assert lib.pwo_realign_row(h, k) == 0
    lib.pwo_compact(h)
    assert g.dims() == (T, lib.pwo_width(h))
    for k in list(range(24)) + [T - 1]:
        assert g.debug_row_columns(k) == oracle.row_columns(h, k), k
    assert g.total_score() == lib.pwo_total_score(h)
    st = g.stats()
    assert st["rows_wide"] == 0 and st["rows_committed"] == 24    # none of them went to k_fill64
    lib.pwo_destroy(h)
    g.close()
