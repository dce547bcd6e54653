"""-m gpu: k_fill_v3 hands ONE tagged word per DP row to the next wave (M_last is P_end wherever it is read).
What matters here is strip boundaries, not scale: rows of 2 500 to 3 600 columns, so that with the default 256-column strips
every wave takes a strip over two or three times per realignment -- the run entry and the first row on a strip read the word
of row x - 1 from the ring, not from a register --, at bandwidths on both sides of a strip's width.  The checker is the CPU
oracle, realignment by realignment (test_gpu_parity._row_by_row: Way, entry column, placement, MSA); k_fill_v2, which keeps
both words and the true score, runs the same rows against the same oracle, so the two kernels give the same MSA."""
import numpy as np
import pytest

from test_gpu_parity import _row_by_row

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"acgt", dtype=np.uint8)


def _long_rows(n_rows, W, seed, holes=()):
    """Rows that span (nearly) the whole MSA of W columns: copies of one template with 4 % substitutions and 5 % single blanks.
    holes: (shortest, longest) run of blanks, one or two of them per row (every other row two).  The first two rows start at column
    0 and the last two end at column W - 1 (the band is clamped at the MSA's edges there); the others start and end within
    150 columns of them."""
    rng = np.random.default_rng(seed)
    tmpl = rng.integers(0, 4, W)
    rows = []
    for r in range(n_rows):
        s = 0 if r < 2 else int(rng.integers(0, 150))
        e = W if r >= n_rows - 2 else W - int(rng.integers(0, 150))
        seg = tmpl[s:e].copy()
        sub = rng.random(e - s) < 0.04
        seg[sub] = rng.integers(0, 4, int(sub.sum()))
        txt = ACGT[seg]
        txt[1:-1][rng.random(e - s - 2) < 0.05] = ord("-")
        if holes:
            for i in range(1 + (r % 2)):
                n = int(rng.integers(holes[0], holes[1] + 1))
                at = int(rng.integers(200, e - s - 200 - n)) if i == 0 else int(rng.integers((e - s) // 2, e - s - 100 - n))
                txt[at:at + n] = ord("-")
        row = np.full(W, ord("-"), dtype=np.uint8)
        row[s:e] = txt
        rows.append(bytes(row))
    assert rows[0][0] != ord("-") and rows[-1][-1] != ord("-")
    return rows


WIDE = dict(n_rows=24, W=3000, seed=61)                 # 12 strips of 256 columns: every wave of five has two or three


def test_every_wave_takes_strips_over_several_times(oracle):
    """Bandwidth 400 on 256-column strips: a band covers two or three strips, every role (LEFT, INTERIOR, RIGHT, mixed groups)
    occurs in every lap, and the DP's last row always falls in a strip that has a left neighbour inside the band (the band is
    wider than a strip), which is where the equality test of PW:1386 takes the neighbour's last score from the one word."""
    _row_by_row(_long_rows(**WIDE), 400, 1, oracle)


def test_k_fill_v2_agrees_on_the_same_rows(oracle):
    """the independent cross-check: two words and the true score M, against the same oracle on the same rows"""
    _row_by_row(_long_rows(**WIDE), 400, 1, oracle, fill=3)


def test_long_runs_of_blanks(oracle):
    """Blank runs of 120 to 900 columns at bandwidth 600: the shorter ones move the band past the left strips in one step (the
    score left of a strip is then INF, PW:276: yq < a_prev), the longer ones tear it (no hand-over across a tear)."""
    _row_by_row(_long_rows(28, 3600, 62, holes=(120, 900)), 600, 1, oracle)


def test_band_clamped_at_both_edges_of_the_msa(oracle):
    """every row starts at column 0 or ends at the last column (or both)"""
    rows = _long_rows(24, 2500, 63)
    W = len(rows[0])
    full = [r for r in rows if r[0] != ord("-") or r[W - 1] != ord("-")]
    rows = (full * 6)[:24]
    rng = np.random.default_rng(64)
    out = []
    for r in rows:                                       # (copies of the four edge rows, each with blanks of its own)
        a = np.frombuffer(r, dtype=np.uint8).copy()
        a[1:-1][rng.random(W - 2) < 0.03] = ord("-")
        out.append(bytes(a))
    _row_by_row(out, 300, 1, oracle)


def test_bandwidth_below_a_strips_width(oracle):
    """Bandwidth 100: the band lies inside one strip or across one boundary, so a strip is LEFT and RIGHT at once (run-time
    flags) and changes hands every few rows (the one-row loop)."""
    _row_by_row(_long_rows(24, 2500, 65, holes=(30, 160)), 100, 1, oracle)


@pytest.mark.parametrize("src_start", [0, 1])
def test_segments_of_64_rows_with_their_check(src_start, oracle):
    """64 own rows per segment after a warm-up of 1.5 bandwidths, from the free start and from the one-cell start (an unreachable
    prefix); k_seg_check compares every segment's first vector with its predecessor's last"""
    _row_by_row(_long_rows(24, 2600, 66, holes=(120, 500)), 300, 1, oracle, seg_rows=64, seg_max=64, warm_pct=150, src_start=src_start)


GEOMETRIES = [dict(waves=w, onewg=o) for w in (5, 4, 8, 3, 9) for o in (0, 1)] + [dict(waves=17), dict(waves=9, wave_cols=4)]


@pytest.mark.parametrize("geo", GEOMETRIES, ids=["-".join("%s%d" % kv for kv in g.items()) for g in GEOMETRIES])
def test_every_shipped_geometry(geo, oracle):
    """All instantiations of k_fill_v3 (strips of 64 to 576 columns), one work-group per wave and one per segment (hand-over
    through LDS), in short segments so that every wave starts on many strips"""
    _row_by_row(_long_rows(**WIDE), 400, 1, oracle, seg_rows=256, warm_pct=150, **geo)


def test_a_stalled_wave_still_flags_its_job_and_nothing_else(oracle):
    """the existing test hook (the first wave of the next launch behaves as if its neighbour never answered): one stall, the job
    repeated by k_fill_v2, the result the oracle's"""
    from repeatresolver_amd.realigner import PWReAligner
    rows = _long_rows(**WIDE)
    g = PWReAligner(rows, bandwidth=400, window=1)
    g.trim_ends()
    h = oracle.create(rows, 400)
    oracle.lib.pwo_trim(h)
    g.realign_rows(0, 3)
    g.set_option("stall_test", 1)
    g.realign_rows(3, len(rows) - 3)
    oracle.lib.pwo_realign_round(h)
    assert g.total_score() == oracle.lib.pwo_total_score(h)
    assert g.export_rows() == oracle.export(h)
    assert g.stats()["stalls"] == 1
    oracle.lib.pwo_destroy(h)
    g.close()
