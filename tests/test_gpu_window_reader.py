"""-m gpu: the device window reader pgr_msa_window (include/pgr.h; k_win_kept and k_win_bits of pgr_win_device.hip) against
the host reader pgr_read_window on the same text: every field of pgr_window bit for bit -- kept, kept_rows, sc, von, bis,
width, groups, local_coverage, coverage -- and the same return code.  Everything is an integer; nothing is approximate."""
import ctypes

import numpy as np
import pytest

from test_gpu_group_refinement import planted_msa, windowed_msa

ALPHABET = np.frombuffer(b"acgtACGT-_ acgt-NnxX*.\x00\x7f\xff", dtype=np.uint8)   # bases in both cases, both gaps, blanks, junk bytes


def as_array(rows):
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), len(rows[0])).copy()


def host_window(text, von, bis):
    """pgr_read_window on a 2-D uint8 array, by pointer: (rc, dict of every field)"""
    from repeatresolver_amd import _lib
    lib = _lib.load()
    win = _lib.PgrWindow()
    rc = lib.pgr_read_window(text.shape[0], text.shape[1], ctypes.cast(text.ctypes.data, ctypes.c_char_p), -1 if von is None else von,
                             -1 if bis is None else bis, ctypes.byref(win))
    try:
        return rc, fields(win, text.shape[0]) if rc == 0 else None
    finally:
        lib.pgr_window_free(ctypes.byref(win))


def device_window(msa, von, bis):
    from repeatresolver_amd import _lib
    lib = _lib.load()
    win = _lib.PgrWindow()
    rc = lib.pgr_msa_window(msa.handle, -1 if von is None else von, -1 if bis is None else bis, ctypes.byref(win))
    try:
        return rc, fields(win, msa.rows) if rc == 0 else None
    finally:
        lib.pgr_window_free(ctypes.byref(win))


def fields(win, rows):
    from repeatresolver_amd.group_refinement import _copy
    w, sc = win.width, win.sc
    return {"rows": win.rows, "kept_rows": win.kept_rows, "von": win.von, "bis": win.bis, "width": w, "sc": sc,
            "kept": _copy(win.kept, (rows,), np.uint8), "groups": _copy(win.groups, (w * 5, sc), np.uint64),
            "local_coverage": _copy(win.local_coverage, (w, sc), np.uint64), "coverage": _copy(win.coverage, (w,), np.int32)}


def same(msa, text, von, bis):
    rc_h, exp = host_window(text, von, bis)
    rc_d, got = device_window(msa, von, bis)
    assert rc_d == rc_h, (von, bis, rc_d, rc_h)
    if rc_h:
        return None
    for k, v in exp.items():
        assert np.array_equal(got[k], v), (von, bis, k)
    assert exp["sc"] == exp["kept_rows"] // 64 + 1
    return exp


def interleaved(kept, W, seed):
    """`kept` rows that cover both end columns, a row blank at one end (or both) in front of every one of them and two behind
    the last: the j-th kept row is not the j-th row, so compaction matters.  Inner blanks, both cases, '_' and junk bytes."""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(2 * kept + 2):
        row = ALPHABET[rng.integers(0, len(ALPHABET), W)].copy()
        if r % 2 == 1 and r < 2 * kept:
            row[0] = ord("a") if row[0] == 32 else row[0]
            row[-1] = ord("_") if row[-1] == 32 else row[-1]
        else:
            e = (r // 2) % 3
            if e != 1:
                row[:int(rng.integers(1, W // 2))] = 32
            if e != 0:
                row[W - int(rng.integers(1, W // 2)):] = 32
        rows.append(row)
    return np.array(rows, dtype=np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("kept", [0, 1, 63, 64, 65, 128, 129])
def test_word_boundaries_and_compaction(kept):
    from repeatresolver_amd.resolution import open_msa
    text = interleaved(kept, 70, seed=kept)
    with open_msa(text) as msa:
        exp = same(msa, text, None, None)
        assert exp["kept_rows"] == kept and exp["sc"] == kept // 64 + 1 and exp["rows"] == 2 * kept + 2
        assert not exp["kept"][0] and (kept == 0 or exp["kept"][1])
        if kept:
            assert exp["groups"].any() and (exp["coverage"] < kept).any()     # inner blanks and junk: not covered everywhere
            last = np.bitwise_or.reduce(exp["local_coverage"][:, (kept - 1) // 64])
            assert (int(last) >> ((kept - 1) % 64)) & 1                       # the last kept row's bit is set somewhere
        else:
            assert not exp["groups"].any() and not exp["coverage"].any()


@pytest.mark.gpu
def test_widths_and_ends_from_one_handle():
    """window widths 1, 255, 256, 257 and 300 (one, just under / exactly / just over one block of 256 columns, two blocks);
    von = 0, bis = the last column, bis beyond the width, the whole width as -1 / -1; von beyond bis after clipping and a
    negative von are the host reader's argument errors.  All from one open handle, one after the other."""
    from repeatresolver_amd.resolution import open_msa
    rng = np.random.default_rng(11)
    text = ALPHABET[rng.integers(0, len(ALPHABET), (150, 640))].copy()
    text[::2, 100:500] = np.frombuffer(b"acgt", dtype=np.uint8)[rng.integers(0, 4, (75, 400))]   # half the rows cover the middle
    W = text.shape[1]
    with open_msa(text) as msa:
        for width in (1, 255, 256, 257, 300):
            exp = same(msa, text, 120, 120 + width - 1)
            assert exp["width"] == width and exp["kept_rows"] >= 75
        for von, bis in ((0, 0), (0, 299), (0, W - 1), (W - 1, W - 1), (300, W - 1), (300, 5000), (0, 1500000), (None, None)):
            exp = same(msa, text, von, bis)
            assert exp["bis"] <= W - 1
        assert same(msa, text, W, W + 10) is None and same(msa, text, 10, 9) is None and same(msa, text, -2, 9) is None
        assert device_window(msa, W, W + 10)[0] == -1


@pytest.mark.gpu
def test_group_refinement_inputs():
    """the MSAs of tests/test_gpu_group_refinement.py: upper case, '_', inner blanks, rows blank at their ends"""
    from repeatresolver_amd.group_refinement import read_window
    from repeatresolver_amd.resolution import open_msa, window
    for rows, cuts in ((planted_msa(129, 129, 300, [8, 8, 8]), [(None, None), (10, 280)]),
                       (windowed_msa(), [(120, 330), (0, 419), (200, 200), (60, 5000)])):
        text = as_array(rows)
        with open_msa(rows) as msa:                                   # from the list of bytes
            for von, bis in cuts:
                exp = same(msa, text, von, bis)
                assert 0 < exp["kept_rows"] <= len(rows)
                got, ref = window(msa, von, bis), read_window(rows, von, bis)
                assert all(np.array_equal(g, r) for g, r in zip(got, ref))


@pytest.mark.gpu
def test_offsets_beyond_2_to_the_31():
    """30 000 x 72 000 characters = 2.16e9 > 2^31: a seeded pattern in the last 70 rows and the last 300 columns, everything
    else ' '.  The window over those columns reads offsets that a 32-bit index gets wrong."""
    from repeatresolver_amd.resolution import open_msa
    T, W = 30000, 72000
    assert T * W > 2 ** 31
    text = np.full((T, W), 32, dtype=np.uint8)
    rng = np.random.default_rng(2031)
    text[T - 70:, W - 300:] = ALPHABET[rng.integers(0, len(ALPHABET), (70, 300))]
    text[T - 70::2, W - 300] = ord("a")
    text[T - 70::2, W - 1] = ord("T")
    with open_msa(text) as msa:
        exp = same(msa, text, W - 300, W - 1)
        assert 35 <= exp["kept_rows"] <= 70 and exp["width"] == 300 and not exp["kept"][:T - 70].any()
        assert exp["groups"].any() and exp["coverage"].max() > 10
        exp = same(msa, text, W - 300, 10 ** 6)
        assert exp["bis"] == W - 1
