"""Runs without a GPU: the host pieces of the group refinement (pgr_host.c: window reader, MaxCorrs slice, coverage
restriction, default cutoff) against the literal restatement tests/gr_checker.py, and two properties of the checker on the
inputs of tests/test_gpu_group_refinement.py -- TheBestUpdater's insertion scan equals a sort by (-Z, index), and the share
of variations that the GPU tests may treat as undecided is what those tests state."""
import ctypes
import math

import numpy as np
import pytest

import gr_checker as gc
from test_gpu_group_refinement import CASES, checked, fixture_cases, planted_msa, windowed_msa


def _lib():
    import os
    import subprocess
    from conftest import ROOT
    subprocess.run(["make", "-C", os.path.join(ROOT, "repeatresolver_amd", "csrc"), "all"], check=True, stdout=subprocess.DEVNULL)
    from repeatresolver_amd import _lib
    return _lib.load()


HAND = [b"  acgtACGT-_acgtn acgt  ",          # blank at both ends
        b"acgtacgtac--ACGTxxacgtac",           # 'x': not covered
        b"a   acgt_-acgt   acgtaca",           # inner blanks
        b" cgtacgtac__ACGT..acgtac",
        b"TTTTTTTTTTTTTTTTTTTTTTT ",          # blank at the right end only
        b"________________________"]


@pytest.mark.parametrize("von,bis", [(None, None), (0, 23), (1, 22), (2, 21), (4, 19), (5, 500), (0, 0), (23, 23), (7, 7)])
def test_window_reader_on_a_hand_made_msa(von, bis):
    from repeatresolver_amd.group_refinement import read_window
    _lib()
    rows = [r.ljust(24)[:24] for r in HAND]
    kept, v, b, G, LC, cover = read_window(rows, von, bis)
    ekept, ev, eb, codes = gc.read_window(rows, von, bis)
    assert (v, b) == (ev, eb) and np.array_equal(kept, ekept)
    T, w = codes.shape
    assert G.shape == (w * 5, T // 64 + 1) and LC.shape == (w, T // 64 + 1)
    member = np.zeros((w * 5, T), dtype=np.int64)
    for k in range(5):
        member[k::5] = (codes == k).T
    assert np.array_equal(G, gc.pack(member)) and np.array_equal(LC, gc.pack((codes < 5).T.astype(np.int64)))
    assert np.array_equal(cover, (codes < 5).sum(axis=0))


def test_window_reader_cases():
    """mixed case, '_', blanks at one window end, inner blanks, bis beyond the width; 64 kept rows give sc = 2"""
    from repeatresolver_amd.group_refinement import read_window
    from repeatresolver_amd.realigner import PwrError
    _lib()
    for rows, von, bis in ((planted_msa(64, 64, 300, [8, 8, 8]), None, None), (windowed_msa(), 120, 330),
                           (windowed_msa(seed=22, T=80, W=300), 60, 5000), (planted_msa(3, 129, 90, [4, 4]), 10, 80)):
        kept, v, b, G, LC, cover = read_window(rows, von, bis)
        win = gc.Window(rows, np.zeros(len(rows[0]) * 5), von, bis)
        assert (v, b) == (win.von, win.bis) and np.array_equal(kept, win.kept)
        assert G.shape[1] == win.T // 64 + 1
        assert np.array_equal(G, gc.pack(win.G)) and np.array_equal(LC, gc.pack(win.LC)) and np.array_equal(cover, win.coverage)
    kept = read_window(planted_msa(64, 64, 300, [8, 8, 8]))[0]
    assert kept.sum() == 64 and read_window(planted_msa(64, 64, 300, [8, 8, 8]))[3].shape[1] == 2
    for von, bis in ((5, 4), (-2, 5), (300, 400)):
        with pytest.raises(PwrError) as e:
            read_window(planted_msa(64, 64, 300, [8, 8, 8]), von, bis)
        assert e.value.code == -1


def test_maxcorrs_slice_file_cutoff_and_coverage_restriction(tmp_path):
    lib = _lib()
    pd, pi = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    rng = np.random.default_rng(2)
    full = np.round(rng.random(400 * 5) * 20, 6)
    for von, bis in ((0, 399), (17, 230), (399, 399)):
        out = np.zeros((bis + 1 - von) * 5)
        assert lib.pgr_slice_maxcorrs(full.ctypes.data_as(pd), len(full), von, bis, out.ctypes.data_as(pd)) == 0
        exp = np.array([full[i] for i in range(len(full)) if von <= i // 5 <= bis])
        assert np.array_equal(out, exp)
        path = tmp_path / "MaxCorrsOf_x"
        path.write_text("".join("%f\n" % v for v in full))               # as MaxCorrelation writes it (MC:526-529)
        p, n = ctypes.c_void_p(), ctypes.c_int()
        assert lib.pgr_read_maxcorrs_file(str(path).encode(), von, bis, ctypes.byref(p), ctypes.byref(n)) == 0
        got = np.ctypeslib.as_array(ctypes.cast(p, pd), shape=(n.value,)).copy()
        assert n.value == len(exp) and np.array_equal(got, exp)
    out = np.zeros(10)
    assert lib.pgr_slice_maxcorrs(full.ctypes.data_as(pd), len(full), 399, 400, out.ctypes.data_as(pd)) == -4
    p, n = ctypes.c_void_p(), ctypes.c_int()
    assert lib.pgr_read_maxcorrs_file(str(tmp_path / "nope").encode(), 0, 3, ctypes.byref(p), ctypes.byref(n)) == -4    # RR:621
    for cutoff, width in ((0.0, 300), (0.0999, 1), (0.1, 300), (5.5, 10), (-3.0, 5000)):
        assert lib.pgr_default_cutoff(cutoff, width) == gc.default_cutoff(cutoff, width)
    assert lib.pgr_default_cutoff(0.0, 200) == -1.0 * math.log10(1.0 / 1000.0)
    for cover in ([10, 9, 8, 10, 0], [100, 89, 90, 91, 100], [0, 0, 0, 0, 0], [7, 7, 7, 7, 7]):
        c = np.array(cover, dtype=np.int32)
        mc = np.arange(1.0, 26.0)
        exp = mc.copy()
        emax = gc.restrict_coverage(c, exp)
        m = ctypes.c_int()
        assert lib.pgr_restrict_coverage(5, c.ctypes.data_as(pi), mc.ctypes.data_as(pd), ctypes.byref(m)) == 0
        assert m.value == emax and np.array_equal(mc, exp)


def test_library_exports_every_symbol_of_pgr_h():
    import os
    import re
    from conftest import ROOT
    from repeatresolver_amd._lib import PGR_EXPORTS
    lib = _lib()
    declared = set(re.findall(r"\b(pgr_[a-z_]+)\s*\(", open(os.path.join(ROOT, "include", "pgr.h")).read()))
    assert declared == set(PGR_EXPORTS)
    for name in declared:
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("name", list(CASES) + ["fixtures"])
def test_insertion_scan_equals_sort_and_undecided_share(name):
    """The clique is the top 29 by (Z descending, index ascending) -- what the kernels rely on -- on every clique of the GPU
    tests' inputs; and the checker alone meets what those tests state about undecided variations."""
    for n in (fixture_cases() if name == "fixtures" else [name]):
        exp = checked(n)[5]
        S = len(exp["significant"])
        for s in range(S):
            r = gc.ranked(exp["candidates"][s], exp["cutoff"])[:gc.MAXCLIQUE - 1]
            want = [int(exp["significant"][s])] + [i for _, i in r]
            assert list(exp["cliques"][s]) == want + [-1] * (gc.MAXCLIQUE + 1 - len(want))
        und = sum(gc.undecided(c, exp["cutoff"]) for c in exp["candidates"])
        assert und <= 0.02 * S, (n, und, S)
        if n in ("cut30", "index0", "saturation"):
            assert und == 0
