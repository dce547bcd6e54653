"""ReadCutter port, host side (no GPU): the C ABI's declarations, the CPU checker against the reference's fixtures, and the
library's plain-C pieces (reader, last-row scan, cut selection, writer) against the checker."""
import ctypes
import gzip
import json
import os
import random
import re

import numpy as np
import pytest

import rc_checker as ck
from repeatresolver_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = json.load(open(os.path.join(GOLDEN, "rc_cases.json")))["cases"]
IDS = [c["name"] for c in CASES]
PI = ctypes.POINTER(ctypes.c_int)


def gz(name) -> bytes:
    with gzip.open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def inputs(c):
    return gz(f"rc_{c['input']}.template.gz"), gz(f"rc_{c['input']}.reads.gz")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def ints(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int32))
    return a, a.ctypes.data_as(PI)


def test_prc_header_matches_exports(lib):
    src = open(os.path.join(ROOT, "include", "prc.h")).read()
    declared = re.findall(r"^(?:int|void)\s+\**(prc_\w+)\s*\(", src, flags=re.M)
    assert sorted(declared) == sorted(_lib.PRC_EXPORTS)
    for name in _lib.PRC_EXPORTS:
        getattr(lib, name)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_checker_reproduces_reference(case):
    templ, reads = inputs(case)
    out, seq, info = ck.run(case["template_name"], templ, reads, case["args"])
    assert case["exit_code"] == 0
    assert out == case["stdout"]
    assert seq == gz(f"rc_{case['name']}.seq.gz")
    assert info == gz(f"rc_{case['name']}.info.gz")


def test_checker_myers_equals_matrix():
    rng = random.Random(5)
    for _ in range(300):
        m = rng.choice((1, 2, 5, 31, 32, 33, 40))
        pat = "".join(rng.choice("acgtN" if rng.random() < 0.2 else "acgt") for _ in range(m))
        read = "".join(rng.choice("acgt") for _ in range(rng.randrange(0, 120)))
        assert ck.last_row_myers(pat, read) == ck.last_row_dense(pat, read)


def _random_scores(rng, n, cutoff):
    """score sequences around the cutoff: runs one column apart, runs reaching column 1, column 0 below the cutoff"""
    s = [cutoff + rng.randrange(0, 4) for _ in range(n)]
    y = n - 1
    while y >= 0:
        y -= rng.choice((1, 1, 2, 3, 7))
        k = rng.randrange(1, 6)
        for x in range(max(y - k, 0), y + 1):
            s[x] = max(0, cutoff - rng.randrange(1, 5))
        y -= k + rng.choice((1, 1, 1, 2))
    if rng.random() < 0.3 and n > 0:
        s[0] = cutoff - 1
    if rng.random() < 0.3 and n > 1:
        s[1] = cutoff - 1
    return s


def _runs_of(score, cutoff):
    runs, y = [], 0
    while y < len(score):
        if score[y] < cutoff:
            lo, mn, ey = y, score[y], y
            while y < len(score) and score[y] < cutoff:
                if score[y] <= mn:
                    mn, ey = score[y], y
                y += 1
            runs.append((lo, y - 1, mn, ey))
        else:
            y += 1
    return runs


def test_host_scan_dense_and_runs_equal_checker(lib):
    rng = random.Random(7)
    for it in range(4000):
        n = rng.choice((0, 1, 2, 3, 5, 17, 60, 200))
        cutoff = rng.randrange(1, 30)
        len1 = rng.choice((1, 2, 7, 10, 31, 50))
        s = _random_scores(rng, n, cutoff)
        exp = ck.scan(s, len1, cutoff)
        arr, p = ints(s if s else [0])
        out, po = ints(np.zeros(n + 2))
        got = lib.prc_scan_dense(p, n, len1, cutoff, po)
        assert list(out[:got]) == exp, (it, s, len1, cutoff)
        runs = _runs_of(s, cutoff)
        ra, rp = ints(np.array(runs, dtype=np.int32).reshape(-1) if runs else [0])
        out2, po2 = ints(np.zeros(len(runs) + 1))
        got2 = lib.prc_scan_runs(rp, len(runs), len1, po2)
        assert list(out2[:got2]) == exp, (it, s, len1, cutoff, runs)


def _read_fasta(lib, path):
    n, ln = ctypes.c_int(), ctypes.c_int()
    b, o, last = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.prc_read_fasta(path.encode(), ctypes.byref(n), ctypes.byref(b), ctypes.byref(o), ctypes.byref(last), ctypes.byref(ln)) == 0
    off = np.ctypeslib.as_array(ctypes.cast(o, ctypes.POINTER(ctypes.c_longlong)), shape=(n.value + 1,)).copy()
    bases = ctypes.string_at(b, int(off[-1])).decode()
    lastb = ctypes.string_at(last, ln.value).decode()
    for p in (b, o, last):
        lib.prc_free(p)
    return [bases[off[i]:off[i + 1]] for i in range(n.value)], lastb


@pytest.mark.parametrize("name", sorted({c["input"] for c in CASES}))
def test_host_reader_equals_checker(lib, tmp_path, name):
    data = gz(f"rc_{name}.reads.gz")
    p = tmp_path / "r.fasta"
    p.write_bytes(data)
    assert _read_fasta(lib, str(p)) == ck.read_records(data)
    t = tmp_path / "t.fasta"
    t.write_bytes(gz(f"rc_{name}.template.gz"))
    tp, tl = ctypes.c_void_p(), ctypes.c_int()
    assert lib.prc_read_template(str(t).encode(), ctypes.byref(tp), ctypes.byref(tl)) == 0
    assert ctypes.string_at(tp, tl.value).decode() == ck.read_template(t.read_bytes())
    lib.prc_free(tp)


def host_cut(lib, templ, read, parts, overlap, e):
    """the library's cut selection fed the checker's positions"""
    ln, _ = ck.params(templ, parts, overlap, e)
    occ = ck.occurrences(templ, read, parts, overlap, e)
    a0, p0 = ints(occ[0] or [0])
    aL, pL = ints(occ[-1] or [0])
    out, po = ints(np.zeros(3 * len(occ[0]) + 2 * len(occ[-1]) + 1))
    n = lib.prc_select_cuts(parts, ln, len(templ), len(read), p0, len(occ[0]), pL, len(occ[-1]), po)
    assert n >= 0
    return list(out[:n])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_selection_and_writer_write_fixture(lib, tmp_path, case):
    templ_b, reads = inputs(case)
    templ = ck.read_template(templ_b)
    o = ck.parse_args([case["template_name"], "reads"] + case["args"])
    cut_fn = lambda r: host_cut(lib, templ, r, o["parts"], o["overlap"], o["e"])
    out, _, _ = ck.run(case["template_name"], templ_b, reads, case["args"], cut_fn=cut_fn)
    assert out == case["stdout"]
    # the writer: the records as the reference writes them, the library's cut points
    recs, last = ck.read_records(reads)
    n = len(recs)
    written = recs[:-1] + [last] if n >= 2 else ([""] if n == 1 else [])
    cuts = [cut_fn(r) for r in recs[:n - 2]] + ([cut_fn(last)] * 2 if n >= 2 else [[]] * n)
    counts = [len(c) for c in cuts[:n - 1]] + [0] if n else []
    off = np.zeros(len(written) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in written])
    nc, pnc = ints([len(c) for c in cuts] or [0])
    flat, pflat = ints([x for c in cuts for x in c] or [0])
    ci, pci = ints(counts or [0])
    seq, info = tmp_path / "Seq.fasta", tmp_path / "Info"
    assert lib.prc_write_seq(str(seq).encode(), len(written), "".join(written).encode(),
                             off.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), pnc, pflat) == 0
    assert lib.prc_write_info(str(info).encode(), len(written), pci) == 0
    assert seq.read_bytes() == gz(f"rc_{case['name']}.seq.gz")
    assert info.read_bytes() == gz(f"rc_{case['name']}.info.gz")


def test_select_cuts_without_first_cut_is_empty(lib):
    """candidates exist but none is below 1.5 T: the reference reads CuttingPoints[-1]; the port reports no cuts"""
    assert ck.select_cuts(3, 10, 100, 1000, [400, 700], [500]) == []
    a0, p0 = ints([700, 400])
    aL, pL = ints([500])
    out, po = ints(np.zeros(16))
    assert lib.prc_select_cuts(3, 10, 100, 1000, p0, 2, pL, 1, po) == 0
