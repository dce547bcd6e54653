"""Reads from either strand, the part that needs no GPU: the new entries' declarations and their argument errors on the paths
that touch no context, the two host-side pieces (pia_turn, prc_merge_cuts) against plain Python, and -- with the oracle and the
checker -- the conditions the inputs of test_gpu_strands.py rely on."""
import ctypes
import os
import re

import numpy as np
import pytest

import rc_checker as ck
import strand_checker as sc
from repeatresolver_amd import _lib
from repeatresolver_amd.strands import reverse_complement, seeded_mask, turn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = ctypes.POINTER(ctypes.c_int)
PLL = ctypes.POINTER(ctypes.c_longlong)
ARG, INPUT = -1, -4                 # PWR_ERR_ARG, PWR_ERR_INPUT


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def oracle():
    return sc.ia_oracle()


def ints(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int32))
    return a, a.ctypes.data_as(PI)


def offsets(reads):
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return off, off.ctypes.data_as(PLL)


def test_new_entries_are_declared_and_exported(lib):
    pia = open(os.path.join(ROOT, "include", "pia.h")).read()
    prc = open(os.path.join(ROOT, "include", "prc.h")).read()
    for name in ("pia_align_strands", "pia_turn", "pia_run_files_strands"):
        assert re.search(r"^int\s+%s\s*\(" % name, pia, flags=re.M) and name in _lib.PIA_EXPORTS
        getattr(lib, name)
    for name in ("prc_occurrences_strands", "prc_cut_strands", "prc_merge_cuts", "prc_run_files_strands"):
        assert re.search(r"^int\s+%s\s*\(" % name, prc, flags=re.M) and name in _lib.PRC_EXPORTS
        getattr(lib, name)
    assert "both orientations" in pia[pia.index("pia_align_strands("):pia.index("int pia_get_stats")]     # what the cells count


def test_argument_errors_before_any_context(lib):
    off, poff = offsets([b"acgt"])
    al, pal = ints(np.zeros(4))
    d, pd = ints([0])
    o, po = ints([0])
    st = (ctypes.c_ubyte * 1)()
    assert lib.pia_align_strands(None, 1, b"acgt", poff, pal, pd, po, st) == ARG             # no context
    pos_off = (ctypes.c_longlong * 5)()
    p = ctypes.c_void_p()
    assert lib.prc_occurrences_strands(None, 1, b"acgt", poff, 2, 0, 0.3, pos_off, ctypes.byref(p)) == ARG
    n, pn = ints([0])
    nf, pnf = ints([0])
    nr, pnr = ints([0])
    assert lib.prc_cut_strands(None, 1, b"acgt", poff, 2, 0, 0.3, pn, ctypes.byref(p), pnf, pnr) == ARG
    out = ctypes.create_string_buffer(8)
    assert lib.pia_turn(-1, b"acgt", poff, st, out) == ARG
    assert lib.pia_turn(1, b"acgt", None, st, out) == ARG
    assert lib.pia_turn(1, None, poff, st, out) == ARG
    assert lib.pia_turn(1, b"acgt", poff, None, out) == ARG
    assert lib.pia_turn(1, b"acgt", poff, st, None) == ARG
    assert lib.pia_turn(1, b"acnt", poff, st, out) == INPUT                                   # as pia_align refuses it
    assert lib.pia_turn(0, None, poff, None, None) == 0
    bad = (ctypes.c_longlong * 2)(4, 0)
    assert lib.pia_turn(1, b"acgt", bad, st, out) == ARG                                      # a negative length
    a, pa = ints([5])
    assert lib.prc_merge_cuts(10, -1, pa, 0, pa, pa) == ARG
    assert lib.prc_merge_cuts(10, 0, pa, -1, pa, pa) == ARG
    assert lib.prc_merge_cuts(10, 1, None, 0, None, pa) == ARG
    assert lib.prc_merge_cuts(10, 1, pa, 0, None, None) == ARG


def test_reverse_complement():
    assert reverse_complement(b"") == b""
    assert reverse_complement(b"a") == b"t" and reverse_complement(b"G") == b"C"
    assert reverse_complement(b"aacgT") == b"Acgtt"                                           # odd, the case kept
    assert reverse_complement(b"acgt") == b"acgt"                                             # even, its own reverse complement
    assert reverse_complement(b"ACgtTT") == b"AAacGT"
    import random
    rng = random.Random(1)
    for n in (1, 2, 3, 64, 65, 1001):
        r = bytes(rng.choice(list(b"acgtACGT")) for _ in range(n))
        assert reverse_complement(r) == sc.rc(r) and reverse_complement(reverse_complement(r)) == r
    assert seeded_mask(50, 7) == sc.mask(50, 7) and 10 < sum(seeded_mask(50, 7)) < 40
    assert turn([b"aac", b"aac"], [0, 1]) == [b"aac", b"gtt"]


def test_pia_turn_equals_reverse_complement(lib):
    import random
    rng = random.Random(2)
    reads = [b"", b"a", b"T", b"aC", b"acG", b"aacgT", b"ACgtTT", b""] + \
        [bytes(rng.choice(list(b"acgtACGT")) for _ in range(n)) for n in (63, 64, 65, 700, 701)]
    for strands in ([1] * len(reads), [0] * len(reads), [j & 1 for j in range(len(reads))], [~j & 1 for j in range(len(reads))]):
        off, poff = offsets(reads)
        st = (ctypes.c_ubyte * len(reads))(*strands)
        out = ctypes.create_string_buffer(int(off[-1]) + 1)
        assert lib.pia_turn(len(reads), b"".join(reads), poff, st, out) == 0
        got = [out.raw[off[j]:off[j + 1]] for j in range(len(reads))]
        assert got == [reverse_complement(r) if s else r for r, s in zip(reads, strands)]
        assert out.raw[int(off[-1])] == 0                                                      # nothing behind the last read
    # the offsets need not start at 0: only [off[0], off[n]) is read and written
    off = (ctypes.c_longlong * 3)(2, 5, 6)
    out = ctypes.create_string_buffer(b"........", 8)
    assert lib.pia_turn(2, b"nnaagcnn", off, (ctypes.c_ubyte * 2)(1, 1), out) == 0
    assert out.raw[:8] == b"..cttg.."


def merge(lib, readlen, fwd, rev):
    f, pf = ints(fwd or [0])
    r, pr = ints(rev or [0])
    out, po = ints(np.zeros(len(fwd) + len(rev) + 1))
    n = lib.prc_merge_cuts(readlen, len(fwd), pf, len(rev), pr, po)
    assert 0 <= n <= len(fwd) + len(rev)
    return [int(v) for v in out[:n]]


def test_prc_merge_cuts(lib):
    assert merge(lib, 1000, [], []) == []
    assert merge(lib, 1000, [300, 600], []) == [300, 600]
    assert merge(lib, 1000, [], [100, 400, 700]) == [300, 600, 900]                           # only reverse: ascending
    assert merge(lib, 1000, [300, 650], [400, 700]) == [300, 600, 650]                        # 300 == 1000 - 700: once
    assert merge(lib, 1000, [500], [500]) == [500]
    assert merge(lib, 1001, [500], [500]) == [500, 501]
    assert merge(lib, 1000, [200, 800], [300, 500]) == [200, 500, 700, 800]                   # interleaved
    import random
    rng = random.Random(4)
    for _ in range(300):
        L = rng.randrange(1, 60)
        f = sorted(rng.sample(range(L + 1), rng.randrange(0, min(L, 8))))
        r = sorted(rng.sample(range(L + 1), rng.randrange(0, min(L, 8))))
        assert merge(lib, L, f, r) == sc.merge_cuts(L, f, r)


def test_checker_occurrences_mirror():
    """what the composition means: an exact hit of a piece ending at column y of rc(read) is the piece's reverse complement
    starting at read[len - 1 - y]"""
    templ = "acgtacggattacagcatcgatcgacgatgcatgcaagtc" * 3
    pc = ck.piece(templ, 3, 0, 0)
    read = "ttttttgggtgtgtgtgtgtg" + sc.rc(pc) + "cacacacattatatacc"
    f, r = sc.occurrences_strands(templ, read, 3, 0, 0.1)
    assert f[0] == [] and len(r[0]) == 1
    y = r[0][0]
    assert read[len(read) - 1 - y:len(read) - 1 - y + len(pc)] == sc.rc(pc)


# ---- the conditions the GPU inputs rely on ----------------------------------------------------------------------------

def test_pipeline_reads_are_nearer_on_their_own_strand(oracle):
    """every cut read of the pipeline case aligns strictly nearer as it is than turned: pia_align_strands then takes a turned
    one back and leaves the others, which is what makes the MSA of the mixed input the MSA of the original"""
    templ, reads = sc.pipeline_reads()
    assert len(reads) > 20
    m = sc.mask(len(reads), sc.PIPELINE_SEED)
    assert 0.25 * len(reads) < sum(m) < 0.75 * len(reads)
    for r in reads:
        (_, df), (_, dr) = oracle(r, templ), oracle(sc.rc(r), templ)
        assert df < dr and df / len(r) < 0.30 <= dr / len(r)


def test_chunk_case_is_exact_on_one_strand_only(oracle):
    templ, subs = sc.chunk_case()
    assert [len(s) for _, s in subs] == list(sc.CHUNK_LENGTHS)
    for a, s in subs:
        p, d = oracle(s, templ)
        assert d == 0 and p == list(range(a, a + len(s)))
        assert oracle(sc.rc(s), templ)[1] > 0


def test_cli_case_conditions(oracle):
    templ, reads, m = sc.cli_case()
    passing = 0
    for j, r in enumerate(reads):
        if len(r) == 0:
            continue
        (_, df), (_, dr) = oracle(r, templ), oracle(sc.rc(r), templ)
        if df / len(r) < 0.30:
            assert df < dr and dr / len(r) >= 0.30
            passing += 1
        else:
            assert sc.rc(r) == r and df == dr                     # rejected on both strands, and turning it is no change
    assert passing == 40 and 10 < sum(m) < 32 and sum(1 for r in reads if len(r) == 0) == 1


def test_chain_case_conditions(oracle):
    """no read of the chain case is cut on its reverse strand, every piece passes the cut-off on its own strand and is strictly
    nearer there: the -b chain on the mixed file then writes the rows of the plain chain on the original file"""
    templ, reads, m = sc.chain_case()
    assert m[-2:] == [0, 0] and 4 < sum(m) < 12
    last = (reads[-1] + reads[-2][len(reads[-1]):])[:len(reads[-2])]                          # RC:86-89
    assert last == reads[-1] == reads[-2]                                                     # so both are cut at their own points
    npieces = 0
    for r in reads[:-1]:
        cuts, nf, nr = sc.cut_strands(templ, r, sc.CHAIN_PARTS, 0, 0.30)
        assert nf >= 1 and nr == 0 and cuts == ck.cut(templ, r, sc.CHAIN_PARTS, 0, 0.30)
        assert sc.cut_strands(templ, sc.rc(r), sc.CHAIN_PARTS, 0, 0.30) == ([len(r) - c for c in reversed(cuts)], 0, nf)
        for p in sc.pieces(r, cuts):
            (_, df), (_, dr) = oracle(p.encode(), templ.encode()), oracle(sc.rc(p).encode(), templ.encode())
            assert df < dr and df / len(p) < 0.30
            npieces += 1
    assert npieces > 30


def test_cut_cases_exercise_both_strands():
    templ, reads = sc.cut_case()
    assert len(reads) == 18
    parts, overlap, e = sc.CUT_CONFIGS[0]
    res = [sc.cut_strands(templ, r, parts, overlap, e) for r in reads]
    assert sum(nf for _, nf, _ in res[0::3]) > 6 and all(nr == 0 for _, _, nr in res[0::3])   # as they are
    assert [(c, nr, nf) for c, nf, nr in res[1::3]] == [([len(r) - x for x in reversed(c)], nf, nr)
                                                        for r, (c, nf, nr) in zip(reads[0::3], res[0::3])]   # turned: mirrored
    assert sum(1 for _, nf, nr in res[2::3] if nf > 0 and nr > 0) >= 3                         # inverted neighbours: both
    templ, read = sc.overflow_case()
    f, r = sc.occurrences_strands(templ, read, 2, 0, 0.30)
    assert len(f[0]) < 8 < 20 < len(r[0])                                                     # PRC_RUN_CAP = 8: the re-run is a reverse job's
