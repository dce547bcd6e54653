"""The locus anchorer (include/pla.h), everything that needs no GPU: the checker against a cell-by-cell double loop, the four
walks against explicit reverse complements, the chunked table with its warm-up against the whole one, every status of
pla_place, the readers and the writers byte for byte, every refusal of pla_search and pla_open_text, datagen.true_loci and
collapsed_assembly, and the host C under the sanitizers as a program of its own."""
import ctypes
import hashlib
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import la_checker as la

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rand(rng, n, alphabet=b"acgt") -> bytes:
    return bytes(rng.choice(list(alphabet), size=n).astype(np.uint8))


# ---- the checker ----
def test_last_row_against_the_double_loop_on_all_short_pairs():
    words = [bytes(w) for n in range(1, 6) for w in itertools.product(b"ac", repeat=n)]
    for q in words:
        for w in words:
            assert la.last_row(la.codes(q), la.codes(w)).tolist() == la.last_row_loops(la.codes(q), la.codes(w)).tolist(), (q, w)


def test_last_row_against_the_double_loop_on_random_pairs_with_unknown_bases():
    rng = np.random.default_rng(1)
    for _ in range(300):
        q = la.codes(rand(rng, int(rng.integers(1, 40)), b"acgt" if rng.random() < 0.5 else b"ac"))
        w = la.codes(rand(rng, int(rng.integers(0, 90)), b"acgtnN-R" if rng.random() < 0.5 else b"acn"))
        assert la.last_row(q, w).tolist() == la.last_row_loops(q, w).tolist()


def test_an_unknown_base_matches_nothing_and_keeps_its_place():
    assert la.codes(b"aCgTnNx-").tolist() == [0, 1, 2, 3, 4, 4, 4, 4]
    # "acgt" in "acNgt": one edit (the N is a base too many), found where the pattern ends: coordinates are the file's
    hits = la.search([b"ttacNgttt"], [b"tgca"], [0], 4, 1, 250)
    assert (0, 0, 0, 7, 7, 7, 1) in hits


def test_the_four_walks_against_explicit_reverse_complements():
    """a job's (backwards, complemented) walk finds what the forward plain walk finds in the text turned accordingly"""
    from repeatresolver_amd.strands import reverse_complement
    rng = np.random.default_rng(2)
    for _ in range(40):
        t = rand(rng, 120, b"acgtn")
        a = rand(rng, 12)
        for side in (0, 1):
            for o in (0, 1):
                got = la.runs(la.last_row(la.rows_of(a, 12), la.walk(la.codes(t), side, o)), 2)
                # by hand: reverse the text iff side != o, complement it iff o == 1
                turned = t
                if side != o and o == 1:
                    turned = reverse_complement(t)
                elif side != o:
                    turned = t[::-1]
                elif o == 1:
                    turned = reverse_complement(t)[::-1]
                assert got == la.runs(la.last_row(la.rows_of(a, 12), la.codes(turned)), 2)
    # a left flank on the - strand: its reverse complement stands behind the repeat in the contig
    flank, rest = b"acgtgtcaag", b"tttttttttttt"                                 # template orientation: flank, then the repeat
    contig = reverse_complement(flank + rest)
    hits = la.search([contig], [flank[::-1]], [0], 10, 1, 0)
    assert hits == [(0, 1, 0, len(rest), len(rest), len(rest), 0)]
    # and a right flank on the + strand is found by the backward walk, boundary in front of its first base
    hits = la.search([rest + flank], [flank], [1], 10, 1, 0)
    assert hits == [(0, 0, 0, len(rest), len(rest), len(rest), 0)]


def test_chunks_with_a_warm_up_of_m_plus_k_give_the_thresholded_table():
    rng = np.random.default_rng(3)
    bad = 0
    for case in range(60):
        alphabet = b"ac" if case % 3 == 0 else b"acgt"
        m = int(rng.integers(1, 24))
        q = la.codes(rand(rng, m, alphabet))
        w = la.codes(rand(rng, int(rng.integers(1, 160)), alphabet + (b"n" if case % 4 == 0 else b"")))
        k = int(rng.integers(0, 501)) * m // 1000
        whole = np.minimum(la.last_row(q, w), k + 1)
        for chunk in range(1, 51):
            bad += int((la.chunked_last_row(q, w, k, chunk)[1:] != whole[1:]).any())
    assert bad == 0


def test_runs_minimum_and_first_column_of_the_minimum():
    last = np.array([9, 3, 2, 2, 5, 1, 9, 0, 0], dtype=np.int64)                   # column 0 is never part of a run
    assert la.runs(last, 3) == [(1, 3, 2, 2), (5, 5, 1, 5), (7, 8, 0, 7)]
    assert la.runs(last, 0) == [(7, 8, 0, 7)] and la.runs(np.array([0, 5]), 3) == []


# ---- pla_place ----
def hit(p, o, c, b, d=0):
    return (p, o, c, b, b, b, d)


def c_place(hits, lp, rp, max_span):
    from repeatresolver_amd import anchors
    got = anchors.place(anchors.Hits.of(hits), lp, rp, max_span=max_span)
    exp = la.place(hits, lp, rp, max_span)
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g.status == e[0] and (g.lo, g.hi, g.span) == e[3:], (g, e)
        for side, h in (("left", e[1]), ("right", e[2])):
            want = (-1, -1, -1, -1) if h is None else (h[2], h[1], h[3], h[6])
            assert tuple(getattr(g, f"{side}_{f}") for f in ("contig", "orientation", "boundary", "distance")) == want
    return [g.name for g in got]


def test_every_status_of_place():
    hits = sorted([
        hit(0, 0, 0, 100), hit(1, 0, 0, 400, 2),            # locus 0: placed +, span 300
        hit(2, 1, 1, 900), hit(3, 1, 1, 500),               # locus 1: placed -, span 400
        hit(4, 0, 0, 50), hit(5, 0, 2, 60),                 # locus 2: bridge
        hit(6, 0, 3, 10),                                   # locus 3: left only
        hit(9, 1, 3, 700),                                  # locus 4: right only
        # locus 5: nothing
        hit(12, 0, 4, 10), hit(12, 1, 5, 10), hit(13, 0, 4, 90),   # locus 6: the left flank twice
        hit(14, 0, 6, 10), hit(15, 1, 6, 90),               # locus 7: orientations differ
        hit(16, 0, 6, 500), hit(17, 0, 6, 400),             # locus 8: + with the right boundary in front of the left
        hit(18, 0, 7, 100), hit(19, 0, 7, 601),             # locus 9: span 501 = max_span + 1
        hit(20, 0, 8, 100), hit(21, 0, 8, 600),             # locus 10: span 500 = max_span
        hit(22, 0, 9, 77), hit(23, 0, 9, 77),               # locus 11: span 0
        hit(24, 0, 4, 5), hit(24, 0, 4, 50), hit(24, 1, 4, 70),   # locus 12: three hits left, none right: still ambiguous
    ])
    lp = list(range(0, 26, 2))
    rp = list(range(1, 26, 2))
    names = c_place(hits, lp, rp, 500)
    assert names == ["PLACED", "PLACED", "BRIDGE", "LEFT_ONLY", "RIGHT_ONLY", "NONE", "AMBIGUOUS", "INCONSISTENT", "INCONSISTENT",
                     "INCONSISTENT", "PLACED", "PLACED", "AMBIGUOUS"]
    from repeatresolver_amd import anchors
    got = anchors.place(anchors.Hits.of(hits), lp, rp, max_span=500)
    assert (got[0].lo, got[0].hi, got[0].span) == (100, 400, 300) and (got[1].lo, got[1].hi, got[1].span) == (500, 900, 400)
    assert got[7].span is None and got[8].span == -100 and got[9].span == 501 and got[11].span == 0 and got[2].span is None
    assert (got[6].left_hits, got[6].right_hits, got[6].left_contig, got[6].right_contig) == (2, 1, -1, 4)
    # a locus without a pattern on a side: its hits cannot be there
    assert c_place(hits, [0, -1], [-1, 1], 500) == ["LEFT_ONLY", "RIGHT_ONLY"]
    assert c_place([], [0], [1], 0) == ["NONE"]


def test_conflicts_overlap_but_do_not_touch():
    hits = sorted([hit(0, 0, 0, 100), hit(1, 0, 0, 200),    # [100, 200)
                   hit(2, 0, 0, 200), hit(3, 0, 0, 300),    # [200, 300): touches the first
                   hit(4, 1, 0, 350), hit(5, 1, 0, 299),    # [299, 350) on the - strand: overlaps the second by one base
                   hit(6, 0, 1, 150), hit(7, 0, 1, 250),    # the same numbers on another contig: no conflict
                   hit(8, 0, 0, 320), hit(9, 0, 0, 330)])   # [320, 330) inside the third
    assert c_place(hits, [0, 2, 4, 6, 8], [1, 3, 5, 7, 9], 1000) == ["PLACED", "CONFLICT", "CONFLICT", "PLACED", "CONFLICT"]
    # precedence: a locus that is ambiguous is never placed, so it conflicts with nothing
    more = sorted(hits + [hit(10, 0, 0, 100), hit(10, 0, 0, 120), hit(11, 0, 0, 180)])
    assert c_place(more, [0, 10], [1, 11], 1000) == ["PLACED", "AMBIGUOUS"]


def test_place_refusals():
    from repeatresolver_amd import anchors
    from repeatresolver_amd.realigner import PwrError
    with pytest.raises(PwrError):
        anchors.place(anchors.Hits.of([]), [0], [1], max_span=-1)
    with pytest.raises(ValueError):
        anchors.place(anchors.Hits.of([]), [0, 1], [1], max_span=5)


# ---- the readers ----
def test_read_contigs(tmp_path):
    from repeatresolver_amd import anchors
    from repeatresolver_amd.realigner import PwrError
    p = tmp_path / "a.fasta"
    p.write_bytes(b">one first contig\nacgtNN\nACGTry\n\n>two\n>three\tx\r\nac gt\r\nnnnn-*\n>\nA")
    assert anchors.read_contigs(p) == [("one", b"acgtnnACGTnn"), ("two", b""), ("three", b"acgtnnnnnn"), ("", b"A")]
    (tmp_path / "empty.fasta").write_bytes(b"")
    assert anchors.read_contigs(tmp_path / "empty.fasta") == []
    (tmp_path / "bad.fasta").write_bytes(b"acgt\n>x\nac\n")
    with pytest.raises(PwrError):
        anchors.read_contigs(tmp_path / "bad.fasta")
    with pytest.raises(PwrError):
        anchors.read_contigs(tmp_path / "missing.fasta")


def loci_of(parts):
    from repeatresolver_amd.resolution import Locus
    return [Locus(thread=t, left_label=L, right_label=R, rows=5, left_len=len(l), copy_len=len(c), right_len=len(r), sequence=l + c + r)
            for t, (L, l, c, R, r) in enumerate(parts)]


def test_read_loci_against_write_loci(tmp_path):
    from repeatresolver_amd import anchors
    from repeatresolver_amd.realigner import PwrError
    from repeatresolver_amd.resolution import write_loci
    loci = loci_of([(3, "ACGTT", "GGGG", 7, "CCA"), (-1, "", "ACAC", 2, "TTTG"), (4, "AC", "G", 0, "")])
    write_loci(tmp_path / "l.fasta", loci, "toy")
    got = anchors.read_loci(tmp_path / "l.fasta")
    assert [g["name"] for g in got] == ["toy_locus0", "toy_locus1", "toy_locus2"]
    assert [(g["left_len"], g["copy_len"], g["right_len"]) for g in got] == [(5, 4, 3), (0, 4, 4), (2, 1, 0)]
    assert [(g["left"], g["right"]) for g in got] == [(b"TTGCA", b"CCA"), (b"", b"TTTG"), (b"CA", b"")]
    assert all(g["sides"] == (0, 1) for g in got) and got[0]["sequence"] == b"ACGTTGGGGCCA"
    anchored, side, lp, rp = anchors.locus_patterns(loci)
    assert anchored == [x for g in got for x in (g["left"], g["right"])] and side == [0, 1] * 3 and lp == [0, -1, 4] and rp == [1, 3, -1]
    for text in (">x left=1:2 copy=1 right=1:1\nACG\n", ">x left=1:2 copy=1\nACG\n", ">x left=1:1 copy=1 right=1:1\nANG\n"):
        (tmp_path / "bad.fasta").write_text(text)
        with pytest.raises(PwrError):
            anchors.read_loci(tmp_path / "bad.fasta")


# ---- the writers ----
def test_writers_byte_for_byte(tmp_path):
    from repeatresolver_amd import anchors
    from repeatresolver_amd.strands import reverse_complement
    contigs = [("c0", b"aaaaaCCCCCgggggTTTTTnnnnn"), ("c1", b"acgtacgtacgt"), ("c2", b"")]
    hits = sorted([hit(0, 0, 0, 5, 1), hit(1, 0, 0, 10, 2),         # locus 0: [5, 10) of c0, +
                   hit(2, 1, 0, 20), hit(3, 1, 0, 15),              # locus 1: [15, 20) of c0, -
                   hit(4, 0, 1, 4), hit(5, 0, 1, 4),                # locus 2: an empty interval at 4 of c1
                   hit(6, 0, 1, 8), hit(7, 0, 0, 22),               # locus 3: a bridge from c1 to c0
                   hit(8, 1, 1, 11)])                               # locus 4: left only
    pl = anchors.place(anchors.Hits.of(hits), [0, 2, 4, 6, 8, 10], [1, 3, 5, 7, 9, 11], max_span=10)
    assert [p.name for p in pl] == ["PLACED", "PLACED", "PLACED", "BRIDGE", "LEFT_ONLY", "NONE"]
    names = ["t_locus0", "t_locus1", "t_locus2", "t_locus3", "t_locus4", "t_locus5"]
    anchors.write_placements(tmp_path / "p", names, pl, contigs)
    assert (tmp_path / "p").read_text() == (
        "t_locus0\tPLACED\tc0\tc0\t+\t+\t5\t10\t5\t10\t5\t1\t2\n"
        "t_locus1\tPLACED\tc0\tc0\t-\t-\t20\t15\t15\t20\t5\t0\t0\n"
        "t_locus2\tPLACED\tc1\tc1\t+\t+\t4\t4\t4\t4\t0\t0\t0\n"
        "t_locus3\tBRIDGE\tc1\tc0\t+\t+\t8\t22\t-\t-\t-\t0\t0\n"
        "t_locus4\tLEFT_ONLY\tc1\t-\t-\t-\t11\t-\t-\t-\t-\t0\t-\n"
        "t_locus5\tNONE\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\n")
    copies = ["ACGTA", b"AAACG", "tt", "GGGG", "", "C"]
    anchors.write_patched(tmp_path / "f", contigs, pl, copies)
    want = (b">c0 patched=2\naaaaaACGTAgggggCGTTTnnnnn\n>c1 patched=1\nacgtttacgtacgt\n>c2 patched=0\n\n")
    assert (tmp_path / "f").read_bytes() == want
    assert reverse_complement(b"AAACG") == b"CGTTT"
    assert b"".join(b">%s patched=%d\n%s\n" % (n.encode(), k, s) for n, s, k in anchors.patch(contigs, pl, copies)) == want
    # plain sequences are named contig<j>
    anchors.write_patched(tmp_path / "g", [s for _, s in contigs], pl, copies)
    assert (tmp_path / "g").read_bytes() == want.replace(b">c", b">contig")
    assert anchors.anchor_lines(anchors.Hits.of(hits[:2]), names, contigs) == "t_locus0\tleft\t+\tc0\t5\t5\t5\t1\nt_locus0\tright\t+\tc0\t10\t10\t10\t2\n"


# ---- refusals, none of which touches a device ----
def test_every_refusal_of_search_and_open_text():
    from repeatresolver_amd import _lib
    lib = _lib.load()
    ARG, RANGE, INPUT, UNSUPPORTED = -1, -5, -4, -7
    h = ctypes.c_void_p()
    assert lib.pla_create(ctypes.byref(h), 0) == 0 and lib.pla_create(None, 0) == ARG and lib.pla_create(ctypes.byref(ctypes.c_void_p()), -1) == ARG
    ll = ctypes.c_longlong
    res = _lib.PlaHits()

    def search(np_=2, anchored=b"acgtACGT", off=(0, 4, 8), side=(0, 1), reach=4, min_len=1, permille=0, ctx=h, out=res, null=()):
        o = (ll * len(off))(*off)
        s = (ctypes.c_int * max(len(side), 1))(*side)
        return lib.pla_search(ctx, np_, None if "anchored" in null else anchored, None if "off" in null else o,
                              None if "side" in null else s, reach, min_len, permille, None if out is None else ctypes.byref(out))

    try:
        assert search(ctx=None) == ARG and search(out=None) == ARG and search(np_=-1) == ARG
        assert search(null=("off",)) == ARG and search(null=("side",)) == ARG and search(null=("anchored",)) == ARG
        assert search(side=(0, 2)) == ARG and search(side=(-1, 0)) == ARG and search(off=(0, 6, 4)) == ARG
        assert search(reach=0) == RANGE and search(reach=513) == RANGE and search(permille=-1) == RANGE and search(permille=501) == RANGE
        assert search(min_len=0) == RANGE and search(np_=65537, off=tuple([0] * 65538), side=tuple([0] * 65537)) == RANGE
        assert search(anchored=b"acgtACNT") == INPUT and search(anchored=b"acg-ACGT", min_len=100) == INPUT   # short patterns are read too
        assert search(side=(0, 2), reach=0, anchored=b"acgtACNT") == ARG and search(reach=0, anchored=b"acgtACNT") == RANGE   # the order
        assert search() == UNSUPPORTED and search(np_=0, off=(0,), side=()) == UNSUPPORTED                   # no text is open
        assert res.n == 0 and not res.pattern
        off = (ll * 3)(0, 4, 8)
        assert lib.pla_open_text(None, 2, b"acgtacgt", off) == ARG and lib.pla_open_text(h, -1, b"acgtacgt", off) == ARG
        assert lib.pla_open_text(h, 2, b"acgtacgt", None) == ARG and lib.pla_open_text(h, 2, None, off) == ARG
        assert lib.pla_open_text(h, 2, b"acgtacgt", (ll * 3)(0, 6, 4)) == ARG
        assert lib.pla_open_text(h, 1, b"acgtacgt", (ll * 2)(0, 1 << 31)) == RANGE
        assert search() == UNSUPPORTED                                              # a refused text opens nothing
        for name, value, want in ((b"chunk", 31, RANGE), (b"chunk", 34, RANGE), (b"chunk", 65540, RANGE), (b"chunk", 0, RANGE),
                                  (b"chunk", 32, 0), (b"chunk", 36, 0), (b"chunk", 65536, 0), (b"chunks", 64, ARG)):
            assert lib.pla_set_option(h, name, value) == want, (name, value)
        assert lib.pla_set_option(None, b"chunk", 64) == ARG and lib.pla_set_option(h, None, 64) == ARG
        cells, ms = ctypes.c_uint64(7), ctypes.c_double(7)
        assert lib.pla_get_stats(h, ctypes.byref(cells), ctypes.byref(ms)) == 0 and cells.value == 0 and ms.value == 0.0
        lib.pla_close_text(h)
        lib.pla_close_text(None)
    finally:
        lib.pla_destroy(h)
    lib.pla_destroy(None)
    for name in _lib.PLA_EXPORTS:
        getattr(lib, name)
    assert [lib.pla_status_name(s).decode() for s in range(8)] == list(_lib.PLA_STATUS_NAMES) and lib.pla_status_name(8) == b"?"


def test_value_errors():
    from repeatresolver_amd import anchors, datagen as dg
    with pytest.raises(ValueError):
        anchors.write_placements("x", ["a"], [], [])
    with pytest.raises(ValueError):
        anchors.write_patched("x", [], [], ["A"])
    with pytest.raises(ValueError):
        dg.collapsed_assembly(dg.CONFIGS["toy_a"], ["placed+"], 10, 1)
    with pytest.raises(ValueError):
        dg.collapsed_assembly(dg.CONFIGS["toy_a"], ["placed+", "placed-", "bridge", "joined"], 10, 1)


# ---- datagen ----
def test_true_loci_and_the_unchanged_digest():
    from repeatresolver_amd import datagen as dg
    import test_flank_consensus as tfc
    cfg = dg.CONFIGS["toy_b"]
    seq, full, starts, cids, cut_b, cut_t = dg.simulate_dataset(cfg)
    h = hashlib.sha256()
    h.update(seq.tobytes())
    for r in full:
        h.update(r.tobytes()); h.update(b"|")
    h.update(np.array(starts, dtype=np.int64).tobytes()); h.update(np.array(cids, dtype=np.int64).tobytes())
    for b, t in zip(cut_b, cut_t):
        h.update(b"-" if b is None else b.tobytes() + t.astype(np.int32).tobytes()); h.update(b"|")
    assert h.hexdigest() == tfc.TOY_B_DIGEST
    loci, flanks = dg.true_loci(cfg), dg.true_flanks(cfg)
    assert len(loci) == cfg.copies == len(flanks)
    for (l, c, r), (fl, fr) in zip(loci, flanks):
        assert np.array_equal(l, fl) and np.array_equal(r, fr) and c.dtype == np.uint8 and abs(len(c) - cfg.repeat_len) < cfg.repeat_len // 10
    # a read of copy c that starts in the left flank begins with the bases the locus has there, up to the read's own errors:
    # the three parts lie side by side as the reads were drawn from them
    assert len({c.tobytes() for _, c, _ in loci}) == cfg.copies


def test_collapsed_assembly_holds_what_its_truth_says():
    from repeatresolver_amd import datagen as dg
    from repeatresolver_amd.strands import reverse_complement
    cfg = dg.CONFIGS["toy_a"]
    layouts = ["placed-", "bridge", "duplicated", "left_only"]
    contigs, truth = dg.collapsed_assembly(cfg, layouts, 40, 5)
    assert dg.collapsed_assembly(cfg, layouts, 40, 5)[0] == contigs and dg.collapsed_assembly(cfg, layouts, 40, 6)[0] != contigs
    assert [n for n, _ in contigs] == [f"contig{j}" for j in range(6)] and [t["layout"] for t in truth] == layouts
    text = lambda a: dg.ASCII[a].tobytes()
    template = text(dg.simulate_dataset(cfg)[0])
    for (left, _copy, right), t in zip(dg.true_loci(cfg), truth):
        for side, flank in (("left", text(left)), ("right", text(right))):
            if t[side] is None:
                assert not any(flank in s or reverse_complement(flank) in s for _, s in contigs)
                continue
            c, o, b = t[side]
            s = contigs[c][1] if o == 0 else reverse_complement(contigs[c][1])
            b = b if o == 0 else len(s) - b
            assert s[b - len(flank):b] == flank if side == "left" else s[b:b + len(flank)] == flank
            if t["layout"] != "bridge":
                assert (s[b:b + len(template)] if side == "left" else s[b - len(template):b]) == template
    h = len(template) // 2
    assert contigs[1][1].endswith(template[:h]) and contigs[2][1].startswith(template[h:]) and len(contigs[1][1]) == 40 + cfg.flank + h
    assert contigs[4][1].count(text(dg.true_loci(cfg)[2][0])) == 1 and truth[2]["left"][0] == 3 and truth[3]["right"] is None


# ---- the host C under the sanitizers, as a program of its own ----
def test_host_code_under_the_sanitizers(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no host C compiler")
    exe = tmp_path / "anchor_sanitize"
    cmd = [cc, "-std=c11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "anchor_sanitize_main.c"), os.path.join(ROOT, "repeatresolver_amd", "csrc", "pla_host.c"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("cannot find" in built.stderr or "unrecognized" in built.stderr or "unsupported" in built.stderr):
        pytest.skip("the host compiler has no sanitizer runtime")
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    if run.returncode != 0 and "runtime does not come first" in run.stderr:
        pytest.skip("another library is preloaded into every process here: the sanitizer runtime refuses to start behind it")
    assert run.returncode == 0, run.stdout + run.stderr
    assert "anchor_sanitize: ok" in run.stdout
