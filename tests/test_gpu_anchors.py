"""-m gpu: pla_search on the device (k_la_search, k_la_collect in pla_device.hip) against tests/la_checker.py, every field of every
hit, no tolerance; place_loci and the drop-in's three files on a collapsed assembly of toy_b against its truth; the flank
consensus sequences of toy_b's reads searched in that assembly.

k_la_search is compiled per ceil(m / 32) (1 .. 16); a wave takes one job (pattern, orientation) and 64 chunks of the text, and a
chunk starts its table m + k columns early.  The shapes below straddle the word, the chunk, the contig and the cap of runs per
chunk; test_gpu_anchor_widths.py runs every one of the 16 instances."""
import functools

import numpy as np
import pytest

import la_checker as la

pytestmark = pytest.mark.gpu


def rand(rng, n, alphabet=b"acgt") -> bytes:
    return bytes(rng.choice(list(alphabet), size=n).astype(np.uint8))


def same(g, contigs, anchored, side, reach, min_len, permille, expected=None):
    got = g.search(anchored, side, max_permille=permille, reach=reach, min_len=min_len).rows()
    exp = la.search(contigs, anchored, side, reach, min_len, permille) if expected is None else expected
    assert len(got) == len(exp), (len(got), len(exp))
    bad = [(a, e) for a, e in zip(got, exp) if a != e]
    assert not bad, bad[:5]
    return exp


def edited(rng, seq: bytes, kind: str) -> bytes:
    """one edit in the middle third of seq"""
    at = len(seq) // 3 + int(rng.integers(0, max(len(seq) // 3, 1)))
    other = bytes([next(b for b in b"acgt" if b != seq[at])])
    return {"sub": seq[:at] + other + seq[at + 1:], "ins": seq[:at] + other + seq[at:], "del": seq[:at] + seq[at + 1:]}[kind]


@pytest.mark.parametrize("m", [1, 31, 32, 33, 63, 64, 65, 255, 256, 511, 512])
def test_planted_loci_in_contigs_of_every_kind(m):
    """one locus (left flank, a stretch of repeat, right flank), both its patterns in both orientations, against contigs of 0,
    1, m - 1 and m bases (the last being the left flank itself: an occurrence from the contig's first base to its last) and
    against longer ones that hold it exactly, reverse-complemented with a substitution, an insertion and a deletion in its
    flanks, cut by both ends of the contig, and with an N inside; at chunks of 32, 36 and 100 columns, so that the contigs of
    a few hundred bases span several lanes, contigs share a tile, runs straddle chunk edges (k > 0 from m = 31 on) and the
    occurrence at a contig's start has no room for its warm-up"""
    from repeatresolver_amd.anchors import LocusAnchorer
    from repeatresolver_amd.strands import reverse_complement
    rng = np.random.default_rng(m)
    a_left, a_right = rand(rng, m + 5), rand(rng, m + 9)                            # anchored, longer than the reach
    left, right, repeat = a_left[:m][::-1], a_right[:m], rand(rng, 20)              # as the template shows them
    noisy = edited(rng, left, "sub" if m < 8 else "ins") + repeat + edited(rng, edited(rng, right, "del" if m > 8 else "sub"), "sub")
    with_n = left[:m // 2] + b"N" + left[m // 2 + 1:] if m > 1 else b"N"
    contigs = [b"", b"a", rand(rng, m - 1), left,
               rand(rng, 50) + left + repeat + right + rand(rng, 37),
               reverse_complement(rand(rng, 61) + noisy + rand(rng, 45)),
               left[min(3, m - 1):] + repeat + right[:max(m - 4, 1)],
               rand(rng, 40) + with_n + repeat + right.upper() + rand(rng, 10) + b"NNNN"]
    anchored, side = [a_left, a_right], [0, 1]
    permille = 100
    with LocusAnchorer(contigs) as g:
        exp = None
        for chunk in (32, 36, 100):
            g.set_chunk(chunk)
            exp = same(g, contigs, anchored, side, m, 1, permille, exp)
    # the planted ones are there: the exact locus on contig 4 in +, the noisy one on contig 5 in - (from 3 edits in 31 bases on)
    L5 = len(contigs[5])
    if m >= 31:
        k = permille * m // 1000
        assert (0, 0, 4, 50 + m, 0) in [h[:4] + h[6:] for h in exp] and (1, 0, 4, 50 + m + 20, 0) in [h[:4] + h[6:] for h in exp]
        assert (0, 0, 3, m, 0) in [h[:4] + h[6:] for h in exp]
        mine = [h for h in exp if h[1] == 1 and h[2] == 5]
        assert {h[0] for h in mine} == {0, 1} and all(h[6] <= k for h in mine)
        assert any(h[0] == 0 and h[5] - h[4] >= 1 and h[4] <= L5 - 61 - (m + 1) <= h[5] for h in mine)   # a run wider than one column
        assert any(h[0] == 0 and h[2] == 7 and h[6] == 1 for h in exp)              # the N costs one edit and keeps its place


def test_max_permille_zero_and_short_patterns():
    from repeatresolver_amd.anchors import LocusAnchorer
    rng = np.random.default_rng(7)
    p = [rand(rng, 40), rand(rng, 99), rand(rng, 100), rand(rng, 300), b""]
    text = rand(rng, 100) + p[0][::-1] + rand(rng, 30) + p[1][::-1] + p[2][::-1] + rand(rng, 11) + p[3][:256][::-1] + rand(rng, 70)
    flawed = text[:300] + rand(rng, 1) + text[300:]                                 # a base too many inside p[2]'s occurrence
    with LocusAnchorer([text, flawed]) as g:
        g.set_chunk(64)
        exp = same(g, [text, flawed], p, [0] * 5, 256, 100, 0)
        assert [h[:3] + h[6:] for h in exp] == [(2, 0, 0, 0), (3, 0, 0, 0), (3, 0, 1, 0)]   # 40, 99 and 0 bases are short
        exp = same(g, [text, flawed], p, [0] * 5, 256, 1, 0)
        assert sorted({h[0] for h in exp}) == [0, 1, 2, 3]
        assert same(g, [text, flawed], [], [], 256, 1, 0) == []
        assert {h[0] for h in same(g, [text, flawed], p[:2], [1, 0], 30, 41, 0)} == {1}


def test_more_runs_in_a_chunk_than_the_cap():
    """("ac" * 16) in ("ac" * 200) at 0 per mille: every other column from 32 on ends an occurrence, 16 runs in a chunk of 32
    columns, four times the cap: every tile is run again with room"""
    from repeatresolver_amd import _lib
    from repeatresolver_amd.anchors import LocusAnchorer
    text, pattern = b"ac" * 200, (b"ac" * 16)[::-1]
    with LocusAnchorer([text, b"ac" * 9, text[1:]]) as g:
        for chunk in (32, 100):
            g.set_chunk(chunk)
            exp = same(g, [text, b"ac" * 9, text[1:]], [pattern], [0], 32, 1, 0)
        assert len([h for h in exp if h[1] == 0 and h[2] == 0]) == 185 > _lib.PLA_RUN_CAP * (400 // 100)
        assert all(h[4] == h[5] == h[3] for h in exp)


def test_two_searches_on_one_text_and_a_second_text():
    from repeatresolver_amd.anchors import LocusAnchorer
    rng = np.random.default_rng(9)
    a, b = rand(rng, 80), rand(rng, 120)
    one = [rand(rng, 500) + a[::-1] + rand(rng, 200), rand(rng, 90)]
    two = [rand(rng, 30), rand(rng, 77) + b + rand(rng, 900), a[::-1]]
    with LocusAnchorer(one) as g:
        g.set_chunk(128)
        first = same(g, one, [a], [0], 64, 1, 50)
        assert len(first) == 1 and len(same(g, one, [a, b], [0, 1], 100, 1, 50)) == 1
        assert same(g, one, [a], [0], 64, 1, 50) == first
        cells = g.stats()["cells"]
        assert cells == (64 + 80 + 100 + 64) * 2 * 870 and g.stats()["kernel_ms"] > 0
        g.open(two)
        got = same(g, two, [a, b], [0, 1], 100, 1, 50)
        assert [h[:4] for h in got] == [(0, 0, 2, 80), (1, 0, 1, 77)]
        g.open([])
        assert same(g, [], [a], [0], 64, 1, 50) == []


# ---- a collapsed assembly of toy_b ----
LAYOUTS = ["placed+", "placed-", "bridge", "left_only", "right_only", "none", "duplicated", "placed-", "placed+", "bridge"]
EXPECTED = {"placed+": "PLACED", "placed-": "PLACED", "bridge": "BRIDGE", "left_only": "LEFT_ONLY", "right_only": "RIGHT_ONLY",
            "none": "NONE", "duplicated": "AMBIGUOUS"}
SEARCH = dict(max_permille=50, reach=256, min_len=100)


@functools.lru_cache(maxsize=None)
def assembly(layouts=tuple(LAYOUTS)):
    from repeatresolver_amd import datagen as dg
    return dg.collapsed_assembly(dg.CONFIGS["toy_b"], list(layouts), 300, 21)


@functools.lru_cache(maxsize=None)
def edited_loci():
    """toy_b's true loci as resolution.Locus objects, three substitutions planted in the searched part of every flank, at least
    16 bases from the boundary: the true end of the flank stays the first column of the minimum"""
    from repeatresolver_amd import datagen as dg
    from repeatresolver_amd.resolution import Locus
    rng = np.random.default_rng(22)
    out = []
    for t, (left, copy, right) in enumerate(dg.true_loci(dg.CONFIGS["toy_b"])):
        left, right = left.copy(), right.copy()
        for at in rng.choice(np.arange(16, 250), size=3, replace=False):
            left[len(left) - 1 - at] = (left[len(left) - 1 - at] + 1) % 4
            right[at] = (right[at] + 2) % 4
        text = [dg.ASCII[a].tobytes().decode().upper() for a in (left, copy, right)]
        out.append(Locus(thread=t, left_label=t, right_label=t, rows=9, left_len=len(text[0]), copy_len=len(text[1]), right_len=len(text[2]),
                         sequence="".join(text)))
    return out


def test_place_loci_on_a_collapsed_assembly_against_the_truth_and_the_drop_in(tmp_path):
    from repeatresolver_amd import anchors, datagen as dg
    from repeatresolver_amd.resolution import write_loci
    contigs, truth = assembly()
    assert set(LAYOUTS) == set(dg.LAYOUTS)
    loci = edited_loci()
    hits, placements = anchors.place_loci(loci, contigs, max_span=5000, **SEARCH)
    anchored, side, lp, rp = anchors.locus_patterns(loci)
    exp = la.search([s for _, s in contigs], anchored, side, SEARCH["reach"], SEARCH["min_len"], SEARCH["max_permille"])
    assert hits.rows() == exp
    template_len = len(dg.simulate_dataset(dg.CONFIGS["toy_b"])[0])
    for p, t in zip(placements, truth):
        assert p.name == EXPECTED[t["layout"]], (p, t)
        for s in ("left", "right"):
            got = tuple(getattr(p, f"{s}_{f}") for f in ("contig", "orientation", "boundary"))
            if t[s] is None or (t["layout"] == "duplicated" and s == "left"):
                assert got == (-1, -1, -1)
            else:
                assert got == t[s] and getattr(p, f"{s}_distance") == 3
        if p.name == "PLACED":
            assert p.span == template_len == p.hi - p.lo
    assert placements[6].left_hits == 2
    # the drop-in, from the files alone
    names = [f"toy_locus{l.thread}" for l in loci]
    copies = [l.sequence[l.left_len:l.left_len + l.copy_len] for l in loci]
    write_loci(tmp_path / "loci.fasta", loci, "toy")
    (tmp_path / "asm.fasta").write_bytes(b"".join(b">%s a contig\n" % n.encode() + b"".join(s[x:x + 70] + b"\n" for x in range(0, len(s), 70))
                                                 for n, s in contigs))
    code, out = anchors.run_files("loci.fasta", "asm.fasta", SEARCH["max_permille"], 5000, reach=SEARCH["reach"], min_len=SEARCH["min_len"],
                                  prefix="out", cwd=tmp_path)
    assert code == 0, out
    assert (tmp_path / "out_Anchors").read_text() == anchors.anchor_lines(hits, names, contigs)
    anchors.write_placements(tmp_path / "py_Placements", names, placements, contigs)
    anchors.write_patched(tmp_path / "py_Patched.fasta", contigs, placements, copies)
    assert (tmp_path / "out_Placements").read_bytes() == (tmp_path / "py_Placements").read_bytes()
    assert (tmp_path / "out_Patched.fasta").read_bytes() == (tmp_path / "py_Patched.fasta").read_bytes()
    patched = anchors.patch(contigs, placements, copies)
    assert (tmp_path / "py_Patched.fasta").read_bytes() == b"".join(b">%s patched=%d\n%s\n" % (n.encode(), k, s) for n, s, k in patched)
    # a patched contig holds the copy, not the template: placed+ as it is, placed- reverse-complemented
    from repeatresolver_amd.strands import reverse_complement
    assert [k for _, _, k in patched] == [1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0]
    assert copies[0].encode() in patched[0][1] and reverse_complement(copies[1].encode()) in patched[1][1]
    assert "PLACED 4" in out and "BRIDGE 2" in out and "AMBIGUOUS 1" in out


def test_flank_consensus_of_the_reads_searched_in_the_assembly():
    """flank_sequences on toy_b as tests/test_gpu_flank_consensus.py obtains them, at reach 128 in an assembly that holds every
    copy once (+ and - alternating): the device equals the checker, every hit lies on the contig and in the orientation of
    its cluster's true copy (the majority of its rows), and no cluster hits twice.  How many clusters hit and how far the
    boundary lies from the true one is printed, not asserted (DESIGN 26 records it)."""
    import fl_checker as fl
    from repeatresolver_amd.anchors import LocusAnchorer
    from repeatresolver_amd import datagen as dg
    from test_gpu_flank_consensus import toy_b
    cfg, pieces, piece_read, classes, left, right, fcs = toy_b()
    contigs, truth = assembly(tuple("placed+" if c % 2 == 0 else "placed-" for c in range(cfg.copies)))
    cids = dg.simulate_dataset(cfg)[3]
    nb = fl.neighbours(piece_read, classes)
    anchored, side, copy_of = [], [], []
    for s, (labels, fc_) in enumerate(((left, fcs[0]), (right, fcs[1]))):
        for label, seq in zip(fc_.labels, fc_.sequences):
            rows = [t for t in range(len(nb)) if labels[t] == label]
            votes = np.bincount([cids[piece_read[nb[t][0]]] for t in rows], minlength=cfg.copies)
            anchored.append(seq); side.append(s); copy_of.append(int(votes.argmax()))
    with LocusAnchorer(contigs) as g:
        exp = same(g, [s for _, s in contigs], anchored, side, 128, 100, 100)
    seen = set()
    for p, o, c, b, lo, hi, d in exp:
        want = truth[copy_of[p]]["left" if side[p] == 0 else "right"]
        assert (c, o) == want[:2], (p, o, c, want)
        assert p not in seen
        seen.add(p)
        print(f"pattern {p} side {side[p]} copy {copy_of[p]} bases {len(anchored[p])}: boundary {b} true {want[2]} offset {b - want[2]} "
              f"run {lo}..{hi} distance {d}")
    searched = sum(len(a) >= 100 for a in anchored)
    print(f"clusters {len(anchored)}, searched {searched}, hit {len(seen)}")


def test_pipeline_anchored():
    """pipeline.anchored on the synthetic MSA of test_gpu_flank_consensus.py's pipeline.loci case, with flank sequences made
    here and an assembly that holds every copy's two flanks around a stand-in of 50 bases, every other one reverse-complemented:
    loci's nine values, then the hits and placements of place_loci on those loci"""
    from repeatresolver_amd import anchors, pipeline
    from repeatresolver_amd.flanks import FlankConsensus
    from repeatresolver_amd.strands import reverse_complement
    from test_gpu_resolve import COV, ragged
    rows = ragged()
    rng = np.random.default_rng(31)
    kw = dict(parts=3, cov=COV, min_compared=10, min_margin=3, max_iter=8)
    copy = pipeline.threaded(rows, min_side=5, **kw)[6].labels()
    left = np.array([10 + c if c >= 0 and r[:1] != b" " else -1 for c, r in zip(copy, rows)], dtype=np.int32)
    right = np.array([20 + c if c >= 0 and r[-1:] != b" " else -1 for c, r in zip(copy, rows)], dtype=np.int32)

    def hand(labels):
        names = sorted(set(labels[labels >= 0].tolist()))
        return FlankConsensus(np.array(names, np.int32), np.array([3] * len(names), np.int32), np.array([0] * len(names), np.int32),
                              [rand(rng, 120) for _ in names], [np.full(120, 3, np.int32) for _ in names])
    left_fc, right_fc = hand(left), hand(right)
    lefts, rights = left_fc.oriented("left"), right_fc.oriented("right")
    copies = sorted({l - 10 for l in lefts} & {r - 20 for r in rights})
    contigs = []
    for c in copies:
        s = rand(rng, 70 + c) + lefts[10 + c].lower().encode() + rand(rng, 50) + rights[20 + c].lower().encode() + rand(rng, 90)
        contigs.append((f"copy{c}", reverse_complement(s) if c % 2 else s))
    out = pipeline.anchored(rows, left, right, left_fc, right_fc, contigs, anchor_permille=20, max_span=60, reach=100, min_len=100, **kw)
    assert len(out) == 11
    loci, hits, placements = out[8], out[9], out[10]
    assert len(loci) >= 2 and len(placements) == len(loci)
    again_hits, again = anchors.place_loci(loci, contigs, max_permille=20, max_span=60, reach=100, min_len=100)
    assert hits.rows() == again_hits.rows() and placements == again
    for l, p in zip(loci, placements):
        c = l.left_label - 10
        assert l.right_label == 20 + c and p.name == "PLACED" and p.span == 50 and p.left_distance == p.right_distance == 0
        assert (p.left_contig, p.left_orientation) == (copies.index(c), c % 2)
        assert p.left_boundary == (90 + 120 + 50 if c % 2 else 70 + c + 120)
