"""Flank consensus (include/pfl.h: pfl_place, the votes and the call, pfl_consensus), everything that needs no GPU: the checker
against a brute-force edit distance and hand-made cases of every rule, the host functions (pfl_call, the FASTA writer, the
refusals, join_loci, write_loci) against the checker and hand-made cases, datagen.true_flanks, and the accuracy a round of
consensus has on the checker alone."""
import ctypes
import functools
import hashlib
import itertools

import numpy as np
import pytest

import fc_checker as fc
import fl_checker as fl


def lib():
    from repeatresolver_amd import _lib
    return _lib.load()


def text(ops):
    """ops bytes as text: acgt a base, - a gap, . no vote, upper case where an insertion follows, then (x) the inserted base"""
    out = ""
    for o in ops:
        low, high = int(o) & 15, int(o) >> 4
        out += ".acgt-"[0 if low == 15 else 5 if low == 4 else low + 1] + (f"({'acgt'[high - 1]})" if high else "")
    return out


def one_block(P: bytes, T: bytes):
    """(ystar, d, steps as a string, ops as text) of one block of the checker"""
    p, t = fc.codes(P), fc.codes(T)
    D = fc.table(p, t)
    ystar = int(np.argmin(D[len(p)]))
    steps, ops = fc.trace(D, p, t, ystar)
    return ystar, int(D[len(p), ystar]), "".join(steps), text(ops)


# ---- the checker itself ----
def brute(P, T):
    """min over y of the edit distance of P and T[:y], by the textbook recursion"""
    @functools.lru_cache(maxsize=None)
    def lev(x, y):
        if x == 0 or y == 0:
            return x + y
        return min(lev(x - 1, y) + 1, lev(x, y - 1) + 1, lev(x - 1, y - 1) + (P[x - 1] != T[y - 1]))
    return min(lev(len(P), y) for y in range(len(T) + 1))


def test_checker_path_is_valid_and_optimal():
    """the path's cost, recounted step by step, is the brute-force distance; it ends at (0, 0); its ops are its steps"""
    seqs = [bytes(s) for n in range(1, 6) for s in itertools.product(b"ac", repeat=n)]
    rng = np.random.default_rng(7)
    pairs = [(p, t) for p in seqs for t in seqs + [b""]]
    pairs += [tuple(bytes(rng.choice(list(b"acgt"), size=rng.integers(1, 7)).astype(np.uint8)) for _ in range(2)) for _ in range(600)]
    for P, T in pairs:
        p, t = fc.codes(P), fc.codes(T)
        D = fc.table(p, t)
        assert int(D[len(p)].min()) == brute(P, T), (P, T)
        ystar = int(np.argmin(D[len(p)]))
        assert all(D[len(p), y] > D[len(p), ystar] for y in range(ystar))                   # the first of the minima
        steps, ops = fc.trace(D, p, t, ystar)
        x, y, cost, seen = len(p), ystar, 0, []
        for s in steps:
            if s == "u":
                x, cost = x - 1, cost + 1
                seen.append((x, fc.GAP))
            elif s == "l":
                y, cost = y - 1, cost + 1
            else:
                x, y = x - 1, y - 1
                cost += int(p[x] != t[y])
                seen.append((x, int(t[y])))
            assert x >= 0 and y >= 0
        assert (x, y) == (0, 0) and cost == brute(P, T), (P, T, steps)
        assert sorted(seen) == [(i, int(ops[i]) & 15) for i in range(len(p))]               # every position exactly one vote


def test_ties_put_the_gap_at_the_far_end():
    """a homopolymer with one base missing: every placement of the gap costs the same, "up first" takes it where the walk
    starts, at the block's far end -- for every member alike"""
    assert one_block(b"aaaa", b"aaa") == (3, 1, "uddd", "aaa-")
    assert one_block(b"caaaag", b"caaag") == (5, 1, "duddd" + "d", "caaa-g")
    assert one_block(b"caaaag", b"caaagt") == (5, 1, "duddd" + "d", "caaa-g")               # what follows does not move it
    # one base too many: the insertion stands behind the run's last base, again at the far end
    assert one_block(b"caaagt", b"caaaagt") == (7, 1, "ddldddd", "caaa(a)gt")


def test_insertion_nibble_and_the_ignored_leading_insertion():
    assert one_block(b"acgtacgt", b"acgttacgt") == (9, 1, "ddddldddd", "acgt(t)acgt")
    # two inserted bases: the nibble holds the FIRST of the run in the member, the last the walk meets
    assert one_block(b"acgtacgt", b"acgtgcacgt") == (10, 2, "ddddlldddd", "acgt(g)acgt")
    # a gap and an insertion never stand together on a traced path (up and left in a row cost 2, the diagonal at most 1): a
    # foreign base beside a missing one is a substitution and a gap, the gap at the far end of the tie
    assert one_block(b"aaccgg", b"aatgg") == (5, 2, "dduddd", "aat-gg")
    assert one_block(b"accctgg", b"acagg") == (5, 3, "dduuddd", "aca--gg")
    # in front of the block's first base: left steps at x = 0 vote for nothing
    assert one_block(b"cgta", b"acgta") == (5, 1, "ddddl", "cgta")
    assert one_block(b"cgta", b"ttcgta") == (6, 2, "ddddll", "cgta")


def test_ystar_is_the_first_minimum():
    assert one_block(b"ac", b"ag")[:2] == (1, 1)                                             # D(2,1) = D(2,2) = 1: y* = 1, a gap
    assert one_block(b"ac", b"ag")[3] == "a-"
    ops, blocks, used, dist, paths = fc.place(fc.codes(b"ac"), fc.codes(b"ag"), 2, 2, 1000)
    assert (blocks, used, dist) == (1, 1, 1) and text(ops) == "a-" and paths[0][0] == 1
    assert one_block(b"acgt", b"acgtacgt")[:2] == (4, 0)


def test_member_stops_at_max_permille_and_when_it_runs_out():
    B = fc.codes(b"acgtacgtacgt")
    M = fc.codes(b"acgttttt")
    ops, blocks, used, dist, _ = fc.place(B, M, 4, 12, 500)                                 # block 1: d = 3, 3000 > 2000
    assert (blocks, used, dist) == (1, 4, 0) and text(ops) == "acgt........"
    ops, blocks, used, dist, _ = fc.place(B, M, 4, 12, 750)                                 # 3000 > 3000 is false: it votes
    assert blocks == 2 and dist == 3 and text(ops)[8:] == "...." and text(ops)[4] != "."
    ops, blocks, used, dist, _ = fc.place(B, M, 4, 12, 749)
    assert blocks == 1
    ops, blocks, used, dist, _ = fc.place(B, fc.codes(b"acgtacg"), 4, 12, 1000)             # 3 bases left: |M| - s < block
    assert (blocks, used) == (1, 4) and text(ops) == "acgt........"
    ops, blocks, used, dist, _ = fc.place(B, fc.codes(b"acgtacgt"), 4, 12, 1000)            # exactly a block left, then none
    assert (blocks, used) == (2, 8) and text(ops) == "acgtacgt...."
    ops, blocks, used, dist, _ = fc.place(B, fc.codes(b"acgtacgtacgtacgt"), 4, 8, 1000)     # extent cuts the backbone
    assert blocks == 2 and len(ops) == 8
    ops, blocks, used, dist, _ = fc.place(B[:11], fc.codes(b"acgtacgtacgtacgt"), 4, 12, 1000)   # a partial last block is dropped
    assert blocks == 2 and len(ops) == 8


def test_the_call():
    def called(rows, min_depth=1):
        sym, ins, voters = fc.votes(np.array(rows, dtype=np.uint8))
        seq, depth = fc.call(sym, ins, voters, min_depth)
        return seq, depth.tolist()
    assert called([[0], [1]]) == (b"a", [2])                                                # a tie: the first of a c g t gap
    assert called([[3], [1], [1], [3]]) == (b"c", [4])
    assert called([[4], [2]]) == (b"g", [2])                                                # a base before the gap
    assert called([[4], [4], [2]]) == (b"", [])                                             # the gap wins: nothing is emitted
    assert called([[15], [2]]) == (b"g", [1])                                               # no vote is no voter
    assert called([[0x10 | 0], [0x10 | 0], [0], [0]]) == (b"a", [4])                        # 2 * 2 > 4 is false
    assert called([[0x10 | 0], [0x20 | 0], [0x20 | 0], [0]]) == (b"ac", [4, 4])             # 2 * 3 > 4: the first largest, c
    assert called([[0x40 | 4], [0x30 | 4], [1]]) == (b"g", [3])                             # gap, then the insertion: g before t
    rows = [[0, 1, 2, 3], [0, 1, 2, 15], [0, 1, 15, 15]]
    assert called(rows, 1) == (b"acgt", [3, 3, 2, 1]) and called(rows, 2) == (b"acg", [3, 3, 2]) and called(rows, 3) == (b"ac", [3, 3])
    assert called(rows, 4) == (b"", [])
    assert called([[15, 0], [15, 0]], 1) == (b"", [])                                       # it ends at the FIRST shallow position


def test_c_call_equals_the_checker():
    L = lib()
    rng = np.random.default_rng(3)
    pub = ctypes.POINTER(ctypes.c_ubyte)
    for _ in range(60):
        npos = int(rng.integers(0, 80))
        sym = rng.integers(0, 5, size=max(npos, 1)).astype(np.uint8)
        ins = rng.integers(0, 5, size=max(npos, 1)).astype(np.uint8)
        voters = rng.integers(0, 9, size=max(npos, 1)).astype(np.int32)
        for min_depth in (1, 3):
            seq = ctypes.create_string_buffer(2 * npos + 1)
            depth = np.zeros(2 * npos + 1, dtype=np.int32)
            got = L.pfl_call(npos, sym.ctypes.data_as(pub), ins.ctypes.data_as(pub), voters.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                             min_depth, ctypes.cast(seq, ctypes.c_char_p), depth.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
            e_seq, e_depth = fc.call(sym[:npos], ins[:npos], voters[:npos], min_depth)
            assert seq.raw[:got] == e_seq and depth[:got].tolist() == e_depth.tolist()


def test_header_and_loader_agree():
    import os
    from conftest import ROOT
    from repeatresolver_amd import _lib
    head = open(os.path.join(ROOT, "include", "pfl.h")).read()
    assert f"#define PFL_MAX_EXTENT {_lib.PFL_MAX_EXTENT} " in head
    for name in ("pfl_place", "pfl_consensus", "pfl_consensus_free", "pfl_consensus_pack", "pfl_call", "pfl_write_flank_fasta", "pfl_run_files_consensus",
                 "pfl_set_scratch_limit", "pfl_get_place_stats"):
        assert name in _lib.PFL_EXPORTS and f" {name}(" in head and getattr(lib(), name) is not None


# ---- refusals: all before the device is touched ----
def test_refusals_need_no_device():
    from repeatresolver_amd.flanks import FlankClusterer
    from repeatresolver_amd.realigner import PwrError
    ARG, INPUT, RANGE = -1, -4, -5
    pieces = [b"acgt" * 20, b"acgt" * 20, b"acgn" * 20]
    g = FlankClusterer()

    def place(piece=(0, 1), mode=(0, 0), cluster=(0, 0), backbones=(b"acgt" * 16,), **kw):
        args = dict(block=32, extent=64, max_permille=400)
        args.update(kw)
        with pytest.raises(PwrError) as e:
            g.place(pieces, list(piece), list(mode), list(cluster), list(backbones), **args)
        return e.value.code

    def cons(piece=(0, 1), mode=(0, 0), labels=(0, 0), **kw):
        args = dict(block=32, extent=64, max_permille=400, min_depth=1, rounds=1)
        args.update(kw)
        with pytest.raises(PwrError) as e:
            g.consensus(pieces, list(piece), list(mode), list(labels), **args)
        return e.value.code
    for f in (place, cons):
        for block in (31, 33, 16, 544, 1024):
            assert f(block=block, extent=2048) == RANGE
        assert f(extent=31) == RANGE and f(extent=8193) == RANGE and f(block=64, extent=63) == RANGE
        assert f(max_permille=-1) == ARG
        assert f(mode=(0, 4)) == ARG and f(mode=(-1, 0)) == ARG and f(piece=(0, -1)) == ARG
        assert f(piece=(0, 2)) == INPUT                                                     # a byte outside acgtACGT in a listed piece
    assert place(backbones=(b"acgt" * 8 + b"n",)) == INPUT                                  # and in a backbone, also past its last block
    assert cons(rounds=0) == RANGE and cons(min_depth=0) == ARG and cons(labels=(0, -2)) == ARG
    with pytest.raises(ValueError):
        g.place(pieces, [0, 1], [0, 0], [0, 1], [b"acgt" * 16], block=32, extent=64, max_permille=400)   # no backbone 1
    with pytest.raises(ValueError):
        g.place(pieces, [0, 1], [0], [0, 0], [b"acgt" * 16], block=32, extent=64, max_permille=400)
    with pytest.raises(ValueError):
        g.consensus(pieces, [0, 5], [0, 0], [0, 0], block=32, extent=64, max_permille=400, min_depth=1)
    # the raw entry: a cluster without a backbone, null pointers, a stride below the longest backbone's blocks
    L = lib()
    pi, pll, pub = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_ubyte)
    off = np.array([0, 80, 160], dtype=np.int64)
    boff = np.array([0, 64], dtype=np.int64)
    ints = lambda *v: np.array(v, dtype=np.int32)
    ops, three = np.zeros((2, 64), dtype=np.uint8), [np.zeros(2, dtype=np.int32) for _ in range(3)]

    def raw(cluster=(0, 0), stride=64, ctx=g._h, ops_p=ops.ctypes.data_as(pub), nb=1):
        return L.pfl_place(ctx, 2, pieces[0] + pieces[1], off.ctypes.data_as(pll), ints(0, 1).ctypes.data_as(pi), ints(0, 0).ctypes.data_as(pi),
                           ints(*cluster).ctypes.data_as(pi), nb, b"acgt" * 16, boff.ctypes.data_as(pll), 32, 64, 400, ops_p, stride,
                           *[t.ctypes.data_as(pi) for t in three])
    assert raw(cluster=(0, 1)) == ARG and raw(cluster=(-2, 0)) == ARG and raw(ctx=None) == ARG and raw(ops_p=None) == ARG
    assert raw(stride=63) == RANGE and raw(stride=-1) == RANGE and raw(nb=-1) == ARG
    res = __import__("repeatresolver_amd")._lib.PflConsensusResult()
    assert L.pfl_consensus(g._h, 0, None, None, None, None, None, 32, 64, 400, 1, 1, None) == ARG
    assert L.pfl_consensus(None, 0, None, None, None, None, None, 32, 64, 400, 1, 1, ctypes.byref(res)) == ARG and not res.label
    assert L.pfl_set_scratch_limit(None, 5) == ARG and L.pfl_get_place_stats(None, None, None, None) == ARG
    # what is valid and needs no device: no flank, no flank of a cluster, no member of a block's length
    ops, blocks, used, dist = g.place(pieces, [], [], [], [b"acgt" * 16], block=32, extent=64, max_permille=400)
    assert ops.shape == (0, 64) and blocks.shape == (0,)
    ops, blocks, used, dist = g.place(pieces, [0, 1], [0, 3], [-1, -1], [b"acgt" * 16], block=32, extent=64, max_permille=400)
    assert (ops == 15).all() and ops.shape == (2, 64) and not blocks.any() and not used.any() and not dist.any()
    got = g.consensus(pieces, [0, 1], [0, 0], [-1, -1], block=32, extent=64, max_permille=400, min_depth=1)
    assert got.labels.tolist() == [] and got.sequences == []
    got = g.consensus(pieces, [0, 1, 0], [0, 0, 1], [4, -1, 2], block=96, extent=128, max_permille=400, min_depth=1)   # 80 bases < block
    assert got.labels.tolist() == [2, 4] and got.members.tolist() == [0, 0] and got.backbone.tolist() == [-1, -1]
    assert got.sequences == [b"", b""] and [d.tolist() for d in got.depths] == [[], []]
    assert got.oriented("left") == {2: "", 4: ""}
    with pytest.raises(ValueError):
        got.oriented("middle")
    assert g.place_stats() == {"cells": 0, "place_ms": 0.0, "votes_ms": 0.0}
    g.close()


# ---- the FASTA writer and the loci ----
def hand_fc(labels, seqs, members=None):
    from repeatresolver_amd.flanks import FlankConsensus
    return FlankConsensus(np.array(labels, np.int32), np.array(members or [3] * len(labels), np.int32), np.zeros(len(labels), np.int32),
                          list(seqs), [np.full(len(s), 3, np.int32) for s in seqs])


def test_write_flank_fasta(tmp_path):
    from repeatresolver_amd import _lib
    L = lib()
    labels, members = (ctypes.c_int * 3)(0, 4, 11), (ctypes.c_int * 3)(7, 0, 2)
    off = (ctypes.c_longlong * 4)(0, 5, 5, 6)
    seq = ctypes.create_string_buffer(b"aacgtc")
    res = _lib.PflConsensusResult(3, labels, members, (ctypes.c_int * 3)(3, -1, 9), off, ctypes.cast(seq, ctypes.c_void_p), (ctypes.c_int * 6)())
    path = tmp_path / "x_FlankLeft.fasta"
    assert L.pfl_write_flank_fasta(str(path).encode(), b"left", ctypes.byref(res)) == 0
    assert path.read_text() == ">left_0 flanks=7 bases=5\nTGCAA\n>left_4 flanks=0 bases=0\n\n>left_11 flanks=2 bases=1\nC\n"
    assert L.pfl_write_flank_fasta(str(path).encode(), b"right", ctypes.byref(res)) == 0
    assert path.read_text() == ">right_0 flanks=7 bases=5\nAACGT\n>right_4 flanks=0 bases=0\n\n>right_11 flanks=2 bases=1\nC\n"
    assert L.pfl_write_flank_fasta(str(path).encode(), b"up", ctypes.byref(res)) == -1
    assert L.pfl_write_flank_fasta(str(tmp_path / "none" / "x").encode(), b"left", ctypes.byref(res)) == -8
    fcs = hand_fc([0, 4, 11], [b"aacgt", b"", b"c"])
    assert fcs.oriented("left") == {0: "TGCAA", 4: "", 11: "C"} and fcs.oriented("right") == {0: "AACGT", 4: "", 11: "C"}


def test_join_loci_and_write_loci(tmp_path):
    from repeatresolver_amd import resolution
    # six rows; the flank labellings in front and behind, two windows' labellings between them.  Copy A: rows 0 1 2, flanks 5
    # (left) and 2 (right); copy B: rows 3 4, left flank 1, but no right flank: its thread does not span; row 5 is nobody's
    left = [5, 5, -1, 1, 1, -1]
    win1 = [0, 0, 0, 1, 1, -1]
    win2 = [1, 1, 1, 0, 0, -1]
    right = [2, -1, 2, -1, -1, -1]
    threads = resolution.thread([left, win1, win2, right])
    lab = threads.labels()
    a, b = int(threads.row_thread[0]), int(threads.row_thread[3])
    assert lab.tolist() == [a, a, a, -1, -1, -1] and b >= 0 and b != a
    assert threads.first[a] == 0 and threads.last[a] == 3 and threads.last[b] == 2
    # the whole consensus by hand: part a over 8 columns (a column nobody covers: depth 0, code 0; a gap column), and, as if
    # somebody had asked for it, part b
    cons = np.array([[1, 2, 0, 4, 3, 3, 0, 1], [0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.uint8)
    depth = np.array([[3, 3, 0, 3, 2, 1, 3, 3], [2, 2, 2, 2, 2, 2, 2, 2]], dtype=np.int32)
    whole = resolution.Consensus(von=0, bis=7, part_label=np.array([a, b], np.int32), part_rows=np.array([3, 2], np.int32), consensus=cons,
                                 depth=depth, counts=None, selected=np.arange(8, dtype=np.int32), diff=np.zeros((2, 2), np.int32),
                                 diff_all=np.zeros((2, 2), np.int32))
    left_fc, right_fc = hand_fc([1, 5], [b"ttt", b"acg"]), hand_fc([2], [b"ggc"])
    loci = resolution.join_loci(threads, whole, left_fc, right_fc)
    assert len(loci) == 1                                                                   # b does not span: no locus
    l = loci[0]
    # the left flank is the anchored consensus reversed, not complemented; the depth-0 column is left out, the gap too
    assert l.sequence == "GCA" + "CGTTAC" + "GGC" and whole.sequences()[0] == b"CGATTAC"
    assert (l.thread, l.left_label, l.right_label, l.rows, l.left_len, l.copy_len, l.right_len) == (a, 5, 2, 3, 3, 6, 3)
    l2 = resolution.join_loci(threads, whole, left_fc, right_fc, min_depth=2)[0]
    assert l2.sequence == "GCA" + "CGTAC" + "GGC" and l2.copy_len == 5
    assert resolution.join_loci(threads, whole, left_fc, right_fc, min_depth=4)[0].sequence == "GCAGGC"
    none = resolution.join_loci(threads, whole, hand_fc([], []), right_fc)[0]              # a label without a consensus adds nothing
    assert none.sequence == "CGTTACGGC" and none.left_len == 0 and none.left_label == 5
    with pytest.raises(ValueError):
        resolution.join_loci(threads, whole, left_fc, right_fc, min_depth=0)
    resolution.write_loci(tmp_path / "loci.fasta", loci + [l2], "ds")
    assert (tmp_path / "loci.fasta").read_text() == (f">ds_locus{a} left=5:3 copy=6 right=2:3 rows=3\nGCACGTTACGGC\n"
                                                     f">ds_locus{a} left=5:3 copy=5 right=2:3 rows=3\nGCACGTACGGC\n")


# ---- the simulator's flanks ----
TOY_B_DIGEST = "925b05bf0508c9b926c7aa479ab292ad31568aaacbdc00eee73827e149dbc279"      # taken before true_flanks existed


def test_simulate_dataset_is_unchanged_and_true_flanks_are_its_flanks():
    from repeatresolver_amd import datagen as dg
    cfg = dg.CONFIGS["toy_b"]
    seq, full, starts, cids, cut_b, cut_t = dg.simulate_dataset(cfg)
    h = hashlib.sha256()
    h.update(seq.tobytes())
    for f in full:
        h.update(f.tobytes()); h.update(b"|")
    h.update(np.array(starts, dtype=np.int64).tobytes()); h.update(np.array(cids, dtype=np.int64).tobytes())
    for b, t in zip(cut_b, cut_t):
        h.update(b"-" if b is None else b.tobytes() + t.astype(np.int32).tobytes()); h.update(b"|")
    assert h.hexdigest() == TOY_B_DIGEST
    truth = dg.true_flanks(cfg)
    assert len(truth) == cfg.copies and all(len(l) == len(r) == cfg.flank and l.dtype == np.uint8 for l, r in truth)
    # every flank piece of the true cut lies within the same-copy rates of two READS (DESIGN 23's table: at most 345 per mille
    # at reach 256) of the true flank of its copy, which has no errors of its own
    pieces, piece_read, classes, copy = fl.true_flanks(cfg)
    nb = fl.neighbours(piece_read, classes)
    seen = 0
    for col, side in ((1, 0), (3, 1)):
        for r in nb:
            if r[col] < 0 or len(pieces[r[col]]) < 100:
                continue
            member = fl.anchored(pieces[r[col]], r[col + 1])
            m = min(len(member), 256)
            true = truth[copy[r[0]]][side]
            true = true[::-1] if side == 0 else true                                        # anchored: from the boundary outwards
            rate = 1000 * fl.anchored_distance(member[:m], true[:m + m // 4]) // m
            assert rate <= 345, (side, r, rate)
            seen += 1
    assert seen > 150


# ---- what a round of consensus is worth, on the checker alone ----
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_round_one_is_nearer_to_the_truth_than_every_member(seed):
    """a synthetic cluster of 12 members (the test owns the truth; the members are datagen.pacbio_error of prefixes of it), block
    128, min_depth 3: round 1's consensus is nearer to the truth per base than every member is.  DESIGN 25 records the rates."""
    from repeatresolver_amd import datagen as dg
    rng = np.random.default_rng([seed, 0xF1A])
    truth = rng.integers(0, 4, size=700, dtype=np.uint8)
    members = []
    for cut in [700] + rng.integers(300, 701, size=11).tolist():
        read, _ = dg.pacbio_error(rng, truth[:cut], np.arange(cut, dtype=np.int32))
        members.append(read)
    longest = max(range(12), key=lambda k: (len(members[k]), -k))
    seq, depth = fc.round_of(members, members[longest], 128, 1024, 400, 3)
    assert len(seq) >= 256 and depth.min() >= 3
    mine = fc.per_mille_to(truth, fc.codes(seq))
    theirs = [fc.per_mille_to(truth, m) for m in members]
    print(f"seed {seed}: consensus of {len(seq)} bases {mine:.1f} per mille; members {min(theirs):.1f} .. {max(theirs):.1f}")
    assert all(mine < t for t in theirs)
