"""-m gpu: the placements with traceback and the consensus of pfl_device.hip (k_fl_place, k_fl_votes) against
tests/fc_checker.py, every byte and every integer, no tolerance; flank_sequences and the drop-in's -c on toy_b; pipeline.loci.

k_fl_place is compiled per block / 32 (1 .. 16), a wave takes one backbone and 64 of its members and walks the backbone's
blocks; a member's text in a block has between block and block + block / 4 bases.  The lengths below straddle the block, the
slack, the extent and the 64-member tile; two letters make the ties the traceback's preference decides.
test_gpu_flank_place_widths.py runs every one of the 16 instances."""
import functools

import numpy as np
import pytest

import fc_checker as fc
from test_gpu_flanks import noisy, turned

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    from repeatresolver_amd.flanks import FlankClusterer
    h = FlankClusterer()
    yield h
    h.close()


def rand(rng, n, alphabet=b"acgt") -> bytes:
    return bytes(rng.choice(list(alphabet), size=n).astype(np.uint8))


def compare_place(g, pieces, piece, mode, cluster, backbones, block, extent, max_permille):
    got = g.place(pieces, piece, mode, cluster, backbones, block=block, extent=extent, max_permille=max_permille)
    exp = fc.place_all(pieces, piece, mode, cluster, backbones, block, extent, max_permille)
    for name, a, e in zip(("blocks", "used", "dist"), got[1:], exp[1:]):
        assert a.tolist() == e.tolist(), name
    assert got[0].shape == exp[0].shape
    bad = np.argwhere(got[0] != exp[0])
    assert len(bad) == 0, (bad[:5].tolist(), [(int(got[0][i, j]), int(exp[0][i, j])) for i, j in bad[:5]])
    return got


@pytest.mark.parametrize("block", [32, 64, 96, 256, 512])
def test_backbone_lengths_and_member_remainders(g, block):
    """five backbones in one call: block - 1 bases (nothing is used), block, block + 1, 2 * block and 2 * block + 31; of each,
    exact and noisy members whose remainder in front of the second block is block - 1 (it stops), block, block + 1, the whole
    slack and one more"""
    rng = np.random.default_rng(block)
    backbones = [rand(rng, n) for n in (block - 1, block, block + 1, 2 * block, 2 * block + 31)]
    source = [b + rand(rng, 2 * block) for b in backbones]
    pieces, cluster = [], []
    for j, s in enumerate(source):
        for rest in (block - 1, block, block + 1, block + block // 4, block + block // 4 + 1):
            pieces.append(s[:block + rest]); cluster.append(j)
            pieces.append(noisy(rng, s[:block + rest + 8], rate=0.1)); cluster.append(j)
    n = len(pieces)
    ops, blocks, used, dist = compare_place(g, pieces, list(range(n)), [0] * n, cluster, backbones, block, 4 * block, 400)
    assert blocks[:10].tolist() == [0] * 10                             # the backbone of block - 1 bases has no block
    assert blocks[30] == 1 and blocks[32] == 2 and used[32] == 2 * block and dist[32] == 0
    assert (ops[32, :2 * block] < 4).all() and (ops[30, block:] == 15).all()


@pytest.mark.parametrize("alphabet", [b"ac", b"acg", b"acgt"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
def test_member_counts_across_the_tile_and_alphabets(g, n, alphabet):
    rng = np.random.default_rng(n * 7 + len(alphabet))
    block = 32 if n > 65 else 64
    truth = rand(rng, 3 * block, alphabet)
    pieces = [noisy(rng, truth, rate=0.15, alphabet=alphabet) for _ in range(n)]
    pieces = [p if len(p) >= block else truth for p in pieces]
    compare_place(g, pieces, list(range(n)), [0] * n, [0] * n, [truth[:2 * block + 5]], block, 8 * block, 500)


def test_three_backbones_in_one_call_and_no_cluster(g):
    """members of three backbones interleaved, some of them of no cluster: those are not placed"""
    rng = np.random.default_rng(3)
    block = 64
    truths = [rand(rng, 4 * block) for _ in range(3)]
    pieces, cluster = [], []
    for k in range(150):
        j = k % 4 - 1
        pieces.append(noisy(rng, truths[max(j, 0)], rate=0.12)); cluster.append(j)
    ops, blocks, used, dist = compare_place(g, pieces, list(range(150)), [0] * 150, cluster, [t[:3 * block + k] for k, t in enumerate(truths)],
                                            block, 8 * block, 400)
    out = np.array(cluster) < 0
    assert (ops[out] == 15).all() and not blocks[out].any() and not used[out].any() and (blocks[~out] == 3).sum() > 80


def test_extent_cuts_the_backbone(g):
    rng = np.random.default_rng(4)
    block = 64
    truth = rand(rng, 5 * block)
    pieces = [noisy(rng, truth, rate=0.1) for _ in range(9)]
    for extent in (block, block + block // 2, 2 * block, 3 * block + 63):
        ops, blocks, _used, _dist = compare_place(g, pieces, list(range(9)), [0] * 9, [0] * 9, [truth], block, extent, 400)
        assert ops.shape[1] == extent // block * block and blocks.max() == extent // block


def test_identical_deleted_inserted_and_turning_random(g):
    """identical members (no gap, no insertion), a member that lacks the second block, one with a block inserted in front of
    it and one with a foreign block in its place: all three stop there at 200 per mille, their votes of the first block kept; a
    member that turns random from its second block on likewise; at 1000 per mille nobody stops"""
    rng = np.random.default_rng(5)
    block = 96
    truth = rand(rng, 4 * block)
    gone = truth[:block] + truth[2 * block:]
    inserted = truth[:block] + rand(rng, block) + truth[block:]
    foreign = truth[:block] + rand(rng, block) + truth[2 * block:]
    wild = truth[:block] + rand(rng, 3 * block)
    pieces = [p + rand(rng, 2 * block) for p in (truth, truth, truth, gone, inserted, foreign, wild)]   # (nobody runs out of bases)
    ops, blocks, used, dist = compare_place(g, pieces, list(range(7)), [0] * 7, [0] * 7, [truth], block, 4 * block, 200)
    assert blocks.tolist() == [4, 4, 4, 1, 1, 1, 1] and dist[:3].tolist() == [0, 0, 0] and used[3:].tolist() == [block] * 4
    assert (ops[:3] < 4).all() and (ops[3:, :block] < 4).all() and (ops[3:, block:] == 15).all()
    ops, blocks, _used, _dist = compare_place(g, pieces, list(range(7)), [0] * 7, [0] * 7, [truth], block, 4 * block, 1000)
    assert blocks.tolist() == [4] * 7 and (ops != 15).all()


def test_modes_equal_mode_zero_on_turned_sequences(g):
    rng = np.random.default_rng(6)
    block = 64
    truth = rand(rng, 3 * block + 20)
    anchored = [noisy(rng, truth, rate=0.12) for _ in range(40)]
    base = compare_place(g, anchored, list(range(40)), [0] * 40, [0] * 40, [truth], block, 4 * block, 400)
    mode = [k % 4 for k in range(40)]
    got = compare_place(g, [turned(p, m) for p, m in zip(anchored, mode)], list(range(40)), mode, [0] * 40, [truth], block, 4 * block, 400)
    for a, b in zip(base, got):
        assert np.array_equal(a, b)


def test_two_ranges_of_members():
    """a scratch limit below one tile: every tile of 64 members is a range (a launch) of its own"""
    from repeatresolver_amd.flanks import FlankClusterer
    rng = np.random.default_rng(8)
    block = 64
    truth = rand(rng, 3 * block)
    pieces = [noisy(rng, truth, rate=0.12) for _ in range(130)]
    with FlankClusterer() as h:
        h.set_scratch_limit(1)
        small = compare_place(h, pieces, list(range(130)), [0] * 130, [0] * 130, [truth], block, 4 * block, 400)
        h.set_scratch_limit(0)
        whole = h.place(pieces, list(range(130)), [0] * 130, [0] * 130, [truth], block=block, extent=4 * block, max_permille=400)
        for a, b in zip(small, whole):
            assert np.array_equal(a, b)
        assert h.place_stats()["cells"] == 2 * int(small[1].sum()) * block * (block + block // 4)


# ---- pfl_consensus ----
def clusters(seed=11, block=64, alphabet=b"acgt"):
    """flanks of four labels, the labels 0, 3, 7 and 9: noisy prefixes of three truths; label 7's flanks are all shorter than
    the block (a cluster without a member); a few flanks of label -1; the modes vary"""
    rng = np.random.default_rng(seed)
    truths = {0: rand(rng, 6 * block + 10, alphabet), 3: rand(rng, 5 * block, alphabet), 9: rand(rng, 4 * block + 3, alphabet)}
    pieces, mode, labels = [], [], []
    for name, size in ((0, 14), (3, 9), (9, 5)):
        for k in range(size):
            cut = int(rng.integers(block // 2, len(truths[name]) + 1))
            m = int(rng.integers(0, 4))
            pieces.append(turned(noisy(rng, truths[name][:cut], rate=0.12, alphabet=alphabet), m)); mode.append(m); labels.append(name)
    for k in range(3):
        pieces.append(rand(rng, block - 1 - k, alphabet)); mode.append(0); labels.append(7)
        pieces.append(rand(rng, 3 * block, alphabet)); mode.append(1); labels.append(-1)
    order = rng.permutation(len(pieces))
    return [pieces[k] for k in order], [mode[k] for k in order], [labels[k] for k in order], truths


def same_consensus(got, exp):
    assert got.labels.tolist() == exp[0] and got.members.tolist() == exp[1] and got.backbone.tolist() == exp[2]
    assert got.sequences == exp[3]
    for a, e in zip(got.depths, exp[4]):
        assert a.tolist() == e.tolist()


@pytest.mark.parametrize("min_depth", [1, 3])
@pytest.mark.parametrize("rounds", [1, 2, 3])
def test_consensus_rounds_against_the_checker(g, rounds, min_depth):
    pieces, mode, labels, _ = clusters()
    n = len(pieces)
    got = g.consensus(pieces, list(range(n)), mode, labels, block=64, extent=512, max_permille=400, min_depth=min_depth, rounds=rounds)
    exp = fc.consensus(pieces, list(range(n)), mode, labels, 64, 512, 400, min_depth, rounds)
    same_consensus(got, exp)
    assert got.labels.tolist() == [0, 3, 7, 9] and got.members[2] == 0 and got.backbone[2] == -1 and got.sequences[2] == b""
    assert len(got.sequences[0]) > 128 and len(got.sequences[1]) > 128


def test_round_two_is_place_against_round_one(g):
    pieces, mode, labels, _ = clusters(seed=12, alphabet=b"ac")
    n = len(pieces)
    kw = dict(block=64, extent=512, max_permille=500)
    one = g.consensus(pieces, list(range(n)), mode, labels, min_depth=2, rounds=1, **kw)
    two = g.consensus(pieces, list(range(n)), mode, labels, min_depth=2, rounds=2, **kw)
    same_consensus(two, fc.consensus(pieces, list(range(n)), mode, labels, 64, 512, 500, 2, 2))
    index = {int(l): j for j, l in enumerate(one.labels)}
    cluster = [index[l] if l >= 0 and len(p) >= 64 else -1 for l, p in zip(labels, pieces)]
    ops, _blocks, _used, _dist = g.place(pieces, list(range(n)), mode, cluster, one.sequences, **kw)
    for j, seq in enumerate(one.sequences):
        if len(seq) < 64:
            assert two.sequences[j] == seq
            continue
        rows = ops[np.array(cluster) == j][:, :len(seq) // 64 * 64]
        seq2, depth2 = fc.call(*fc.votes(rows), 2)
        assert two.sequences[j] == seq2 and two.depths[j].tolist() == depth2.tolist()


# ---- the toy chain ----
TOY = dict(block=128, extent=640, max_permille=400, min_depth=3, rounds=2)


@functools.lru_cache(maxsize=None)
def toy_b():
    from repeatresolver_amd import datagen as dg
    from repeatresolver_amd import flanks, pipeline
    cfg = dg.CONFIGS["toy_b"]
    rows, info, left, right = pipeline.flank_labels(cfg, parts=50, max_permille=400)
    pieces, piece_read, classes = info["pieces_list"], info["piece_read"], info["classes"]
    return cfg, pieces, piece_read, classes, left, right, flanks.flank_sequences(pieces, piece_read, classes, None, left, right, **TOY)


def test_flank_sequences_of_toy_b_against_the_checker_and_the_truth():
    """ReadCutter's own cuts and FlankClusterer's own labels: the consensus of every cluster is the checker's, and every
    consensus that has a base is nearer to the true flank of its members' copy than the member it started from was over the
    same number of bases.  Nothing is left out but the empty ones, which have no distance; one of fewer bases than a block may
    tie (a handful of bases can stand at 0 errors on both sides).  COMPARED and EMPTY pin how many there are of each."""
    from repeatresolver_amd import datagen as dg
    cfg, pieces, piece_read, classes, left, right, fcs = toy_b()
    import fl_checker as fl
    nb = fl.neighbours(piece_read, classes)
    truth = dg.true_flanks(cfg)
    _seq, _full, _starts, cids, _cut, _ = dg.simulate_dataset(cfg)
    compared, empty, worse = 0, 0, []
    for side, col, labels, got in (("left", 1, left, fcs[0]), ("right", 3, right, fcs[1])):
        have = [t for t, r in enumerate(nb) if r[col] >= 0]
        piece, mode, lab = [nb[t][col] for t in have], [nb[t][col + 1] for t in have], [int(labels[t]) for t in have]
        same_consensus(got, fc.consensus(pieces, piece, mode, lab, TOY["block"], TOY["extent"], TOY["max_permille"], TOY["min_depth"],
                                         TOY["rounds"]))
        for j, k in enumerate(got.backbone):
            n = len(got.sequences[j])
            if n == 0:
                empty += 1
                print(f"{side} cluster {int(got.labels[j])}: {int(got.members[j])} members, no consensus")
                continue
            copy = cids[piece_read[piece[k]]]
            true = truth[copy][0][::-1] if side == "left" else truth[copy][1]      # anchored: from the boundary outwards
            start = fl.anchored(pieces[piece[k]], mode[k])[:n]
            a, b = fc.per_mille_to(true, fc.codes(got.sequences[j])), fc.per_mille_to(true, start)
            print(f"{side} cluster {int(got.labels[j])}: {int(got.members[j])} members, {n} bases, consensus {a:.0f} per mille, "
                  f"backbone member {b:.0f}")
            compared += 1
            if not (a < b or (n < TOY["block"] and a <= b)):
                worse.append((side, int(got.labels[j]), n, a, b))
    assert not worse, worse
    assert (compared, empty) == (COMPARED, EMPTY)


COMPARED, EMPTY = 20, 1                                                 # toy_b's flank clusters with a consensus and without


def test_drop_in_writes_the_sequences_of_the_api(tmp_path):
    from repeatresolver_amd import flanks
    _cfg, pieces, piece_read, classes, _left, _right, (left_fc, right_fc) = toy_b()
    nreads = int(max(piece_read)) + 1
    (tmp_path / "ds_Seq.fasta").write_bytes(b"".join(b">\n" + p + b"\n" for p in pieces))
    (tmp_path / "ds_ReadSeqInfo").write_text("".join("".join(f"{k} " for k in range(len(piece_read)) if piece_read[k] == r) + "\n"
                                                     for r in range(nreads)))
    (tmp_path / "ds_SeqClass").write_text("".join(c + "\n" for c in classes))
    code, out = flanks.run_files("ds_Seq.fasta", "ds_ReadSeqInfo", "ds_SeqClass", 400, cwd=tmp_path, extent=TOY["extent"], block=TOY["block"],
                                 min_depth=TOY["min_depth"], rounds=TOY["rounds"])
    assert code == 0, out
    for side, res in (("left", left_fc), ("right", right_fc)):
        want = "".join(f">{side}_{int(l)} flanks={int(m)} bases={len(s)}\n{s}\n"
                       for l, m, s in zip(res.labels, res.members, (res.oriented(side)[int(l)] for l in res.labels)))
        assert (tmp_path / f"ds_Flank{side.capitalize()}.fasta").read_text() == want
        assert len(res.labels) >= 4
    code, out = flanks.run_files("ds_Seq.fasta", "ds_ReadSeqInfo", "ds_SeqClass", 400, prefix="plain", cwd=tmp_path)
    assert code == 0 and not (tmp_path / "plain_FlankLeft.fasta").exists() and (tmp_path / "plain_FlankingLeft").exists()


# ---- whole loci ----
def test_pipeline_loci():
    """the synthetic MSA of test_gpu_cross.py's pipeline.threaded case.  Its generator hands out no truth, so the flank
    labellings are derived from the whole copies `threaded` finds: a row that reaches the MSA's first (last) column carries
    its copy as left (right) label."""
    from repeatresolver_amd import pipeline, resolution
    from repeatresolver_amd.flanks import FlankConsensus
    from repeatresolver_amd.max_correlation import max_correlations
    from test_gpu_resolve import COV, ragged
    rows = ragged()
    kw = dict(parts=3, cov=COV, min_compared=10, min_margin=3, max_iter=8)
    plain = pipeline.threaded(rows, min_side=5, **kw)
    copy = plain[6].labels()
    left = np.array([10 + c if c >= 0 and r[:1] != b" " else -1 for c, r in zip(copy, rows)], dtype=np.int32)
    right = np.array([20 + c if c >= 0 and r[-1:] != b" " else -1 for c, r in zip(copy, rows)], dtype=np.int32)
    assert len(set(left[left >= 0].tolist())) >= 2 and len(set(right[right >= 0].tolist())) >= 2

    def hand(labels, tag):
        names = sorted(set(labels[labels >= 0].tolist()))
        return FlankConsensus(np.array(names, np.int32), np.array([3] * len(names), np.int32), np.array([0] * len(names), np.int32),
                              [(tag + b"acg" * (2 + n % 5)) for n in names], [np.full(len(tag) + 3 * (2 + n % 5), 3, np.int32) for n in names])
    left_fc, right_fc = hand(left, b"tt"), hand(right, b"gg")
    out = pipeline.loci(rows, left, right, left_fc, right_fc, **kw)
    assert len(out) == 9
    for a, b in zip(out[4], plain[4]):
        assert np.array_equal(a.labels, b.labels)                       # settled as `threaded` settles
    threads, whole, loci = out[6], out[7], out[8]
    exp_threads = resolution.thread([left] + [s.labels for s in out[4]] + [right])
    assert np.array_equal(threads.thread_of, exp_threads.thread_of) and np.array_equal(threads.row_thread, exp_threads.row_thread)
    mc = max_correlations(rows, COV)
    with resolution.open_msa(rows) as msa:
        exp_whole = resolution.consensus(msa, exp_threads.labels(), None, None, mc, min(w.cutoff for w in out[1]))
    assert np.array_equal(whole.consensus, exp_whole.consensus) and np.array_equal(whole.depth, exp_whole.depth)
    assert whole.von == 0 and whole.bis == len(rows[0]) - 1
    assert loci == resolution.join_loci(exp_threads, exp_whole, left_fc, right_fc, 1) and len(loci) >= 2
    for l in loci:
        assert l.sequence.startswith(left_fc.oriented("left")[l.left_label]) and l.sequence.endswith(right_fc.oriented("right")[l.right_label])
        assert l.left_label - 10 == l.right_label - 20 and l.copy_len > 500
