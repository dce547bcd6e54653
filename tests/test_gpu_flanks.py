"""-m gpu: the flank distances of pfl_device.hip against tests/fl_checker.py, entry for entry (integers, no tolerance), the
labellings that come out of them, the drop-in and RepeatResolver's -l / -r.

The kernel is compiled per number of 32-row pattern words (1 .. 16), a wave takes one pattern and 64 texts, and a text has
between m and m + m / 4 bases: the lengths below straddle the word boundaries, the reach, the end of the text's slack and the
64-text tile; flanks of equal a are ordered by their index.  test_gpu_kernel_widths.py runs every one of the 16 word counts,
each at the first and the last pattern length of its word."""
import numpy as np
import pytest

import fl_checker as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    from repeatresolver_amd.flanks import FlankClusterer
    h = FlankClusterer()
    yield h
    h.close()


def noisy(rng, base: bytes, rate=0.12, alphabet=b"acgt") -> bytes:
    out = bytearray()
    for ch in base:
        r = rng.random()
        if r < rate / 3:
            continue                                                    # deletion
        out.append(int(rng.choice(list(alphabet))) if r < 2 * rate / 3 else ch)
        if rng.random() < rate / 3:
            out.append(int(rng.choice(list(alphabet))))                 # insertion
    return bytes(out) or base[:1]


def family(rng, lengths, alphabet=b"acgt", parents=3):
    """one flank per length: noisy copies of a few parents (near and far pairs), cut to the length"""
    longest = max(lengths) + 64
    roots = [bytes(rng.choice(list(alphabet), size=longest).astype(np.uint8)) for _ in range(parents)]
    out = []
    for k, n in enumerate(lengths):
        s = noisy(rng, roots[k % parents], alphabet=alphabet)
        while len(s) < n:
            s += s
        out.append(s[:n])
    return out


def turned(piece: bytes, mode: int) -> bytes:
    """the piece whose mode-0 reading is `piece` read in `mode`"""
    s = piece[::-1] if mode & 1 else piece
    return s.translate(bytes.maketrans(b"acgtACGT", b"tgcaTGCA")) if mode & 2 else s


def compare(g, pieces, piece, mode, reach, min_len):
    lens, dist = g.distances(pieces, piece, mode, reach, min_len)
    a, exp = fc.distances(pieces, piece, mode, reach, min_len)
    assert lens.tolist() == [len(pieces[p]) for p in piece]
    assert np.minimum(lens, reach).tolist() == a.tolist()
    bad = np.argwhere(dist != exp)
    assert len(bad) == 0, (bad[:5].tolist(), [(int(dist[i, j]), int(exp[i, j])) for i, j in bad[:5]])
    return dist


@pytest.mark.parametrize("reach", [32, 33, 256, 512])
def test_lengths_across_every_boundary(g, reach):
    rng = np.random.default_rng(reach)
    wide = reach + reach // 4
    lengths = [1, 31, 32, 33, 63, 64, 65, reach - 1, reach, reach + 1, wide - 1, wide, wide + 1, 2 * reach + 7, reach, reach, 33, 33]
    if reach == 512:
        lengths += [700, 255, 256, 257, 480, 481, 511]
    pieces = family(rng, lengths)
    mode = rng.integers(0, 4, size=len(pieces)).tolist()
    compare(g, pieces, list(range(len(pieces))), mode, reach, 1)


@pytest.mark.parametrize("n,alphabet", [(1, b"acgt"), (2, b"ac"), (63, b"a"), (64, b"acgt"), (65, b"ac"), (130, b"acgt"), (130, b"a")])
def test_flank_counts_across_the_tile_and_alphabets(g, n, alphabet):
    rng = np.random.default_rng(n * 7 + len(alphabet))
    lengths = rng.integers(20, 400, size=n).tolist()
    lengths[0] = 300
    if n > 2:
        lengths[1] = lengths[2] = 77                                    # equal a below the reach: the index decides who is the pattern
    pieces = family(rng, lengths, alphabet)
    mode = rng.integers(0, 4, size=n).tolist()
    order = rng.permutation(n).tolist()                                 # flank k is not piece k
    compare(g, pieces, order, mode, 256, 20)                            # none is short: n flanks are n sorted positions


def test_identical_deleted_and_inserted_blocks(g):
    rng = np.random.default_rng(9)
    s = bytes(rng.choice(list(b"acgt"), size=400).astype(np.uint8))
    pat = s[:200]
    deleted = s[:170] + s[185:400]                                      # the pattern's rows 170 .. 184 are missing from the text
    inserted = s[:100] + bytes(rng.choice(list(b"acgt"), size=10).astype(np.uint8)) + s[100:195]   # 205 bases: the text ends before the pattern does
    exact = s[:200]                                                     # len_j == m: the text has no slack
    longer = s[:200] + bytes(rng.choice(list(b"acgt"), size=3000).astype(np.uint8))      # len_j far above m + m / 4
    pieces = [pat, pat, deleted, inserted, exact, longer]
    dist = compare(g, pieces, list(range(6)), [0] * 6, 200, 100)
    assert dist[0, 1] == 0 and dist[0, 4] == 0 and dist[0, 5] == 0
    row = fc._last_rows(fc.anchored(pat, 0), fc.anchored(deleted, 0)[:250].reshape(1, -1))[0]
    assert row.argmin() == 185 and row.min() == 15 and row[200:].min() > 15    # the minimum lies left of column m
    assert dist[0, 2] == 15
    row = fc._last_rows(fc.anchored(pat, 0), fc.anchored(inserted, 0).reshape(1, -1))[0]
    assert len(inserted) == 205 and row.argmin() == len(inserted) and (row[:-1] > row[-1]).all()   # the minimum lies at |T|
    assert dist[0, 3] == row[-1]


@pytest.mark.parametrize("min_len", [99, 100])
def test_min_len_marks_short_flanks(g, min_len):
    rng = np.random.default_rng(4)
    pieces = family(rng, [99, 100, 101, 150, 99, 260])
    dist = compare(g, pieces, list(range(6)), [0, 1, 2, 3, 0, 1], 256, min_len)
    short = [0, 4] if min_len == 100 else []
    for k in range(6):
        assert (dist[k, k] == -1) == (k in short)
        assert ((dist[k] == -1).all() and (dist[:, k] == -1).all()) if k in short else (dist[k, [j for j in range(6) if j not in short]] >= 0).all()


def test_modes_equal_mode_zero_on_turned_sequences(g):
    rng = np.random.default_rng(6)
    pieces = family(rng, [120, 256, 257, 300, 190, 64, 330, 256, 95, 500, 33, 280])
    n = len(pieces)
    mode = [k % 4 for k in range(n)]
    assert sorted(set(mode)) == [0, 1, 2, 3]
    got = compare(g, pieces, list(range(n)), mode, 256, 30)
    plain = [turned(p, m) for p, m in zip(pieces, mode)]
    assert [bytes(b"acgt"[c] for c in fc.anchored(p, m)) for p, m in zip(pieces, mode)] == plain
    _lens, base = g.distances(plain, list(range(n)), [0] * n, 256, 30)
    assert (got == base).all()
    for m in (1, 2, 3):                                                 # and every flank in the same mode
        _lens, d = g.distances([turned(p, m) for p in plain], list(range(n)), [m] * n, 256, 30)
        assert (d == base).all(), m
    upper = [p.upper() if k % 2 else p for k, p in enumerate(pieces)]   # either case
    _lens, d = g.distances(upper, list(range(n)), mode, 256, 30)
    assert (d == got).all()


def test_an_invalid_byte_counts_only_in_a_listed_piece(g):
    from repeatresolver_amd.realigner import PwrError
    rng = np.random.default_rng(8)
    pieces = family(rng, [150, 160, 170])
    pieces[1] = pieces[1][:155] + b"n" + pieces[1][156:]                # past the reach of any distance, still refused
    with pytest.raises(PwrError) as e:
        g.distances(pieces, [0, 1, 2], [0, 0, 0], 100, 50)
    assert e.value.code == -4
    compare(g, pieces, [0, 2], [0, 1], 100, 50)
    compare(g, pieces, [2, 0], [3, 2], 100, 50)


def test_stats_count_the_cells_of_the_tables(g):
    from repeatresolver_amd.flanks import FlankClusterer
    rng = np.random.default_rng(10)
    lengths = [40, 100, 101, 130, 300, 20]
    pieces = family(rng, lengths)
    with FlankClusterer() as h:
        h.distances(pieces, list(range(6)), [0] * 6, 100, 30)
        st = h.stats()
        kept = sorted(min(n, 100) for n in lengths if n >= 30)
        order = sorted((min(n, 100), k) for k, n in enumerate(lengths) if n >= 30)
        cells = sum(m * min(lengths[j], m + m // 4) for p, (m, _i) in enumerate(order) for _a, j in order[p + 1:])
        assert kept == [40, 100, 100, 100, 100] and st["cells"] == cells and st["kernel_ms"] > 0
        h.distances(pieces, list(range(6)), [0] * 6, 100, 30)           # the buffers of the context are reused
        assert h.stats()["cells"] == 2 * cells


@pytest.mark.parametrize("side", ["left", "right"])
def test_toy_b_true_cut_every_pair_and_the_copies(g, side):
    from repeatresolver_amd.flanks import cluster
    pieces, piece, mode, copy, a, exp = fc.truth_case("toy_b", side)
    lens, dist = g.distances(pieces, piece, mode, 256, 100)
    assert np.minimum(lens, 256).tolist() == a.tolist() and (dist == exp).all()
    label = cluster(a, dist, 400)
    kept = [k for k in range(len(piece)) if lens[k] >= 100]
    copies_of = {}
    for k in kept:
        copies_of.setdefault(int(label[k]), set()).add(copy[k])
    assert -1 not in copies_of and all(len(v) == 1 for v in copies_of.values())
    assert len(copies_of) == len({copy[k] for k in kept}) == 10


@pytest.mark.parametrize("both_strands", [False, True])
def test_toy_b_through_the_pipeline(both_strands):
    """ReadCutter's own cuts: the labels are the checker's on the same pieces, no component holds two copies, and every copy
    with two or more flanks of min_len on a side has a labelled row there.  parts = 50: ReadCutter cuts a repeat's right end
    where its last template piece ends, at parts * (T // parts), so with the default 60 parts toy_b's 4000-base template
    leaves its last 40 bases on every right flank, a start all copies share; 50 divides 4000."""
    from repeatresolver_amd import datagen as dg
    from repeatresolver_amd import pipeline
    cfg = dg.CONFIGS["toy_b"]
    assert cfg.repeat_len % 50 == 0
    rows, info, left, right = pipeline.flank_labels(cfg, parts=50, both_strands=both_strands, max_permille=400)
    pieces, piece_read, classes = info["pieces_list"], info["piece_read"], info["classes"]
    strands = info.get("strands")
    assert (strands is not None) == both_strands
    assert len(left) == len(right) == len(rows) == classes.count("r") and len(pieces) == len(piece_read) == len(classes)
    _seq, full, _starts, cids, _cut, _ = dg.simulate_dataset(cfg)
    assert int(piece_read.max()) + 1 == len(full)                       # one read per record of the reads file
    print(f"both_strands={both_strands}: {len(pieces)} pieces of {len(full)} reads")
    for k, p in enumerate(pieces):                                      # a piece lies in the read it is said to lie in (the last
        if piece_read[k] < len(full) - 2 and len(p) >= 20:              # two records are written from the reference's own buffer)
            assert p in dg.ASCII[full[piece_read[k]]].tobytes(), k
    nb = fc.neighbours(piece_read, classes, strands)
    assert len(nb) == len(rows)
    for got, col in ((left, 1), (right, 3)):
        have = [t for t, r in enumerate(nb) if r[col] >= 0]
        a, dist = fc.distances(pieces, [nb[t][col] for t in have], [nb[t][col + 1] for t in have], 256, 100)
        exp = np.full(len(rows), -1, dtype=np.int32)
        exp[have] = fc.cluster(a, dist, 400)
        assert got.tolist() == exp.tolist()
        copy_of_row = [cids[piece_read[r[0]]] for r in nb]
        copies_of, long_flanks = {}, {}
        for k, t in enumerate(have):
            if dist[k, k] == 0:
                long_flanks[copy_of_row[t]] = long_flanks.get(copy_of_row[t], 0) + 1
            if got[t] >= 0:
                copies_of.setdefault(int(got[t]), set()).add(copy_of_row[t])
        print(f"both_strands={both_strands} side={col}: {len(have)} flanks, {sum(long_flanks.values())} of min_len, "
              f"{len(copies_of)} components, {len(long_flanks)} copies with a flank")
        assert all(len(v) == 1 for v in copies_of.values())
        labelled = set().union(*copies_of.values()) if copies_of else set()
        assert all(c in labelled for c, k in long_flanks.items() if k >= 2)
        assert len(long_flanks) >= 8                                    # (the test is about something: most of the 10 copies)


def test_drop_in_writes_the_labels_of_the_api(tmp_path):
    from repeatresolver_amd import datagen as dg
    from repeatresolver_amd import flanks
    pieces, piece_read, classes, _copy = fc.true_flanks(dg.CONFIGS["toy_a"])
    rng = np.random.default_rng(12)
    strands = rng.integers(0, 2, size=len(pieces)).tolist()
    ncut = np.bincount(piece_read, minlength=max(piece_read) + 1) - 1
    assert (ncut >= 0).all()
    (tmp_path / "ds_Seq.fasta").write_bytes(b"".join(b">\n" + p + b"\n" for p in pieces))
    (tmp_path / "ds_ReadSeqInfo").write_text("".join("".join(f"{k} " for k in range(len(piece_read)) if piece_read[k] == r) + "\n"
                                                     for r in range(len(ncut))))
    (tmp_path / "ds_SeqClass").write_text("".join(c + "\n" for c in classes))
    (tmp_path / "ds_Strands").write_text("".join("-\n" if s else "+\n" for s in strands))
    for st, st_path, prefix in ((None, None, None), (strands, "ds_Strands", "turned")):
        code, out = flanks.run_files("ds_Seq.fasta", "ds_ReadSeqInfo", "ds_SeqClass", 400, strands_path=st_path, prefix=prefix,
                                     cwd=tmp_path)
        assert code == 0, out
        left, right = flanks.flank_labels(pieces, piece_read, classes, st, max_permille=400)
        name = prefix or "ds"
        assert (tmp_path / f"{name}_FlankingLeft").read_text() == "".join(f"{v}\n" for v in left)
        assert (tmp_path / f"{name}_FlankingRight").read_text() == "".join(f"{v}\n" for v in right)
        nb = fc.neighbours(piece_read, classes, st)
        for got, col in ((left, 1), (right, 3)):
            have = [t for t, r in enumerate(nb) if r[col] >= 0]
            a, dist = fc.distances(pieces, [nb[t][col] for t in have], [nb[t][col + 1] for t in have], 256, 100)
            exp = np.full(len(nb), -1, dtype=np.int32)
            exp[have] = fc.cluster(a, dist, 400)
            assert got.tolist() == exp.tolist() and (got >= 0).sum() >= 4
    code, out = flanks.run_files("ds_Seq.fasta", "ds_ReadSeqInfo", "ds_SeqClass", 400, min_len=60, reach=64, min_size=2, prefix="opt",
                                 cwd=tmp_path)
    assert code == 0, out
    left, right = flanks.flank_labels(pieces, piece_read, classes, max_permille=400, reach=64, min_len=60, min_size=2)
    assert (tmp_path / "opt_FlankingLeft").read_text() == "".join(f"{v}\n" for v in left)
    assert (tmp_path / "opt_FlankingRight").read_text() == "".join(f"{v}\n" for v in right)
    (tmp_path / "short_SeqClass").write_text("".join(c + "\n" for c in classes[:-1]))
    code, out = flanks.run_files("ds_Seq.fasta", "ds_ReadSeqInfo", "short_SeqClass", 400, prefix="bad", cwd=tmp_path)
    assert code == 1 and not (tmp_path / "bad_FlankingLeft").exists()
    # a ReadSeqInfo that lists one piece for the last read, as ReadCutter writes it: the last read takes the rest.  (The data
    # set up to the last read that has more than one piece.)
    end = max(k for k in range(1, len(pieces)) if piece_read[k] == piece_read[k - 1]) + 1
    pieces, piece_read, classes = pieces[:end], piece_read[:end], classes[:end]
    mine = [k for k in range(end) if piece_read[k] == piece_read[end - 1]]
    assert len(mine) >= 2 and "r" in [classes[k] for k in mine]
    (tmp_path / "t_Seq.fasta").write_bytes(b"".join(b">\n" + p + b"\n" for p in pieces))
    (tmp_path / "t_SeqClass").write_text("".join(c + "\n" for c in classes))
    lines = (tmp_path / "ds_ReadSeqInfo").read_text().splitlines()[:piece_read[end - 1]]
    (tmp_path / "t_ReadSeqInfo").write_text("".join(l + "\n" for l in lines) + f"{mine[0]} \n")
    code, out = flanks.run_files("t_Seq.fasta", "t_ReadSeqInfo", "t_SeqClass", 400, prefix="tail", cwd=tmp_path)
    assert code == 0 and f"the last read takes the other {len(mine) - 1}" in out, out
    left, right = flanks.flank_labels(pieces, piece_read, classes, max_permille=400)
    assert (tmp_path / "tail_FlankingLeft").read_text() == "".join(f"{v}\n" for v in left)
    assert (tmp_path / "tail_FlankingRight").read_text() == "".join(f"{v}\n" for v in right)


def test_repeat_resolver_connects_flank_to_flank(tmp_path):
    """-w with -l and -r: ConnectionsOf_ is connect([left] + windows + [right]); without the two flags it is connect(windows),
    the file test_gpu_resolve.py pins"""
    from repeatresolver_amd.resolution import connect
    from test_gpu_resolve import CLI, COV, SITES, label_files, ragged, run, write_inputs
    rows = len(ragged())
    rng = np.random.default_rng(14)
    left = rng.integers(-1, 5, size=rows).astype(np.int32)
    right = rng.integers(-1, 7, size=rows).astype(np.int32)
    plain, flanked = tmp_path / "plain", tmp_path / "flanked"
    write_inputs(plain, True)
    write_inputs(flanked, True)
    (flanked / "ds_FlankingLeft").write_text("".join(f"{v}\n" for v in left))
    (flanked / "ds_FlankingRight").write_text("".join(f"{v}\n" for v in right))
    args = [CLI, "MSA", "-c", str(COV), "-w"] + [str(s) for s in SITES]
    p = run(args, plain)
    q = run(args + ["-l", "ds_FlankingLeft", "-r", "ds_FlankingRight"], flanked)
    assert p.returncode == 0 and q.returncode == 0, p.stdout + q.stdout
    assert label_files(plain) == label_files(flanked) and len(label_files(plain)) == 9
    windows = [np.array(label_files(plain)[f"KmeansSubdivisionOf_{a}_{b}_MSA"].split(), dtype=np.int32)
               for a, b in zip(SITES[:-1], SITES[1:])]

    def parsed(path):
        text = path.read_text().splitlines()
        return text[0].split(), np.array([[float(v) for v in l.split(" ")] for l in text[1:]])
    for d, con in ((plain, connect(windows)), (flanked, connect([left] + windows + [right]))):
        head, m = parsed(d / "ConnectionsOf_100_850_MSA")
        assert head == [str(con.matrix.shape[0]), str(con.matrix.shape[1])]
        assert m.shape == con.matrix.shape and np.abs(m - con.matrix).max() <= 5e-7      # %f: six decimals
    assert "Flanking" not in p.stdout                                   # without the flags: a run that knows nothing of flanks
    (flanked / "cut_FlankingLeft").write_text("".join(f"{v}\n" for v in left[:-1]))
    bad = run(args + ["-l", "cut_FlankingLeft", "-r", "ds_FlankingRight"], flanked)
    assert bad.returncode == 1 and "cut_FlankingLeft" in bad.stdout
