"""Checker for the flank consensus (include/pfl.h: pfl_place, the votes and the call, pfl_consensus): a literal restatement
of its semantics in numpy.  Every block's DP table is computed in full, over integers, and the traceback reads that table;
there is no bit vector here and nothing is shared with the C code.

  table(P, T)                                 D(0 .. |P|, 0 .. |T|), D(0, y) = y, D(x, 0) = x, unit costs
  trace(D, P, T, ystar)                       the path from (|P|, ystar) to (0, 0) as a list of 'u' / 'l' / 'd' steps, and its ops
  place(B, M, block, extent, max_permille)    one member against one backbone -> (ops, blocks, used, dist, paths)
  place_all(pieces, piece, mode, cluster, backbones, ...)   pfl_place's outputs
  votes(rows)                                 sym, ins, voters of the members' ops rows
  call(sym, ins, voters, min_depth)           (sequence as lower-case bytes, depths)
  consensus(pieces, piece, mode, labels, ...) pfl_consensus: (labels, members, backbone, sequences, depths)
"""
import numpy as np

from fl_checker import anchored, anchored_distance

NO_VOTE = 15
GAP = 4
LETTERS = b"acgt"


def codes(seq: bytes) -> np.ndarray:
    return anchored(seq, 0)


def table(P, T) -> np.ndarray:
    """the whole table, one row at a time: vertical and diagonal predecessors first, then the horizontal one as a running
    minimum of (value - column) + column"""
    P, T = np.asarray(P, dtype=np.uint8), np.asarray(T, dtype=np.uint8)
    m, n = len(P), len(T)
    idx = np.arange(n + 1, dtype=np.int64)
    D = np.zeros((m + 1, n + 1), dtype=np.int64)
    D[0] = idx
    for x in range(1, m + 1):
        tmp = np.empty(n + 1, dtype=np.int64)
        tmp[0] = x
        tmp[1:] = np.minimum(D[x - 1, 1:] + 1, D[x - 1, :-1] + (T != P[x - 1]))
        D[x] = np.minimum.accumulate(tmp - idx) + idx
    return D


def trace(D, P, T, ystar):
    """up if x > 0 and D(x,y) = D(x-1,y) + 1; else left if y > 0 and D(x,y) = D(x,y-1) + 1; else diagonal.  Returns the steps in
    the order they are taken (from the end of the alignment to its start) and the m ops bytes."""
    m = len(P)
    ops = np.full(m, NO_VOTE, dtype=np.uint8)
    high = np.zeros(m, dtype=np.uint8)
    x, y, steps = m, ystar, []
    while x > 0 or y > 0:
        if x > 0 and D[x, y] == D[x - 1, y] + 1:
            steps.append("u")
            ops[x - 1] = GAP
            x -= 1
        elif y > 0 and D[x, y] == D[x, y - 1] + 1:
            steps.append("l")
            if x > 0:                                   # member base y - 1 follows backbone position x - 1; the run's first
                high[x - 1] = 1 + int(T[y - 1])         # base in the member is the last one this walk meets
            y -= 1
        else:
            steps.append("d")
            ops[x - 1] = int(T[y - 1])
            x -= 1
            y -= 1
    return steps, ops | (high << 4)


def place(B, M, block, extent, max_permille):
    """B, M: codes.  Returns (ops over the used positions, blocks voted, bases consumed, summed d, [(ystar, steps)] per
    voted block)."""
    B, M = np.asarray(B, dtype=np.uint8), np.asarray(M, dtype=np.uint8)
    nb = min(len(B), extent) // block
    ops = np.full(nb * block, NO_VOTE, dtype=np.uint8)
    s = blocks = dist = 0
    paths = []
    for b in range(nb):
        if len(M) - s < block:
            break
        m = block
        P = B[b * block:(b + 1) * block]
        T = M[s:s + min(len(M) - s, m + m // 4)]
        D = table(P, T)
        last = D[m]
        ystar = int(np.argmin(last))                    # (argmin: the first of the minima)
        d = int(last[ystar])
        if 1000 * d > max_permille * m:
            break
        steps, o = trace(D, P, T, ystar)
        ops[b * block:(b + 1) * block] = o
        paths.append((ystar, steps))
        s += ystar
        blocks += 1
        dist += d
    return ops, blocks, s, dist, paths


def place_all(pieces, piece, mode, cluster, backbones, block, extent, max_permille):
    """pfl_place: (ops [n, stride], blocks, used, dist), stride = the used bases of the longest backbone"""
    n = len(piece)
    stride = max([min(len(b), extent) // block * block for b in backbones] + [0])
    ops = np.full((n, stride), NO_VOTE, dtype=np.uint8)
    out = np.zeros((3, n), dtype=np.int32)
    bb = [codes(b) for b in backbones]
    for k in range(n):
        if cluster[k] < 0:
            continue
        o, out[0, k], out[1, k], out[2, k], _ = place(bb[cluster[k]], anchored(pieces[piece[k]], mode[k]), block, extent, max_permille)
        ops[k, :len(o)] = o
    return ops, out[0], out[1], out[2]


def votes(rows):
    """rows: [members, positions] ops bytes.  sym: the first largest of the counts of a c g t gap; ins: 1 + the first largest
    inserted base where 2 * insertions > voters, else 0."""
    rows = np.asarray(rows, dtype=np.uint8).reshape(len(rows), -1)
    npos = rows.shape[1]
    sym, ins, voters = np.zeros(npos, np.uint8), np.zeros(npos, np.uint8), np.zeros(npos, np.int32)
    for i in range(npos):
        low = [int(v) & 15 for v in rows[:, i]]
        high = [int(v) >> 4 for v in rows[:, i]]
        count = [low.count(c) for c in range(5)]
        voters[i] = sum(count)
        sym[i] = count.index(max(count))
        icount = [high.count(1 + c) for c in range(4)]
        if 2 * sum(icount) > voters[i]:
            ins[i] = 1 + icount.index(max(icount))
    return sym, ins, voters


def call(sym, ins, voters, min_depth):
    seq, depth = bytearray(), []
    for i in range(len(sym)):
        if voters[i] < min_depth:
            break
        if sym[i] < 4:
            seq.append(LETTERS[sym[i]])
            depth.append(int(voters[i]))
        if ins[i]:
            seq.append(LETTERS[ins[i] - 1])
            depth.append(int(voters[i]))
    return bytes(seq), np.array(depth, dtype=np.int32)


def round_of(members, B, block, extent, max_permille, min_depth):
    """one round of one cluster: members (codes) against the backbone B (codes) -> (sequence, depths)"""
    rows = [place(B, M, block, extent, max_permille)[0] for M in members]
    return call(*votes(rows), min_depth)


def consensus(pieces, piece, mode, labels, block, extent, max_permille, min_depth, rounds, every_round=False):
    """pfl_consensus: (labels, members, backbone, sequences, depths); every_round: sequences[j] is the list of all rounds'"""
    names = sorted({int(l) for l in labels if l >= 0})
    out = ([], [], [], [], [])
    for name in names:
        ks = [k for k in range(len(piece)) if labels[k] == name and len(pieces[piece[k]]) >= block]
        out[0].append(name)
        out[1].append(len(ks))
        if not ks:
            out[2].append(-1); out[3].append([] if every_round else b""); out[4].append(np.zeros(0, np.int32))
            continue
        longest = max(len(pieces[piece[k]]) for k in ks)
        first = [k for k in ks if len(pieces[piece[k]]) == longest][0]
        members = [anchored(pieces[piece[k]], mode[k]) for k in ks]
        B = anchored(pieces[piece[first]], mode[first])
        history = []
        for _ in range(rounds):
            seq, depth = round_of(members, B, block, extent, max_permille, min_depth)
            history.append(seq)
            if len(seq) < block:
                break
            B = codes(seq)
        out[2].append(first); out[3].append(history if every_round else seq); out[4].append(depth)
    return out


def per_mille_to(truth, seq):
    """the anchored distance of seq (as the pattern) to truth per 1000 bases of seq, both codes; what the accuracy conditions
    compare.  truth is cut to |seq| + |seq| / 4 as every text is."""
    seq, truth = np.asarray(seq, dtype=np.uint8), np.asarray(truth, dtype=np.uint8)
    if len(seq) == 0:
        return None
    T = truth[:len(seq) + len(seq) // 4]
    return 1000.0 * anchored_distance(seq, T) / len(seq)
