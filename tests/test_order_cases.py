"""CPU, oracle only: the preconditions of test_gpu_commit_two_launches.py hold on the MSA of order_cases.py.

Rows realigned one by one, W_Con (pwo_compact) after each.  A realignment is STRUCTURAL if it opens a column (any
pwo_dbg_newins) or empties one (the width after compaction is not the width before plus the columns opened); its position
is the column of the row's first base (pwo_dbg_way[0]).  Among consecutive structural realignments the jumps of more than
1 000 columns are counted, to the right and to the left.  Measured: round 1 has 127 structural realignments of 129, 50
jumps to the right and 49 to the left; two rounds 250, 97 and 96.  The bounds below are conditions on the input, not
tolerances: far fewer would mean the GPU test no longer alternates."""
import numpy as np

import order_cases as oc


def _structural_positions(oracle, rounds):
    """per round: the positions of the structural realignments, in the order of the k loop"""
    rows = oc.alternating_rows()
    lib = oracle.lib
    h = oracle.create(rows, oc.BANDWIDTH)
    lib.pwo_trim(h)
    lib.pwo_compact(h)
    out = []
    for _ in range(rounds):
        pos = []
        for k in range(len(rows)):
            w0 = lib.pwo_width(h)
            assert lib.pwo_realign_row(h, k) == 0
            L = lib.pwo_dbg_L(h)
            if L <= 0:
                continue
            nins = int(np.ctypeslib.as_array(lib.pwo_dbg_newins(h), (L,)).astype(np.int64).sum())
            way0 = int(lib.pwo_dbg_way(h)[0])
            lib.pwo_compact(h)
            if nins > 0 or lib.pwo_width(h) != w0 + nins:
                pos.append(way0)
        out.append(pos)
    lib.pwo_destroy(h)
    return rows, out


def _jumps(pos):
    d = np.diff(np.asarray(pos, dtype=np.int64))
    return int((d > oc.JUMP).sum()), int((d < -oc.JUMP).sum())


def test_the_k_loop_alternates_between_the_ends(oracle):
    rows, per_round = _structural_positions(oracle, oc.ROUNDS)
    assert (len(rows), len(rows[0])) == (129, 5659)
    spans = []                                                      # columns from a row's first base to its last
    for r in rows:
        at = np.flatnonzero(np.frombuffer(r, dtype=np.uint8) != ord("-"))
        spans.append(int(at[-1] - at[0]))
    assert (min(spans), max(spans)) == (121, 1602)
    right1, left1 = _jumps(per_round[0])
    both = [p for r in per_round for p in r]
    right2, left2 = _jumps(both)
    print(f"round 1: {len(per_round[0])} structural realignments of {len(rows)}, {right1} jumps right, {left1} left; "
          f"{oc.ROUNDS} rounds: {len(both)} structural, {right2} / {left2} jumps")
    assert len(per_round[0]) >= 120
    assert right1 >= 40 and left1 >= 40
