"""An MSA whose k loop alternates between the two ends of the width (helper of test_order_cases.py and
test_gpu_commit_two_launches.py).

The commit keeps two buffers of the column order and renumbers from one into the other: the buffer it writes holds the
state of two restructuring commits ago, valid only as far as Hdr::agree says.  What that can get wrong needs consecutive
commits that open or empty columns and whose first changed ordinal jumps back and forth across the width: a copy that
starts at this commit's first change instead of min(first, agree) leaves the stretch the commit before changed, far to
the left, as it was two commits ago.  The rows of a simulated MSA are sorted by the column of their first base and taken
leftmost, rightmost, second leftmost, second rightmost, ...: nearly every realignment of the first rounds opens or empties
a column (test_order_cases.py counts them), near its row, so the first change alternates between the ends."""
import numpy as np

from repeatresolver_amd import datagen as dg

CFG = dg.SimConfig(kind="Tree", copies=3, coverage=4, difference=0.01, repeat_len=3000, flank=500,
                   length_scale=0.03, min_aligned=60, seed=31)
BANDWIDTH = 100
ROUNDS = 2
JUMP = 1000                                    # columns between two consecutive structural realignments that count as a jump

_rows = None


def alternating_rows():
    """the MSA's rows (bytes of equal length), reordered; computed once"""
    global _rows
    if _rows is None:
        msa = dg.build_msa(dg.simulate(CFG))
        first = np.argmax(msa != dg.GAP, axis=1)                 # column of every row's first base (no row is empty)
        assert (msa != dg.GAP).any(axis=1).all()
        by_start = [int(k) for k in np.argsort(first, kind="stable")]
        order = []
        a, b = 0, len(by_start) - 1
        while a <= b:
            order.append(by_start[a]); a += 1
            if a <= b:
                order.append(by_start[b]); b -= 1
        _rows = [bytes(msa[k]) for k in order]
    return _rows
