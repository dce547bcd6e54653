"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

The semantics of pgr_msa_settle (include/pgr.h, last section: consensus and assignment iterated until no row moves) restated as
the loop the header writes out, from the checkers of its two halves: tests/ta_checker.py (or its vectorised form
cs_cases.numpy_consensus) for the consensus, tests/as_checker.py for the assignment and the label rule.  No call into the library
and no code shared with repeatresolver_amd/resolution.py.  The reference has no counterpart for this operation.  Everything
returned is an integer or a name."""
import numpy as np

import as_checker as ac
import cs_cases as cs
import ta_checker as ta

FIELDS = ("compared", "best", "second", "best_mismatches", "second_mismatches")


def one_consensus(msa, lab, von, bis, plain):
    """(part_label, consensus, depth) of the labelling `lab` over [von, bis]"""
    if plain:
        con = ta.consensus(msa, [int(x) for x in lab], von, bis)
        return con["part_label"], con["consensus"], con["depth"]
    kon, depth, _ = cs.numpy_consensus(msa, lab, von, bis)
    return np.array([x for x in range(int(lab.max()) + 1) if (lab == x).any()], dtype=np.int32), kon, depth


def settle(msa, labels, von, bis, maxcorrs, cutoff, min_compared, min_margin, max_iter, min_depth=1, all_columns=False, hold=False,
           plain=False):
    """msa: bytes rows with plain=True (the character-by-character checkers), a uint8 array [rows, width] otherwise (their
    vectorised forms).  A dict named as the fields of resolution.Settlement; `last` is the assignment the labels were made from."""
    initial = np.array([-1 if x is None else x for x in labels], dtype=np.int32)
    candidates = list(range(von, bis + 1)) if all_columns else ta.selected_columns(maxcorrs, von, bis, cutoff)   # fixed for the call
    lab, history, last, stop = initial.copy(), [], None, "MAX_ITER"
    for _ in range(max_iter):
        part_label, kon, depth = one_consensus(msa, lab, von, bis, plain)
        columns = ac.compared_columns(depth, von, bis, candidates, min_depth)
        if len(columns) == 0:
            stop = "NO_COLUMN"
            break
        a = ac.assign(msa, kon, von, columns) if plain else ac.numpy_assign(msa, kon, von, columns)
        new = ac.labels(a, part_label, min_compared, min_margin, initial if hold else None)
        changed = int((new != lab).sum())
        history.append((changed, len(part_label), len(columns)))
        last = dict(a, part_label=np.asarray(part_label, dtype=np.int32), columns=np.array(columns, dtype=np.int32))
        if changed == 0:
            stop = "CONVERGED"
            break
        if not (new >= 0).any():
            stop = "EMPTY"                                             # lab stays the labelling before
            break
        lab = new
    out = {"labels": lab, "stop": stop, "iterations": len(history), "changed": np.array([h[0] for h in history], dtype=np.int32),
           "parts_at": np.array([h[1] for h in history], dtype=np.int32), "ncolumns_at": np.array([h[2] for h in history], dtype=np.int32)}
    for name in ("part_label", "columns", "mismatches") + FIELDS:      # (the matrix: for the hand-made case; the library returns none)
        out[name] = None if last is None else last[name]
    return out


def same(got, exp):
    """a resolution.Settlement against the dict of `settle`, field by field, exactly"""
    assert (got.stop, got.iterations) == (exp["stop"], exp["iterations"]), (got.stop, got.iterations, exp["stop"], exp["iterations"])
    for name in ("changed", "parts_at", "ncolumns_at", "labels"):
        assert getattr(got, name).dtype == np.int32 and np.array_equal(getattr(got, name), exp[name]), name
    for name in ("part_label", "columns") + FIELDS:
        if exp[name] is None:
            assert getattr(got, name) is None, name
        else:
            assert getattr(got, name) is not None and np.array_equal(getattr(got, name), exp[name]), name
