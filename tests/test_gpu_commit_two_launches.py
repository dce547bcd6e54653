"""-m gpu: the commit as two launches -- k_commit_scan, then k_commit_finish, which applies the changes and writes the
renumbered order into the OTHER order buffer -- on the MSA of order_cases.py, whose k loop alternates
between the ends of the width: nearly every commit opens or empties columns, and the first changed ordinal jumps back and
forth by thousands of columns (test_order_cases.py shows that on the CPU).  The buffer a commit writes holds the order of two
restructuring commits ago, so a copy that starts anywhere right of min(first, Hdr::agree) would surface here as a wrong MSA
one commit later (the rule itself and its mutation: test_order_buffers_model.py).

The rows are advanced in slabs of 1 row (window 1) or 4 rows, and after EVERY slab the MSA and the score are compared with the
CPU oracle advanced by the same rows: integers and bytes, no tolerance.  "evcap" picks the renumbering: default = from the
list of events, 0 = always by the pass over the width, 2 = mixed; window 16 puts several jobs' events into one sort."""
import hashlib

import pytest

import order_cases as oc

pytestmark = pytest.mark.gpu

_expected = {}


def _digest(rows):
    return hashlib.sha256(b"\n".join(rows)).hexdigest()


def _oracle(oracle):
    """after every row of ROUNDS rounds: (score, digest of the MSA, width); and the cells, the live rows.  Computed once."""
    if not _expected:
        rows = oc.alternating_rows()
        lib = oracle.lib
        h = oracle.create(rows, oc.BANDWIDTH)
        lib.pwo_trim(h)
        live = sum(1 for k in range(len(rows)) if lib.pwo_row_length(h, k) > 0)
        after = {}
        for rnd in range(oc.ROUNDS):
            for k in range(len(rows)):
                assert lib.pwo_realign_row(h, k) == 0
                lib.pwo_compact(h)
                after[(rnd, k + 1)] = (lib.pwo_total_score(h), _digest(oracle.export(h)), lib.pwo_width(h))
        _expected.update(after=after, cells=lib.pwo_cells(h), live=live)
        lib.pwo_destroy(h)
    return _expected


@pytest.mark.parametrize("evcap", [None, 2, 0], ids=["evcap_default", "evcap_2", "evcap_0"])
@pytest.mark.parametrize("window", [1, 3, 16])
def test_every_slab_against_the_oracle(window, evcap, oracle):
    from repeatresolver_amd.realigner import PWReAligner
    rows = oc.alternating_rows()
    exp = _oracle(oracle)
    T = len(rows)
    slab = 1 if window == 1 else 4
    g = PWReAligner(rows, bandwidth=oc.BANDWIDTH, window=window)
    if evcap is not None:
        g.set_option("evcap", evcap)
    g.trim_ends()
    for rnd in range(oc.ROUNDS):
        for k0 in range(0, T, slab):
            k1 = min(T, k0 + slab)
            g.realign_rows(k0, k1 - k0)
            score, digest, width = exp["after"][(rnd, k1)]
            got = g.export_rows()
            assert len(got[0]) == width, (rnd, k1)
            assert _digest(got) == digest, (rnd, k1)
            assert g.total_score() == score, (rnd, k1)
    st = g.stats()
    print(f"window {window} evcap {evcap}: batches {st['batches']} rows_committed {st['rows_committed']} rows_ahead {st['rows_ahead']} "
          f"rows_recomputed {st['rows_recomputed']}")
    assert st["cells_reference"] == exp["cells"]
    assert st["rows_committed"] == oc.ROUNDS * exp["live"]
    if window == 16:
        assert st["rows_ahead"] > 0, st                                            # several jobs' events in one sort
    g.close()
