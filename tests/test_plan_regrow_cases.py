"""The designed MSA of plan_cases.py does what test_gpu_plan_regrow.py needs it to do -- shown on the CPU oracle alone, no
GPU: no column is trimmed, the MSA has widened by 80 columns or more when the first long row comes into the planner's
sight (so a context with "slack" 0 must regrow at that row), only rows of region B are long enough to be stopped, and the
order in which the long rows are realigned shows in the exported MSA (so a plan that reorders them cannot pass unseen)."""
import pytest

import plan_cases as pc

BASES = b"acgtACGT"


def _round(oracle, rows, bw, order, probe=None):
    """one round over the rows in `order`: (width after trimming, width at the fill of row `probe`, exported MSA, score)"""
    lib = oracle.lib
    h = oracle.create(rows, bw)
    lib.pwo_trim(h)
    w0, w_at = lib.pwo_width(h), None
    for k in order:
        assert lib.pwo_realign_row(h, k) == 0
        if k == probe:
            w_at = lib.pwo_dbg_W_at_fill(h)
    out = (w0, w_at, oracle.export(h), lib.pwo_total_score(h))
    lib.pwo_destroy(h)
    return out


def test_the_layout_is_the_documented_one():
    rows, bw, first_long = pc.regrow_case(pc.SEEDS[0])
    assert bw == 100 and len(rows) == first_long + pc.N_LONG
    assert first_long == pc.N_M_STRETCHES * pc.N_M_COPIES + pc.N_CB + pc.N_CA + pc.N_INSERT + pc.N_FILLER
    assert {len(r) for r in rows} == {pc.WIDTH_A + pc.WIDTH_M + pc.LMAX}
    assert not any(b"-" in r or b"_" in r for r in rows)
    assert pc.SEEDS[0] != pc.SEEDS[1]
    assert pc.regrow_case(pc.SEEDS[0])[0] == rows                               # the same rows every time
    # the first long row comes into the planner's sight at a filler row, after the last insert row
    first_filler = first_long - pc.N_FILLER
    assert first_filler <= first_long - (pc.HORIZON - 1) < first_long
    assert len(set(rows[first_filler:first_long])) == 1


@pytest.mark.parametrize("seed", pc.SEEDS)
def test_preconditions_of_the_regrow_case(seed, oracle):
    rows, bw, first_long = pc.regrow_case(seed)
    T, width = len(rows), len(rows[0])
    nbases = [sum(1 for c in r if c in BASES) for r in rows]
    first_cb = pc.N_M_STRETCHES * pc.N_M_COPIES
    for k in range(T):
        if k >= first_long:
            assert nbases[k] == pc.LMAX, k                                       # the long rows: exactly Lmax bases
        elif first_cb <= k < first_cb + pc.N_CB:
            assert nbases[k] == pc.LMAX, k
        else:
            assert 0 < nbases[k] < pc.LMAX - 1000, k                             # never stopped for a regrow
    assert max(nbases) == pc.LMAX
    inorder, swap_21, swap_312 = pc.long_row_orders(T, first_long)
    assert sorted(swap_21) == sorted(swap_312) == inorder == list(range(T))
    probe = first_long - (pc.HORIZON - 1)
    w0, w_at, msa, score = _round(oracle, rows, bw, inorder, probe)
    print(f"seed {seed}: W0 {w0}, width at the fill of row {probe}: {w_at} (+{w_at - w0}), width after the round {len(msa[0])}")
    assert w0 == width                                                           # EntAlGapper removed no column
    assert w_at - w0 >= 80                                                       # > 64 + pad, pad <= 15: a row of Lmax bases no longer fits
    # the in-order loop is the round of the reference
    h = oracle.create(rows, bw)
    oracle.lib.pwo_trim(h)
    oracle.lib.pwo_realign_round(h)
    assert oracle.export(h) == msa and oracle.lib.pwo_total_score(h) == score
    oracle.lib.pwo_destroy(h)
    # the orders a stale plan gives the long rows: another MSA, both of them
    for name, order in (("l2 l1 l3 l4", swap_21), ("l3 l1 l2 l4", swap_312)):
        _, _, other, other_score = _round(oracle, rows, bw, order)
        print(f"seed {seed}: order {name}: score {other_score} (in order {score}), same MSA: {other == msa}")
        assert other != msa, name
