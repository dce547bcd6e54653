"""A designed MSA on which the column arrays MUST be regrown in the middle of a batch while a batch plan with a row picked
ahead is live (include/pwr.h "plan_ahead", "slack" 0).  Plain Python, no GPU: test_plan_regrow_cases.py shows
on the CPU oracle alone that the preconditions hold, test_gpu_plan_regrow.py and test_gpu_intra_round.py run the case.

Three column regions, rows without a single '-' (EntAlGapper has nothing to trim, no column is empty):

    A   403 columns   a random consensus CA of 400 bases
    M  2600 columns   nothing but rows that keep its columns alive (EntAlGapper would remove them otherwise, and regions A
                      and B would come to lie side by side): the band intervals of A rows and B rows stay about 2 400 columns
                      apart, more than the 2 048 a jump keeps, so every plan option stays at its default
    B  1500 columns   a random consensus CB, Lmax = 1 500

Rows, in input order:

    12  region M: six stretches of 433 or 434 bases, each as 2 identical rows (every row but the long ones and the CB rows
        has to be shorter than Lmax - 1000, so that the capacity test of the commit can only stop a row of region B; two
        stretches of 1 300 bases would keep the columns alive as well but are not that short)
     4  exactly CB
     8  exactly CA (columns 0 .. 399)
    40  "insert" rows: CA with 3 random bases inserted at 20 + 9 i, written into columns 0 .. 402 without a gap: the
        realignment of each opens about 3 columns
    64  "filler" rows, exactly CA: they change nothing, and there are as many as the planner looks ahead, so every insert
        row is committed when the first long row comes into its sight
     4  "long" rows of exactly Lmax bases in region B: long row t is CB with four 2-base insertions at 100 + 300 i + 7 t,
        each paired with a 2-base deletion 150 bases later, and 30 substitutions.  They need column changes and they overlap
        one another, and the i-th insertion of every long row lies within 21 bases of the others', so that the columns one
        of them opens are columns the next one may use: the order in which they are realigned shows in the MSA.  (With the
        insertions of different long rows 300 bases apart, 100 + 300 t + 37 i, 2 seeds in 400 were sensitive to both
        changes of order below, whether beside 4, 2 or 1 CB rows; with this layout 12 of the seeds 1 .. 40 are.)

With "slack" 0 the capacity is roundup16(W0 + Lmax + 128) columns, and a commit stops a row of L bases for a regrow iff
W + nnew + L + 64 exceeds it: for a row of Lmax bases as soon as the MSA is (64 + pad) columns wider than W0, pad <= 15, for
the short rows never.  The insert rows widen the MSA by more than 80 columns, so the first long row is stopped wherever it
stands in its batch -- and the planner picks it ahead of 62 fillers, as the last job of a batch whose first job commits.
"""
import random

BANDWIDTH = 100
WIDTH_A, WIDTH_M, LMAX = 403, 2600, 1500
LEN_CA = 400
N_M_STRETCHES, N_M_COPIES = 6, 2
N_CB, N_CA, N_INSERT, N_FILLER, N_LONG = 4, 8, 40, 64, 4
HORIZON = 64                       # rows from the row pointer on that the planner picks from

# Seeds for which the oracle exports another MSA when the long rows are realigned in the order l2, l1, l3, l4 and in the
# order l3, l1, l2, l4 than in input order (the first two of the seeds 1 .. 40 that qualify; test_plan_regrow_cases.py
# asserts it): what a stale plan does to the order of the long rows then shows in the result.
SEEDS = (7, 10)


def _bases(rng, n):
    return [rng.choice("ACGT") for _ in range(n)]


def _other(rng, b):
    return rng.choice([c for c in "ACGT" if c != b])


def _long_row(rng, cb, t):
    ins = {100 + 300 * i + 7 * t for i in range(4)}
    dele = set()
    for p in ins:
        dele.update((p + 150, p + 151))
    out = []
    for x, b in enumerate(cb):
        if x in ins:
            out.extend(_bases(rng, 2))
        if x not in dele:
            out.append(b)
    assert len(out) == len(cb)
    for x in rng.sample(range(len(out)), 30):
        out[x] = _other(rng, out[x])
    return out


def regrow_case(seed):
    """(rows, bandwidth, first_long): the rows as equal-length bytes, blank = ' '; the index of the first long row"""
    rng = random.Random(seed)
    width = WIDTH_A + WIDTH_M + LMAX
    ca, cb = _bases(rng, LEN_CA), _bases(rng, LMAX)

    def row(col, bases):
        assert col + len(bases) <= width
        return (" " * col + "".join(bases) + " " * (width - col - len(bases))).encode()

    rows = []
    col = WIDTH_A
    for s in range(N_M_STRETCHES):
        n = WIDTH_M * (s + 1) // N_M_STRETCHES - WIDTH_M * s // N_M_STRETCHES
        stretch = _bases(rng, n)
        rows += [row(col, stretch)] * N_M_COPIES
        col += n
    assert col == WIDTH_A + WIDTH_M
    rows += [row(col, cb)] * N_CB
    rows += [row(0, ca)] * N_CA
    for i in range(N_INSERT):
        p = 20 + 9 * i
        rows.append(row(0, ca[:p] + _bases(rng, WIDTH_A - LEN_CA) + ca[p:]))
    rows += [row(0, ca)] * N_FILLER
    first_long = len(rows)
    for t in range(N_LONG):
        rows.append(row(col, _long_row(rng, cb, t)))
    assert all(len(r) == width for r in rows)
    return rows, BANDWIDTH, first_long


def long_row_orders(T, first_long):
    """The in-order round and the two orders a stale plan would give the long rows: (l2, l1, l3, l4) and (l3, l1, l2, l4)"""
    head = list(range(first_long))
    l1, l2, l3, l4 = range(first_long, first_long + N_LONG)
    assert first_long + N_LONG == T
    return head + [l1, l2, l3, l4], head + [l2, l1, l3, l4], head + [l3, l1, l2, l4]
