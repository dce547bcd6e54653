"""CPU, numpy: the commit's two-buffer renumbering restated as a model, and its mutation check.

The state keeps the column order twice (order0 / order1, Hdr::cur names the current one) and Hdr::agree, the number of
leading ordinals on which the two agree.  A commit that opens or empties columns reads the current buffer and writes the
OTHER one -- nothing it reads is overwritten, so all its work-groups can run in one launch -- and then flips:

    s0 = max(0, min(first, agree))                 first = the first ordinal with an event
    for every old ordinal y in [s0, W) that is not emptied:  other[y + shift(y)] = cur[y],  shift(y) = sum of dl over events with key < 2y
    rank[slot] is written only where the shift is not 0
    a column opened after y, the tt-th there:      other[y + shift(y) + kept + tt],  kept = 1 unless y itself is emptied
    cur ^= 1;  agree = max(0, min(first, W))

Events: key 2y = column y is emptied (dl -1), key 2y + 1 = a column opens after y (dl +1, y = -1: before the first column);
several columns may open after one y, a set of events may have net 0, and a step may have no event at all (nothing flips).
The truth is kept beside it as a plain list that is rebuilt from the events in the obvious way.  After every step:
current[0:W] is the truth, other[0:agree] == current[0:agree], rank[current[y]] == y.

The negative control is the same rule with s0 = first: the buffer it writes still holds, between the last commit's first
change and this one's, the order of two commits ago.  It must fail on the sequence that alternates between the ends.  (This
check is made on the model only: a wrong renumbering on the device leaves stale ordinals that index out of a job's buffers.)"""
import numpy as np
import pytest

CAP = 4096
STALE = -7                                     # what a buffer holds where nothing valid was ever written


class Model:
    def __init__(self, W, s0_rule="min(first, agree)"):
        self.truth = list(range(W))
        self.buf = [np.full(CAP, STALE, dtype=np.int64), np.full(CAP, STALE, dtype=np.int64)]
        self.buf[0][:W] = self.truth
        self.cur, self.agree, self.W = 0, 0, W               # as a fresh context: only order0 is filled
        self.rank = {s: y for y, s in enumerate(self.truth)}
        self.nslots = W
        self.s0_rule = s0_rule

    def step(self, keys):
        """keys: the events' keys, any order, opens after one y as often as columns open there"""
        keys = sorted(keys)
        if not keys:
            return
        W = self.W
        emptied = {k >> 1 for k in keys if not k & 1}
        assert len(emptied) == sum(1 for k in keys if not k & 1) and all(0 <= y < W for y in emptied)
        opens = {}
        for k in keys:
            if k & 1:
                assert -1 <= k >> 1 < W
                opens[k >> 1] = opens.get(k >> 1, 0) + 1
        new_slots = {}
        for y in sorted(opens):
            new_slots[y] = list(range(self.nslots, self.nslots + opens[y]))
            self.nslots += opens[y]
        # the truth, rebuilt
        truth = list(new_slots.get(-1, []))
        for y in range(W):
            if y not in emptied:
                truth.append(self.truth[y])
            truth.extend(new_slots.get(y, []))
        # the rule
        skey = np.asarray(keys, dtype=np.int64)
        scum = np.cumsum(np.where(skey & 1, 1, -1))
        first = int(skey[0] >> 1)
        src, dst = self.buf[self.cur], self.buf[self.cur ^ 1]

        def shift(y):
            a = int(np.searchsorted(skey, 2 * y, side="left"))        # events with key < 2y
            return int(scum[a - 1]) if a else 0

        s0 = max(0, min(first, self.agree)) if self.s0_rule == "min(first, agree)" else max(0, first)
        for y in range(s0, W):
            if y in emptied:
                continue
            sh = shift(y)
            dst[y + sh] = src[y]
            if sh:
                self.rank[int(src[y])] = y + sh
        for y, slots in new_slots.items():
            kept = 0 if y in emptied else 1
            for tt, s in enumerate(slots):
                dst[y + shift(y) + kept + tt] = s
                self.rank[s] = y + shift(y) + kept + tt
        for y in emptied:
            del self.rank[int(src[y])]
        self.cur ^= 1
        self.agree = max(0, min(first, W))
        self.W = W + int(scum[-1])
        self.truth = truth
        assert self.W == len(truth)

    def check(self):
        cur, other = self.buf[self.cur], self.buf[self.cur ^ 1]
        assert list(cur[:self.W]) == self.truth, "the current buffer is not the truth"
        assert (other[:self.agree] == cur[:self.agree]).all(), "the buffers differ below `agree`"
        assert all(self.rank[int(cur[y])] == y for y in range(self.W)), "rank"


def alternating(W0, steps, rng):
    """events a few columns from the left end, then a few from the right end, and so on: opens, emptyings, both"""
    W = W0
    for i in range(steps):
        base = 3 + int(rng.integers(0, 5)) if i % 2 == 0 else W - 12 + int(rng.integers(0, 5))
        kind = i // 2 % 4
        if kind == 0:
            keys = [2 * base + 1]                                       # one column opens
        elif kind == 1:
            keys = [2 * base]                                           # one is emptied
        elif kind == 2:
            keys = [2 * base + 1, 2 * base + 1, 2 * (base + 2)]         # two open after one y, one emptied: net +1
        else:
            keys = [2 * base, 2 * base + 1]                             # y emptied and a column opened after it: net 0
        W += sum(1 if k & 1 else -1 for k in keys)
        yield keys


def random_steps(W0, steps, rng, idle_every=0):
    W = W0
    for i in range(steps):
        if idle_every and i % idle_every == idle_every - 1:
            yield []                                                    # a commit that changes no column's place
            continue
        keys = []
        n_del = int(rng.integers(0, max(1, min(6, W - 8))))
        keys += [2 * int(y) for y in rng.choice(W, size=n_del, replace=False)]
        for _ in range(int(rng.integers(0, 6))):
            y = int(rng.integers(-1, W))
            keys += [2 * y + 1] * int(rng.integers(1, 4))
        if W > CAP // 2:                                                # widths shrink and grow
            keys = [k for k in keys if not k & 1] or [2 * int(rng.integers(0, W))]
        W += sum(1 if k & 1 else -1 for k in keys)
        yield keys


def run(model, steps):
    """the index of the first step after which a property fails, or None"""
    model.check()
    for i, keys in enumerate(steps):
        model.step(keys)
        try:
            model.check()
        except AssertionError as e:
            return i, str(e)
    return None


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_alternating_ends(seed):
    rng = np.random.default_rng(seed)
    assert run(Model(300), alternating(300, 64, rng)) is None


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
@pytest.mark.parametrize("idle_every", [0, 3])
def test_random_event_sets(seed, idle_every):
    rng = np.random.default_rng(100 + seed)
    m = Model(40 if seed % 2 else 500)
    assert run(m, random_steps(m.W, 200, rng, idle_every)) is None


def test_edges_of_the_width():
    """a column before the first one, after the last one, the first and the last emptied, a net-0 set at both ends at once"""
    m = Model(20)
    for keys in ([-1], [2 * 20 + 1], [0], [2 * 20], [-1, -1, 0, 2 * 19, 2 * 19 + 1], [], [2 * 5 + 1], [2 * 19], [1, 2 * 3]):
        m.step(keys)
        m.check()


def test_negative_control_copy_from_first_alone():
    """the mutation: s0 = first.  It must break the first property on the alternating sequence -- and the rule itself not."""
    rng = np.random.default_rng(1)
    bad = run(Model(300, s0_rule="first"), alternating(300, 64, rng))
    assert bad is not None and "not the truth" in bad[1], bad
    # ... and still does when both buffers start out equal (so that not the fresh context's empty second buffer is what shows):
    # the third commit writes the buffer that missed the first one's change at the other end
    m = Model(300, s0_rule="first")
    m.buf[1][:300] = m.buf[0][:300]
    m.agree = 300
    rng = np.random.default_rng(1)
    bad = run(m, alternating(300, 64, rng))
    assert bad is not None and bad[0] == 1 and "not the truth" in bad[1], bad
