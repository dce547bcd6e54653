"""-m gpu: every compiled width of k_la_search (pla_device.hip), NW = ceil(m / 32) = 1 .. 16, each on one case whose contigs span
two chunks, with one planted hit per orientation, against tests/la_checker.py."""
import numpy as np
import pytest

import la_checker as la

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nw", range(1, 17))
def test_every_instance_of_k_la_search(nw):
    from repeatresolver_amd.anchors import LocusAnchorer
    from repeatresolver_amd.strands import reverse_complement
    rng = np.random.default_rng(100 + nw)
    rand = lambda n: bytes(rng.choice(list(b"acgt"), size=n).astype(np.uint8))
    m = 32 * nw - 5                                                                 # the last word is not full
    a = rand(m)
    plus = rand(29) + a[::-1] + rand(40)                                            # the left flank as the template shows it
    minus = reverse_complement(rand(33) + a[::-1] + rand(26))
    chunk = max(32, (len(plus) // 2 + 7) // 4 * 4)                                  # two chunks a contig, the hit in the second
    assert chunk < len(minus) < len(plus) <= 2 * chunk
    with LocusAnchorer([plus, minus]) as g:
        g.set_chunk(chunk)
        got = g.search([a], [0], max_permille=60, reach=m, min_len=1).rows()
    assert got == la.search([plus, minus], [a], [0], m, 1, 60)
    assert [h[:4] + h[6:] for h in got] == [(0, 0, 0, 29 + m, 0), (0, 1, 1, 26, 0)]
