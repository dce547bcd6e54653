"""-m gpu: every compiled instance of k_fl_place<NW> (pfl_device.hip), NW = block / 32 = 1 .. 16, on one two-block case against
tests/fc_checker.py, every byte and integer; one case per width, so that a failure names it.  test_gpu_kernel_widths.py does
the same for k_fl_tiles and the other two bit-vector kernels."""
import numpy as np
import pytest

import fc_checker as fc
from test_gpu_flanks import noisy, turned

pytestmark = pytest.mark.gpu


def width_case(nw):
    """a backbone of two blocks and a rest; members: an exact one, noisy ones in all four modes, two-letter stretches that make
    ties, one that stops in front of the second block and one that stops at it"""
    block = 32 * nw
    rng = np.random.default_rng(100 + nw)
    half = bytes(rng.choice(list(b"acgt"), size=block).astype(np.uint8))
    ties = bytes(rng.choice(list(b"ac"), size=block).astype(np.uint8))
    backbone = half + ties + b"acgtacg"
    tail = bytes(rng.choice(list(b"acgt"), size=block).astype(np.uint8))
    anchored = [backbone + tail, backbone[:2 * block - 1]]
    anchored += [noisy(rng, backbone + tail, rate=0.12) for _ in range(4)]
    anchored += [noisy(rng, backbone + tail, rate=0.2, alphabet=b"ac") for _ in range(2)]
    anchored += [half + bytes(rng.choice(list(b"gt"), size=2 * block).astype(np.uint8))]   # no base of its second block matches: stopped
    mode = [k % 4 for k in range(len(anchored))]
    return block, backbone, [turned(p, m) for p, m in zip(anchored, mode)], mode


@pytest.mark.parametrize("nw", range(1, 17))
def test_place_every_word_count(nw):
    from repeatresolver_amd.flanks import FlankClusterer
    block, backbone, pieces, mode = width_case(nw)
    n = len(pieces)
    with FlankClusterer() as g:
        got = g.place(pieces, list(range(n)), mode, [0] * n, [backbone], block=block, extent=2 * block + 31, max_permille=400)
    exp = fc.place_all(pieces, list(range(n)), mode, [0] * n, [backbone], block, 2 * block + 31, 400)
    assert got[1].tolist() == exp[1].tolist() and got[2].tolist() == exp[2].tolist() and got[3].tolist() == exp[3].tolist()
    bad = np.argwhere(got[0] != exp[0])
    assert len(bad) == 0, (bad[:5].tolist(), [(int(got[0][i, j]), int(exp[0][i, j])) for i, j in bad[:5]])
    assert got[1][0] == 2 and got[3][0] == 0 and got[1][1] == 1 and got[1][-1] == 1 and got[0].shape == (n, 2 * block)
