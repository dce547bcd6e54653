"""-m gpu: pgr_subdivide (include/pgr.h: stage 1 on the host, stage 2's votes in the HIP kernel k_gr_reldrop) against the
literal restatement tests/sd_checker.py.  Everything compared is an integer and is compared exactly: both label arrays, both
part counts and, per part of stage 1, the winning variation and its cutoff.

The device is fed the CHECKER's refined arrays (gr_checker.Window.refine(), or hand-made cliques for `synthetic`), not the
device refinement's: that keeps the refinement's near-tie "undecided" variations (tests/test_gpu_group_refinement.py) out of
this comparison.  Inputs and their structure: tests/test_subdivision.py, which asserts on the CPU what the cases here rely on."""
import numpy as np
import pytest

import sd_checker as sd
from test_subdivision import SD_CASES, SYN_BITS, as_refined, sd_case

KERNEL_TILE = 64                                                    # PGR_SD_TILE of pgr_device.hip: parts per LDS pass


def compare(name):
    from repeatresolver_amd.subdivision import subdivide
    rows, von, bis, cov, win, ref, exp = sd_case(name)
    got = subdivide(rows, as_refined(ref), von, bis, cov)
    print(f"{name}: {win.T} kept rows, {got.selected} selected, {got.dropoff_parts} parts ({got.eligible} eligible) -> "
          f"{got.reldrop_parts}, winners {[(int(v), int(c)) for v, c in zip(got.winner, got.winner_cutoff) if v >= 0][:6]}")
    assert got.selected == exp["selected"]
    assert got.dropoff_parts == exp["dropoff_parts"] and got.reldrop_parts == exp["reldrop_parts"]
    assert np.array_equal(got.dropoff_labels, exp["dropoff_labels"]) and np.array_equal(got.reldrop_labels, exp["reldrop_labels"])
    assert np.array_equal(got.winner, exp["winner"]) and np.array_equal(got.winner_cutoff, exp["winner_cutoff"])
    return got, exp, ref, win


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in SD_CASES if n not in ("kept63", "kept64", "kept65", "kept129", "index0", "synthetic")])
def test_equals_the_checker(name):
    """the refinement's inputs (stage 2 splits nothing in them) and the three where it does"""
    got, exp, ref, win = compare(name)
    if name.startswith("rel"):
        assert (got.winner >= 0).sum() >= 1 and got.reldrop_parts > got.dropoff_parts


@pytest.mark.gpu
@pytest.mark.parametrize("kept", [63, 64, 65, 129])
def test_word_boundaries(kept):
    """sc = kept / 64 + 1 steps at 64 and 128 (64 kept rows: an empty last word whose lanes carry the skip label)"""
    got, exp, ref, win = compare(f"kept{kept}")
    assert win.T == kept and got.dropoff_parts == 3
    if kept > 64:
        lab = exp["dropoff_labels"][ref["kept"]]
        assert any(len({r // 64 for r in np.flatnonzero(lab == k)}) > 1 for k in range(3))   # a part straddles a word boundary


@pytest.mark.gpu
def test_more_parts_than_one_pass_first_variation_lowest_index_and_sizes_below_length():
    """`synthetic` (tests/test_subdivision.py): 2^7 = 128 parts of 4 to 6 rows with cov = 2, so mingroup = 1 and every part has
    more than 2 rows: 128 eligible parts, two passes of the kernel's 64 histograms per block.  In the parts p % 4 == 1 the
    first selected variation already splits (every later one then sees the part empty) and 14 variations pass: the lowest
    index must win the atomic minimum.  The parts p % 4 == 2 are split by cliques with variation 0 at place 6: Sizes = 6,
    length 8, v_sizes != v_all."""
    got, exp, ref, win = compare("synthetic")
    assert got.eligible == 1 << SYN_BITS > KERNEL_TILE
    splits = exp["splits"]
    assert any(k >= KERNEL_TILE for k, _, _ in splits) and any(k < KERNEL_TILE for k, _, _ in splits)   # (all parts are eligible: e = k)
    first = int(ref["significant"][sd.selected(ref)[0]])
    assert (got.winner == first).sum() >= (1 << SYN_BITS) // 4
    y = min(int(ref["significant"][s]) for s in range(len(ref["significant"])) if 0 in list(ref["cliques"][s, 1:]))
    assert (got.winner == y).sum() >= (1 << SYN_BITS) // 4


@pytest.mark.gpu
def test_index_0():
    """the refinement's index-0 input: cliques with variation 0 inside, Sizes below the clique's length"""
    got, exp, ref, win = compare("index0")
    sel = sd.selected(ref)
    assert any(ref["sizes"][s] < (ref["cliques"][s] >= 0).sum() for s in sel)


@pytest.mark.gpu
def test_nothing_selected():
    """cutoff 99.5: nothing over it -- label 0 for every kept row in both outputs, and no upload or launch"""
    from repeatresolver_amd.group_refinement import refine_groups
    from repeatresolver_amd.subdivision import last_timing, subdivide
    from test_gpu_group_refinement import checked
    rows, von, bis, cov, win, ref, exp = sd_case("kept65")
    none = refine_groups(rows, checked("kept65")[1], cov=cov, cutoff=99.5)
    got = subdivide(rows, none, von, bis, cov)
    assert got.selected == 0 and got.dropoff_parts == got.reldrop_parts == 1
    assert np.array_equal(got.dropoff_labels, np.where(ref["kept"], 0, -1)) and np.array_equal(got.reldrop_labels, got.dropoff_labels)
    t = last_timing()
    assert t["upload_ms"] == 0 and t["kernel_ms"] == 0


@pytest.mark.gpu
def test_pipeline_chain():
    """pipeline.subdivided: MaxCorrelation, refinement and subdivision on the device, against the labels the checker's
    refined arrays give"""
    from repeatresolver_amd.pipeline import subdivided
    from repeatresolver_amd.subdivision import last_timing
    rows, von, bis, cov, win, ref, exp = sd_case("kept65")
    chain = subdivided(rows, von, bis, cov)
    assert np.array_equal(chain.dropoff_labels, exp["dropoff_labels"]) and np.array_equal(chain.reldrop_labels, exp["reldrop_labels"])
    assert chain.dropoff_parts == exp["dropoff_parts"] and chain.reldrop_parts == exp["reldrop_parts"]
    assert last_timing()["kernel_ms"] > 0


def _raises_arg(**kw):
    from repeatresolver_amd.realigner import PwrError
    from repeatresolver_amd.subdivision import subdivide
    rows, von, bis, cov, win, ref, exp = sd_case("kept65")
    args = {"refined": as_refined(ref), "von": von, "bis": bis, "cov": cov}
    args.update(kw)
    with pytest.raises(PwrError) as e:
        subdivide(rows, **args)
    assert e.value.code == -1


@pytest.mark.gpu
def test_error_negative_cov():
    _raises_arg(cov=-1)


@pytest.mark.gpu
def test_error_window_and_result_differ():
    """a window of another width than the refined arrays'"""
    _raises_arg(von=10, bis=200)


@pytest.mark.gpu
def test_error_clique_member_outside_the_window():
    ref = sd_case("kept65")[5]
    bad = as_refined(ref)
    bad.cliques = bad.cliques.copy()
    bad.cliques[sd.selected(ref)[0], 3] = ref["width"] * 5
    _raises_arg(refined=bad)
