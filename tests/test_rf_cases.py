"""not-gpu: the inputs of test_gpu_rf_models.py reach every place the census of rf_cases.py names, by the oracle's windows alone.  A change to
the generator (or to a seed) that empties a class fails here instead of the GPU tests quietly losing the rows they exist for."""
import pytest

import rf_cases as R


@pytest.mark.parametrize("half", R.HALVES)
def test_census_has_every_class(half):
    for name in R.INPUTS:
        for batch in R.BATCHES:
            for mode in R.MODES:
                print(f"half {half} {name} batch {batch} mode {mode}: {R.census(name, batch, mode, half)}")
    tot = R.census_union(half)
    print(f"half {half} edges + dense: {tot}")
    need = "ehi" if half == 0 else R.CLASSES     # a one-row field cannot leave its window
    for k in need:
        assert tot[k] >= 1, f"half {half}: class ({k}) is empty: {tot}"


def test_inputs_are_what_the_gpu_tests_assume():
    edges, e_off, _ = R.windows("edges")
    assert [e_off[t + 1] - e_off[t] for t in range(3)] == [4, 4, 4]
    last = [edges[e_off[t + 1] - 1] for t in range(3)]
    assert all(w.len < 13 for w in last) and any(w.n_sup and w.len < 9 for w in last)     # shorter than both wide fields, and the model is asked about one
    dense, _, _ = R.windows("dense")
    sup = [w.n_sup for w in dense]
    assert max(sup) > 78 and 64 in sup and 0 < min(sup) < 64, sup        # sibling tiles next to ordinary ones, the tile's own size, two passes of k_quals<false> at half 6
    for batch in R.BATCHES:                                 # both batch sizes, both modes: batches of different padding lengths in one launch
        for mode in R.MODES:
            lmax = {max(edges[w].len for w in mem) for mem, _ in R.groups(edges, e_off, batch, mode)}
            assert len(lmax) > 1, (batch, mode)


def test_groups_follow_the_flush_rule():
    """mode 0 counts the empty windows of a read towards the flush (features.rs:884-893); mode 1 does not see them."""
    class Wn:
        def __init__(self, n):
            self.n_sup = n
    wins = [Wn(n) for n in (2, 0, 3, 1, 0, 0, 4, 5)]
    off = [0, 5, 8]
    assert R.groups(wins, off, 3, 0) == [([0, 2], [0, 1, 2]), ([3], [3, 4]), ([6, 7], [5, 6, 7])]
    assert R.groups(wins, off, 3, 1) == [([0, 2, 3], [0, 1, 2, 3]), ([6, 7], [6, 7])]
