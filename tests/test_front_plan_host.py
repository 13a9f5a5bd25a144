"""not-gpu: what the front end of a model launch decides from its tokens and the compute units of the device (csrc/infer_plan.h front_end_plan, through
herro_debug_front_end_plan) against a plain restatement of the rule as launch_model_h stated it before it had a function of its own: the grid of k_conv_m's
stride loop, the tile height of k_fc_r (`busiest`), and k_conv_fc where its rounds cost less than 85 % of the two kernels' line (conv_fc_faster).  Every token
count a launch group can have and then some (1 .. 131 072), on 1, 2, 3, 4, 8, 64, 256 and 304 compute units; and the facts the project states for 256 units
(profiles/conv_fc_ab.txt) pinned as numbers."""
import numpy as np
import pytest

from herro_amd import api

N_MAX = 131072
CUS = [1, 2, 3, 4, 8, 64, 256, 304]
ROWS, TILE = 31, 128        # read rows of a token; tokens of a k_conv_fc tile
FUSED, FC_ROWS, FC_GRID, CONV_GRID, CONV_UNITS = range(5)


def restated(n_cu, mode=-1):
    """[N_MAX, 5] for 1 .. N_MAX tokens"""
    n = np.arange(1, N_MAX + 1, dtype=np.int64)
    # conv_fc_faster: rounds of one 128-token tile per compute unit at 133 us against 85 % of 44 us + 4.85 us per 1000 tokens (on 256 units; both scale with them)
    tiles = (n + TILE - 1) // TILE
    rounds = (tiles + n_cu - 1) // n_cu
    t_fused = 133.0 * rounds.astype(np.float64) * (float(TILE) / 128)
    t_two = 44.0 + 4.85e-3 * n.astype(np.float64) * (256.0 / n_cu)
    fused = {-1: t_fused <= 0.85 * t_two, 0: np.zeros(N_MAX, bool), 1: np.ones(N_MAX, bool)}[mode]

    # k_fc_r: the height (16-row blocks, 8 down to 4) that leaves the busiest unit the fewest rows, a third workgroup on a unit being out of the question; ties to the taller
    def busiest(rows):
        wg = (n + rows - 1) // rows
        return (wg + n_cu - 1) // n_cu * rows + np.where(wg > 2 * n_cu, 1 << 20, 0)
    nb = np.full(N_MAX, 8, np.int64)
    best = busiest(128)
    for b in (7, 6, 5, 4):
        cur = busiest(16 * b)
        take = cur < best
        nb[take], best[take] = b, cur[take]
    # k_conv_m: one block of 16 (token, row) pairs per wave and trip, four waves, three workgroups per unit (768 on 256 units)
    units = (n * ROWS + 15) // 16
    grid = np.minimum((units + 3) // 4, 3 * n_cu)
    out = np.zeros((N_MAX, 5), np.int64)
    out[:, FUSED] = fused
    out[:, FC_ROWS] = np.where(fused, TILE, 16 * nb)
    out[:, FC_GRID] = np.where(fused, tiles, (n + 16 * nb - 1) // (16 * nb))
    out[:, CONV_GRID] = np.where(fused, 0, grid)
    out[:, CONV_UNITS] = np.where(fused, 0, units)
    return out


def hook(n_cu, mode=-1):
    return api.debug_front_end_plans(1, N_MAX, n_cu, mode).astype(np.int64)


@pytest.fixture(scope="module")
def on256():
    return hook(256)


def at(tab, n):
    return api.FrontPlan(bool(tab[n - 1, FUSED]), *(int(x) for x in tab[n - 1, 1:]))


@pytest.mark.parametrize("n_cu", CUS)
def test_the_hook_equals_the_restated_rule(n_cu):
    got, want = hook(n_cu), restated(n_cu)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (n_cu, int(bad[0]) + 1, got[bad[0]].tolist(), want[bad[0]].tolist())
    assert 0 < got[:, FUSED].sum() < N_MAX             # both answers occur on every device size
    assert set(np.unique(got[got[:, FUSED] == 0, FC_ROWS]).tolist()) <= {64, 80, 96, 112, 128}


@pytest.mark.parametrize("n_cu", [1, 256])
def test_a_forced_mode_is_the_rule_with_its_choice_replaced(n_cu):
    for mode in (0, 1):
        assert np.array_equal(hook(n_cu, mode), restated(n_cu, mode))
    auto, two = hook(n_cu), hook(n_cu, 0)
    sel = auto[:, FUSED] == 0
    assert np.array_equal(auto[sel], two[sel])
    one = api.debug_front_end_plan(27000, 256, 1)
    assert one == api.debug_front_end_plan(27000, 256) == at(hook(256, 1), 27000)


def test_the_single_entry_and_its_argument_checks():
    assert api.debug_front_end_plan(65, 1, 0) == api.FrontPlan(False, 80, 1, 3, 126)
    for bad in [(0, 1, 256, -1), (1, 0, 256, -1), (1, 1, 0, -1), (1, 1, 256, 2), (1, 1, 256, -2), (0xFFFFFFFF, 2, 256, 0)]:
        with pytest.raises(api.HerroError):
            api.debug_front_end_plans(*bad)


def test_tile_heights_on_256_units(on256):
    two = hook(256, 0)
    assert (two[:16384, FC_ROWS] == 64).all()                         # one workgroup or two per unit: the lowest tile
    assert at(two, 16385).fc_rows == 80 and at(two, 16385).fc_grid == 205
    assert (on256[:16384, FUSED] == 0).all() and at(on256, 16385) == at(two, 16385)
    # the driver's launch, 2560 windows (38.7 k tokens): two kernels, 80-row tiles on 484 workgroups
    assert at(on256, 38700) == api.FrontPlan(False, 80, 484, 768, (38700 * 31 + 15) // 16)


def test_the_fused_kernel_on_256_units(on256):
    assert at(on256, 27100) == api.FrontPlan(True, 128, 212, 0, 0)    # 1792 windows, 27 k tokens
    assert at(on256, 61900) == api.FrontPlan(True, 128, 484, 0, 0)    # 4096 windows, 62 k tokens
    f = on256[:, FUSED]
    edge = np.flatnonzero(np.diff(np.concatenate([[0], f, [0]])))     # 0-based index of each range's first count, and of the first count behind it
    ranges = [(int(a) + 1, int(b)) for a, b in zip(edge[0::2], edge[1::2])]
    # a last round about 70 % full up to a full one: 23.2 - 32.7 k, 55.5 - 65.5 k, 87.7 - 98.3 k, and the fourth round up to the end of the table
    assert ranges == [(23190, 32768), (55452, 65536), (87714, 98304), (119976, 131072)]
    # the ranges from the rule's own numbers: rounds x 133 us <= 0.85 x (44 + 4.85e-3 n)
    for r, (lo, hi) in enumerate(ranges, 1):
        assert hi == r * 256 * 128 and lo == int(np.ceil((133.0 * r / 0.85 - 44.0) / 4.85e-3))
    assert [lo // 100 for lo, _ in ranges[:3]] == [231, 554, 877]


def test_the_conv_grid_on_256_units():
    two = hook(256, 0)
    assert at(two, 1).conv_grid == 1 and at(two, 1).conv_units == 2
    assert (two[1585:, CONV_GRID] == 768).all() and (np.diff(two[:, CONV_GRID]) >= 0).all()          # 768 from 1586 tokens on, whatever the launch
    # (the cap is met at 3069 units, 1584 tokens; its 3072 waves are all taken at 1585.)  Below 1586 tokens every wave makes one trip, from there on some wave a second
    assert int(np.flatnonzero(two[:, CONV_GRID] == 768)[0]) + 1 == 1584
    assert (two[:1585, CONV_UNITS] <= 4 * two[:1585, CONV_GRID]).all() and (two[1585:, CONV_UNITS] > 4 * 768).all()


def test_one_and_two_units_make_small_launches_large():
    """the token counts tests/test_gpu_front_plan.py takes its cases from"""
    two = hook(1, 0)
    heights = {4: [(1, 64)], 5: [(65, 80), (129, 160)], 6: [(81, 96), (161, 192), (257, 257)], 7: [(97, 112), (193, 224), (513, 513)], 8: [(113, 128), (225, 256)]}
    for nb, spans in heights.items():
        for lo, hi in spans:
            assert (two[lo - 1:hi, FC_ROWS] == 16 * nb).all(), (nb, lo, hi)
    assert (two[:, CONV_GRID] <= 3).all() and at(two, 63).conv_units == 123 and at(two, 513).conv_units == 994     # 11 and 83 trips of 12 units
    two2 = hook(2, 0)
    assert (two2[:128, FC_ROWS] == 64).all()
    assert [int(np.flatnonzero(two2[:, FC_ROWS] == 16 * nb)[0]) + 1 for nb in (5, 6, 7, 8)] == [129, 161, 193, 225]
    auto = hook(1)
    assert [bool(auto[n - 1, FUSED]) for n in (90, 91, 128, 129, 216, 217, 256, 257)] == [False, True, True, False, False, True, True, False]
