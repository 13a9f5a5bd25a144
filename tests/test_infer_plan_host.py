"""not-gpu: the launch plan of herro_job_infer (csrc/infer_plan.h: plan_batches, group_batches, build_launch) through herro_debug_launch_plan,
against a plain restatement of its rules: the two flush rules of the batches (inference.rs:241-250, features.rs:884-893), launch groups of whole
batches under 2^16 tokens, and per group the split into the windows the fused stack takes and the rest.  The order inside a fused part is the
token-tile plan's (api.debug_tile_plan_sib on that part's counts, tested on its own in test_host_job_layout.py).  Every window must agree on its
launch, its position in the launch and the padding length it carries."""
import numpy as np
import pytest

from herro_amd import api

TOK_CAP = 1 << 16
NONE = 0xFFFFFFFF


def batches_of(nsup, two, bs, mode):
    out, cur = [], []

    def flush():
        if cur:
            out.append(list(cur))
            cur.clear()
    if mode == 0:      # per target: a flush after every `bs` windows SEEN, informative or not, and one at the target's end
        for t in range(len(two) - 1):
            seen = 0
            for w in range(two[t], two[t + 1]):
                if nsup[w] > 0:
                    cur.append(w)
                seen += 1
                if seen == bs:
                    flush()
                    seen = 0
            flush()
    else:              # chunks of `bs` informative windows across the job
        for w in range(len(nsup)):
            if nsup[w] > 0:
                cur.append(w)
                if len(cur) == bs:
                    flush()
        flush()
    return out


def groups_of(batches, nsup):
    out, tok = [], 0
    for b in batches:
        t = sum(int(nsup[w]) for w in b)
        if out and tok + t <= TOK_CAP:
            out[-1].append(b)
            tok += t
        else:          # (a batch above the cap lands here too, and the next one cannot join it)
            out.append([b])
            tok = t
    return out


def expected(nsup, Lf, two, bs, mode, fused, rows, packed, qmode, n_cu):
    n = len(nsup)
    launch, pos, lmax = np.full(n, NONE, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    n_launch = 0
    batches = batches_of(nsup, two, bs, mode)
    for g in groups_of(batches, nsup):
        wins = [w for b in g for w in b]
        for b in g:
            for w in b:
                lmax[w] = max(int(Lf[v]) for v in b)
        small = [w for w in wins if not (fused and nsup[w] > rows)]
        large = [w for w in wins if fused and nsup[w] > rows]
        if small and fused:
            order = api.debug_tile_plan_sib(np.array([nsup[w] for w in small], np.uint32), packed=packed, qmode=qmode, n_cu=n_cu)[3]
            small = [small[i] for i in order]
        for part in (small, large):
            if part:
                for k, w in enumerate(part):
                    launch[w], pos[w] = n_launch, k
                n_launch += 1
    return n_launch, launch, pos, lmax, batches


def check(nsup, Lf, two, bs, mode, fused=True, rows=512, packed=True, qmode=1, n_cu=256):
    nsup, Lf = np.asarray(nsup, np.uint32), np.asarray(Lf, np.uint32)
    want = expected(nsup, Lf, two, bs, mode, fused, rows, packed, qmode, n_cu)
    got = api.debug_launch_plan(nsup, Lf, two, bs, mode, fused=fused, fused_rows=rows, packed=packed, qmode=qmode, n_cu=n_cu)
    ctx = (bs, mode, fused, rows, packed, qmode, n_cu, nsup.tolist(), list(two))
    assert got[0] == want[0], ctx
    assert got[1].astype(np.int64).tolist() == want[1].tolist(), ctx
    inf = nsup > 0
    assert got[2][inf].astype(np.int64).tolist() == want[2][inf].tolist(), ctx
    assert got[3][inf].astype(np.int64).tolist() == want[3][inf].tolist(), ctx
    return want


# targets: 0 without windows; 1 with 6 windows (a multiple of 1, 2, 3: the flush at its end finds nothing); 2 with 7, windows without informative
# rows in the middle of its batches; 3 with one window; 4 without informative rows at all
NSUP = [5, 9, 3, 7, 2, 8] + [4, 0, 6, 0, 0, 11, 1] + [13] + [0, 0]
LF = [100, 140, 90, 200, 120, 130] + [300, 999, 310, 999, 999, 250, 260] + [77] + [500, 600]
TWO = [0, 0, 6, 13, 14, 16]


@pytest.mark.parametrize("bs", [1, 2, 3, 64])
@pytest.mark.parametrize("mode", [0, 1])
def test_flush_rules(bs, mode):
    want = check(NSUP, LF, TWO, bs, mode)
    batches = want[4]
    if mode == 0 and bs == 2:     # windows 7, 9, 10 count as seen: (6, 7) (8, 9) (10, 11) (12) -> the batch of 11 is alone, padding length 250
        assert batches == [[0, 1], [2, 3], [4, 5], [6], [8], [11], [12], [13]]
    if mode == 1 and bs == 2:     # they do not count: chunks of two informative windows, across targets
        assert batches == [[0, 1], [2, 3], [4, 5], [6, 8], [11, 12], [13]]
    if mode == 0 and bs == 3:     # target 1's end finds nothing to flush after (3, 4, 5)
        assert batches == [[0, 1, 2], [3, 4, 5], [6, 8], [11], [12], [13]]
    assert want[0] == 1           # one group, everything fits the fused stack


def test_job_without_informative_windows_has_no_launch():
    for mode in (0, 1):
        n, launch, _, _ = api.debug_launch_plan([0, 0, 0], [10, 20, 30], [0, 2, 3], 2, mode)
        assert n == 0 and launch.tolist() == [NONE] * 3
    assert api.debug_launch_plan([], [], [0], 4, 0)[0] == 0
    assert api.debug_launch_plan([], [], [0, 0, 0], 4, 1)[0] == 0


@pytest.mark.parametrize("rows", [64, 512])
def test_split_around_the_fused_row_cap(rows):
    nsup = [rows, 3, rows + 1, rows - 1, 17, rows + 1, 1]
    Lf = [1000 + i for i in range(len(nsup))]
    for mode in (0, 1):
        for packed in (True, False):
            want = check(nsup, Lf, [0, 4, 7], 3, mode, rows=rows, packed=packed)
            assert want[0] == 2
            assert [want[1][w] for w in (2, 5)] == [1, 1] and [want[2][w] for w in (2, 5)] == [0, 1]   # the windows above the cap, in batch order
    want = check([rows + 1, rows + 1], Lf[:2], [0, 2], 2, 0, rows=rows)    # nothing fits: one launch, the unfused one
    assert want[0] == 1
    want = check(nsup, Lf, [0, 4, 7], 3, 0, fused=False, rows=rows)        # an unfused precision: one part, batch order
    assert want[0] == 1 and want[2].tolist() == list(range(len(nsup)))


def test_launch_groups_under_the_token_cap():
    # two batches of 40 000 rows each: two groups
    nsup = [400] * 200
    want = check(nsup, [50] * 200, [0, 200], 100, 1)
    assert want[0] == 2 and want[1][:100].tolist() == [0] * 100 and want[1][100:].tolist() == [1] * 100
    # one batch of 70 000 rows between two small ones: a group of its own, and the small ones do not join it
    nsup = [10] * 10 + [400] * 175 + [10] * 10
    Lf = [60] * 10 + [70] * 175 + [80] * 10
    want = check(nsup, Lf, [0, 10, 185, 195], 175, 0)
    assert want[0] == 3 and sorted(set(want[1].tolist())) == [0, 1, 2]
    assert set(want[1][10:185].tolist()) == {1} and set(want[3][10:185].tolist()) == {70}
    # 65 536 rows exactly share a group, one more row does not
    assert check([256] * 256, [9] * 256, [0, 128, 256], 128, 0)[0] == 1
    assert check([256] * 255 + [257], [9] * 256, [0, 128, 256], 128, 0)[0] == 2


def test_seeded_random_jobs():
    rng = np.random.default_rng(20240611)
    pool = np.array([0, 0, 1, 2, 5, 15, 16, 30, 31, 32, 33, 63, 64, 65, 100, 511, 512, 513, 700, 30000], np.uint32)
    for trial in range(300):
        n = int(rng.integers(0, 41))
        nsup = rng.choice(pool, n) if trial % 3 else rng.integers(0, 40, n).astype(np.uint32)
        Lf = rng.integers(1, 5000, n).astype(np.uint32)
        n_t = int(rng.integers(0, 6))
        two = [0] + sorted(int(x) for x in rng.integers(0, n + 1, max(n_t - 1, 0))) + [n] if n_t else [0]
        if not n_t:
            nsup, Lf = nsup[:0], Lf[:0]
        check(nsup, Lf, two, int(rng.choice([1, 2, 3, 4, 7, 64])), int(rng.integers(0, 2)), fused=bool(rng.integers(0, 4)),
              rows=int(rng.choice([64, 512])), packed=bool(rng.integers(0, 2)), qmode=int(rng.integers(0, 3)), n_cu=int(rng.choice([4, 8, 256])))


def test_arguments_are_checked():
    with pytest.raises(api.HerroError):
        api.debug_launch_plan([1], [1], [0, 1], 0)           # batch size 0, as herro_job_infer refuses it
    with pytest.raises(api.HerroError):
        api.debug_launch_plan([1], [1], [0, 2], 1)           # a target reaching past the windows
