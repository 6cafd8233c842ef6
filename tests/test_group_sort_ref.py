"""The sort form of grouped aggregates without a device
(include/mbx_group_sort.h): the numpy restatement (tests/group_sort_ref.py)
against a brute-force dict loop on random small inputs, and the proof that the
shapes of tests/test_group_sort.py put their run boundaries on the seams they
claim -- asserted on the restated launch geometry (index_grid, 256-entry rounds,
64-lane waves)."""
import numpy as np
import pytest

import group_sort_ref as S


def same(a, b, what):
    assert a["keys"] == b["keys"], (what, "keys")
    assert np.array_equal(a["first"], b["first"]), (what, "first")
    S.same_aggregates(a, b, what)


@pytest.mark.parametrize("seed", range(6))
def test_reference_equals_brute_force(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(rng.integers(1, 400))
    ints = rng.integers(-3, 4, n, dtype=np.int32)
    wide = rng.choice(np.array([S.I32_MIN, -1, 0, 1, S.I32_MAX], dtype=np.int32), n)
    names = S.pad_bytes([bytes(rng.choice([b"a", b"ab", b"abc", b"b"])) for _ in range(n)], 5)
    mask = rng.random(n) < 0.8
    vi = rng.integers(S.I32_MIN, S.I32_MAX, n, dtype=np.int32, endpoint=True)
    vf = (rng.integers(-2048, 2048, n) / 1024.0).astype(np.float32)
    vf[rng.random(n) < 0.05] = np.float32("nan")
    vf[rng.random(n) < 0.05] = np.float32(-0.0)
    for key_cols in ([ints], [wide], [names], [ints, wide], [names, ints], [wide, names, ints]):
        for values in (None, vi, vf):
            same(S.group_sort_ref(mask, key_cols, values), S.brute_force(mask, key_cols, values),
                 (seed, len(key_cols), None if values is None else values.dtype))
    none = np.zeros(n, dtype=bool)
    assert S.group_sort_ref(none, [ints], vf)["keys"] == [] and len(S.group_sort_ref(none, [ints], vf)["sum"]) == 0


def test_signed_and_byte_order():
    wide = np.array([S.I32_MAX, 0, S.I32_MIN, -1, 1], dtype=np.int32)
    got = S.group_sort_ref(np.ones(5, dtype=bool), [wide])
    assert [k[0] for k in got["keys"]] == [S.I32_MIN, -1, 0, 1, S.I32_MAX] and list(got["first"]) == [2, 3, 1, 4, 0]
    names = S.pad_bytes([b"b", b"ab", b"a", b"a\x7f"], 3)
    assert [k[0].rstrip(b"\0") for k in S.group_sort_ref(np.ones(4, dtype=bool), [names])["keys"]] == \
        [b"a", b"ab", b"a\x7f", b"b"]      # bytes, not characters: 'b' is 0x62


def test_a_sum_starts_from_plus_zero_and_min_max_order_the_zeros():
    v = np.array([-0.0, -0.0, 0.0, np.nan, np.nan], dtype=np.float32)
    k = np.array([0, 0, 0, 1, 1], dtype=np.int32)
    got = S.group_sort_ref(np.ones(5, dtype=bool), [k], v)
    assert not np.signbit(got["sum"][0]) and np.isnan(got["sum"][1])
    assert np.signbit(got["min"][0]) and not np.signbit(got["max"][0])
    assert got["min"][1] == np.inf and got["max"][1] == -np.inf
    only_neg = S.group_sort_ref(np.ones(2, dtype=bool), [k[:2]], v[:2])
    assert not np.signbit(only_neg["sum"][0])


def test_geometry():
    assert S.index_grid(1) == (1, 1) and S.index_grid(1024) == (1, 1) and S.index_grid(1025) == (1, 2)
    assert S.index_grid(1 << 20) == (1, 1024) and S.index_grid((1 << 20) + 1) == (2, 513)
    assert S.index_grid(S.TWO_TILE_N) == (2, 513)
    assert S.coords(0, 5000) == (0, 0, 0, 0) and S.coords(63, 5000) == (0, 0, 0, 63)
    assert S.coords(64, 5000) == (0, 0, 1, 0) and S.coords(256, 5000) == (0, 1, 0, 0)
    assert S.coords(1024, 5000) == (1, 0, 0, 0)
    assert S.coords(1024, S.TWO_TILE_N) == (0, 4, 0, 0) and S.coords(2048, S.TWO_TILE_N) == (1, 0, 0, 0)


@pytest.mark.parametrize("runs", [S.SEAM_RUNS_ONES, S.SEAM_RUNS_LONG, S.HEADLESS_RUNS, S.INT64_RUNS, S.NAN_RUNS])
def test_place_runs_puts_the_runs_where_it_says(runs):
    keys, rows_of_entry = S.place_runs(runs)
    n = sum(runs)
    rows, heads = S.sorted_rows(np.ones(n, dtype=bool), [keys])
    assert np.array_equal(rows, rows_of_entry)
    assert list(np.nonzero(heads)[0]) == list(np.cumsum([0] + runs)[:-1])
    assert not np.array_equal(rows, np.arange(n))      # the sort has work to do


def test_the_seam_shapes_end_runs_on_every_seam():
    for runs in (S.SEAM_RUNS_ONES, S.SEAM_RUNS_LONG):
        n = sum(runs)
        ends = set(np.cumsum(runs)[:-1])       # entry e: a run ends at e - 1 | e
        assert S.index_grid(n) == (1, 2)
        assert {64, 256, 1024} <= ends
        assert "wave" in S.seam_kinds(64, n) and "round" not in S.seam_kinds(64, n)
        assert "round" in S.seam_kinds(256, n) and "block" not in S.seam_kinds(256, n)
        assert "block" in S.seam_kinds(1024, n)
    # one-entry runs on both sides of each seam
    starts = list(np.cumsum([0] + S.SEAM_RUNS_ONES)[:-1])
    for e in (63, 64, 255, 256, 1023, 1024):
        assert S.SEAM_RUNS_ONES[starts.index(e)] == 1, e


def test_the_carry_shapes_leave_blocks_without_a_head():
    assert sum(S.HEADLESS_RUNS) == 3074 and S.index_grid(3074) == (1, 4)
    assert S.blocks_without_a_head(S.HEADLESS_RUNS) == [1, 2]       # the carry passes through two headless blocks
    assert S.coords(3073, 3074)[0] == 3                            # the last run's head is in block 3
    assert S.blocks_without_a_head([2049]) == [1, 2]               # one group over three blocks
    assert S.blocks_without_a_head([1] * 2049) == []               # every row its own group


def test_the_two_tile_shape_crosses_a_tile_edge_inside_a_block():
    runs = S.two_tile_runs()
    assert sum(runs) == S.TWO_TILE_N and S.index_grid(S.TWO_TILE_N)[0] == 2
    assert runs[0] < 1024 < runs[0] + runs[1]                      # run 1 holds entries 1000 .. 1099
    assert S.seam_kinds(1024, S.TWO_TILE_N) == {"tile", "round", "wave"}      # a tile edge, not a block seam
    assert "block" in S.seam_kinds(2048, S.TWO_TILE_N)


def test_the_int64_and_nan_shapes_span_their_seams():
    n = sum(S.INT64_RUNS)
    lo, hi = S.INT64_RUNS[0], S.INT64_RUNS[0] + S.INT64_RUNS[1]
    assert S.INT64_RUNS[1] == 1025 and lo < 1024 < hi and "block" in S.seam_kinds(1024, n)
    assert 1025 * S.I32_MAX > (1 << 32) and 1025 * S.I32_MIN < -(1 << 32)
    lo, hi = S.NAN_RUNS[0], S.NAN_RUNS[0] + S.NAN_RUNS[1]
    assert lo < 64 < hi and S.seam_kinds(64, sum(S.NAN_RUNS)) == {"wave"}


def test_the_tail_lane_sizes_cover_every_partial_unit():
    sizes = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]
    assert {S.coords(n - 1, n)[3] for n in sizes} >= {0, 62, 63}            # last lane: first, last, one short
    assert {S.index_grid(n)[1] for n in sizes} == {1, 2, 3}
    assert {S.coords(n - 1, n)[1] for n in sizes} >= {0, 1, 3}              # rounds
