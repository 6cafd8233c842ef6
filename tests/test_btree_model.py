"""The tie order of a BTREE scan (include/mbx_index.h): entries with equal keys
leave the reference's B-tree in insertion order, i.e. by ascending position,
so the GPU index's (key, position) order is the leaf walk's.  No recorded
transcript holds a `query ... BTREE`; tests/btree_model.py restates the insert
path, and this file holds its leaf walk against sorted((key, position)).

Page capacities 4 and 6: even, as the reference's leaf of int keys is
((1024 - 20) // 16 = 62 entries), small enough that every input below splits
leaves and index pages and descends three or more levels.

Where the claim ends (pinned below, so that nobody reads more into it):
  * an odd capacity lets the leaf split's undo step run
    (R/btree/BTreeFile.java:882-893); its sorted insert puts the entry after
    the equal keys already on the new page.  Capacity 5 with descending runs
    of 7 equal keys: 30 inserts leave a walk that is not in position order;
  * an index-page split whose inserted separator belongs on the old page moves
    that page's last entry to the new page by a sorted insert (:719-736); when
    it equals the new page's first separator it lands behind it, and later
    equal keys descend to the older leaf.  Keys cycling 0, 1, 2 at capacity 4:
    120 inserts do it.
Both need a run of equal keys across a page boundary at the moment of a split.
The GPU index returns (key, position) order always: where the reference's tree
would have scrambled a run of equal keys, the divergence is deliberate
(DESIGN.md)."""
import pytest

import btree_model

CAPACITIES = [4, 6]
SIZES = [1, 5, 37, 120, 400]

INPUTS = {
    "all_equal": lambda n: [7] * n,
    "two_alternating": lambda n: [5 if i % 2 else -3 for i in range(n)],
    "runs_straddling_splits": lambda n: [i // 7 for i in range(n)],       # runs of 7 > one page
    "long_runs": lambda n: [i // 23 for i in range(n)],                   # a run spans several leaves
    "ascending": lambda n: list(range(n)),
    "descending": lambda n: list(range(n, 0, -1)),
    "descending_pairs": lambda n: [-(i // 2) for i in range(n)],
}


@pytest.mark.parametrize("capacity", CAPACITIES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_leaf_walk_is_key_then_position(name, n, capacity):
    keys = INPUTS[name](n)
    t = btree_model.build(keys, capacity)
    walk = t.leaf_walk()
    assert walk == sorted((k, p) for p, k in enumerate(keys))
    assert t.undo_moves == 0  # an even capacity never takes the undo step


@pytest.mark.parametrize("capacity", CAPACITIES)
def test_the_inputs_split_and_descend(capacity):
    """the model is exercised: several levels, not one root leaf"""
    for name in INPUTS:
        assert btree_model.build(INPUTS[name](400), capacity).height() >= 3, name


def test_sorted_insert_lands_after_equal_keys():
    page = [(1, 0), (2, 1), (2, 2), (3, 3)]
    btree_model._sorted_insert(page, (2, 9))
    assert page == [(1, 0), (2, 1), (2, 2), (2, 9), (3, 3)]


def test_descent_takes_the_rightmost_child_not_above_the_key():
    ix = btree_model.Index()
    ix.prev = "p"
    ix.entries = [(2, "a"), (2, "b"), (5, "c")]
    assert [ix.child_for(k) for k in (1, 2, 3, 5, 9)] == ["p", "b", "b", "c", "c"]


def _keys_ascend_and_nothing_is_lost(keys, walk):
    assert [k for k, _ in walk] == sorted(keys)
    assert sorted(walk) == sorted((k, p) for p, k in enumerate(keys))


def test_odd_capacity_undo_step_reorders_equal_keys():
    keys = [-(i // 7) for i in range(30)]
    t = btree_model.build(keys, 5)
    walk = t.leaf_walk()
    _keys_ascend_and_nothing_is_lost(keys, walk)
    assert t.undo_moves > 0 and walk != sorted(walk)


def test_index_split_can_reorder_equal_separators():
    keys = [i % 3 for i in range(120)]
    t = btree_model.build(keys, 4)
    walk = t.leaf_walk()
    _keys_ascend_and_nothing_is_lost(keys, walk)
    assert t.undo_moves == 0 and walk != sorted(walk)
