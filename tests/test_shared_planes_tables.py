"""The CNF lists of tests/shared_planes_cases.py reach the truth tables the plane-group tests
(tests/test_graph_shared_planes.py) rely on: each CNF is evaluated here on every combination of
its plane bits, as bits1_plan_of (mbx_planes.hip) does on probe words before a launch."""
import helpers  # noqa: F401
import shared_planes_cases as cases


def _tables(cnfs, cols):
    return [cases.truth_table(c, cols) for c in cnfs]


def test_two_planes_reach_fourteen_tables():
    tables = _tables(cases.NP2_CNFS, (1, 2))
    assert len(set(tables)) == len(tables) == 14 >= 12
    # bit i of a table: x0 = bit 0 of i, x1 = bit 1 of i
    assert tables[0] == 0b0001 and tables[1] == 0b0111          # ~x0 & ~x1, ~x0 | ~x1
    assert tables[8:12] == [0b0101, 0b1010, 0b0011, 0b1100]     # ~x0, x0, ~x1, x1
    assert tables[12:] == [0b1111, 0b0000]                      # both constant tables
    assert set(range(16)) - set(tables) == {0b0110, 0b1001}     # XOR and XNOR: not two reading terms
    assert sum(t & 1 for t in tables) >= 6                      # tables that select the all-zero minterm


def test_other_slots_give_the_same_tables():
    assert _tables(cases.np2_cnfs(3, 4), (3, 4)) == _tables(cases.NP2_CNFS, (1, 2))


def test_one_three_and_four_planes():
    assert _tables(cases.NP1_CNFS, (1,)) == [0b01, 0b10]
    for cnfs, cols in [(cases.NP3_CNFS, (1, 2, 3)), (cases.NP4_CNFS, (1, 2, 3, 4))]:
        tables = _tables(cnfs, cols)
        assert len(set(tables)) == len(tables) >= 4
        assert tables[0] == 1                                   # the all-zero minterm alone
        assert tables[1] & 1 and tables[1] != 1                 # and with others
        assert all(0 < t < (1 << (1 << len(cols))) - 1 for t in tables)
