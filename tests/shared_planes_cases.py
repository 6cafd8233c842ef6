"""CNFs for the plane groups of fused COUNT scans (tests/test_graph_shared_planes.py) and their
truth tables worked out on the CPU (tests/test_shared_planes_tables.py).

The tables of those tests have int32 columns 1..4 over [0, 2^20), whose top kept bit is 2^19
(HALF), and a two-key column 5 over {6, 7}.  A term `column >= HALF` is the column's plane bit x
and `column < HALF` its complement; `column 5 != 6` is that column's.  A shallow plan reads one
plane per such term, in term order: the plans of one list below all read the same planes in the
same slots, so a chain of them is one plane group, and they differ only in the truth table over
the plane bits (bit i of the table: the rows whose plane-k bit is bit k of i are selected).

Two terms joined by a CNF reach the 4 conjunctions and the 4 disjunctions.  A term that reads no
plane -- `column >= -5` holds for every row of these tables, `column < -5` for none, both
decided from the column's range -- adds the tables that ignore a plane and both constant tables:
14 of the 16 tables over two planes.  x0 XOR x1 and its complement need four reading terms.
"""
import oracle

LT, GE, NE = oracle.LT, oracle.GE, oracle.NE
HALF = 1 << 19
# the value a column takes for plane bit 0 / 1 when a CNF is evaluated on bit combinations
BIT_VALUE = {1: (0, HALF), 2: (0, HALF), 3: (0, HALF), 4: (0, HALF), 5: (6, 7)}


def lt(col):
    return (LT, ("sym", col), ("int", HALF))


def ge(col):
    return (GE, ("sym", col), ("int", HALF))


def true(col):
    return (GE, ("sym", col), ("int", -5))  # reads no plane: every row


def false(col):
    return (LT, ("sym", col), ("int", -5))  # reads no plane: no row


def np2_cnfs(a=1, b=2):
    """14 CNFs over planes (a, b) in these slots, the all-zero minterm's first"""
    out = [[[lt(a)], [lt(b)]], [[lt(a), lt(b)]]]                         # ~x0 & ~x1, ~x0 | ~x1: both select minterm 0
    out += [[[lt(a)], [ge(b)]], [[ge(a)], [lt(b)]], [[ge(a)], [ge(b)]]]  # the other conjunctions
    out += [[[lt(a), ge(b)]], [[ge(a), lt(b)]], [[ge(a), ge(b)]]]        # the other disjunctions
    out += [[[lt(a)], [ge(b), true(a)]], [[ge(a)], [lt(b), true(a)]]]    # ~x0, x0
    out += [[[ge(a), true(a)], [lt(b)]], [[lt(a), true(a)], [ge(b)]]]    # ~x1, x1
    out += [[[ge(a), lt(b), true(a)]], [[lt(a)], [ge(b)], [false(a)]]]   # every row, no row
    return out


NP1_CNFS = [[[lt(1)]], [[ge(1)]]]
NP2_CNFS = np2_cnfs()
NP3_CNFS = [[[lt(1)], [lt(2)], [lt(3)]], [[lt(1), lt(2), lt(3)]], [[ge(1), ge(2), ge(3)]], [[lt(1)], [ge(2), lt(3)]],
            [[ge(1), lt(2)], [ge(3)]]]
NP4_CNFS = [[[lt(1)], [lt(2)], [lt(3)], [lt(4)]], [[lt(1), lt(2)], [lt(3), lt(4)]], [[ge(1), ge(2), ge(3), ge(4)]],
            [[lt(1), ge(2)], [lt(3), ge(4)]], [[ge(1)], [lt(2), lt(3)], [ge(4)]]]


def _holds(op, value, literal):
    return {LT: value < literal, GE: value >= literal, NE: value != literal}[op]


def truth_table(cnf, cols):
    """the CNF evaluated on every combination of the plane bits of cols (slot order)"""
    table = 0
    for i in range(1 << len(cols)):
        value = {c: BIT_VALUE[c][(i >> k) & 1] for k, c in enumerate(cols)}
        if all(any(_holds(op, value[sym[1]], lit[1]) for op, sym, lit in conj) for conj in cnf):
            table |= 1 << i
    return table
