"""The reference B-tree's insert path, restated small (R/ = minijava/src of
the reference), to check the order in which a leaf walk returns entries with
equal keys -- the tie order of a BTREE scan (include/mbx_index.h).  No
recorded transcript holds a `query ... BTREE`, so this model is the evidence.

Restated:
  * BTSortedPage.insertRecord (R/btree/BTSortedPage.java:124-142): the new
    entry is appended and moved down only while it is STRICTLY less than its
    neighbour, so it lands after every equal key of the page;
  * BTIndexPage.getPageNoByKey (R/btree/BTIndexPage.java:164-172): descend to
    the rightmost child whose separator is <= the key, else the leftmost child;
  * the leaf split (R/btree/BTreeFile.java:854-915): every entry moves to the
    new page, entries move back from its front while the new page has less
    space than the old one; if the inserted key is less than the last entry
    moved back (`undoEntry`) and the old page now has less space than the new
    one, that entry is moved to the new page again -- by a sorted insert; the
    key goes to the new page when it is >= undoEntry's key, else to the old;
  * the index split (R/btree/BTreeFile.java:632-762) and the new root.

Pages hold `capacity` entries of one size (available space = capacity - count),
so splits and multi-level descents happen within a few dozen inserts.  The
reference's leaf of int keys holds (1024 - 20) // (4 + 8 + 4) = 62 entries: an
even number, so a split leaves both pages equally full and the undo step never
runs (it needs the old page to be fuller).  With an odd capacity -- or entries
of different sizes, as string keys have -- the undo step can run, and its
sorted insert puts the entry AFTER the equal keys already on the new page:
test_btree_model.py pins both facts.
"""


def _sorted_insert(entries, entry):
    """BTSortedPage.insertRecord: append, then swap down while strictly less"""
    entries.append(entry)
    i = len(entries) - 1
    while i > 0 and entries[i][0] < entries[i - 1][0]:
        entries[i], entries[i - 1] = entries[i - 1], entries[i]
        i -= 1


class Leaf:
    def __init__(self):
        self.entries = []  # (key, position)
        self.next = None


class Index:
    def __init__(self):
        self.prev = None   # the leftmost child
        self.entries = []  # (separator key, child)

    def child_for(self, key):
        """getPageNoByKey"""
        for k, child in reversed(self.entries):
            if key >= k:
                return child
        return self.prev


class BTree:
    def __init__(self, capacity):
        assert capacity >= 3
        self.capacity = capacity
        self.root = None
        self.undo_moves = 0  # leaf splits whose undo step ran

    def _space(self, page):
        return self.capacity - len(page.entries)

    def insert(self, key, position):
        """BTreeFile.insert: an empty tree gets a leaf root; a split of the
        root gets an index root over the two halves (:377-466)"""
        if self.root is None:
            self.root = Leaf()
        up = self._insert(self.root, key, position)
        if up is not None:
            root = Index()
            root.prev = self.root
            root.entries.append(up)
            self.root = root

    def _insert(self, page, key, position):
        if isinstance(page, Index):
            up = self._insert(page.child_for(key), key, position)
            if up is None:
                return None
            if self._space(page) >= 1:
                _sorted_insert(page.entries, up)
                return None
            return self._split_index(page, up)
        if self._space(page) >= 1:
            _sorted_insert(page.entries, (key, position))
            return None
        return self._split_leaf(page, key, position)

    def _split_leaf(self, cur, key, position):
        new = Leaf()
        new.next, cur.next = cur.next, new
        for e in cur.entries:                       # :854-863
            _sorted_insert(new.entries, e)
        cur.entries = []
        undo = None
        while self._space(new) < self._space(cur):  # :871-880
            undo = new.entries.pop(0)
            _sorted_insert(cur.entries, undo)
        if key < undo[0] and self._space(cur) < self._space(new):  # :882-893
            _sorted_insert(new.entries, undo)
            cur.entries.pop()
            self.undo_moves += 1
        if key >= undo[0]:                          # :899-915
            _sorted_insert(new.entries, (key, position))
        else:
            _sorted_insert(cur.entries, (key, position))
        return (new.entries[0][0], new)             # :927-928

    def _split_index(self, cur, up):
        new = Index()
        for e in cur.entries:                       # :665-671
            _sorted_insert(new.entries, e)
        cur.entries = []
        undo = None
        while self._space(cur) > self._space(new):  # :680-691
            undo = new.entries.pop(0)
            _sorted_insert(cur.entries, undo)
        if self._space(cur) < self._space(new):     # :694-703
            _sorted_insert(new.entries, undo)
            cur.entries.pop()
        if up[0] >= new.entries[0][0]:              # :711-736
            _sorted_insert(new.entries, up)
        else:
            _sorted_insert(cur.entries, up)
            _sorted_insert(new.entries, cur.entries.pop())
        first = new.entries.pop(0)                  # :742-760
        new.prev = first[1]
        return (first[0], new)

    def leaf_walk(self):
        """BTFileScan from the leftmost leaf: (key, position) in scan order"""
        page = self.root
        if page is None:
            return []
        while isinstance(page, Index):
            page = page.prev
        out = []
        while page is not None:
            out += page.entries
            page = page.next
        return out

    def height(self):
        h, page = 0, self.root
        while page is not None:
            h += 1
            page = page.prev if isinstance(page, Index) else None
        return h


def build(keys, capacity):
    """createBTreeIndex (R/columnar/Columnarfile.java:659-689): every record
    of the column in scan order, key = its value, rid = its position"""
    t = BTree(capacity)
    for position, key in enumerate(keys):
        t.insert(key, position)
    return t
