"""UnionFind -- drop-in for ``instantsfm/utils/union_find.py`` (reference :2-23): a dict-backed forest without ranks.
``Union(x, y)`` hangs x's root under y's root; that direction decides every root, and the callers compare roots."""


class UnionFind:
    def __init__(self):
        self.parent = {}

    def Find(self, x):
        """The root of x (x becomes its own root on first sight); the walked path is compressed onto the root."""
        parent = self.parent
        if x not in parent:
            parent[x] = x
            return x
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    def Union(self, x, y):
        root_x, root_y = self.Find(x), self.Find(y)
        if root_x != root_y:
            self.parent[root_x] = root_y

    def Clear(self):
        self.parent.clear()
