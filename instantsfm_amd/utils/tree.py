"""MaximumSpanningTree -- drop-in for ``instantsfm/utils/tree.py`` (reference :7-47) without networkx.

Kruskal over the valid pairs between registered images, weighted by ``len(pair.inliers)``, heaviest first, with the
package's UnionFind; then a breadth-first walk from image 0 gives every image's parent.  Tie rule: of two pairs with
the same number of inliers the one that comes first in the view graph (``view_graph.image_pairs`` order) is tried
first.  Where all weights differ the tree is unique and the rule never acts.

The root is image 0 whatever its state, as in the reference: when image 0 is not registered (or has no valid pair)
nothing is reachable and every other parent is -1.
"""
from collections import deque

from .union_find import UnionFind


def BFS(edges_list, root=0):
    """tree.py:7-23: parents over the adjacency lists, ``parents[root] = root``, -1 for what the root does not reach."""
    parents = [-1] * len(edges_list)
    if not edges_list:
        return parents
    parents[root] = root
    queue = deque([root])
    while queue:
        current = queue.popleft()
        for neighbor in edges_list[current]:
            if parents[neighbor] == -1:
                parents[neighbor] = current
                queue.append(neighbor)
    return parents


def MaximumSpanningTree(view_graph, images):
    """tree.py:25-47: ``(parents, 0)``."""
    edges = []
    for order, pair in enumerate(view_graph.image_pairs.values()):
        if not pair.is_valid:
            continue
        if not images[pair.image_id1].is_registered or not images[pair.image_id2].is_registered:
            continue
        edges.append((-len(pair.inliers), order, pair.image_id1, pair.image_id2))
    edges.sort()  # heaviest first, ties by view-graph order
    forest = UnionFind()
    edges_list = [[] for _ in range(len(images))]
    for _, _, u, v in edges:
        if forest.Find(u) != forest.Find(v):
            forest.Union(u, v)
            edges_list[u].append(v)
            edges_list[v].append(u)
    return BFS(edges_list), 0
