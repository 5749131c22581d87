"""The canonical copy-constraint permutation of typlonk_permutation_from_pairs in Python integers and numpy: the pairs generate
an equivalence relation on the cells 0 .. cells - 1; inside a class the cells ascend and each maps to the next, the highest to
the lowest.  A union-find for the classes (the lower root wins, so a class's label is its lowest cell), a stable argsort by
label, successor linking.  Shared by the CPU and the GPU tests of the feature; nothing here calls the library."""
import numpy as np


def labels(cells, pairs):
    """label[x] = the lowest cell of x's class"""
    parent = list(range(cells))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for a, b in pairs:
        a, b = int(a), int(b)
        if not (0 <= a < cells and 0 <= b < cells):
            raise ValueError(f"pair ({a}, {b}) names a cell that is not below {cells}")
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(x) for x in range(cells)], dtype=np.uint32)


def link(label):
    """(perm, classes) of a label array: cells in (label, cell) order, each linked to the next of its run, the last to the first"""
    label = np.asarray(label, dtype=np.uint32)
    cells = label.shape[0]
    order = np.argsort(label, kind="stable").astype(np.uint32)
    sorted_label = label[order]
    nxt = np.empty(cells, dtype=np.uint32)
    nxt[:-1] = order[1:]
    last = np.ones(cells, dtype=bool)
    last[:-1] = sorted_label[1:] != sorted_label[:-1]
    nxt[last] = sorted_label[last]          # a run's first cell is its label
    perm = np.empty(cells, dtype=np.uint32)
    perm[order] = nxt
    return perm, int(last.sum())


def canonical(cells, pairs):
    """(perm as a uint32 array, classes)"""
    return link(labels(cells, pairs))


def pairs_array(pairs):
    """any pair list as the (count, 2) uint32 array the library takes"""
    return np.ascontiguousarray(np.asarray(list(pairs), dtype=np.uint32).reshape(-1, 2))
