"""Adversarial pair lists for typlonk_permutation_from_pairs, written with numpy over `cells` = 3n flat cells and shared by the
host test (2^12 rows) and the GPU test (2^12 and 2^16 rows).  Every list is a (count, 2) uint32 array."""
import numpy as np

# the shapes in which one class holds every cell: classes == 1 and perm[x] = (x + 1) mod cells
ONE_CLASS = ("path_up", "path_down_flipped", "path_shuffled", "star_0", "star_top", "star_mid", "binary_tree", "two_half_paths")
ADVERSARIAL = ONE_CLASS + ("strided_hypercube", "high_classes", "low_digit_classes")


def _arr(a, b):
    return np.ascontiguousarray(np.stack([np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)], axis=1))


def adversarial(shape, cells):
    x = np.arange(cells, dtype=np.int64)
    if shape == "path_up":              # (x, x + 1), ascending
        return _arr(x[:-1], x[1:])
    if shape == "path_down_flipped":    # the same path from the top down, every pair flipped
        return _arr(x[1:][::-1], x[:-1][::-1])
    if shape == "path_shuffled":
        p = _arr(x[:-1], x[1:])
        return np.ascontiguousarray(p[np.random.default_rng(1201).permutation(cells - 1)])
    if shape in ("star_0", "star_top", "star_mid"):   # star_top: every hook has to travel to the minimum
        hub = {"star_0": 0, "star_top": cells - 1, "star_mid": cells // 2}[shape]
        others = x[x != hub]
        return _arr(np.full(cells - 1, hub), others)
    if shape == "binary_tree":          # (x, 2x + 1), (x, 2x + 2)
        kids = np.concatenate([2 * x + 1, 2 * x + 2])
        par = np.concatenate([x, x])
        keep = kids < cells
        return _arr(par[keep], kids[keep])
    if shape == "two_half_paths":       # two paths of half the cells each, joined by the very last pair
        h = cells // 2
        a = np.concatenate([x[:h - 1], x[h:-1], [cells - 1]])
        b = np.concatenate([x[1:h], x[h + 1:], [0]])
        return _arr(a, b)
    if shape == "strided_hypercube":    # (x, x ^ 2^k) for every seventh x and every k
        xs = x[::7]
        a, b = [], []
        for k in range(int(cells - 1).bit_length()):
            y = xs ^ (1 << k)
            keep = y < cells
            a.append(xs[keep])
            b.append(y[keep])
        return _arr(np.concatenate(a), np.concatenate(b))
    if shape == "high_classes":
        # classes {b, b + 1, b + 3} among the lowest cells and the same again 2n higher, in the last column: the labels of
        # the two families differ in the key's top bit alone
        n = cells // 3
        b = np.arange(0, n - 3, 5, dtype=np.int64)
        lo_a, lo_b = np.concatenate([b + 3, b + 1]), np.concatenate([b, b + 3])
        return _arr(np.concatenate([lo_a + 2 * n, lo_a]), np.concatenate([lo_b + 2 * n, lo_b]))
    if shape == "low_digit_classes":    # class L = {L, L + 256, L + 512, ...} for L < 256: labels differ in the lowest digit alone
        return _arr(x[256:][::-1], x[:-256][::-1])
    raise ValueError(shape)
