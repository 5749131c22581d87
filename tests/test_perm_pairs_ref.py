"""perm_pairs_ref, the reference of typlonk_permutation_from_pairs, pinned without a GPU: against a brute force that takes the
classes by breadth-first search over the pairs, against witness_check_ref.cycles_of, and under every rearrangement of the pair
list that must not matter."""
import itertools
import random

import numpy as np
import pytest

import perm_pairs_ref as P
import witness_check_ref as W


def brute_classes(cells, pairs):
    """the classes as sorted lists, by breadth-first search over the pairs' graph"""
    adj = {x: set() for x in range(cells)}
    for a, b in pairs:
        adj[a].add(b)
        adj[b].add(a)
    seen, out = set(), []
    for x in range(cells):
        if x in seen:
            continue
        comp, frontier = {x}, [x]
        while frontier:
            frontier = [z for y in frontier for z in adj[y] if z not in comp and not comp.add(z)]
        seen |= comp
        out.append(sorted(comp))
    return out


def brute_perm(cells, pairs):
    perm = list(range(cells))
    classes = brute_classes(cells, pairs)
    for c in classes:
        for i, x in enumerate(c):
            perm[x] = c[(i + 1) % len(c)]
    return perm, len(classes)


def random_pairs(cells, count, rng):
    return [(rng.randrange(cells), rng.randrange(cells)) for _ in range(count)]


@pytest.mark.parametrize("cells", [6, 24])
def test_reference_equals_the_brute_force(cells):
    rng = random.Random(1900 + cells)
    lists = [[], [(0, cells - 1)], [(x, x) for x in range(cells)], [(x, x + 1) for x in range(cells - 1)]]
    lists += [random_pairs(cells, count, rng) for count in (1, 2, 3, cells // 2, cells, 3 * cells) for _ in range(20)]
    if cells == 6:   # every graph on three of the cells, and every single pair
        lists += [list(c) for r in range(4) for c in itertools.combinations(itertools.combinations((0, 3, 5), 2), r)]
        lists += [[p] for p in itertools.product(range(6), repeat=2)]
    for pairs in lists:
        perm, classes = P.canonical(cells, pairs)
        want, want_classes = brute_perm(cells, pairs)
        assert perm.dtype == np.uint32 and perm.tolist() == want and classes == want_classes, pairs


@pytest.mark.parametrize("cells", [6, 24, 96])
def test_cycles_are_the_classes_and_ascend_from_their_lowest_cell(cells):
    rng = random.Random(1950 + cells)
    for count in (0, 1, cells // 3, cells, 2 * cells):
        pairs = random_pairs(cells, count, rng)
        perm, classes = P.canonical(cells, pairs)
        cycles = W.cycles_of(perm.tolist())
        assert sorted(map(sorted, cycles)) == brute_classes(cells, pairs) and len(cycles) == classes
        for c in cycles:
            assert c == sorted(c)      # cycles_of starts a cycle at its lowest cell: the walk then only ever ascends
        lab = P.labels(cells, pairs)
        assert all(lab[x] == c[0] for c in cycles for x in c)


def test_only_the_partition_matters():
    cells, rng = 48, random.Random(1999)
    for count in (5, 20, 60):
        pairs = random_pairs(cells, count, rng)
        want, classes = P.canonical(cells, pairs)
        shuffled = list(pairs)
        rng.shuffle(shuffled)
        flipped = [(b, a) for a, b in pairs]
        doubled = pairs + pairs[::2] + [(x, x) for x in range(0, cells, 5)]
        # a spanning set of the same partition: every cell tied to its class's lowest
        spanning = [(int(l), x) for x, l in enumerate(P.labels(cells, pairs)) if l != x]
        for other in (shuffled, flipped, doubled, spanning, pairs[::-1]):
            got, got_classes = P.canonical(cells, other)
            assert np.array_equal(got, want) and got_classes == classes


def test_a_cell_outside_the_table_is_refused():
    for bad in ((0, 6), (6, 0), (2**32 - 1, 1)):
        with pytest.raises(ValueError):
            P.canonical(6, [(0, 1), bad])


def test_pairs_array_shapes():
    assert P.pairs_array([]).shape == (0, 2) and P.pairs_array([(1, 2), (3, 4)]).tolist() == [[1, 2], [3, 4]]
    assert P.pairs_array(np.arange(6).reshape(3, 2)).dtype == np.uint32
