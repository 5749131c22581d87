"""CPU half of tests/test_gpu_reduce.py: the harness builds and stays out of the shipped library, the bucket pool holds what
it claims, and the reference of the bit planes is right -- recombined with their powers of two, the planes give the weighted
sum of the buckets computed straight from the bucket weights w(k) = (k >> v) + 1."""
import os
import subprocess

import numpy as np
import pytest

import arith_cases as C
import reduce_cases as RC
from helpers import ROOT
from oracle import bls12_381 as O

HARNESS = os.path.join(ROOT, "tests", "cpp", "libdevice_reduce.so")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_harness_builds_and_exports(built):
    assert os.path.exists(HARNESS)
    assert "dr_reduce" in _exports(HARNESS)
    assert "dr_reduce" not in _exports(os.path.join(ROOT, "typlonk_amd", "libtyplonk_hip.so"))


def test_pool_entries_are_the_points_they_claim():
    pl = RC.pool()
    assert len(pl.e) == 2 * RC.N_POINTS * RC.N_Z + 2 and len(set(map(tuple, pl.words))) == len(pl.e)
    for words, e in zip(pl.words, pl.e):
        c = RC.unpack48(words)
        assert C._xyzz_ok(c) and all(v < 1 << 384 for v in c)
        assert C.xyzz_point(c) == RC.point_of(int(e))
    for (j, sign), ids in pl.of.items():
        assert len(set(pl.e[ids])) == 1 and len({tuple(pl.words[i][24:36]) for i in ids}) == RC.N_Z   # one point, N_Z scalings
        assert pl.e[ids[0]] == -pl.e[pl.of[(j, -sign)][0]]
    assert list(pl.e[pl.identity]) == [0, 0]
    assert RC.point_of(5) == O.g1_mul(O.G1, 5) and RC.point_of(-5) == O.g1_mul(O.G1, O.R - 5) and RC.point_of(0) is None


SHAPES = [(8, 1, 0), (13, 1, 0), (14, 1, 0), (17, 1, 0), (18, 1, 0), (20, 1, 0)] \
    + [(c, 3, v) for c in (8, 13) for v in (0, 1, RC.shape_of(c)["cl"], RC.shape_of(c)["cl"] + 2)]


@pytest.mark.parametrize("c,nsets,top_v", SHAPES)
def test_reference_planes_recombine_to_the_weighted_sum(c, nsets, top_v):
    sh = RC.shape_of(c, nsets, top_v)
    assert sh["cl"] + sh["ch"] == c - 1 and 0 <= sh["cl"] - sh["ch"] <= 1
    for s in range(nsets):
        nbr, nbc, shift = RC.plane_counts(sh, s)
        assert nbr <= RC.RC_NB and nbc <= RC.RC_NB
        # every weight fits its planes, and the split is exact: wr(hi) 2^shift + wc(lo) = (k >> v) + 1
        wr, wc = RC.row_weights(sh, s), RC.col_weights(sh, s)
        assert wr.max() < 1 << nbr and wc.max() < 1 << max(nbc, 1)
        k = np.arange(1 << sh["c1"])
        assert (((wr[k >> sh["cl"]] << shift) + wc[k & ((1 << sh["cl"]) - 1)]) == (k >> RC.set_v(sh, s)) + 1).all()
    for name in RC.FILLS if c < 20 else ("random", "adjacent"):
        idx = RC.fill(sh, name)
        assert idx.shape == (nsets << sh["c1"],) and idx.min() >= 0 and idx.max() < len(RC.pool().e)
        planes = RC.ref_planes(sh, idx)
        want = RC.ref_set_sums(sh, idx)
        assert [x % O.R for x in RC.recombine(sh, planes)] == [x % O.R for x in want], name
        e = RC.pool().e[idx]
        if name.startswith("one_"):
            assert all(np.count_nonzero(e[s << sh["c1"]:(s + 1) << sh["c1"]]) == 1 for s in range(nsets))
        if name == "adjacent":
            same = (e[0::2] == e[1::2]) & (e[0::2] != 0) & (idx[0::2] != idx[1::2])
            assert same.sum() >= len(e) // 10, "a quarter of the bucket pairs: one point, two representations"
        if name == "alternating":
            assert (e[0::2] == -e[1::2]).all() and e[0] != 0
        if name == "same_point":
            assert len(set(e)) == 1 and len(set(idx)) == RC.N_Z


def test_reference_against_the_group_law_on_a_small_shape():
    """the integer bookkeeping against point additions: c = 8, every bucket added with its weight"""
    sh = RC.shape_of(8, 2, 1)
    idx = RC.fill(sh, "random")
    pl = RC.pool()
    pts = [C.xyzz_point(RC.unpack48(w)) for w in pl.words]
    for s, want in enumerate(RC.ref_set_sums(sh, idx)):
        acc = None
        for k in range(1 << sh["c1"]):
            acc = O.g1_add(acc, O.g1_mul(pts[idx[(s << sh["c1"]) + k]], (k >> RC.set_v(sh, s)) + 1))
        assert acc == RC.point_of(want)
