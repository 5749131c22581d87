"""open_chunks_plan (csrc/open_chunks_plan.hpp), the launch shape of typlonk_open_chunks_*'s pointwise pass, without a GPU: the
header as the host compiles it on its own (tests/cpp/open_chunks_plan_host, a program with its own main and no HIP include) over
a grid of (count, r, l).  The number of slices g is a power of two no larger than l or 64 and depends on nothing else; the launch,
walked thread by thread the way the kernel indexes it, takes every (output, term) exactly once; g follows the rule the header
states -- the least (8 + 10 l / g) x (1.12 for one wave a SIMD, else the waves a SIMD) over the 1024 SIMDs, the smaller g on a
tie -- and, for the four shapes whose pointwise pass was timed at every g (profiles/r31_open_chunks.txt), is the fastest one."""
import json
import os
import subprocess

import pytest

from helpers import ROOT

COUNTS = [1, 2, 3, 5, 64, 1000]
LOG_R = [1, 2, 5, 6, 7, 10, 12, 14, 16, 17, 20]
LOG_L = [0, 1, 2, 3, 4, 5, 6, 7, 10]


@pytest.fixture(scope="module")
def plans(built):
    cases = [(c, 1 << lr, 1 << ll) for c in COUNTS for lr in LOG_R for ll in LOG_L if lr + ll <= 24 and c << (lr + 1) <= 1 << 25]
    text = "\n".join(" ".join(map(str, c)) for c in cases) + "\n"
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "open_chunks_plan_host")], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(cases) and [(p["count"], p["r"], p["l"]) for p in out] == cases
    return out


def test_the_grid_reaches_every_number_of_slices(plans):
    assert {p["g"] for p in plans} == {1, 2, 4, 8, 16, 32, 64}
    assert sum(p["covered"] == 1 for p in plans) >= 100


def test_slices_are_a_power_of_two_within_the_terms(plans):
    for p in plans:
        g = p["g"]
        assert g >= 1 and g & (g - 1) == 0 and g <= min(p["l"], 64), p
        assert p["per"] * g == p["l"] and p["outputs"] == p["count"] * 2 * p["r"] and p["threads"] == p["outputs"] * g, p
        assert p["blocks"] == -(-p["threads"] // 64), p


def test_the_launch_takes_every_term_of_every_output_once(plans):
    for p in plans:
        assert p["covered"] in (1, -1), p          # -1: more than 2^24 (output, term) pairs, not walked
        assert p["covered"] == 1 or p["outputs"] * p["l"] > 1 << 24, p


def _cost(outputs, l, g):
    waves = -(-outputs * g // 64)
    q = -(-waves // 1024)                              # wavefronts per SIMD, rounded up
    return (8 + 10 * (l // g)) * (112 if q == 1 else 100 * q)


def test_the_rule(plans):
    for p in plans:
        gs = [g for g in (1, 2, 4, 8, 16, 32, 64) if g <= p["l"]]
        want = min(gs, key=lambda g: (_cost(p["outputs"], p["l"], g), g))
        assert p["g"] == want, p
        if p["outputs"] * min(p["l"], 64) <= 64 * 1024:      # no g gives a SIMD a second wave: the shortest chain
            assert p["g"] == min(p["l"], 64), p


def test_the_measured_shapes_get_their_fastest_g(plans):
    """(count, r, l) -> the g of the shortest launch in the sweep of profiles/r31_open_chunks.txt"""
    fastest = {(1, 1 << 14, 64): 4, (64, 128, 64): 8, (1, 1 << 12, 16): 8, (1, 1 << 17, 8): 1}
    got = {(p["count"], p["r"], p["l"]): p["g"] for p in plans}
    for shape, g in fastest.items():
        assert got[shape] == g, shape


def test_a_case_cut_short_is_an_error(built):
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "open_chunks_plan_host")], input="1 2\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
