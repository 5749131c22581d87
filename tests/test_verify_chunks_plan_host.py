"""verify_chunks_plan (csrc/verify_chunks_plan.hpp), the launch shape of typlonk_verify_chunks's fold, without a GPU: the header as
the host compiles it on its own (tests/cpp/verify_chunks_plan_host, a program with its own main and no HIP include) for every
log_l in 0..10 and N in {1, 2, 63, 64, 65, 4097, 16385}, with the plan's own strip and with named ones.  The strips, walked the way the
kernel indexes them, cover [0, N) exactly once and every coefficient of a cell has exactly one thread; the LDS stays within
32 KiB for the cells and the table of l / 2 twiddles beside them; and the number of partial vectors -- what the sum kernel is
told -- is the number of workgroups, each with at least one cell.  A bisection folds sub-ranges into the buffer sized for the whole
call: planned with the call's strip no sub-range has more workgroups than the call, where its own plan may (N = 4097 and 16385)."""
import json
import os
import subprocess

import pytest

from helpers import ROOT

LOG_L = list(range(11))
CELLS = [1, 2, 63, 64, 65, 4097, 16385]
STRIPS = [0, 1, 3, 4, 5, 64, 5000]
BIG = [(1 << 25, 0, 0), (1 << 15, 10, 0), (1 << 19, 6, 0)]     # the largest calls the library admits


@pytest.fixture(scope="module")
def plans(built):
    cases = [(n, ll, s) for ll in LOG_L for n in CELLS for s in STRIPS] + BIG
    text = "\n".join(" ".join(map(str, c)) for c in cases) + "\n"
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "verify_chunks_plan_host")], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(cases) and [(p["cells"], p["log_l"], p["named"]) for p in out] == cases
    return out


def test_the_strips_cover_the_cells_exactly_once(plans):
    for p in plans:
        assert p["covered"] == 1 or (p["covered"] == -1 and p["cells"] > 1 << 22), p
    assert sum(p["covered"] == 1 for p in plans) >= len(LOG_L) * len(CELLS) * len(STRIPS)


def test_the_groups(plans):
    for p in plans:
        l = 1 << p["log_l"]
        assert p["group"] == (64 if l <= 64 else 256) and p["groups"] * p["group"] == 256, p
        assert p["per"] == max(1, l // p["group"]) and p["per"] in (1, 2, 4), p
        assert p["iters"] == -(-p["strip"] // p["groups"]), p


def test_the_partial_vectors_are_the_workgroups(plans):
    for p in plans:
        assert p["strip"] >= 1 and p["blocks"] == -(-p["cells"] // p["strip"]), p
        if p["named"]:
            assert p["strip"] == p["named"], p
        else:                                             # the plan's own: at most 2048 vectors, no group without a first cell
            assert p["blocks"] <= 2048 and p["strip"] == max(p["groups"], -(-p["cells"] // 2048)), p


def test_no_sub_range_outgrows_the_whole_calls_partial_vectors(plans):
    """every hi - lo <= N, planned with the strip of N's plan, fits the `blocks` vectors allocated for N"""
    walked = [p for p in plans if p["sub_max_blocks"] >= 0]
    assert len(walked) >= len(LOG_L) * len(CELLS) * len(STRIPS)
    for p in walked:
        assert p["sub_max_blocks"] == p["blocks"], p
    # the trap this rule avoids: a sub-range's own plan may ask for more than the whole call's
    own = {(p["cells"], p["log_l"]): p for p in plans if not p["named"]}
    for key in [(4097, 7), (4097, 10), (16385, 6)]:
        assert own[key]["own_sub_max_blocks"] == 2048 > own[key]["blocks"], own[key]


def test_the_lds_stays_within_its_bound(plans):
    for p in plans:
        l = 1 << p["log_l"]
        assert p["tw"] == max(l // 2, 1), p
        assert p["lds_cells"] == p["groups"] * l * 32 <= 32 << 10, p
        assert p["lds_bytes"] == p["lds_cells"] + 32 * p["tw"] <= (32 << 10) + 32 * p["tw"] <= 48 << 10, p


def test_a_case_cut_short_is_an_error(built):
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "verify_chunks_plan_host")], input="1 2\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
