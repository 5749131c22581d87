"""solve_plan (csrc/solve_plan.hpp), every decision of a witness solve, without a GPU: the header as the host compiles it on its
own (tests/cpp/solve_plan_host, a program with its own main and no HIP include; tests/cpp/solve_plan_host_san is the same
program under the address and undefined-behaviour sanitizers) against the Python statement of the contract
(tests/witness_solve_ref.py) on the generated circuits: src, the level of every row and the launch schedule are equal, every
source's level is below its user's, every driven row is scheduled once, runs split at the 256 boundary and at the run cut, and
dependency cycles are refused with the lowest row named."""
import json
import os
import subprocess

import pytest

import witness_check_ref as W
import witness_solve_ref as S
from helpers import ROOT


def _text(q, perm, narrow=S.NARROW, cut=S.RUN_CUT):
    n = len(q["q_o"])
    return f"{n} {narrow} {cut}\n" + " ".join(map(str, perm)) + "\n" + " ".join(str(int(d)) for d in S.driven_rows(q)) + "\n"


def _plans(cases, exe="solve_plan_host"):
    """cases: [(q, perm, narrow, cut)] -> the program's plans, from one run"""
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", exe)], input="".join(_text(*c) for c in cases), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return out


def _cases():
    out = []
    for log_n in (3, 4, 6, 10):
        _, q, perm, _, _ = S.chain(log_n)
        out.append((q, perm, S.NARROW, S.RUN_CUT))
    _, q, perm, _, _ = S.chain(10)
    out += [(q, perm, S.NARROW, 100), (q, perm, S.NARROW, 1021), (q, perm, S.NARROW, 1)]     # 1021 = the depth: no cut
    n, q, perm, _, _ = S.readme()
    out.append((q, perm, S.NARROW, S.RUN_CUT))
    c = S.layered(12, 7, [255, 1, 1500, 256, 1, 257, 255, 1500])
    out.append((c["q"], c["perm"], S.NARROW, S.RUN_CUT))
    c = S.layered(11, 8, [255, 256, 257, 256, 255, 8])
    out += [(c["q"], c["perm"], S.NARROW, S.RUN_CUT), (c["q"], c["perm"], 255, 2), (c["q"], c["perm"], 8, 3)]
    c = S.layered(6, 9, [3, 1, 9, 4, 12], S.public_values(64, 64, 9))
    out += [(c["q"], c["perm"], 4, 2), (c["q"], c["perm"], 1, 1)]
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.fixture(scope="module")
def plans(built, cases):
    return _plans(cases)


def test_every_field_equals_the_python_statement(cases, plans):
    for (q, perm, narrow, cut), got in zip(cases, plans):
        assert got == S.plan(q, perm, narrow, cut), (len(perm) // 3, narrow, cut)


def test_sources_come_first_and_every_row_is_scheduled_once(cases, plans):
    for (q, perm, narrow, cut), p in zip(cases, plans):
        n, driven = len(perm) // 3, S.driven_rows(q)
        level, src = p["level"], p["src"]
        assert sorted(p["order"]) == [j for j in range(n) if driven[j]] and p["driven_rows"] == len(p["order"])
        for j in range(n):
            assert (level[j] > 0) == driven[j]
            if driven[j]:
                below = [0 if s & S.FREE else level[s] for s in (src[j], src[n + j])]
                assert level[j] == 1 + max(below) and src[2 * n + j] == j
        # the schedule covers levels 0 .. depth - 1 once, in order; order holds level l at [level_off[l], level_off[l + 1])
        at = 0
        for first, levels, wide in p["schedule"]:
            assert first == at and levels >= 1
            widths = [p["level_off"][l + 1] - p["level_off"][l] for l in range(first, first + levels)]
            assert (levels == 1 and widths[0] > narrow) if wide else (levels <= cut and max(widths) <= narrow)
            at += levels
        assert at == p["depth"] and p["launches"] == len(p["schedule"]) + 1
        assert [level[j] for j in p["order"]] == sorted(level[j] for j in p["order"])
        assert all(level[j] == l + 1 for l in range(p["depth"]) for j in p["order"][p["level_off"][l]:p["level_off"][l + 1]])
        # free slots: one per free class, numbered by the lowest cell
        slots = [src[cyc[0]] & ~S.FREE for cyc in W.cycles_of(perm) if src[cyc[0]] & S.FREE]
        assert slots == list(range(p["free_classes"]))


def test_runs_split_at_the_256_boundary_and_at_the_cut(cases, plans):
    by = {(len(c[1]) // 3, c[2], c[3]): p for c, p in zip(cases, plans)}
    # widths 255, 1 | 1500 | 256, 1 | 257 | 255 | 1500
    assert by[(4096, 256, 65536)]["schedule"] == [[0, 2, 0], [2, 1, 1], [3, 2, 0], [5, 1, 1], [6, 1, 0], [7, 1, 1]]
    # widths 255, 256 | 257 | 256, 255, 8
    assert by[(2048, 256, 65536)]["schedule"] == [[0, 2, 0], [2, 1, 1], [3, 3, 0]]
    # a narrow limit of 255: 256 is wide now; runs of at most two levels
    assert by[(2048, 255, 2)]["schedule"] == [[0, 1, 0], [1, 1, 1], [2, 1, 1], [3, 1, 1], [4, 2, 0]]
    assert by[(2048, 8, 3)]["schedule"] == [[k, 1, 1] for k in range(5)] + [[5, 1, 0]]
    # the chain's 1021 levels: one run; cut every 100; a cut equal to the depth; a cut of one level
    assert by[(1024, 256, 65536)]["schedule"] == [[0, 1021, 0]]
    assert by[(1024, 256, 100)]["schedule"] == [[100 * k, 100, 0] for k in range(10)] + [[1000, 21, 0]]
    assert by[(1024, 256, 1021)]["schedule"] == [[0, 1021, 0]]
    assert by[(1024, 256, 1)]["schedule"] == [[k, 1, 0] for k in range(1021)]
    # widths 3, 1, 9, 4, 12 under a narrow limit of 4 and a cut of 2
    assert by[(64, 4, 2)]["schedule"] == [[0, 2, 0], [2, 1, 1], [3, 1, 0], [4, 1, 1]]
    assert by[(64, 1, 1)]["schedule"] == [[0, 1, 1], [1, 1, 0], [2, 1, 1], [3, 1, 1], [4, 1, 1]]


def _cyclic():
    n = 8
    q = {name: [0] * n for name in W.SELECTORS}
    for j in (2, 5, 6):
        q["q_o"][j] = 1
    two = list(range(3 * n))
    two[2 * n + 5], two[2] = 2, 2 * n + 5                              # a_2 = c_5
    two[2 * n + 2], two[5], two[n + 6] = 5, n + 6, 2 * n + 2           # a_5 = b_6 = c_2
    own = list(range(3 * n))
    own[2 * n + 6], own[n + 6] = n + 6, 2 * n + 6                      # b_6 = c_6
    return q, two, own


def test_cycles_are_refused_with_the_lowest_row_named(built):
    q, two, own = _cyclic()
    a, b = _plans([(q, two, 256, 65536), (q, own, 256, 65536)])
    assert (a["status"], a["bad"]) == (2, 2) and "src" not in a
    assert (b["status"], b["bad"]) == (2, 6)
    # a map that is no permutation of the cells is refused, not walked
    broken = list(range(24))
    broken[3] = 4
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "solve_plan_host")], input=_text(q, broken), capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0 and json.loads(r.stdout)["status"] == 1


def test_the_sanitized_build_gives_the_same_plans(built, cases, plans):
    q, two, own = _cyclic()
    small = [c for c in cases if len(c[1]) <= 3 * 2048]
    assert _plans(small + [(q, two, 256, 65536), (q, own, 256, 65536)], exe="solve_plan_host_san")[:len(small)] == \
        [p for c, p in zip(cases, plans) if len(c[1]) <= 3 * 2048]


def test_host_program_refuses_a_circuit_cut_short(built):
    exe = os.path.join(ROOT, "tests", "cpp", "solve_plan_host")
    assert subprocess.run([exe], input="8 256 65536\n0 1 2\n", capture_output=True, text=True, timeout=60).returncode == 2
    r = subprocess.run([exe], input="", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == ""
