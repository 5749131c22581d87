"""ntt_plan (csrc/ntt_plan.hpp), every decision of a batch of NTTs, without a GPU: the header as the host compiles it on its own
(tests/cpp/ntt_plan_host, a program with its own main and no HIP include) over the cases of tests/golden/ntt_plans.json, which
records what ntt_run_batch and its table getters of the commit before the plan existed did for the same cases (the fixture's
"about" says how it was captured).  The plan is walked the way ntt_run_batch (ntt_host.hip) walks it -- requests in order, the
30-bit kernel's until one of its full tables comes back empty, the 8 x 32 kernel's own full tables unless the 30-bit kernel runs
-- once with every table built and once with every full table refused, and must give the recorded ensure() size, the recorded
table requests (order, key, entries, kind, base, scale, a full table's pair, h and S) and the recorded launches (kernel form,
blocks, threads, LDS bytes, every scalar of NttPassArgs, where in / out point, which table is behind each pointer).
The same plans on the device: tests/test_gpu_ntt.py."""
import json
import os
import subprocess

import pytest

from helpers import ROOT

EXE = os.path.join(ROOT, "tests", "cpp", "ntt_plan_host")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ntt_plans.json")
OK, DOMAIN, EMPTY, IDENTITY = range(4)            # NttPlanStatus
F32, F30 = 0, 1                                   # NttForm
SUB, TW, PRE, POST, SCALE = range(5)              # NttRole
POW, POW30, PAIR_LO, PAIR_HI, FULL = range(5)     # NttKind
B_ONE, B_ROOT, B_ROOT_INV, B_SHIFT, B_SHIFT_INV = range(5)
SCALES = ["1", "ninv", "c14", "ninv*c14"]
ERR_DOMAIN = -3
# the pointers of NttPassArgs in the fixture's numbering ("ptrs" legend)
SLOT = {(SUB, F32, POW): 0, (SUB, F30, POW30): 1, (TW, F32, PAIR_LO): 2, (TW, F32, PAIR_HI): 3, (TW, F32, FULL): 4, (TW, F30, FULL): 4,
        (PRE, F32, PAIR_LO): 5, (PRE, F32, PAIR_HI): 6, (PRE, F32, FULL): 7, (PRE, F30, FULL): 7,
        (POST, F32, PAIR_LO): 8, (POST, F32, PAIR_HI): 9, (POST, F32, FULL): 10, (POST, F30, FULL): 10,
        (SCALE, F32, POW): 11, (SCALE, F30, POW): 11}
SHAPE = ["threads", "k", "last", "logT", "tw_h", "blocks_per_vec", "S", "row_len", "N1", "Q", "N2", "N3", "out_stride"]


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def case_input(g, case):
    c = list(case[:9])
    c[2] = g["shift"] if c[2] else "-"
    return c


@pytest.fixture(scope="module")
def plans(built, golden):
    """the plan of every case of the fixture, from one run of the host program"""
    text = "\n".join(" ".join(map(str, case_input(golden, c))) for c in golden["cases"]) + "\n"
    r = subprocess.run([EXE], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(golden["cases"])
    return out


def base_name(r):
    """the value of a request's base under the fixture's names (w1 = -1 is its own inverse, w0 = 1)"""
    j = r["base_log"] - r["base_sqr"]
    if r["base"] == B_ONE or (r["base"] in (B_ROOT, B_ROOT_INV) and j <= 0):
        return "1"
    if r["base"] in (B_ROOT, B_ROOT_INV):
        return ("wi%d" if r["base"] == B_ROOT_INV and j > 1 else "w%d") % j
    return ("g%d" if r["base"] == B_SHIFT else "gi%d") % r["base_sqr"]


def walk(plan, refuse_full):
    """ntt_run_batch's walk of the plan's tables: the requests it makes, the kernel form it ends with, the tables it holds"""
    f30, more30, asked, held = bool(plan["f30_eligible"]), True, [], set()
    for i, r in enumerate(plan["tables"]):
        if (not more30) if r["form"] == F30 else (r["unless30"] and f30):
            continue
        asked.append(i)
        if r["kind"] == FULL and refuse_full:
            if r["form"] == F30:
                f30 = more30 = False
        else:
            held.add(i)
    return asked, (F30 if f30 else F32), held


def test_fixture_holds_the_cases_it_says(golden):
    cases = [tuple(c[:9]) for c in golden["cases"]]
    assert len(set(cases)) == len(cases)
    assert "231f66a" in golden["about"]
    sweep = {c[:3] + (c[5],) for c in cases if c[3:5] == (1, 0) and c[6:] == (1, 0, 1)}
    assert sweep >= {(lg, inv, cs, m) for lg in list(range(29)) + [30, 32, 33] for inv in (0, 1) for cs in (0, 1) for m in (0, 1, 2)}
    assert {(c[0], c[6], c[7], c[8]) for c in cases} >= {(lg, b, r, t) for lg in (19, 20, 21) for b in (0, 1, 2) for r in (0, 1) for t in (0, 1)}
    assert {c[3] for c in cases if c[0] == 12} >= {0, 1, 2, 3, 8, 9, 11, 17}
    assert {(c[0], c[3]) for c in cases} >= {(lg, n) for lg in (22, 23, 24, 25) for n in (1, 2, 3, 5, 8)}
    assert {c[4] for c in cases} == {0, 1}
    assert os.path.getsize(FIXTURE) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "column_refusals.json"))


def test_status_groups_and_scratch_equal_the_recorded_ones(golden, plans):
    for case, p in zip(golden["cases"], plans):
        log_n, count = case[0], case[3]
        rc, groups, ensure = golden["outcome"][case[9]][:3]
        groups = golden["groups"][groups]
        if log_n > 32:
            assert p["status"] == DOMAIN and rc == ERR_DOMAIN and not groups, case
            continue
        assert rc == 0, case
        if count == 0:
            assert p["status"] == EMPTY and not groups and not ensure, case
            continue
        assert p["status"] == (IDENTITY if log_n == 0 else OK), case
        # the loop over groups reproduces the recursion
        assert [[g0, min(p["group"], count - g0)] for g0 in range(0, count, p["group"])] == groups, case
        # one ensure() per group in the parent, the first being the largest: the plan's one size is that one
        assert ensure == ([g[1] * (32 << log_n) for g in groups] if p["P"] >= 2 else []), case
        assert p["scratch_bytes"] == (max(ensure) if ensure else 0) == (ensure[0] if ensure else 0), case


def test_table_requests_equal_the_recorded_ones_in_both_modes(golden, plans):
    for case, p in zip(golden["cases"], plans):
        for mode in (0, 1):
            want = [golden["req"][i] for s in golden["reqlist"][golden["outcome"][case[9]][3 + mode]] for i in golden["seg"][s]]
            asked, _, _ = walk(p, refuse_full=bool(mode))
            assert len(asked) == len(want), (case, mode)
            for i, w in zip(asked, want):
                r = p["tables"][i]
                key = w[1].replace("$", golden["shift"])
                assert r["key"] == key and r["n"] == w[2], (case, mode, key)
                assert {POW: 0, PAIR_LO: 0, PAIR_HI: 0, POW30: 1, FULL: 2}[r["kind"]] == w[0], (case, mode, key)
                if r["kind"] == FULL:
                    lo, hi = p["tables"][r["lo"]], p["tables"][r["hi"]]
                    assert [r["h"], r["S"], lo["key"], hi["key"]] == \
                        [w[3], w[4]] + [golden["req"][x][1].replace("$", golden["shift"]) for x in w[5:7]], (case, mode, key)
                    assert r["lo"] in asked and r["hi"] in asked and lo["kind"] == PAIR_LO and hi["kind"] == PAIR_HI, (case, mode, key)
                else:
                    # (a one-entry table never multiplies by its base)
                    # (... and the fixture names values: n^-1 2^14 = 1 at n = 2^14)
                    scale = "1" if (SCALES[r["scale"]], case[0]) == ("ninv*c14", 14) else SCALES[r["scale"]]
                    assert (base_name(r) == w[3] or r["n"] == 1) and scale == w[4], (case, mode, key)
                # the coset group of a key, for the eviction
                assert r["group"] == (key[:key.index(golden["shift"]) + 64] if key.startswith("cs:") else ""), (case, mode, key)


def test_launches_equal_the_recorded_ones_in_both_modes(golden, plans):
    seen = set()
    for case, p in zip(golden["cases"], plans):
        log_n, count, short_in = case[0], case[3], case[4]
        groups = golden["groups"][golden["outcome"][case[9]][1]]
        for mode in (0, 1):
            want = [golden["launch"][i] for i in golden["launchlist"][golden["outcome"][case[9]][5 + mode]]]
            if p["status"] != OK:
                assert not want, (case, mode)
                continue
            _, form, held = walk(p, refuse_full=bool(mode))
            seen.add((mode, form))
            got = []
            for _, cnt in groups:
                for i, a in enumerate(p["passes"]):
                    ptrs = {}
                    for t in held:
                        r = p["tables"][t]
                        slot = SLOT.get((r["role"], r["form"], r["kind"]))
                        if r["pass"] == i and r["form"] == form and slot is not None:
                            assert slot not in ptrs, (case, mode)
                            ptrs[slot] = r["key"]
                    got.append([form, i, [a[x] for x in SHAPE], a["blocks_per_vec"] * cnt, a["lds"][form], a["pre_h"], a["post_h"],
                                (1 << (log_n - 2)) if a["short_in"] else -1, (2 if short_in else 0) if i == 0 else 1, 0 if a["last"] else 1, ptrs])
            want = [w[:2] + [golden["shape"][w[2]]] + w[3:10] +
                    [{s: golden["req"][r][1].replace("$", golden["shift"]) for s, r in zip(golden["ptrs"][w[10]][::2], golden["ptrs"][w[10]][1::2])}]
                    for w in want]
            assert got == want, (case, mode)
    assert seen == {(0, F32), (0, F30), (1, F32), (1, F30)}   # (a one-pass transform without a coset has no full table to lose)


def test_both_kernel_forms_read_the_same_pass_records(golden):
    """the parent walked the shape once per form: where the 30-bit kernel ran with its tables and the 8 x 32 kernel without them,
    both were launched with the same shape, grid, scalars and vectors"""
    pairs = 0
    for case in golden["cases"]:
        o = golden["outcome"][case[9]]
        a, b = ([golden["launch"][i] for i in golden["launchlist"][o[5 + m]]] for m in (0, 1))
        assert len(a) == len(b), case
        for x, y in zip(a, b):
            assert x[1:4] == y[1:4] and x[5:10] == y[5:10], case   # all but the form, its LDS bytes and its tables
            pairs += x[0] != y[0]
    assert pairs > 100


def test_host_program_refuses_a_case_cut_short(built):
    assert subprocess.run([EXE], input="12 0 - 1 0\n", capture_output=True, text=True, timeout=60).returncode == 2
    r = subprocess.run([EXE], input="", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == ""
