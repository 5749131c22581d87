"""prove_plan (csrc/prove_plan.hpp), where a proof's data lives and what every workspace of a prover call holds, without a GPU:
the header as the host compiles it on its own (tests/cpp/prove_plan_host, a program with its own main and no HIP include) over
the cases of tests/golden/prove_plans.json, which records what the provers of the commit before the plan existed asked ensure()
for over one call (the fixture's "about" says how it was made).  Every planned size must be the largest of those requests --
so a context retains exactly what it retained before -- and, what nothing checked before:
  * every step's own need (grand product, each opening launch, quotient) fits the planned size of its buffer, so no step could
    ever have grown a buffer behind the sizing site;
  * the regions do not overlap, sit where both provers had them, and the accessor finds them at proof x stride + offset;
  * the wave's grand-product scratch, laid over t and q by hand before, lies inside them;
  * the slot maps are distinct per shape and r(zeta), F(zeta) lie behind the slots that are fetched first;
  * ensure() is called by the sizing site and the stand-alone entry points only (read from the two .hip files as text).
The same program runs once more under the address and undefined-behaviour sanitizers (a plain executable).
The same plans on the device: tests/test_gpu_prove_workspaces.py and every prover test."""
import json
import os
import re
import subprocess

import pytest

from helpers import ROOT

EXE = os.path.join(ROOT, "tests", "cpp", "prove_plan_host")
FIXTURE = os.path.join(ROOT, "tests", "golden", "prove_plans.json")
CSRC = os.path.join(ROOT, "typlonk_amd", "csrc")
BUFFERS = ["prover_mem", "ops_tmp", "quot_ext", "quot_tab", "batch_tab"]
SESSION, WAVE = 0, 1
FR = 32


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def text(golden):
    return "\n".join(" ".join(map(str, c[:4])) for c in golden["cases"]) + "\n"


def run_program(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return [json.loads(line) for line in r.stdout.splitlines()]


@pytest.fixture(scope="module")
def plans(built, golden, text):
    out = run_program(EXE, text)
    assert len(out) == len(golden["cases"])
    return out


def test_fixture_holds_the_cases_it_says(golden):
    cases = [tuple(c[:4]) for c in golden["cases"]]
    assert len(set(cases)) == len(cases)
    assert "e6afaa5" in golden["about"] and "by hand" in golden["about"]
    want = {(lg, k, mode, 1) for lg in (0, 1, 3, 10, 11, 12, 16, 20, 22, 24) for k in (1, 2, 5, 64, 70) for mode in (SESSION, WAVE)}
    want |= {(lg, 1, SESSION, 0) for lg in (0, 1, 3, 10, 11, 12, 16, 20, 22, 24)}
    assert set(cases) == want
    assert os.path.getsize(FIXTURE) < 64 << 10


def test_the_formulas_of_the_issue_hold_in_the_fixture(golden):
    """the fixture against the table the work was specified by (nblk = ceil(n / 2048)), so a slip of the hand shows"""
    for lg, proofs, mode, cached, G, slots, big in golden["cases"]:
        n = 1 << lg
        nblk = -(-n // 2048)
        log4 = lg + 2
        n_hi = 1 << (log4 - (log4 + 1) // 2)
        assert big["quot_tab"] == n_hi * FR
        if mode == SESSION and not cached:
            assert big == {"quot_ext": 14 * 4 * n * FR, "quot_tab": n_hi * FR}
        elif mode == SESSION:
            assert (G, slots) == (1, 16)
            assert big == {"prover_mem": 19 * n * FR, "ops_tmp": max(4 * n + nblk + 8, max(16384, 8 * nblk)) * FR,
                           "quot_ext": 5 * 4 * n * FR, "quot_tab": n_hi * FR, "batch_tab": 0}
        else:
            assert G == min(proofs, 64, max(1, (1 << 22) >> lg)) and slots == G * 16
            assert big == {"prover_mem": G * 39 * n * FR, "ops_tmp": G * 8 * nblk * FR, "quot_ext": 0, "quot_tab": n_hi * FR,
                           "batch_tab": big["batch_tab"]}
            assert big["batch_tab"] == 229376


def test_planned_sizes_are_the_largest_recorded_requests(golden, plans):
    for case, p in zip(golden["cases"], plans):
        lg, proofs, mode, cached, G, slots, req = case
        assert (p["log_n"], p["n"], p["fr"]) == (lg, 1 << lg, FR), case
        for b, largest in req.items():
            assert p[b] == largest, (case[:4], b)
        if cached:
            assert set(req) == set(BUFFERS)
            assert (p["G"], p["slots"]) == (G, slots), case[:4]
            assert mode == SESSION or p["tables"] == req["batch_tab"], case[:4]     # sizeof(PbTables)


def test_every_step_fits_the_planned_size_of_its_buffer(golden, plans):
    """need_gp, need_open, gp.end and the launches' carries all come from prove_plan.hpp, so their agreeing with one another only
    says that the plan is the maximum over ITS OWN steps.  What holds the steps' needs themselves to numbers from outside the
    header is test_grand_product_and_open_layouts (the layouts restated here) and the opening launches written out below."""
    for case, p in zip(golden["cases"], plans):
        lg, proofs, mode, cached = case[:4]
        if not cached:
            continue
        n, G = p["n"], p["G"]
        nblk = -(-n // 2048)
        ops = p["ops_tmp"] // FR
        if mode == SESSION:
            assert p["need_gp"] == p["gp"]["end"] <= ops                                # round 2's grand product
            assert p["open_launches"] == [8 * nblk, nblk]                                # round 3's items; r's (F's) opening
            assert 5 * 4 * n * FR <= p["quot_ext"]                                       # the extensions and the quotient
        else:
            assert p["need_gp"] == 0 and p["quot_ext"] == 0                              # both live in the arena
            assert p["open_launches"] == [8 * G * nblk, G * nblk, 2 * G * nblk]          # a wave's carries fit what the plan sizes
        assert all(x <= p["need_open"] <= ops for x in p["open_launches"]), case[:4]
        assert p["ops_tmp"] == max(p["need_gp"], p["need_open"]) * FR
        log4 = lg + 2
        assert p["quot_tab"] == (1 << (log4 - (log4 + 1) // 2)) * FR                     # the quotient's scaled hi table
        assert p["slots"] == G * p["slots_per_proof"] and p["items"] == 8


def test_grand_product_and_open_layouts(golden, plans):
    for case, p in zip(golden["cases"], plans):
        n = p["n"]
        nblk = -(-n // 2048)
        g = p["gp"]       # stand-alone and in a session: over ops_tmp, as typlonk_grand_product_dev carved it
        assert [g[k] for k in ("num", "den", "npre", "dsuf", "carries", "runs", "inv", "end")] == \
            [0, n, 2 * n, 3 * n, 4 * n, 1, 4 * n + nblk, 4 * n + nblk + 8], case[:4]
        # in a wave: the four vectors are t, the carries (two runs per proof) and the inverse the head of q
        w, reg = p["gp_wave"], golden["regions"]
        t0, t1 = reg["t"][0] * n, (reg["t"][0] + reg["t"][1]) * n
        q0, q1 = reg["q"][0] * n, (reg["q"][0] + reg["q"][1]) * n
        assert [w["num"], w["den"], w["npre"], w["dsuf"]] == [t0, t0 + n, t0 + 2 * n, t0 + 3 * n] and w["dsuf"] + n <= t1, case[:4]
        assert w["carries"] == q0 and w["runs"] == 2 and w["inv"] == q0 + 2 * nblk and w["end"] == w["inv"] + 1 <= q1, case[:4]
        # typlonk_open_dev: max(nblk, 2048) carries, then the result
        o = p["open_dev"]
        assert [o["carries"], o["y"], o["end"]] == [0, max(nblk, 2048), max(nblk, 2048) + 8], case[:4]


def test_regions_do_not_overlap_and_sit_where_both_provers_had_them(golden, plans):
    for case, p in zip(golden["cases"], plans):
        n, mode = p["n"], case[2]
        assert p["stride"] == golden["stride"][mode] and p["stride_elems"] == p["stride"] * n
        names = list(golden["regions"])[:8 if mode == WAVE else 7]
        assert list(p["regions"]) == names
        end = 0
        for name in names:
            off, length, last = p["regions"][name]
            assert [off, length] == [x * n for x in golden["regions"][name]], (case[:4], name)
            assert off == end, (case[:4], name)          # each starts where the one before ends: no overlap, no hole
            end = off + length
            assert last == (p["G"] - 1) * p["stride_elems"] + off, (case[:4], name)
        assert end == p["stride_elems"]
        assert p["prover_mem"] == p["G"] * p["stride_elems"] * FR


def test_q_roles_and_slot_maps(golden, plans):
    p = plans[0]
    assert p["q"] == golden["q"]
    q = p["q"]
    assert len({q[k] for k in ("wit_a", "wit_b", "wit_c", "wit_z", "wit_zw", "wit_r")}) == 6 and max(q.values()) < golden["regions"]["q"][1]
    for shape in ("batched", "compact"):     # F, its witness and the witness at zeta w are three different vectors
        assert len({q[shape + "_f"], q[shape + "_wit"], q["wit_zw"]}) == 3
    assert p["slots_per_proof"] == golden["slots_per_proof"]
    for name in ("ref_slots", "compact_slots"):
        s, want = p[name], golden[name]
        assert {k: v for k, v in s.items() if want[k] is not None} == {k: v for k, v in want.items() if v is not None}
        fetched = [s["wire"], s["wire"] + 1, s["wire"] + 2, s["z"], s["sig0"], s["sig1"], s["pi"], s["zw"]]
        every = fetched + [s["r"], s["f"]]
        assert len(set(every)) == len(every) and all(0 <= x < p["slots_per_proof"] for x in every)
        assert all(x < s["count"] for x in fetched) and s["r"] >= s["count"] and s["f"] >= s["count"]
    assert all(pl["q"] == p["q"] and pl["ref_slots"] == p["ref_slots"] and pl["compact_slots"] == p["compact_slots"] for pl in plans)


def functions_calling(path, needle):
    """names of the functions of a .hip unit whose bodies contain `needle` (definitions start in column 0, bodies are indented)"""
    found, name = set(), None
    with open(path) as f:
        for line in f:
            m = re.match(r"^(?:template <[^>]*> )?[A-Za-z_][\w:<>\*& ]*?\b(\w+)\(", line)
            if m and not line.startswith(("//", "#", "namespace", "using", "static_assert", "constexpr", "struct", "}")):
                name = m.group(1)
            if needle in line and not line.lstrip().startswith("//"):
                found.add(name)
    return found


def test_only_the_sizing_site_and_the_stand_alone_entry_points_call_ensure():
    assert functions_calling(os.path.join(CSRC, "prover.hip"), "ensure(") == \
        {"prover_workspaces", "typlonk_quotient_dev", "typlonk_grand_product_dev", "typlonk_open_dev"}
    assert functions_calling(os.path.join(CSRC, "prove_batch.hip"), "ensure(") == set()
    # ... and the two callers of the sizing site are a session's round 1 and a batch call
    assert functions_calling(os.path.join(CSRC, "prover.hip"), "prover_workspaces(") == {"prover_workspaces", "prover_round1_impl"}
    assert functions_calling(os.path.join(CSRC, "prove_batch.hip"), "prover_workspaces(") == {"prove_batch_impl"}
    for unit in ("prover.hip", "prove_batch.hip"):
        assert functions_calling(os.path.join(CSRC, unit), "hipHostMalloc(") <= {"prover_workspaces"}


def test_the_same_cases_under_the_address_and_undefined_behaviour_sanitizers(built, text, plans):
    assert run_program(EXE + "_san", text) == plans


def test_host_program_refuses_a_case_cut_short(built):
    assert subprocess.run([EXE], input="12 1 0\n", capture_output=True, text=True, timeout=60).returncode == 2
    assert subprocess.run([EXE], input="25 1 0 1\n", capture_output=True, text=True, timeout=60).returncode == 2
    r = subprocess.run([EXE], input="", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == ""
