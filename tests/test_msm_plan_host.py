"""msm_plan (csrc/msm_plan.hpp), every decision of an MSM, without a GPU: the header as the host compiles it on its own
(tests/cpp/msm_plan_host, a program with its own main and no HIP include) over the cases of tests/golden/msm_plans.json, which
records what msm_enqueue and launch_msm_segsort of the commit before the plan existed decided for the same cases (the fixture's
"about" says how it was captured).  Every field must be equal; and two things nothing checked before:
  * the one MsmShape of a chunk carries the nseg, nblk, jbits and chunk that the host (which sized the buffers) AND the
    launcher (whose kernels index them) each computed for themselves;
  * every planned buffer size covers what any chunk that uses the buffer asked ensure() for, and is no larger than the largest
    such request -- so a context retains exactly what it retained before.
The same plans on the device: the bit-identity tests of tests/test_gpu_msm.py."""
import json
import os
import subprocess

import pytest

from helpers import ROOT

SORT = ["keys", "sorted", "counts", "offsets", "cursor", "blocksums", "order", "ohist", "heavy", "tasks", "hpart", "blk_hist", "blk_base",
        "blk_cnt", "seg_start"]
# MsmShape in declaration order (the fixture's "lsh" legend)
C_, W_, TOP_V, HB, LB, NSEG, NBLK, CHUNK, IBITS, JBITS, TLEN, NSETS, CENTRED, PRIO = range(14)
ERR_LENGTH = -2


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "msm_plans.json")) as f:
        return json.load(f)


def case_input(g, case):
    m, mode, srs, ov = case[:4]
    ln, c, T, centred = g["srs"][srs]
    return [m, mode, ln if c else m, c, T, centred] + g["ov"][ov]


@pytest.fixture(scope="module")
def plans(built, golden):
    """the plan of every case of the fixture, from one run of the host program"""
    text = "\n".join(" ".join(map(str, case_input(golden, c))) for c in golden["cases"]) + "\n"
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "msm_plan_host")], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(golden["cases"])
    return out


def test_fixture_holds_the_cases_it_says(golden):
    cases = golden["cases"]
    assert 300 <= len(cases) <= 700 and len({tuple(c[:4]) for c in cases}) == len(cases)
    ms = {c[0] for c in cases}
    assert {1, 255, 256, 4095, 1 << 12, (1 << 14) - 1, 1 << 16, 1 << 17, (1 << 17) + 1, 1 << 18, (1 << 18) + 1, (1 << 19) - 1, 1 << 19,
            (1 << 20) - 1, 1 << 20, 3 * (1 << 19) - 1, 3 * (1 << 19), 1 << 21, 1 << 22, 1 << 23, (1 << 23) + 1} <= ms
    assert {tuple(s[:2]) for s in golden["srs"]} == {(0, 0), (1 << 14, 15), (1 << 17, 17), (1 << 20, 20), (1 << 22, 20)}
    assert {c[1] for c in cases} == {0, 1, 2}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "msm_plans.json")) < \
        os.path.getsize(os.path.join(ROOT, "tests", "golden", "column_refusals.json"))


def test_every_field_of_every_plan_equals_the_recorded_one(golden, plans):
    for case, p in zip(golden["cases"], plans):
        inp = case_input(golden, case)
        head, ws_bytes, rc_form, rcs, combine, ws = golden["heads"][case[5]]
        chunks = golden["lists"][case[6]]
        if case[4] != 0:     # the refusal: 32-bit entry indices
            assert case[4] == ERR_LENGTH and p["status"] == 1 and head is None and not p["chunks"], inp
            continue
        assert p["status"] == 0, inp
        tables, centred, c, W, nsets, digit_v, nb, nch, first, overlap = head
        assert [p[k] for k in ("tables", "centred", "c", "W", "nsets", "digit_v", "nb", "nch", "overlap")] == \
            [tables, centred, c, W, nsets, digit_v, nb, nch, overlap], inp
        assert p["scatter_staged"] == inp[8]
        assert len(p["chunks"]) == len(chunks) == nch, inp
        if first:
            assert p["chunks"][0]["mk"] == first, inp
        end = 0
        for k, (pc, (off, a, b)) in enumerate(zip(p["chunks"], chunks)):
            mk, beside, cap, max_tasks, hseg, lsh, _ = golden["sort"][a]
            lanes, split, chain = golden["accum"][b]
            assert [pc[x] for x in ("off", "mk", "beside", "cap", "max_tasks", "lanes", "split")] == \
                [off, mk, beside, cap, max_tasks, lanes, split], (inp, k)
            assert p["chain"] == chain and off == end, (inp, k)
            end = off + mk
            # the segmented sort's shape, as the host (hseg) and the launcher (lsh) of the parent each had it
            assert pc["segsort"] == hseg[5] == (lsh is not None), (inp, k)
            if lsh is None:
                continue
            sh = pc["sh"]
            assert sh == lsh, (inp, k)
            assert [sh[IBITS], sh[HB], sh[NSEG], sh[NBLK], sh[NSEG] * sh[NBLK]] == hseg[:5], (inp, k)
            assert sh[NSEG] == lsh[NSEG] == hseg[2] and sh[NBLK] == lsh[NBLK] == hseg[3], (inp, k)
            assert sh[JBITS] == lsh[JBITS] and sh[CHUNK] == lsh[CHUNK] and sh[NBLK] == -(-mk // sh[CHUNK]), (inp, k)
            assert sh[PRIO] == beside and sh[LB] == c - 1 - sh[HB], (inp, k)
        assert end == inp[0], inp
        # the reduction: shape, form, and how msm_finish reads the landing zone
        assert p["rcs"] == rcs and p["rc2"] == (rc_form == 2), inp
        assert combine == (nsets > 1) and ws == [nsets, 0 if tables else c, int(nsets == 1), 1], inp
        assert p["ws"] == ws_bytes, inp


def test_planned_sizes_cover_every_chunk_and_not_more(golden, plans):
    for case, p in zip(golden["cases"], plans):
        if case[4] != 0:
            continue
        inp = case_input(golden, case)
        asked = [golden["sort"][a][6] for _, a, _ in golden["lists"][case[6]]]     # per chunk: the ensure() sizes of the parent
        assert len(asked) == p["nch"]
        for s in (0, 1):     # chunk k sorts into set k & 1; a single chunk asks nothing of the second set
            users = asked[s::2]
            for i, name in enumerate(SORT):
                # blocksums was asked for twice per chunk with a segmented sort: the later, larger request is the last entry
                per_chunk = [max(e[i], e[15]) if name == "blocksums" else e[i] for e in users] or [0]
                assert all(p["sort"][s][i] >= x for x in per_chunk), (inp, s, name)
                assert p["sort"][s][i] <= max(per_chunk), (inp, s, name)


def test_host_program_refuses_a_case_cut_short(built):
    exe = os.path.join(ROOT, "tests", "cpp", "msm_plan_host")
    assert subprocess.run([exe], input="4096 0 4096 0 0\n", capture_output=True, text=True, timeout=60).returncode == 2
    r = subprocess.run([exe], input="", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == ""
