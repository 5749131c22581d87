"""CPU half of tests/test_gpu_accum.py: the harness builds and stays out of the shipped library, the bases are the points they
claim, every case's arrays pass the admission checks the harness makes (and every malformed one fails them), the heavy and task
lists are what tests/msm_sort_ref.py says a sort hands on, each case reaches the path it is named for -- read off its integers
by accum_cases.paths() -- and the integer expectation equals a sum made point by point."""
import os
import subprocess

import numpy as np
import pytest

import accum_cases as A
import arith_cases as C
import msm_sort_ref as SR
import reduce_cases as RC
from helpers import ROOT
from oracle import bls12_381 as O

HARNESS = os.path.join(ROOT, "tests", "cpp", "libdevice_accum.so")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_harness_builds_and_stays_out_of_the_library(built):
    assert os.path.exists(HARNESS)
    assert {"da_accum", "da_guard_bytes"} <= _exports(HARNESS)
    assert not {"da_accum", "da_guard_bytes"} & _exports(os.path.join(ROOT, "typlonk_amd", "libtyplonk_hip.so"))


def _base(words):
    x, y = C.val(words[:12], 32), C.val(words[12:24], 32)
    assert x < O.P and y < O.P, "canonical coordinates"
    return None if (x, y) == (0, 0) else (C.unmont(x), C.unmont(y))


def test_bases_are_the_points_they_claim():
    pl = A.pool()
    assert pl.words.shape == (len(pl.e), A.PT_WORDS) and len(pl.random) == A.N_RANDOM
    assert len(set(pl.e[pl.random])) == A.N_RANDOM and pl.e[pl.random].max() < 1 << 20 and pl.e[pl.random].min() > max(A.SMALL)
    for i in list(range(0, A.N_RANDOM, 16)) + list(range(A.N_RANDOM, len(pl.e))):
        e = int(pl.e[i])
        want = O.g1_mul(O.G1, abs(e))
        assert _base(pl.words[i]) == (O.g1_neg(want) if e < 0 else want), i
    assert all(pl.e[pl.small[k]] == k and pl.e[pl.neg_small[k]] == -k for k in A.SMALL)
    assert (pl.e[pl.neg_of] == -pl.e[:A.N_NEG]).all() and not pl.e[pl.identity].any() and not pl.words[pl.identity, :24].any()
    for s in (0, 1, -1, 255, 256, (1 << 40) - 1, -(1 << 40), (1 << 41) + 12345, -987654321):
        q = O.g1_mul(O.G1, abs(s))
        assert A.point_of(s) == (O.g1_neg(q) if s < 0 else q), s
    ent = np.array([5, 5 | (1 << 31), pl.identity[0]], dtype=np.uint32)
    assert A.scalars_of(ent).tolist() == [int(pl.e[5]), -int(pl.e[5]), 0]


ALL_CASES = [("thread-falling", lambda: A.thread_case("falling")), ("thread-scrambled", lambda: A.thread_case("scrambled")),
             ("lanes", A.lanes_case), ("lanes-scrambled", lambda: A.lanes_case("scrambled")), ("heavy", A.heavy_case), ("small", A.small_case)]


@pytest.mark.parametrize("name,make", ALL_CASES)
def test_cases_pass_the_admission_checks(name, make):
    a = make()
    n = len(A.pool().e)
    assert all(A.admit(a, n, lanes) for lanes in (1, 2, 4, 8, 16))
    assert A.admit(a, n, 4, 1, A.stored_for(a, 5)) and not A.admit(a, n, 4, 1, None)
    assert a["total"] == int(a["counts"].sum()) and a["offsets"][0] == 0
    assert RC.pool().buckets(A.stored_for(a, 5)).shape == (a["nb"], 48)


def test_whole_file_stays_near_3e5_entries():
    total = sum(make()["total"] for name, make in ALL_CASES if "scrambled" not in name)
    assert 2e5 < total < 3.5e5, total


def test_malformed_inputs_fail_the_admission_checks():
    a = A.small_case()
    n = len(A.pool().e)
    stored = A.stored_for(a, 7)
    assert A.admit(a, n, 4, 1, stored) and int(a["sched"][512]) >= 1 and int(a["sched"][513]) >= 1
    bad = A.malformed(a, n)
    assert len(bad) >= 20 and len({w for w, _, _ in bad}) == len(bad)
    for what, b, kw in bad:
        assert not A.admit(b, kw.get("npoints", n), kw.get("lanes", 4), kw.get("init", 1), None if kw.get("no_stored") else stored), what


@pytest.mark.parametrize("kind,m,cap", [("equal", 600, 32), ("two", 700, 32), ("tiny", 513, 31), ("uniform", 300, 2)])
def test_heavy_and_task_lists_are_what_the_sort_reference_hands_on(kind, m, cap):
    """a sort's output built from scalars by msm_sort_ref, rebuilt bucket by bucket with sort_output(): its schedule, records and
    tasks pass the reference's own conditions"""
    c, centred = 8, False
    W = SR.windows(c, centred)
    top_v, nb = SR.plain_top_v(c, W), W << (c - 1)
    ref = SR.reference(SR.scalars(kind, m, c), c, W, top_v, centred, 0, nb, cap)
    off = ref["offsets"]
    a = A.sort_output([ref["entries"][off[g]:off[g + 1]] for g in range(nb)], cap, "falling", 9, with_heavy=True)
    assert ref["heavy"].size >= 1 and int(a["sched"][512]) == ref["heavy"].size
    got = {k: a[k] for k in ("counts", "offsets", "sorted", "order", "sched", "heavy", "tasks")}
    assert SR.verify(ref, dict(got, guards=0), True, 0) == []
    assert a["max_tasks"] >= int(a["sched"][513])


def _bucket_tags(a, lanes_of_slot, stored_e=None):
    """the union of paths() over the schedule, every bucket under the lanes of its slot (a bucket above cap is skipped)"""
    es, off, tags = A.scalars_of(a["sorted"]), a["offsets"].astype(np.int64), set()
    for slot, g in enumerate(a["order"].astype(np.int64)):
        if a["counts"][g] <= a["cap"]:
            tags |= A.paths(es[off[g]:off[g + 1]], int(lanes_of_slot[slot]), 0 if stored_e is None else int(stored_e[g]))
    return tags


def _entries(a, name):
    g = a["names"][name]
    return A.scalars_of(a["sorted"][int(a["offsets"][g]):int(a["offsets"][g + 1])])


def test_thread_case_reaches_what_it_names():
    f, s = A.thread_case("falling"), A.thread_case("scrambled")
    assert np.array_equal(f["sorted"], s["sorted"]) and not np.array_equal(f["order"], s["order"])
    assert (np.diff(f["counts"][f["order"]]) <= 0).all() and (np.diff(s["counts"][s["order"]]) > 0).any()
    assert f["nb"] == 300 and f["cap"] == 32 and set(f["counts"]) == set(A.THREAD_COUNTS) | {33}
    assert (f["counts"] == 33).sum() == 1 and f["counts"][f["names"]["above cap"]] == 33 and f["counts"][f["names"]["at cap"]] == 32
    assert {"lane:first", "lane:add", "lane:double", "lane:cancel", "lane:identity base"} <= _bucket_tags(f, np.ones(300))
    assert A.paths(_entries(f, "P P"), 1) == {"lane:first", "lane:double"}
    assert A.paths(_entries(f, "P -P by sign"), 1) == A.paths(_entries(f, "P -P as a point"), 1) == {"lane:first", "lane:cancel"}
    assert {"lane:double", "lane:cancel"} <= A.paths(_entries(f, "-P -P 2P then on"), 1)
    assert "lane:double" in A.paths(_entries(f, "2P P 3P then on")[:3], 1) and "lane:cancel" in A.paths(_entries(f, "P 2P -3P then on")[:3], 1)
    sums = A.bucket_sums(f)
    for name in ("ends as the identity", "P -P by sign", "one identity base"):
        assert sums[f["names"][name]] == 0 and f["counts"][f["names"][name]] > 0
    assert np.count_nonzero(_entries(f, "ends as the identity")) >= 28 and sums[f["names"]["one negative entry"]] < 0
    assert (A.sort_output([[1]], 1, "falling", 0)["sorted"] >> 31 == 0).all() and (f["sorted"] >> 31).sum() > 1000


@pytest.mark.parametrize("lanes", A.LANES)
def test_lanes_case_reaches_what_it_names(lanes):
    a = A.lanes_case()
    nb, per = a["nb"], A.ACC_THREADS // lanes
    assert nb == 300 and nb % per != 0 and set(a["counts"]) >= set(A.LANE_COUNTS) | {A.LANE_CAP + 1}
    assert {lanes - 1, lanes, lanes + 1, 4 * lanes + 3, A.LANE_CAP} <= set(A.LANE_COUNTS)
    sp = A.splits(nb, lanes)
    eff = {k: A.effective_split(nb, lanes, v) for k, v in sp.items()}
    assert eff["all"] == nb and sp["half"] == nb // 2 and 0 < eff["half"] <= nb // 2
    assert 0 < eff["rounded"] < sp["rounded"] and eff["none"] == 0 < sp["none"] and len(set(eff.values())) == 4
    assert A.threads(nb, lanes, sp["all"]) % A.ACC_THREADS != 0, "lanes past the last bucket carry the identity into the butterfly"
    for k, v in sp.items():
        ls = A.slot_lanes(nb, lanes, v)
        assert set(ls) == ({lanes} if k == "all" else {lanes // 2} if k == "none" else {lanes, lanes // 2})
        tags = _bucket_tags(a, ls)
        want = {"lane:double", "lane:cancel", "lane:identity base"}
        if ls.max() >= 2:
            want |= {"pair:double", "pair:cancel", "pair:identity", "pair:add"}
        if ls.max() >= 4:
            want |= {"later:double", "later:cancel", "later:identity", "later:add"}
        assert want <= tags, (k, sorted(want - tags))
    # the mirrors by themselves: distance d meets in a lane of a d-lane group and at the step with mask d of a wider one
    for d in (1, 2, 4, 8, 16):
        for word, what in (("equal", "double"), ("opposite", "cancel")):
            es = _entries(a, f"{word} at distance {d}")
            assert f"lane:{what}" in A.paths(es, d)
            if 2 * d <= 16:
                assert f"{'pair' if d == 1 else 'later'}:{what}" in A.paths(es, 2 * d) and f"lane:{what}" not in A.paths(es, 2 * d)


@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_continue_case_reaches_what_it_names(lanes):
    a = A.lanes_case("scrambled")
    idx = A.stored_for(a, 5)
    rp, n = RC.pool(), a["names"]
    e = rp.e[idx]
    assert e[n["only P"]] == 1 and "lane:double" in A.paths(_entries(a, "only P"), lanes, 1)
    assert e[n["only -P"]] == 1 and "lane:cancel" in A.paths(_entries(a, "only -P"), lanes, 1)
    assert e[n["only 2P"]] == 2 and "lane:double" in A.paths(_entries(a, "only 2P"), lanes, 2)
    assert idx[n["at cap"]] == rp.identity[0] and idx[n["one negative entry"]] == rp.identity[1]
    assert a["counts"][n["empty"]] == 0 and idx[n["empty"]] == rp.identity[1] and a["counts"][n["empty too"]] == 0 and e[n["empty too"]] == 3
    words = rp.buckets(idx)
    assert RC.unpack48(words[n["at cap"]])[2] == 0 and RC.unpack48(words[n["one negative entry"]])[2] == O.P   # ZZ = 0 and ZZ = p
    scaled = [i for i in (n["only P"], n["only 2P"], n["3P then on"]) if RC.unpack48(words[i])[2] != C.mont(1)]
    assert len(scaled) == 3, "the named stored points are Z-scaled"
    empty = np.flatnonzero(a["counts"] == 0)
    assert empty.size >= 4 and np.count_nonzero(e[empty]) >= 2 and e[n["above cap"]] != 0
    _, untouched = A.expected(a, e, heavy_pass=False)
    assert untouched[n["above cap"]] and untouched[empty].all() and untouched.sum() == empty.size + 1
    assert len(set(idx)) > 100 and set(A.slot_lanes(a["nb"], lanes, a["nb"] // 2)) == ({1} if lanes == 1 else {lanes, lanes // 2})


def test_heavy_case_reaches_what_it_names():
    a = A.heavy_case()
    n, cnt, cap = a["names"], a["counts"], a["cap"]
    assert cap == 32 and [int(cnt[n[f"{c} entries"]]) for c in A.HEAVY_COUNTS] == list(A.HEAVY_COUNTS)
    rec = {int(b): (int(t0), int(k)) for b, t0, k, _ in a["heavy"]}
    assert sorted(rec) == np.flatnonzero(cnt > cap).tolist()
    assert [rec[n[f"{c} entries"]][1] for c in A.HEAVY_COUNTS] == list(A.HEAVY_TASKS)
    tk = a["tasks"].astype(np.int64)
    length = tk[:, 1] - tk[:, 0]
    for c in A.HEAVY_COUNTS:
        t0, k = rec[n[f"{c} entries"]]
        assert length[t0:t0 + k].max() == min(c, 1024 if c >= 65536 else 256) and length[t0:t0 + k].sum() == c
    ntasks = int(a["sched"][513])
    assert ntasks == tk.shape[0] > A.HEAVY_WAVES and ntasks <= a["max_tasks"], "the grid stride takes a second round"
    assert (length == 1).sum() >= 3 and (length == 33).sum() >= A.N_FILL and (length < 64).any()
    assert n["cap + 1"] == n["at cap"] + 1 and cnt[n["at cap"]] == cap and n["at cap"] not in rec and rec[n["cap + 1"]][1] == 1
    assert not np.array_equal(a["heavy"][:, 0], np.sort(a["heavy"][:, 0])), "the records come in no bucket order"
    es, sums = A.scalars_of(a["sorted"]), A.task_sums(a)

    def task_paths(name):
        t0, k = rec[n[name]]
        return [A.paths(es[tk[t, 0]:tk[t, 1]], 64) for t in range(t0, t0 + k)], A.paths(sums[t0:t0 + k], 64)

    for word, what in (("equal", "double"), ("opposite", "cancel")):
        for d in (1, 2, 4, 8, 16, 32):
            inside, _ = task_paths(f"{word} at distance {d}")
            assert len(inside) == 1 and f"{'pair' if d == 1 else 'later'}:{what}" in inside[0]
        inside, _ = task_paths(f"{word} at distance 64")
        assert len(inside) == 1 and f"lane:{what}" in inside[0]
        inside, closing = task_paths(f"{word} tasks")
        assert len(inside) == 2 and f"pair:{what}" in closing
    for c in (64 * 256 + 1, 65537):   # 65 partials: lane 0 of the closing fold takes two
        t0, k = rec[n[f"{c} entries"]]
        assert k == 65 and "lane:add" in A.paths(sums[t0:t0 + k], 64)
    assert not A.bucket_sums(a)[n["identity bases only"]] and cnt[n["identity bases only"]] > cap
    stored = RC.pool().e[A.stored_for(a, 6)]
    assert np.count_nonzero(stored[sorted(rec)]) > 100 and (stored[sorted(rec)] == 0).any()


def test_expectation_equals_a_sum_made_point_by_point():
    a = A.small_case()
    pl, rp = A.pool(), RC.pool()
    idx = A.stored_for(a, 7)
    want, _ = A.expected(a, rp.e[idx])
    light, _ = A.expected(a, None, heavy_pass=False)
    assert (a["counts"] > a["cap"]).any() and (light[a["counts"] > a["cap"]] == 0).all()
    off = a["offsets"].astype(np.int64)
    for g in range(a["nb"]):
        acc = C.xyzz_point(RC.unpack48(rp.words[idx[g]]))
        for ent in a["sorted"][off[g]:off[g + 1]]:
            q = _base(pl.words[int(ent) & 0x7FFFFFFF])
            acc = O.g1_add(acc, O.g1_neg(q) if int(ent) >> 31 else q)
        assert acc == A.point_of(int(want[g])), g
