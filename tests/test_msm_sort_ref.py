"""The reference of the MSM's bucket sort (tests/msm_sort_ref.py) against big integers, its checker against sorts made here with
one thing wrong, and -- through tests/cpp/msm_plan_host, msm_plan as the host compiles it -- the path every device case of
tests/test_gpu_msm_sort.py takes: segmented or atomic, how many segments, beside an accumulation or not, which window.  No GPU."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import msm_sort_ref as SR
from helpers import ROOT

R = SR.R
PAIRS = [(c, centred) for c in range(8, 21) for centred in (False, True)]


def _scalars(c):
    rng = random.Random(c)
    return SR.edge_values(c) + [rng.randrange(R) for _ in range(1000)] + [rng.randrange(1 << 64) for _ in range(20)]


@pytest.mark.parametrize("c,centred", PAIRS)
def test_digits_sum_to_the_scalar_and_stay_inside_their_windows(c, centred):
    """sum +-d 2^(jc) = k, or r - k where the centred flip is taken; |d| <= 2^(c-1), exactly 2^(c-1) positive; no carry leaves the
    top window; the top bucket index stays below 2^(c-1) -- in the plain layout with its virtual copies and in the shared set"""
    W = SR.windows(c, centred)
    ks = _scalars(c)
    mag, neg, flip, carry = SR.cut(ks, c, W, centred)
    assert not carry.any()
    assert mag.min() >= 0 and mag.max() <= 1 << (c - 1) and not neg[mag == 1 << (c - 1)].any()
    for i, k in enumerate(ks):
        value = sum((-1 if neg[i, j] else 1) * int(mag[i, j]) << (j * c) for j in range(W))
        assert value == (R - k if flip[i] else k), (k, c, centred)
        assert bool(flip[i]) == (centred and k > (R - 1) // 2)
    B = 1 << (c - 1)
    top_v = SR.plain_top_v(c, W, centred)
    for tv, tlen in ((top_v, 0), (0, 8195)):
        bucket, sign, entry = SR.place(mag, neg, flip, c, W, tv, tlen)
        live = bucket >= 0
        assert (live == (mag > 0)).all()
        top = bucket[:, W - 1][live[:, W - 1]] - (0 if tlen else (W - 1) * B)
        assert top.size == 0 or (0 <= top.min() and top.max() < B)
        assert bucket.max() < (B if tlen else W * B)
        for i in (0, 3, len(ks) - 1):
            for j in (0, W - 1):
                s = int(neg[i, j]) ^ int(flip[i])
                assert int(entry[i, j]) == ((j * tlen + i) if tlen else i) | s << 31 and int(sign[i, j]) == s
                if mag[i, j]:
                    d = int(mag[i, j])
                    want = d - 1 if tlen else (j * B + d - 1 if j + 1 < W else j * B + ((d - 1) << tv) + i % (1 << tv))
                    assert int(bucket[i, j]) == want


def test_the_edge_scalars_reach_the_edges():
    """a digit of exactly 2^(c-1), a carry through every window, the centred flip on both sides of (r - 1)/2"""
    for c in (8, 13, 16, 20):
        W = SR.windows(c, False)
        e = SR.edge_values(c)
        mag, neg, _, _ = SR.cut(e, c, W, False)
        assert mag[e.index(1 << (c - 1)), 0] == 1 << (c - 1) and not neg[e.index(1 << (c - 1)), 0]
        nw = 254 // c                                     # sum (2^(c-1) + 1) 2^(jc) below 2^254: every one of these windows carries
        _, chain, _, _ = SR.cut([sum(((1 << (c - 1)) + 1) << (j * c) for j in range(nw))], c, W, False)
        assert chain[0, :nw].all()
        _, _, flip, _ = SR.cut(e, c, SR.windows(c, True), True)
        assert not flip[e.index((R - 1) // 2)] and flip[e.index((R + 1) // 2)] and flip[e.index(R - 1)] and not flip[0]


def _perfect_sort(ref, rng):
    """a sort result that meets every condition, made from the reference: entries shuffled inside their buckets"""
    nb, counts, offsets = ref["nb"], ref["counts"], ref["offsets"]
    srt = ref["entries"].copy()
    for b in np.flatnonzero(counts > 1)[:200]:
        rng.shuffle(srt[offsets[b]:offsets[b + 1]])
    order = np.argsort(-np.minimum(counts, 255), kind="stable").astype(np.uint32)
    sched = np.zeros(514, dtype=np.uint32)
    sched[:256] = np.bincount(np.minimum(counts, 255), minlength=256)
    heavy, tasks = [], []
    for h, b in enumerate(reversed(ref["heavy"].tolist())):   # (any order of the heavy buckets is a valid one)
        tl = SR.task_len(int(counts[b]))
        k = -(-int(counts[b]) // tl)
        heavy.append([b, len(tasks), k, 0])
        tasks += [[int(offsets[b]) + t * tl, min(int(offsets[b]) + (t + 1) * tl, int(offsets[b + 1])), h] for t in range(k)]
    sched[512], sched[513] = len(heavy), len(tasks)
    return {"counts": counts.astype(np.uint32), "offsets": offsets.astype(np.uint32), "sorted": srt, "order": order, "sched": sched,
            "heavy": np.array(heavy, dtype=np.uint32).reshape(-1, 4), "tasks": np.array(tasks, dtype=np.uint32).reshape(-1, 3), "guards": 0x7FFF}


def test_checker_accepts_a_right_sort_and_names_each_wrong_one():
    """the six conditions of verify() on a sort made here, then with one thing wrong at a time: an entry in the neighbouring bucket
    of equal size, a sign, two buckets of different size swapped in the schedule, a task list one entry short, a heavy bucket
    missing, a histogram bin, a guard band"""
    c, m = 12, 2049
    W = SR.windows(c, False)
    nb = W << (c - 1)
    ks = SR.scalars("edge", m, c)[:1500] + SR.scalars("uniform", m - 1500, c)
    ref = SR.reference(ks, c, W, SR.plain_top_v(c, W), False, 0, nb, 32)
    assert ref["heavy"].size >= 3
    rng = np.random.default_rng(5)
    good = _perfect_sort(ref, rng)
    assert SR.verify(ref, good, True, 15) == []

    def wrong(**change):
        return [line[0] for line in SR.verify(ref, dict(good, **change), True, 15)]

    ones = np.flatnonzero(ref["counts"] == 1)
    a, b = int(ref["offsets"][ones[0]]), int(ref["offsets"][ones[1]])
    srt = good["sorted"].copy()
    srt[[a, b]] = srt[[b, a]]
    assert wrong(sorted=srt) == ["2"]
    srt = good["sorted"].copy()
    srt[a] ^= np.uint32(1 << 31)
    assert wrong(sorted=srt) == ["2"]
    order = good["order"].copy()
    order[[0, nb - 1]] = order[[nb - 1, 0]]
    assert wrong(order=order) == ["3"]
    order = good["order"].copy()
    order[1] = order[0]
    assert wrong(order=order) == ["3"]
    tasks = good["tasks"].copy()
    tasks[-1, 1] -= 1
    assert wrong(tasks=tasks) == ["4"]
    sched = good["sched"].copy()
    sched[513] -= 1
    assert wrong(sched=sched) == ["4"]
    sched = good["sched"].copy()
    sched[512] -= 1
    assert wrong(sched=sched) == ["4"]
    heavy = good["heavy"].copy()
    heavy[0, 1], heavy[1, 1] = heavy[1, 1], heavy[0, 1]       # two heavy buckets exchange their task rows
    assert wrong(heavy=heavy) == ["4"]
    sched = good["sched"].copy()
    sched[1] += 1
    sched[0] -= 1
    assert wrong(sched=sched) == ["5"]
    assert wrong(guards=0x7FFF ^ 4) == ["6"]
    counts = good["counts"].copy()
    counts[ones[0]] = 0
    assert "1" in wrong(counts=counts)


def test_harness_builds_and_stays_out_of_the_library(built):
    def exports(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}

    harness = exports(os.path.join(ROOT, "tests", "cpp", "libdevice_sort.so"))
    shipped = exports(os.path.join(ROOT, "typlonk_amd", "libtyplonk_hip.so"))
    mine = {"ds_sort", "ds_plan", "ds_info_words", "ds_guard_buffers"}
    assert mine <= harness and not mine & shipped


# ---- the path every device case takes --------------------------------------------------------------------------------------
def _plans(lines):
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "msm_plan_host")], input="\n".join(lines) + "\n", capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    out = [json.loads(x) for x in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def test_every_device_case_takes_the_path_it_is_there_for(built):
    cases = SR.CASES
    assert len({c["name"] for c in cases}) == len(cases)
    plans = _plans([SR.plan_line(c["m"], c["mode"], c["len"], c["table_c"], c["chunks"], c["staged"]) for c in cases])
    for case, p in zip(cases, plans):
        exp, name = case["expect"], case["name"]
        assert p["status"] == 0 and case["k"] < len(p["chunks"]), name
        ck = p["chunks"][case["k"]]
        sh = ck["sh"]
        assert p["tables"] == exp["tables"] and p["nch"] == exp["nch"], name
        assert p["c"] == exp["c"] and p["W"] == exp.get("W", p["W"]) and p["nb"] == exp.get("nb", p["nb"]), name
        assert p["centred"] == exp.get("centred", 0) and p["scatter_staged"] == exp.get("staged", 1), name
        if case["atomic"]:
            assert not p["tables"] and 2 <= -(-p["nb"] // 2048) <= 256, name
            continue
        assert ck["segsort"] == exp["segsort"] == 1 and sh[SR.S_PRIO] == exp["prio"] == ck["beside"], name
        assert sh[SR.S_NSEG] <= 8192 and sh[SR.S_NBLK] == exp.get("nblk", sh[SR.S_NBLK]) and sh[SR.S_TLEN] == exp.get("tlen", sh[SR.S_TLEN]), name
        assert sh[SR.S_CHUNK] == exp.get("chunk", 256), name
        assert sh[SR.S_C] == p["c"] and sh[SR.S_W] == p["W"] and sh[SR.S_TOP_V] == p["digit_v"] and sh[SR.S_CENTRED] == p["centred"], name
        if exp.get("top_v_positive"):
            assert p["digit_v"] > 0, name
        # the numbers the device test derives for itself are the plan's
        assert p["W"] == SR.windows(p["c"], bool(p["centred"])), name
        assert p["digit_v"] == (0 if p["tables"] else SR.plain_top_v(p["c"], p["W"])), name
    by_name = {c["name"]: p for c, p in zip(cases, plans)}
    # one level-1 workgroup against two; the XCD-ordered column against the identity column; 1024-entry tasks
    assert [by_name[f"plain-{m}"]["chunks"][0]["sh"][SR.S_NBLK] for m in (255, 256, 257, 2048, 2049)] == [1, 1, 2, 8, 9]
    big = by_name["plain-65537"]
    assert big["chunks"][0]["cap"] < 65536 <= 65537 and SR.task_len(65537) == 1024 and SR.task_len(65535) == 256
    assert by_name["atomic-65537"]["nb"] == 256 * 2048
    assert {by_name[f"atomic-{m}"]["nb"] for m in (1, 4097)} == {4096, 81920}


def test_what_only_the_long_msms_reach(built):
    """a stand-alone MSM of 2^23 + 5 terms is eight segmented chunks; the same length queued is one chunk for the atomic counting
    sort; 2^22 + 1 terms queued are the segmented sort's wide form, 16384 segments, and 2^22 still the fused one with 8192"""
    plans = _plans([SR.plan_line(m, mode, (1 << 23) + 5, 0) for m, mode, _ in SR.LONG_PLANS])
    for (m, mode, exp), p in zip(SR.LONG_PLANS, plans):
        assert p["status"] == 0 and not p["tables"] and p["nch"] == exp["nch"] == len(p["chunks"]) and p["c"] == 16, (m, mode)
        assert all(ck["segsort"] == exp["segsort"] for ck in p["chunks"]), (m, mode)
        if "nseg" in exp:
            assert p["chunks"][0]["sh"][SR.S_NSEG] == exp["nseg"], (m, mode)
        if mode == SR.ALONE:
            assert all(ck["sh"][SR.S_NSEG] <= 8192 for ck in p["chunks"]), (m, mode)
