"""What the MSM's bucket accumulation (msm_accum.hip) is given and what it must leave in every bucket, in Python integers (numpy
only for bulk), for tests/test_gpu_accum.py (device, through tests/cpp/libdevice_accum.so) and tests/test_accum_cases.py (the
cases themselves, on the CPU).

Every base is e_i G for a known integer e_i: about 2^10 random ones below 2^20, the small multiples G, 2G, 3G, 5G, the negatives
of some as points of their own, and the identity base (0, 0).  An entry is index | sign << 31 as the sorts emit it and stands for
+-e_i, a stored bucket (reduce_cases.Pool) for its own e, so what a bucket must hold afterwards is (stored e + sum of +-e_i) G:
one cumulative sum over the entries and one short fixed-base multiplication per bucket.  The order of the entries inside a bucket
is fixed here, which decides where equal and opposite points meet: in one lane's g1_madd_acc, in the pair step of the butterfly
or in a later one.  paths() says which, from the integers alone, so a case can assert that it reaches what it is there for.

The offsets, the schedule, the heavy records and the task list are built by the rules tests/msm_sort_ref.py states for the sorts:
count > cap is heavy; a heavy bucket is tiled by tasks of 256 entries, 1024 from 65536 entries on."""
from __future__ import annotations

import random

import numpy as np

import arith_cases as C
import msm_sort_ref as SR
import reduce_cases as RC
from oracle import bls12_381 as O

PT_WORDS = 32                   # words per SRS record (launch.hpp): x, y as 12 packed words each, 8 words of padding
ACC_THREADS = 128               # MSM_ACC_THREADS (msm_common.hpp)
HEAVY_WAVES = 1024 * (ACC_THREADS // 64)   # MSM_HEAVY_GRID workgroups of two wavefronts: the tasks one round of the grid stride takes
SIGN = np.uint32(1 << 31)
N_RANDOM, N_NEG = 1024, 64
SMALL = (1, 2, 3, 5)
LANES = (2, 4, 8, 16)
INVALID = 1                     # hipErrorInvalidValue


# ---- scalars to points -------------------------------------------------------------------------------------------------------
_TABLE: list = []
_MUL_CACHE: dict = {}


def _table():
    """d 2^(8w) G for d < 256, w < 5: a scalar below 2^40 is at most five additions"""
    if not _TABLE:
        base = O.G1
        for _ in range(5):
            row = [None]
            for _ in range(255):
                row.append(O.g1_add(row[-1], base))
            _TABLE.append(row)
            base = O.g1_add(row[255], base)
    return _TABLE


def point_of(scalar: int):
    """scalar * G for a signed integer"""
    scalar = int(scalar)
    if scalar not in _MUL_CACHE:
        k = abs(scalar)
        if k >> 40:
            q = O.g1_mul(O.G1, k % O.R)
        else:
            q = None
            for w, row in enumerate(_table()):
                q = O.g1_add(q, row[(k >> (8 * w)) & 255])
        _MUL_CACHE[scalar] = O.g1_neg(q) if scalar < 0 else q
    return _MUL_CACHE[scalar]


# ---- the bases ---------------------------------------------------------------------------------------------------------------
def pack_base(pt) -> list[int]:
    """an affine point in the SRS's internal form (g1.hpp, fq30.hpp): x 2^390 mod p and y 2^390 mod p, canonical, each as 12 packed
    32-bit words; the identity is (0, 0).  The last 8 words of a record are padding no kernel reads: they hold a pattern here."""
    x, y = (0, 0) if pt is None else (C.mont(pt[0]), C.mont(pt[1]))
    return C.limbs(x, 12, 32) + C.limbs(y, 12, 32) + [0xC0FFEE00 + j for j in range(PT_WORDS - 24)]


class Pool:
    """e[i]: the scalar of base i; words[i]: its record.  random: the indices of the random bases; small[k] / neg_small[k]: k G and
    -k G; neg_of[i]: the base holding -e_i G for the first N_NEG random ones; identity: the two (0, 0) bases"""

    def __init__(self, seed: int = 0xACC0):
        rnd = random.Random(seed)
        es = rnd.sample(range(max(SMALL) + 1, 1 << 20), N_RANDOM)
        e = list(es)
        self.random = np.arange(N_RANDOM)
        self.small = {k: len(e) + j for j, k in enumerate(SMALL)}
        e += list(SMALL)
        self.neg_small = {k: len(e) + j for j, k in enumerate(SMALL)}
        e += [-k for k in SMALL]
        self.neg_of = np.arange(len(e), len(e) + N_NEG)
        e += [-x for x in es[:N_NEG]]
        self.identity = np.array([len(e), len(e) + 1])
        e += [0, 0]
        self.e = np.array(e, dtype=np.int64)
        self.words = np.array([pack_base(point_of(x)) for x in e], dtype=np.uint32)


_POOL: list[Pool] = []


def pool() -> Pool:
    if not _POOL:
        _POOL.append(Pool())
    return _POOL[0]


def scalars_of(entries: np.ndarray) -> np.ndarray:
    """the signed integer every entry stands for"""
    entries = np.asarray(entries, dtype=np.uint32)
    return pool().e[entries & ~SIGN] * (1 - 2 * (entries >> np.uint32(31)).astype(np.int64))


# ---- where equal and opposite points meet ------------------------------------------------------------------------------------
def paths(es, lanes: int, start: int = 0) -> set[str]:
    """es: the scalars a group of `lanes` lanes strides over (entry i goes to lane i mod lanes); start: what lane 0 begins with
    (0: the identity).  The exceptional branches this reaches, by name: in a lane's own additions ("lane:"), in the butterfly's
    first step ("pair:"), in a later one ("later:").  Scalars are far below the group order, so equal integers are equal points."""
    tags, part = set(), []
    for lane in range(lanes):
        acc = start if lane == 0 else 0
        for q in es[lane::lanes]:
            q = int(q)
            if q == 0:
                tags.add("lane:identity base")
                continue
            tags.add("lane:first" if acc == 0 else "lane:double" if acc == q else "lane:cancel" if acc == -q else "lane:add")
            acc += q
        part.append(acc)
    mask = 1
    while mask < lanes:
        step = "pair" if mask == 1 else "later"
        for lane in range(lanes):
            if not lane & mask:
                a, b = part[lane], part[lane ^ mask]
                tags.add(f"{step}:identity" if a == 0 or b == 0 else f"{step}:double" if a == b else f"{step}:cancel" if a == -b else f"{step}:add")
                part[lane] = part[lane ^ mask] = a + b
        mask <<= 1
    return tags


# ---- the launch's slot arithmetic, restated (launch_msm_accum) ---------------------------------------------------------------
def effective_split(nb: int, lanes: int, split: int) -> int:
    """slots [0, split) get `lanes` lanes, the rest lanes / 2; split is rounded down to whole workgroups unless it covers all"""
    if lanes <= 1 or split >= nb:
        return nb
    per = ACC_THREADS // lanes
    return split // per * per


def slot_lanes(nb: int, lanes: int, split: int) -> np.ndarray:
    """lanes of every slot of the schedule"""
    out = np.full(nb, max(lanes // 2, 1), dtype=np.int64)
    out[:effective_split(nb, lanes, split)] = lanes
    return out


def threads(nb: int, lanes: int, split: int) -> int:
    s = effective_split(nb, lanes, split)
    return nb if lanes <= 1 else s * lanes + (nb - s) * (lanes // 2)


def splits(nb: int, lanes: int) -> dict:
    """the four splits of a lanes case: one class; half the slots; one that is rounded down to a whole workgroup; one below a
    workgroup's worth, rounded to 0"""
    per = ACC_THREADS // lanes
    return {"all": nb, "half": nb // 2, "rounded": per + per // 2, "none": per - 1}


# ---- a sort's output from buckets of entries -----------------------------------------------------------------------------------
def task_bound(total: int, cap: int) -> int:
    """max_tasks as msm_plan sizes it"""
    return total // 256 + total // cap + 2


def heavy_lists(counts: np.ndarray, offsets: np.ndarray, cap: int, rng) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(sched[516], heavy (n, 4), tasks (n, 3)): a record (bucket, first task row, tasks, done = 0) per bucket above cap, in an order
    of the generator's choosing as the sorts' atomics leave it, and rows (from, to, record) tiling each in steps of the task length"""
    hb = rng.permutation(np.flatnonzero(counts > cap))
    cnt = counts[hb]
    tl = np.array([SR.task_len(int(c)) for c in cnt], dtype=np.int64)
    k = -(-cnt // tl) if hb.size else cnt
    t0 = np.cumsum(k) - k
    heavy = np.stack([hb, t0, k, np.zeros_like(k)], axis=1).astype(np.uint32).reshape(-1, 4)
    h = np.repeat(np.arange(hb.size), k)
    step = np.arange(int(k.sum())) - np.repeat(t0, k)
    lo = offsets[hb[h]] + step * tl[h] if hb.size else step
    hi = np.minimum(lo + tl[h], offsets[hb[h] + 1]) if hb.size else step
    tasks = np.stack([lo, hi, h], axis=1).astype(np.uint32).reshape(-1, 3)
    sched = np.zeros(516, dtype=np.uint32)
    sched[:256] = np.bincount(np.minimum(counts, 255), minlength=256)
    sched[512], sched[513] = hb.size, tasks.shape[0]
    return sched, heavy, tasks


def sort_output(buckets: list, cap: int, order: str, seed: int, with_heavy: bool = False) -> dict:
    """the arrays of one chunk's sort whose bucket g holds buckets[g], in that order"""
    rng = np.random.default_rng([seed, len(buckets), cap])
    counts = np.array([len(b) for b in buckets], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    srt = np.concatenate([np.asarray(b, dtype=np.uint32) for b in buckets]) if counts.sum() else np.zeros(0, dtype=np.uint32)
    by_size = np.argsort(-np.minimum(counts, 255), kind="stable")
    out = {"nb": len(buckets), "cap": cap, "counts": counts, "offsets": offsets.astype(np.uint32), "sorted": srt.astype(np.uint32),
           "order": (by_size if order == "falling" else rng.permutation(len(buckets))).astype(np.uint32), "total": int(offsets[-1]),
           "sched": None, "heavy": None, "tasks": None, "max_tasks": 0}
    if with_heavy:
        out["sched"], out["heavy"], out["tasks"] = heavy_lists(counts, offsets, cap, rng)
        out["max_tasks"] = task_bound(out["total"], cap)
    return out


def admit(a: dict, npoints: int, lanes: int, init: int = 0, stored=None) -> bool:
    """the harness's admission checks (csrc/harness/device_accum.hip), restated: no kernel index leaves its array"""
    nb, total = a["nb"], a["total"]
    off = a["offsets"].astype(np.int64)
    ok = lanes in (1, 2, 4, 8, 16) and nb >= 1 and npoints >= 1 and init in (0, 1) and (not init or stored is not None)
    ok = ok and off.shape == (nb + 1,) and (np.diff(off) >= 0).all() and int(off[nb]) == total and a["sorted"].shape == (total,)
    ok = ok and (total == 0 or int((a["sorted"] & ~SIGN).max()) < npoints)
    ok = ok and np.array_equal(np.sort(a["order"].astype(np.int64)), np.arange(nb))
    if a["sched"] is None:
        return bool(ok and a["heavy"] is None and a["tasks"] is None)
    if a["heavy"] is None or a["tasks"] is None:
        return False
    nheavy, ntasks = int(a["sched"][512]), int(a["sched"][513])
    hv, tk = a["heavy"].astype(np.int64), a["tasks"].astype(np.int64)
    ok = ok and nheavy <= a["max_tasks"] and ntasks <= a["max_tasks"] and hv.shape == (nheavy, 4) and tk.shape == (ntasks, 3)
    ok = ok and (tk[:, 0] < tk[:, 1]).all() and (tk[:, 1] <= total).all() and (tk[:, 2] < nheavy).all()
    ok = ok and (hv[:, 0] < nb).all() and (hv[:, 2] >= 1).all() and (hv[:, 1] + hv[:, 2] <= ntasks).all() and not hv[:, 3].any()
    return bool(ok)


# ---- what must come back -------------------------------------------------------------------------------------------------------
def bucket_sums(a: dict) -> np.ndarray:
    """per bucket the integer sum of its entries"""
    run = np.concatenate([[0], np.cumsum(scalars_of(a["sorted"]))])
    off = a["offsets"].astype(np.int64)
    return run[off[1:]] - run[off[:-1]]


def task_sums(a: dict) -> np.ndarray:
    run = np.concatenate([[0], np.cumsum(scalars_of(a["sorted"]))])
    tk = a["tasks"].astype(np.int64)
    return run[tk[:, 1]] - run[tk[:, 0]]


def expected(a: dict, stored_e=None, heavy_pass: bool = True) -> tuple[np.ndarray, np.ndarray]:
    """(scalar of every bucket afterwards, whether the bucket's words must be exactly the stored ones).  Without the heavy pass a
    bucket above cap is left to it: the identity with init = 0, the stored bucket otherwise."""
    sums = bucket_sums(a)
    heavy = a["counts"] > a["cap"]
    if not heavy_pass:
        sums = np.where(heavy, 0, sums)
    base = np.zeros(a["nb"], dtype=np.int64) if stored_e is None else np.asarray(stored_e, dtype=np.int64)
    untouched = (a["counts"] == 0) | (heavy & (not heavy_pass)) if stored_e is not None else np.zeros(a["nb"], dtype=bool)
    return base + sums, untouched


# ---- bucket contents -------------------------------------------------------------------------------------------------------------
def _random_entries(rng, n: int) -> np.ndarray:
    """n entries: random bases with random signs, now and then an identity base, a small multiple or a negative held as a point"""
    pl = pool()
    idx = rng.choice(pl.random, n)
    kind = rng.integers(0, 20, n)
    idx = np.where(kind == 0, pl.identity[rng.integers(0, 2, n)], idx)
    idx = np.where(kind == 1, np.array(list(pl.small.values()))[rng.integers(0, len(SMALL), n)], idx)
    idx = np.where(kind == 2, pl.neg_of[rng.integers(0, N_NEG, n)], idx)
    return idx.astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))


def mirror(rng, d: int, opposite: bool, reps: int = 1) -> np.ndarray:
    """Q_0 .. Q_(d-1) and then the same d points again (or their opposites): equal (opposite) points at distance d; `reps` such
    blocks of fresh points one after the other.  A group of d lanes meets each pair in one lane's additions; a group of 2d, 4d, ...
    lanes holds equal (opposite) sums on lanes l and l + d and meets them in the butterfly step with mask d."""
    out = []
    for _ in range(reps):
        q = rng.choice(pool().random, d, replace=False).astype(np.uint32) | (rng.integers(0, 2, d).astype(np.uint32) << np.uint32(31))
        out += [q, q ^ SIGN if opposite else q]
    return np.concatenate(out)


def _light_buckets(cap: int, count_set, mirrors, nb: int, seed: int) -> tuple[list, dict]:
    """nb buckets of at most cap entries, one of cap + 1, and the named ones that place equal and opposite points"""
    pl = pool()
    rng = np.random.default_rng([seed, cap, nb])
    g, g2, g3, g5 = (np.uint32(pl.small[k]) for k in SMALL)
    ident = np.uint32(pl.identity[0])
    some = int(pl.random[7])
    rest = lambda n: _random_entries(rng, n)   # noqa: E731
    named = {
        "P P": [g, g],
        "P -P by sign": [g, g | SIGN],
        "P -P as a point": [g, np.uint32(pl.neg_small[1])],
        "-P -P 2P then on": np.concatenate([[g | SIGN, g | SIGN, g2], rest(28)]),
        "identity bases between": np.concatenate([[ident, g5, ident, ident, g5, np.uint32(pl.identity[1])], rest(26)]),
        "ends as the identity": np.concatenate([q := rest(16), (q ^ SIGN)[::-1]]),
        "one negative entry": [np.uint32(some) | SIGN],
        "one identity base": [ident],
        "two identity bases": [ident, np.uint32(pl.identity[1])],
        "above cap": rest(cap + 1),
        "2P P 3P then on": np.concatenate([[g2, g, g3], rest(29)]),
        "P 2P -3P then on": np.concatenate([[g, g2, g3 | SIGN], rest(28)]),
        "only P": [g],
        "only -P": [g | SIGN],
        "only 2P": [g2],
        "3P then on": np.concatenate([[g3], rest(30)]),
        "at cap": rest(cap),
        "empty": [],
        "empty too": [],
    }
    for d in mirrors:
        named[f"equal at distance {d}"] = mirror(rng, d, False)
        named[f"opposite at distance {d}"] = mirror(rng, d, True)
        # the same at full size, so that the schedule puts it among the largest buckets whatever the split
        named[f"equal at distance {d}, up to cap"] = mirror(rng, d, False, cap // (2 * d))
        named[f"opposite at distance {d}, up to cap"] = mirror(rng, d, True, cap // (2 * d))
    names = {n: i for i, n in enumerate(named)}
    buckets = [np.asarray(b, dtype=np.uint32) for b in named.values()]
    counts = list(count_set) * 2 + list(rng.choice(sorted(count_set), nb))   # every count of the set, then random ones
    buckets += [rest(int(c)) for c in counts[:nb - len(buckets)]]
    return buckets, names


THREAD_COUNTS = (0, 1, 2, 31, 32)
LANE_CAP = 96
LANE_COUNTS = tuple(sorted({0, 1, LANE_CAP} | {c for L in LANES for c in (L - 1, L, L + 1, 4 * L + 3)}))
NB_LIGHT = 300
_CACHE: dict = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def thread_case(order: str) -> dict:
    """one thread per bucket: cap 32, counts 0, 1, 2, 31, 32 and the named buckets"""
    def make():
        buckets, names = _light_buckets(32, THREAD_COUNTS, (), NB_LIGHT, 1)
        return dict(sort_output(buckets, 32, order, 11), names=names)
    return _once(("thread", order), make)


def lanes_case(order: str = "falling") -> dict:
    """the same named buckets with cap 96, counts around every lane count, and equal / opposite points at every power-of-two distance"""
    def make():
        buckets, names = _light_buckets(LANE_CAP, LANE_COUNTS, (1, 2, 4, 8, 16), NB_LIGHT, 2)
        return dict(sort_output(buckets, LANE_CAP, order, 12), names=names)
    return _once(("lanes", order), make)


def stored_for(a: dict, seed: int) -> np.ndarray:
    """reduce_cases pool indices of the stored buckets a continuing chunk starts from: random ones (every Z scaling, both identity
    encodings) and, for the named buckets, P under P, P under -P, 2P under 2P at the largest lifts, 3P, and the two identities --
    the ZZ = p one also under a bucket with nothing to add, which must keep that encoding"""
    rp = RC.pool()
    rng = np.random.default_rng([seed, a["nb"]])
    idx = rng.integers(0, len(rp.e), a["nb"])
    at = {int(rp.e[ids[0]]): ids for (_, sign), ids in rp.of.items() if sign == 1}
    names = a.get("names", {})
    for name, ids in (("only P", at[1][2]), ("only -P", at[1][0]), ("only 2P", at[2][1]), ("3P then on", at[3][2]), ("P P", at[1][1]),
                      ("at cap", rp.identity[0]), ("one negative entry", rp.identity[1]), ("one identity base", at[2][2]),
                      ("empty", rp.identity[1]), ("empty too", at[3][1]), ("above cap", at[2][1])):
        if name in names:
            idx[names[name]] = ids
    return idx


HEAVY_CAP = 32
HEAVY_COUNTS = (33, 256, 257, 64 * 256, 64 * 256 + 1, 65536, 65537)
HEAVY_TASKS = (1, 1, 2, 64, 65, 64, 65)
N_FILL = 1800


def heavy_case() -> dict:
    """cap 32: buckets of every task count that matters, equal and opposite points inside a task and between two tasks, a bucket at
    cap beside one above it, light buckets, and 33-entry buckets until the tasks outnumber the launch's wavefronts"""
    def make():
        rng = np.random.default_rng(3)
        rest = lambda n: _random_entries(rng, n)   # noqa: E731
        named = {f"{c} entries": rest(c) for c in HEAVY_COUNTS}
        named["at cap"] = rest(HEAVY_CAP)
        named["cap + 1"] = rest(HEAVY_CAP + 1)
        for opp in (False, True):
            word = "opposite" if opp else "equal"
            for d in (1, 2, 4, 8, 16):   # a 33-entry task: one entry per lane, the two halves of the mirror meet at the step with mask d
                named[f"{word} at distance {d}"] = np.concatenate([mirror(rng, d, opp), rest(33 - 2 * d)])
            named[f"{word} at distance 32"] = mirror(rng, 32, opp)
            named[f"{word} at distance 64"] = mirror(rng, 64, opp)          # the same lane of one task
            named[f"{word} tasks"] = mirror(rng, 256, opp)                 # two tasks with equal (opposite) partials: the closing fold
        named["identity bases only"] = np.full(40, pool().identity[0], dtype=np.uint32)
        names = {n: i for i, n in enumerate(named)}
        buckets = [np.asarray(b, dtype=np.uint32) for b in named.values()]
        buckets += [rest(int(c)) for c in rng.integers(0, HEAVY_CAP + 1, 40)]
        buckets += [rest(33) for _ in range(N_FILL)]
        return dict(sort_output(buckets, HEAVY_CAP, "falling", 13, with_heavy=True), names=names)
    return _once("heavy", make)


def small_case() -> dict:
    """a case small enough to add point by point"""
    def make():
        buckets, names = _light_buckets(8, (0, 1, 2, 7, 8), (), 24, 4)
        return dict(sort_output(buckets[:3] + buckets[5:9] + buckets[17:], 8, "scrambled", 14, with_heavy=True), names={})
    return _once("small", make)


def malformed(a: dict, npoints: int) -> list[tuple[str, dict, dict]]:
    """(what, arrays, call arguments that differ) for every input the harness must refuse; a has heavy buckets and tasks"""
    def edit(key, at, value):
        b = dict(a)
        b[key] = a[key].copy()
        b[key][at] = value
        return b
    nb, total, ntasks = a["nb"], a["total"], int(a["sched"][513])
    first = int(np.flatnonzero(a["counts"] > 0)[0])
    out = [("three lanes", a, {"lanes": 3}), ("32 lanes", a, {"lanes": 32}), ("no lanes", a, {"lanes": 0}),
           ("offsets fall", edit("offsets", first + 1, int(a["offsets"][first + 1]) + total + 1), {}),
           ("offsets end before total", edit("offsets", nb, total - 1), {}),
           ("offsets end past total", edit("offsets", nb, total + 1), {}),
           ("an entry past the points", edit("sorted", total // 2, npoints), {}),
           ("an entry past the points under its sign bit", edit("sorted", total - 1, np.uint32(npoints) | SIGN), {}),
           ("fewer points than the entries name", a, {"npoints": int((a["sorted"] & ~SIGN).max())}),
           ("order names a bucket twice", edit("order", 0, int(a["order"][1])), {}),
           ("order names a bucket past the last", edit("order", nb - 1, nb), {}),
           ("a task ends past the entries", edit("tasks", (0, 1), total + 1), {}),
           ("a task begins at its end", edit("tasks", (0, 0), int(a["tasks"][0, 1])), {}),
           ("a task names a record past the last", edit("tasks", (0, 2), int(a["sched"][512])), {}),
           ("a record names a bucket past the last", edit("heavy", (0, 0), nb), {}),
           ("a record's tasks end past the task count", edit("heavy", (0, 2), ntasks + 1), {}),
           ("a record's first task lies past the task count", edit("heavy", (0, 1), ntasks), {}),
           ("a record without tasks", edit("heavy", (0, 2), 0), {}),
           ("a done counter that is not zero", edit("heavy", (0, 3), 1), {}),
           ("more tasks than max_tasks", dict(a, max_tasks=ntasks - 1), {}),
           ("more records than max_tasks", edit("sched", 512, a["max_tasks"] + 1), {}),
           ("counters without lists", dict(a, heavy=None, tasks=None), {}),
           ("init without stored buckets", a, {"no_stored": True})]
    return out


def wrong_points(got: np.ndarray, want: np.ndarray, counts=None, untouched=None, stored=None) -> list[str]:
    """got: (n, 48) words.  Every point within the stored-XYZZ bounds, the group element want[i] G, and where nothing was to be added
    the stored words themselves.  One line per point that is not."""
    bad = []
    for i in range(got.shape[0]):
        c = RC.unpack48(got[i])
        try:
            assert C._xyzz_ok(c), "XYZZ invariants X < 5.1p, Y < 3.2p, ZZ, ZZZ < 1.1p"
            assert C.xyzz_point(c) == point_of(int(want[i])), "point"
            if untouched is not None and untouched[i]:
                assert np.array_equal(got[i], stored[i]), "nothing to add, but the stored words changed"
        except AssertionError as e:
            bad.append(f"{i}: {e}" if counts is None else f"{i} ({int(counts[i])} entries): {e}")
    return bad
