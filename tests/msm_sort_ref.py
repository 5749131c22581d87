"""What the MSM's bucket sort (msm_sort.hip) must hand to the accumulation, stated in Python integers (numpy only for bulk), for
tests/test_gpu_msm_sort.py (device, through tests/cpp/libdevice_sort.so) and tests/test_msm_sort_ref.py (the reference itself and
the plan of every device case, on the CPU).

The sort's input is m scalars; its output is, for every (term i, window j) whose digit is not zero, one entry in one bucket:
  * k' = k, or with centred scalars min(k, r - k), the sign of every digit flipped where r - k is taken;
  * k' = sum_j d_j 2^(jc) with signed c-bit digits |d_j| <= 2^(c-1): the c bits of window j plus the carry of the window below; a
    value above 2^(c-1) becomes value - 2^c and carries one into the next window, a value of exactly 2^(c-1) stays positive;
  * a plain MSM gives every window its own 2^(c-1) buckets, bucket j B + |d| - 1, and spreads the top window's few digits over
    2^top_v virtual copies, ((|d| - 1) << top_v) + (i mod 2^top_v); a table-mode MSM has one shared set, bucket |d| - 1;
  * the entry is i | sign << 31, in table mode (j tlen + i) | sign << 31: the gather index of base i in table j.
From the buckets follow counts, their exclusive prefix, the heavy buckets (more than `cap` entries) and the tasks that tile each
of those.  The order of the entries inside a bucket is not defined; verify() compares multisets."""
from __future__ import annotations

import random

import numpy as np

from oracle import bls12_381 as O

R = O.R
INFO_WORDS = 32
# info[] of the harness (csrc/harness/device_sort.hip)
I_C, I_W, I_DIGIT_V, I_NB, I_CAP, I_SEGSORT, I_SHAPE = 0, 1, 2, 3, 4, 5, 6
I_STAGED, I_NCH, I_OFF, I_MK, I_MAX_TASKS, I_TABLES, I_CENTRED, I_ATOMIC, I_GUARDS, I_HEAVY, I_NTASKS = range(20, 31)
# MsmShape in declaration order
S_C, S_W, S_TOP_V, S_HB, S_LB, S_NSEG, S_NBLK, S_CHUNK, S_IBITS, S_JBITS, S_TLEN, S_NSETS, S_CENTRED, S_PRIO = range(14)


def windows(c: int, centred: bool) -> int:
    """windows of the signed c-bit digits of a canonical scalar below 2^255 (centred: |k| below 2^254): one more than
    ceil(bits / c) when the top window is c bits wide, since its digit may then carry"""
    bits = 254 if centred else 255
    w0 = -(-bits // c)
    return w0 + (1 if bits - c * (w0 - 1) == c else 0)


def plain_top_v(c: int, W: int, centred: bool = False) -> int:
    """virtual-copy bits of a plain MSM's top window: its t scalar bits are brought up to the c - 1 bits of a bucket index"""
    t = (254 if centred else 255) - c * (W - 1)
    return 0 if t >= c - 1 else c - 1 - t


def task_len(count: int) -> int:
    return 1024 if count >= 65536 else 256


# ---- digits ----------------------------------------------------------------------------------------------------------------
def cut(ks, c: int, W: int, centred: bool):
    """canonical scalars -> (|d| (m, W) int64, negative (m, W) bool, flipped (m,) bool, carry out of the top window (m,) int64)"""
    m = len(ks)
    flip = np.zeros(m, dtype=bool)
    if centred:
        flip = np.array([R - k < k for k in ks], dtype=bool)   # (k = 0: r - 0 is not below 0, no flip)
        ks = [min(k, R - k) if k else 0 for k in ks]
    # 288 bits per scalar, so that every window of W c <= 288 bits reads inside the array
    limbs = np.frombuffer(b"".join(k.to_bytes(40, "little") for k in ks), dtype="<u4").reshape(m, 10).astype(np.uint64)
    mag = np.zeros((m, W), dtype=np.int64)
    neg = np.zeros((m, W), dtype=bool)
    carry = np.zeros(m, dtype=np.int64)
    half = 1 << (c - 1)
    for j in range(W):
        w, sh = divmod(j * c, 32)
        two = limbs[:, w] | (limbs[:, w + 1] << np.uint64(32))
        d = ((two >> np.uint64(sh)) & np.uint64((1 << c) - 1)).astype(np.int64) + carry
        over = d > half
        mag[:, j] = np.where(over, (1 << c) - d, d)
        neg[:, j] = over
        carry = over.astype(np.int64)
    return mag, neg, flip, carry


def place(mag, neg, flip, c: int, W: int, top_v: int, tlen: int):
    """digits -> (bucket (m, W) int64, -1 where the digit is zero; sign (m, W) uint32; entry (m, W) uint32)"""
    m = mag.shape[0]
    B = 1 << (c - 1)
    i = np.arange(m, dtype=np.int64)[:, None]
    j = np.arange(W, dtype=np.int64)[None, :]
    if tlen:
        bucket = mag - 1
        index = j * tlen + i
    else:
        bucket = j * B + mag - 1
        bucket[:, W - 1] = (W - 1) * B + ((mag[:, W - 1] - 1) << top_v) + (i[:, 0] & ((1 << top_v) - 1))
        index = np.broadcast_to(i, (m, W))
    bucket = np.where(mag == 0, -1, bucket)
    sign = (neg ^ flip[:, None]).astype(np.uint32)
    entry = (index.astype(np.uint32) | (sign << np.uint32(31))).astype(np.uint32)
    return bucket, sign, entry


def reference(ks, c: int, W: int, top_v: int, centred: bool, tlen: int, nb: int, cap: int) -> dict:
    """everything the sort hands on, from canonical scalars"""
    mag, neg, flip, carry = cut(ks, c, W, centred)
    assert not carry.any(), "a carry left the top window"
    bucket, _, entry = place(mag, neg, flip, c, W, top_v, tlen)
    live = bucket >= 0
    b, e = bucket[live], entry[live]
    assert b.size == 0 or (0 <= b.min() and b.max() < nb), "bucket outside the bucket sets"
    counts = np.bincount(b, minlength=nb).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    by_bucket = np.lexsort((e, b))
    return {"counts": counts, "offsets": offsets, "entries": e[by_bucket], "heavy": np.flatnonzero(counts > cap), "nb": nb, "cap": cap}


# ---- the six conditions ------------------------------------------------------------------------------------------------------
def verify(ref: dict, got: dict, atomic: bool, nguards: int) -> list[str]:
    """got: counts, offsets, sorted, order, sched (words 0..513), heavy (n, 4), tasks (n, 3), guards (bit mask) as the harness
    returns them.  The conditions that do not hold, as text; empty when all six do."""
    bad = []
    nb, cap = ref["nb"], ref["cap"]
    counts = got["counts"].astype(np.int64)
    offsets = got["offsets"].astype(np.int64)
    # 1. counts, their exclusive prefix, the number of non-zero digits
    if not np.array_equal(counts, ref["counts"]):
        w = np.flatnonzero(counts != ref["counts"])
        bad.append(f"1: counts differ in {w.size} buckets, first {w[:4].tolist()}: {counts[w[:4]].tolist()} != {ref['counts'][w[:4]].tolist()}")
    if not np.array_equal(offsets, ref["offsets"]):
        bad.append("1: offsets are not the exclusive prefix of the reference's counts")
    total = int(ref["offsets"][nb])
    if int(offsets[nb]) != total:
        bad.append(f"1: offsets[nb] = {int(offsets[nb])}, {total} digits are not zero")
        return bad
    # 2. every bucket's multiset of entries (the entries in bucket order, each bucket sorted by value)
    srt = got["sorted"][:total]
    where = np.repeat(np.arange(nb), ref["counts"])
    mine = srt[np.lexsort((srt, where))]
    if not np.array_equal(mine, ref["entries"]):
        w = np.flatnonzero(mine != ref["entries"])
        bad.append(f"2: {w.size} entries differ, first in bucket {int(where[w[0]])}: {int(mine[w[0]]):#x} != {int(ref['entries'][w[0]]):#x}")
    # 3. the schedule: a permutation, largest size class first
    order = got["order"].astype(np.int64)
    if not np.array_equal(np.sort(order), np.arange(nb)):
        bad.append("3: order is not a permutation of the buckets")
    else:
        key = np.minimum(ref["counts"][order], 255)
        if (np.diff(key) > 0).any():
            bad.append(f"3: min(count, 255) rises along order at {int(np.flatnonzero(np.diff(key) > 0)[0])}")
    # 4. heavy buckets and their tasks
    sched = got["sched"].astype(np.int64)
    nheavy, ntasks = int(sched[512]), int(sched[513])
    want = ref["heavy"]
    if nheavy != want.size:
        bad.append(f"4: word 512 = {nheavy}, {want.size} buckets hold more than cap = {cap}")
    else:
        heavy = got["heavy"][:nheavy].astype(np.int64).reshape(-1, 4)
        tasks = got["tasks"].astype(np.int64).reshape(-1, 3)
        if not np.array_equal(np.sort(heavy[:, 0]), want):
            bad.append("4: heavy[] does not name exactly the buckets above cap")
        else:
            cnt = ref["counts"][heavy[:, 0]]
            tl = np.where(cnt >= 65536, 1024, 256)
            k = -(-cnt // tl)
            if not np.array_equal(heavy[:, 2], k) or heavy[:, 3].any():
                bad.append("4: heavy[4h + 2] != ceil(count / task length) or heavy[4h + 3] != 0")
            elif ntasks != int(k.sum()) or tasks.shape[0] < ntasks:
                bad.append(f"4: word 513 = {ntasks}, the heavy buckets need {int(k.sum())} tasks")
            else:
                # the row ranges [t0, t0 + k) are disjoint and cover [0, word 513): sorted by t0 they follow one another
                by_t0 = np.argsort(heavy[:, 1], kind="stable")
                t0 = heavy[by_t0, 1]
                if not np.array_equal(t0, np.cumsum(k[by_t0]) - k[by_t0]):
                    bad.append("4: the task rows of the heavy buckets are not disjoint ranges covering [0, word 513)")
                else:
                    h = np.repeat(np.arange(nheavy), k)                       # the heavy bucket of every expected row
                    step = np.arange(int(k.sum())) - np.repeat(np.cumsum(k) - k, k)   # the task's number inside its bucket
                    row = heavy[h, 1] + step
                    lo = ref["offsets"][heavy[h, 0]] + step * tl[h]
                    hi = np.minimum(lo + tl[h], ref["offsets"][heavy[h, 0]] + cnt[h])
                    if not (np.array_equal(tasks[row, 0], lo) and np.array_equal(tasks[row, 1], hi) and np.array_equal(tasks[row, 2], h)):
                        bad.append("4: the tasks do not tile their buckets in steps of the task length")
    # 5. the atomic sort's size histogram
    if atomic and not np.array_equal(sched[:256], np.bincount(np.minimum(ref["counts"], 255), minlength=256)):
        bad.append("5: words 0..255 are not the histogram of min(count, 255)")
    # 6. nothing was written past a buffer
    if got["guards"] != (1 << nguards) - 1:
        bad.append(f"6: guard bands overwritten, intact mask {got['guards']:#x}")
    return bad


# ---- scalars -------------------------------------------------------------------------------------------------------------
def edge_values(c: int) -> list[int]:
    nw = -(-255 // c)
    return [0, 1, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, (1 << (c - 1)) - 1, 1 << (c - 1), (1 << (c - 1)) + 1, (1 << c) - 1, 1 << c,
            sum((1 << (c - 1)) << (j * c) for j in range(nw)) % R, sum(((1 << (c - 1)) + 1) << (j * c) for j in range(nw)) % R,
            1 << 254, (1 << 254) - 1]


KINDS = ("edge", "uniform", "equal", "two", "tiny", "zero")


def scalars(kind: str, m: int, c: int, seed: int = 1) -> list[int]:
    """m canonical scalars: the edge set repeated to length m, uniform below r, one value, two values alternating, the values
    0..15 in turn, all zero"""
    rng = random.Random(f"{kind}-{m}-{c}-{seed}")
    if kind == "edge":
        e = edge_values(c)
        return [e[i % len(e)] for i in range(m)]
    if kind == "uniform":
        return [rng.randrange(R) for _ in range(m)]
    if kind == "equal":
        return [rng.randrange(R)] * m
    if kind == "two":
        a, b = rng.randrange(R), rng.randrange(R)
        return [a if i % 2 == 0 else b for i in range(m)]
    if kind == "tiny":
        return [i % 16 for i in range(m)]
    assert kind == "zero"
    return [0] * m


def montgomery_words(ks) -> np.ndarray:
    """canonical scalars -> (m, 8) uint32, the residues k 2^256 mod r the library takes"""
    memo: dict[int, bytes] = {}
    for k in set(ks) if len(ks) > 64 else ():
        memo[k] = (k * O.FR_MONT_R % R).to_bytes(32, "little")
    raw = b"".join(memo[k] if k in memo else (k * O.FR_MONT_R % R).to_bytes(32, "little") for k in ks)
    return np.frombuffer(raw, dtype="<u4").reshape(len(ks), 8).copy()


# ---- the device cases --------------------------------------------------------------------------------------------------
TABLE_LEN = (1 << 13) + 3
QUEUED, ALONE = 2, 0


def _case(name, m, mode, length, table_c, kinds, chunks=0, staged=1, k=0, atomic=0, expect=None):
    return {"name": name, "m": m, "mode": mode, "len": length, "table_c": table_c, "kinds": kinds, "chunks": chunks, "staged": staged, "k": k,
            "atomic": atomic, "expect": expect or {}}


def _cases():
    out = []
    # a plain SRS, queued: one chunk, the segmented sort in its fused form
    plain = [(1, ("uniform", "equal", "zero"), dict(c=8, nblk=1)),
             (255, ("edge", "uniform", "tiny"), dict(c=8, nblk=1)),
             (256, ("edge", "uniform", "tiny"), dict(c=8, nblk=1)),
             (257, KINDS, dict(c=9, nblk=2)),
             (2048, ("edge", "uniform", "equal"), dict(c=11, nblk=8)),                 # the XCD-ordered column
             (2049, ("edge", "uniform", "two", "tiny", "zero"), dict(c=12, nblk=9)),   # the identity column
             (4097, ("edge", "uniform", "equal", "tiny"), dict(c=13, nblk=17, top_v_positive=True)),
             ((1 << 14) + 1, ("edge", "uniform", "equal"), dict(c=15, W=18)),          # the constant-width cutter on a plain SRS
             ((1 << 16) + 1, ("equal", "two", "edge"), dict(c=16))]                    # 65537 entries in a bucket: 1024-entry tasks
    for m, kinds, exp in plain:
        out.append(_case(f"plain-{m}", m, QUEUED, m, 0, kinds, expect=dict(exp, segsort=1, prio=0, tables=0, nch=1)))
    # tables over 2^13 + 3 points: the run-time cutter with tlen (14), the centred windows (15, 17), 20
    for c, centred in ((14, 0), (15, 1), (17, 1), (20, 0)):
        for m in (TABLE_LEN, 2049, 4097):
            kinds = KINDS if m == TABLE_LEN else ("edge", "uniform")
            out.append(_case(f"tables{c}-{m}", m, QUEUED, TABLE_LEN, c, kinds,
                             expect=dict(c=c, segsort=1, prio=0, tables=1, centred=centred, nch=1, tlen=TABLE_LEN)))
    out.append(_case("tables20-4096", 4096, QUEUED, TABLE_LEN, 20, ("edge", "uniform"),                 # XCD-ordered column, table mode
                     expect=dict(c=20, segsort=1, prio=0, tables=1, nch=1, nblk=16)))
    # 2^18 + 1 terms: level-1 workgroups of 2048 scalars -- 512 threads, four scalars each with the next one's load in flight, a last
    # workgroup of one scalar -- and a staging area beyond 64 KiB of LDS: the shape of the level-1 kernels from here up to 2^20 terms
    big = (1 << 18) + 1
    out.append(_case(f"tables20-{big}", big, QUEUED, big, 20, ("uniform", "edge"),
                     expect=dict(c=20, segsort=1, prio=0, tables=1, nch=1, chunk=2048, nblk=129, tlen=big)))
    out.append(_case(f"plain-{big}", big, QUEUED, big, 0, ("uniform",), expect=dict(c=16, segsort=1, prio=0, tables=0, nch=1, chunk=2048, nblk=129)))
    # overrides: two chunks of a stand-alone MSM, the second sorted beside the first's accumulation; the direct level-1 scatter
    for k in (0, 1):
        out.append(_case(f"chunks2-plain-k{k}", 8193, ALONE, 8193, 0, ("edge", "uniform", "tiny"), chunks=2, k=k,
                         expect=dict(c=14, segsort=1, prio=k, tables=0, nch=2)))
        out.append(_case(f"chunks2-tables20-k{k}", 8193, ALONE, TABLE_LEN, 20, ("edge", "uniform", "equal"), chunks=2, k=k,
                         expect=dict(c=20, segsort=1, prio=k, tables=1, nch=2)))
    out.append(_case("direct-plain-2049", 2049, QUEUED, 2049, 0, ("edge", "uniform", "tiny"), staged=0,
                     expect=dict(c=12, segsort=1, prio=0, tables=0, nch=1, staged=0)))
    out.append(_case("direct-tables20", TABLE_LEN, QUEUED, TABLE_LEN, 20, ("edge", "uniform", "equal"), staged=0,
                     expect=dict(c=20, segsort=1, prio=0, tables=1, nch=1, staged=0)))
    # the atomic counting sort on plain inputs the plan gives to the segmented sort: 2 .. 40 scan blocks, then 256
    for m, c in ((1, 8), (257, 9), (2049, 12), (4097, 13)):
        out.append(_case(f"atomic-{m}", m, QUEUED, m, 0, ("edge", "uniform", "tiny"), atomic=1,
                         expect=dict(c=c, nb=windows(c, False) << (c - 1), tables=0, nch=1)))
    out.append(_case("atomic-65537", (1 << 16) + 1, QUEUED, (1 << 16) + 1, 0, ("equal",), atomic=1, expect=dict(c=16, nb=1 << 19, tables=0, nch=1)))
    return out


CASES = _cases()
# what only the C ABI reaches at a size a test can afford once (tests/test_gpu_msm.py, the slow test): (m, mode) on a plain SRS
LONG_PLANS = [((1 << 23) + 5, ALONE, dict(nch=8, segsort=1)), ((1 << 23) + 5, QUEUED, dict(nch=1, segsort=0)),
              ((1 << 23) + 4, QUEUED, dict(nch=1, segsort=0)), ((1 << 22) + 1, QUEUED, dict(nch=1, segsort=1, nseg=16384)),
              (1 << 22, QUEUED, dict(nch=1, segsort=1, nseg=8192))]


def plan_line(m, mode, length, table_c, chunks=0, staged=1) -> str:
    """one case in the input format of tests/cpp/msm_plan_host: T and centred from the window, as typlonk_srs_precompute"""
    centred = int(bool(table_c) and windows(table_c, True) < windows(table_c, False))
    T = windows(table_c, bool(centred)) if table_c else 0
    return f"{m} {mode} {length} {table_c} {T} {centred} {chunks} 0 {staged} 0 -1"
