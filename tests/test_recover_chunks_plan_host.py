"""recover_chunks_plan.hpp, every decision of a typlonk_recover_chunks call, without a GPU: the header as the host compiles it on its
own (tests/cpp/recover_chunks_plan_host, a program with its own main and no HIP include), run plain and under the address and
undefined-behaviour sanitizers over one table of cases; both must print the same lines.  The refusals, each alone and in the
order the header states them (two at once: the earlier one is reported); the number of slices the missing set is cut into at
r = 2, 128, 2^12 and 2^16 with 0, 1 and r - 1 missing cosets and in between; the slices and the scatter's tiles walked the
kernels' way; and the sizes of the temporaries against values worked out by hand."""
import json
import os
import subprocess

import pytest

from helpers import ROOT

INVALID_ARG, LENGTH, DOMAIN, RANGE = -1, -2, -3, -7
PROGRAMS = ["recover_chunks_plan_host", "recover_chunks_plan_host_san"]


def case(log_n, log_l, m, K, count, nulls=0, cosets=None, null_cosets=False, want=(1, 0, 0), bufs=None, offsets_null=False, slices=0):
    """one line of the program's input; cosets: None = 0 .. K - 1; bufs: `count` (buffer, length, offset) with want[2] = 1"""
    t = [log_n, log_l, m, K, count, nulls]
    if null_cosets:
        t.append(2)
    elif cosets is None:
        t.append(0)
    else:
        assert len(cosets) == K
        t += [1] + list(cosets)
    t += list(want)
    if want[2]:
        assert len(bufs) == count
        t.append(int(offsets_null))
        for b in bufs:
            t += list(b)
    t.append(slices)
    return " ".join(map(str, t))


def run(name, lines):
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", name)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
    out = [json.loads(x) for x in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


# (text the verdict must contain, the case): each refusal alone, in the header's order
OK_BUFS = [(1, 100, 0), (1, 100, 50), (2, 64, 14)]
REFUSALS = [
    (INVALID_ARG, "null argument", case(4, 1, 4, 2, 1, nulls=1)),
    (INVALID_ARG, "null argument", case(4, 1, 4, 2, 1, null_cosets=True)),
    (INVALID_ARG, "null argument", case(4, 1, 4, 2, 1, nulls=2)),
    (INVALID_ARG, "null argument", case(4, 1, 4, 2, 1, nulls=4)),
    (INVALID_ARG, "null argument", case(4, 1, 4, 2, 1, nulls=8)),
    (INVALID_ARG, "no output", case(4, 1, 4, 2, 1, want=(0, 0, 0))),
    (INVALID_ARG, "null entry", case(4, 1, 4, 2, 3, want=(0, 0, 1), bufs=[(1, 100, 0), (0, 0, 0), (2, 64, 0)])),
    (DOMAIN, "log_n outside", case(0, 0, 1, 1, 1)),
    (DOMAIN, "log_n outside", case(25, 10, 1, 1, 1)),
    (DOMAIN, "log_l >= log_n", case(4, 4, 1, 1, 1)),
    (DOMAIN, "log_l >= log_n", case(4, 7, 1, 1, 1)),
    (DOMAIN, "> 16", case(17, 0, 1, 1, 1)),
    (DOMAIN, "> 16", case(24, 7, 1, 1, 1)),
    (LENGTH, "at least one cell", case(4, 1, 1, 0, 1)),
    (LENGTH, "more cells than cosets", case(4, 1, 1, 9, 1)),
    (LENGTH, "at least one polynomial", case(4, 1, 1, 2, 0)),
    (LENGTH, "at least one coefficient", case(4, 1, 0, 2, 1)),
    (LENGTH, "too few cells for this degree bound", case(4, 1, 5, 2, 1)),
    (LENGTH, "2^26", case(20, 6, 1, 1, 65)),
    (RANGE, "a coset >= r", case(4, 1, 4, 2, 1, cosets=[3, 8])),
    (RANGE, "range outside buffer", case(4, 1, 4, 2, 3, want=(0, 0, 1), bufs=[(1, 100, 0), (1, 100, 97), (2, 64, 0)])),
    (RANGE, "range outside buffer", case(4, 1, 4, 2, 1, want=(0, 0, 1), bufs=[(1, 3, 0)], offsets_null=True)),
    (RANGE, "range outside buffer", case(4, 1, 4, 2, 1, want=(0, 0, 1), bufs=[(1, 100, 101)])),
    (INVALID_ARG, "a coset named twice", case(4, 1, 4, 3, 1, cosets=[5, 2, 5])),
    (INVALID_ARG, "the same range", case(4, 1, 4, 2, 3, want=(0, 0, 1), bufs=[(1, 100, 10), (2, 64, 0), (1, 100, 13)])),
    (INVALID_ARG, "the same range", case(4, 1, 4, 2, 2, want=(0, 0, 1), bufs=[(1, 100, 77), (1, 100, 0)], offsets_null=True)),
]
# two refusals at once: the earlier in the header's order is the one reported
PAIRS = [
    (INVALID_ARG, "null argument", case(0, 0, 1, 1, 1, nulls=4)),                                       # a null status and log_n = 0
    (INVALID_ARG, "no output", case(4, 1, 9, 2, 1, want=(0, 0, 0))),                                     # no output and m > K l
    (INVALID_ARG, "null entry", case(4, 4, 4, 2, 2, want=(0, 0, 1), bufs=[(0, 0, 0), (1, 9, 0)])),      # a null entry and log_l = log_n
    (DOMAIN, "> 16", case(20, 3, 1, 0, 1)),                                                             # too many cosets and K = 0
    (DOMAIN, "log_l >= log_n", case(4, 5, 1, 1, 0)),                                                    # log_l and count = 0
    (LENGTH, "at least one cell", case(4, 1, 0, 0, 0)),                                                 # K = 0 before count = 0 and m = 0
    (LENGTH, "too few cells", case(4, 1, 5, 2, 1, cosets=[9, 9])),                                      # m > K l and cosets out of range, twice
    (RANGE, "a coset >= r", case(4, 1, 4, 2, 1, cosets=[8, 8])),                                        # out of range and named twice
    (RANGE, "a coset >= r", case(4, 1, 4, 2, 1, cosets=[8, 1], want=(0, 0, 1), bufs=[(1, 2, 0)])),      # a coset, then a buffer too short
    (RANGE, "range outside buffer", case(4, 1, 4, 2, 2, cosets=[1, 1], want=(0, 0, 1), bufs=[(1, 4, 0), (1, 4, 1)])),   # before the coset named twice
    (INVALID_ARG, "a coset named twice", case(4, 1, 4, 2, 2, cosets=[1, 1], want=(0, 0, 1), bufs=[(1, 8, 0), (1, 8, 1)])),   # before the shared range
]
ADMITTED = [
    case(4, 1, 4, 2, 3, want=(1, 1, 1), bufs=OK_BUFS),
    case(4, 1, 4, 2, 2, want=(0, 0, 1), bufs=[(1, 8, 0), (1, 8, 4)]),                                   # ranges that touch
    case(4, 1, 4, 2, 2, want=(0, 0, 1), bufs=[(1, 4, 0), (2, 4, 0)], offsets_null=True),                # the same offset of two buffers
    case(24, 8, 1 << 23, 1 << 15, 4),                                                                   # the largest call: count n = 2^26
    case(16, 0, 1, 1, 1),
]
# the slices: (log_r, missing) -> the plan's own
SLICE_SHAPES = [(lr, mi) for lr in (1, 7, 12, 16) for mi in sorted({0, 1, 7, 8, 15, 16, 17, 255, 256, 257, 600, (1 << lr) // 2, (1 << lr) - 1})
                if mi < 1 << lr]
NAMED = [(10, mi, s) for mi in (0, 1, 255, 256, 257, 600, 1023) for s in (1, 2, 3, 64)]


@pytest.fixture(scope="module")
def outputs(built):
    lines = [c for _, _, c in REFUSALS + PAIRS] + ADMITTED
    lines += [case(lr, 0, 1, (1 << lr) - mi, 1) for lr, mi in SLICE_SHAPES]
    lines += [case(lr, 0, 1, (1 << lr) - mi, 1, slices=s) for lr, mi, s in NAMED]
    plain, san = run(PROGRAMS[0], lines), run(PROGRAMS[1], lines)
    assert plain == san
    return plain


def test_every_refusal_in_the_headers_order(outputs):
    for (code, text, _), out in zip(REFUSALS + PAIRS, outputs):
        assert out["code"] == code and text in out["text"], (code, text, out)
    header = open(os.path.join(ROOT, "include", "typlonk.h")).read()
    assert "too few cells for this degree bound" in header


def test_admitted_calls_and_their_sizes(outputs):
    base = len(REFUSALS) + len(PAIRS)
    outs = outputs[base:base + len(ADMITTED)]
    assert all(o["code"] == 0 and o["covered"] in (1, -1) for o in outs), outs
    p = outs[0]                                     # (4, 1): n = 16, l = 2, r = 8; K = 2, m = 4, count = 3, every output
    assert (p["n"], p["l"], p["r"], p["known"], p["missing"]) == (16, 2, 8, 2, 6)
    assert p["slices"] == 1 and p["per_slice"] == 6 and p["tiles"] == 1 and p["vanish_xblocks"] == 1
    assert p["bytes_consts"] == 4 * 8 * 32 and p["bytes_partial"] == 1 * 16 * 32 and p["bytes_index"] == (8 + 6) * 4
    assert p["bytes_cells"] == 3 * 2 * 2 * 32 and p["bytes_work"] == 3 * 16 * 32 and p["bytes_out"] == 3 * 4 * 32 and p["bytes_evals"] == 3 * 16 * 32
    assert p["excess_len"] == 0 and p["excess_blocks"] == 1 and p["excess_iters"] == 0 and p["bytes_verdict"] == 3 * (25 + 8)
    assert p["bytes_total"] == 1024 + 512 + 56 + 384 + 1536 + 384 + 1536 + 99
    assert (p["log_tk"], p["log_tt"], p["scatter_tiles"]) == (3, 1, 1)
    p = outs[1]                                     # the device output alone: no host staging
    assert p["bytes_out"] == 0 and p["bytes_evals"] == 0
    p = outs[3]                                     # (24, 8) with K = 2^15, m = 2^23, count = 4
    assert p["missing"] == 1 << 15 and p["slices"] == 1 and p["per_slice"] == 1 << 15 and p["tiles"] == (1 << 15) // p["tile"]
    assert p["bytes_work"] == 4 << 29 and p["bytes_cells"] == 4 << 28 and p["bytes_out"] == 4 << 28 and p["bytes_evals"] == 0
    assert (p["log_tk"], p["log_tt"], p["scatter_tiles"]) == (4, 4, 1 << 16)
    assert p["excess_len"] == 0
    p = outs[4]                                     # (16, 0), K = 1: the most factors a value has
    assert p["missing"] == 65535 and p["slices"] == 1 and p["vanish_xblocks"] == 512 and (p["log_tk"], p["log_tt"]) == (8, 0)


def test_the_slice_count(outputs):
    base = len(REFUSALS) + len(PAIRS) + len(ADMITTED)
    own = dict(zip(SLICE_SHAPES, outputs[base:base + len(SLICE_SHAPES)]))
    for (lr, mi), p in own.items():
        r = 1 << lr
        assert p["code"] == 0 and p["covered"] == 1 and p["missing"] == mi, p
        xb = -(-2 * r // 256)
        want = max(1, min(512 // xb, mi // 8, 64))                      # to 512 workgroups, 8 factors a slice at least, 64 at most
        per = max(1, -(-mi // want))
        assert p["vanish_xblocks"] == xb and p["per_slice"] == per and p["slices"] == (-(-mi // per) if mi else 1), p
        assert p["tiles"] == -(-per // p["tile"]) and p["slices"] * p["per_slice"] >= mi
        assert p["bytes_partial"] == p["slices"] * 2 * r * 32
    assert own[(7, 64)]["slices"] == 8 and own[(7, 127)]["slices"] == 15        # r = 128: one workgroup of values, cut by the factors
    assert own[(12, 2048)]["slices"] == 16 and own[(12, 4095)]["slices"] == 16  # r = 2^12: 32 workgroups of values, 16 slices
    assert all(own[(16, mi)]["slices"] == 1 for lr, mi in SLICE_SHAPES if lr == 16)   # r = 2^16: no split
    assert all(own[(lr, mi)]["slices"] == 1 for lr, mi in SLICE_SHAPES if mi < 16)    # nothing to cut
    named = outputs[base + len(SLICE_SHAPES):]
    for (lr, mi, s), p in zip(NAMED, named):
        assert p["code"] == 0 and p["covered"] == 1, p
        assert p["slices"] <= max(1, min(s, mi)) and p["slices"] * p["per_slice"] >= mi > (p["slices"] - 1) * p["per_slice"] - (mi == 0), p


def test_the_finish_spans(built):
    lines = [case(20, 4, m, 1 << 15, 1) for m in (1, (1 << 19) - 4096, (1 << 19) - 4097, (1 << 19) - 1, 1 << 19)]
    for p, m in zip(run(PROGRAMS[0], lines), (1, (1 << 19) - 4096, (1 << 19) - 4097, (1 << 19) - 1, 1 << 19)):
        length = (1 << 19) - m
        assert p["excess_len"] == length and p["excess_blocks"] * p["excess_span"] >= length and p["excess_iters"] * 256 >= p["excess_span"]
        assert p["excess_blocks"] == (max(1, min(256, -(-length // 4096))) if length else 1), p
        assert length == 0 or (p["excess_blocks"] - 1) * p["excess_span"] < length          # no workgroup without an index


def test_a_case_cut_short_is_an_error(built):
    for name in PROGRAMS:
        r = subprocess.run([os.path.join(ROOT, "tests", "cpp", name)], input="4 1 4\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 2
