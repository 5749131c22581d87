"""Cases and checks of the paired Fq30 products (fq30.hpp: fq30_mul_pair, fq30_sqr_pair, fq30_mul2_add), shared by the
host test (tests/test_fq30_pair.py) and the device test (tests/test_gpu_fq30_pair.py).

The operands are tests/arith_cases.py's fq30_mul / fq30_sqr / fq30_mul2_add lists: random, lifted (x + k p) and extreme
(all-ones digits, 2^390 - 1, the fused columns 10..14 near their maxima).  A pair takes case i as its first product and
case (i + SHIFT) as its second, so the two chains of one call carry different operands, extremes beside random ones.
Every result is checked as arith_cases.fq_check checks the single products: the exact REDC value, the residue and the
value bound p + T / 2^390, and limbs < 2^30."""
from __future__ import annotations

import numpy as np

import arith_cases as C

OP_MUL_PAIR, OP_SQR_PAIR, OP_MUL2_ADD = 0, 1, 2
SHIFT = 97


def _arr(vals) -> np.ndarray:
    out = np.zeros((len(vals), 13), dtype=np.uint32)
    for i, v in enumerate(vals):
        out[i] = C.limbs(v, 13)
    return out


def cases(op: int) -> list[tuple]:
    """(a, b, c, d) per call"""
    if op == OP_MUL2_ADD:
        return C._fq_mul2_cases(43)
    src = C._fq_mul_cases(41, False) if op == OP_MUL_PAIR else [(x[0], x[0]) for x in C._fq_mul_cases(42, True)]
    n = len(src)
    return [src[i] + src[(i + SHIFT) % n] for i in range(n)]


def run_and_check(fn, op: int) -> None:
    """fn(op, a, b, c, d, out0, out1, n) -> return code: the host or the device entry point"""
    cs = cases(op)
    n = len(cs)
    assert C.distinct(cs) >= 2000
    ins = [np.ascontiguousarray(_arr([c[k] for c in cs])) for k in range(4)]
    out0 = np.zeros((n, 13), dtype=np.uint32)
    out1 = np.zeros((n, 13), dtype=np.uint32)
    rc = fn(op, *ins, out0, out1, n)
    assert rc == 0, f"error {rc}"
    fails = []
    for i, (a, b, c, d) in enumerate(cs):
        try:
            assert (out0[i] <= C.M30).all() and (out1[i] <= C.M30).all(), "limbs not normalised (< 2^30)"
            if op == OP_MUL2_ADD:
                assert a * b + c * d < C.FQ_R * C.FQ_R, "precondition"
                C.fq_check("fq30_mul2_add", (a, b, c, d), C.val(out0[i]), 0)
            else:
                name = "fq30_mul" if op == OP_MUL_PAIR else "fq30_sqr"
                for (x, y), out in (((a, b), out0[i]), ((c, d), out1[i])):
                    assert x * y < C.FQ_R * C.FQ_R, "precondition"
                    C.fq_check(name, (x, y) if op == OP_MUL_PAIR else (x,), C.val(out), 0)
        except AssertionError as e:
            fails.append(f"#{i} {[hex(x) for x in (a, b, c, d)]}: {e}")
    assert not fails, f"op {op}: {len(fails)} of {n} cases wrong, first: " + "; ".join(fails[:4])
