"""Writes typlonk_amd/csrc/fq30_pair.hpp: the device bodies of the paired Fq30 products -- fq30_mul_pair and
fq30_sqr_pair (two fused Montgomery products as two interleaved column chains) and the two un-reduced products of
fq30_mul2_add.

Why generated.  Each column of the two chains is ONE inline-asm statement in which the v_mad_u64_u32 of chain A and
chain B alternate, each chain accumulating in place from its shifted carry.  Inside a statement the order is kept as
written: the compiler can neither split a column into fresh accumulators that it then merges with a 64-bit add
(v_lshl_add_u64, ~26 per multiplication) nor pad between two mads of the statement (its one-state pad after an asm
statement falls at the column boundary, where the Montgomery digit is computed in C++).  Every column reads a different
set of limbs, so each statement has its own operand list: 26 statements per product kind, written out by this script.

Program order inside one chain is fq30_mulsqr_fused's: reduction terms m_i p_(k-i), then the product terms, then (C++,
after the statement) m_k p_0; the carry-capture schedule is the same (columns 11..14 from product term 10 of a
multiplication / 5 of a squaring, m_k p_0 of columns 10..12), so tools/fq30_fused_bounds.py proves each chain's columns.

usage: python tools/gen_fq30_pair.py       (rewrites the header; the build does not run it)"""
from __future__ import annotations

import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "typlonk_amd", "csrc", "fq30_pair.hpp")
IND = "    "


def chain_terms(sqr: bool, k: int, reduce: bool, x: str, y: str, m: str, d: str):
    """(left, right, capture) of one chain's column k in program order; p limbs as ('P', j)"""
    terms = []
    wide = 10 <= k <= 14
    first = 5 if sqr else 10
    if reduce:
        for i in range(k - 12 if k > 12 else 0, k if k < 13 else 13):
            terms.append((f"{m}[{i}]", ("P", k - i), False))
    if k < 25:
        lo, hi = (k - 12 if k > 12 else 0), (k if k < 12 else 12)
        idx = 0
        if sqr:
            if k % 2 == 0:
                terms.append((f"{x}.v[{k // 2}]", f"{x}.v[{k // 2}]", False))
                idx += 1
            for i in range(lo, hi + 1):
                if 2 * i >= k:
                    break
                terms.append((f"{d}[{i}]", f"{x}.v[{k - i}]", reduce and wide and k >= 11 and idx >= first))
                idx += 1
        else:
            for i in range(lo, hi + 1):
                terms.append((f"{x}.v[{i}]", f"{y}.v[{k - i}]", reduce and wide and k >= 11 and idx >= first))
                idx += 1
    return terms


def merge(la, lb):
    """interleave two ordered lists as evenly as their lengths allow, A first"""
    out, i, j = [], 0, 0
    while i < len(la) or j < len(lb):
        if j >= len(lb) or (i < len(la) and i * len(lb) <= j * len(la)):
            out.append(("A", la[i]))
            i += 1
        else:
            out.append(("B", lb[j]))
            j += 1
    return out


def column_asm(ta, tb) -> str:
    if not ta and not tb:
        return f"{IND}// (no terms)"
    caps = {"A": any(t[2] for t in ta), "B": any(t[2] for t in tb)}
    outs = ["accA", "accB"] + [f"hi{c}" for c in "AB" if caps[c]]
    onum = {n: i for i, n in enumerate(outs)}
    ins: list[tuple[str, str]] = []
    inum: dict[str, int] = {}

    def opnd(e):
        con = "v"
        if isinstance(e, tuple):
            e, con = f"fq30_kp(1, {e[1]})", "s"
        if e not in inum:
            inum[e] = len(outs) + len(ins)
            ins.append((con, e))
        return f"%{inum[e]}"

    lines = []
    for who, (l, r, cap) in merge(ta, tb):
        acc = f"%{onum['acc' + who]}"
        lines.append(f"v_mad_u64_u32 {acc}, vcc, {opnd(l)}, {opnd(r)}, {acc}")
        if cap:
            hi = f"%{onum['hi' + who]}"
            lines.append(f"v_addc_co_u32 {hi}, vcc, 0, {hi}, vcc")
    text = "\n".join(f'{IND}    "{ln}\\n\\t"' for ln in lines[:-1])
    text += ("\n" if len(lines) > 1 else "") + f'{IND}    "{lines[-1]}"'
    o = ", ".join(f'"+v"({n})' for n in outs)
    i = ", ".join(f'"{c}"({e})' for c, e in ins)
    return f"{IND}asm({text.lstrip()}\n{IND}    : {o}\n{IND}    : {i}\n{IND}    : \"vcc\");"


def reduced_pair(sqr: bool) -> str:
    if sqr:
        s = ["// a*a and c*c, both reduced (fq30_sqr_pair)",
             "__device__ __forceinline__ void fq30_sqr_pair_dev(const Fq30& a, const Fq30& c, Fq30& ra, Fq30& rc) {",
             f"{IND}uint32_t mA[13], mB[13], dA[13], dB[13];",
             f"#pragma unroll",
             f"{IND}for (int i = 0; i < 13; ++i) {{",
             f"{IND}    dA[i] = a.v[i] << 1;",
             f"{IND}    dB[i] = c.v[i] << 1;",
             f"{IND}}}"]
        args = ("a", "a", "mA", "dA"), ("c", "c", "mB", "dB")
        res = ("ra", "rc")
    else:
        s = ["// a*b and c*d, both reduced (fq30_mul_pair)",
             "__device__ __forceinline__ void fq30_mul_pair_dev(const Fq30& a, const Fq30& b, const Fq30& c, const Fq30& d, Fq30& ra, Fq30& rc) {",
             f"{IND}uint32_t mA[13], mB[13];"]
        args = ("a", "b", "mA", ""), ("c", "d", "mB", "")
        res = ("ra", "rc")
    s.append(f"{IND}uint64_t accA = 0, accB = 0;")
    s.append(f"{IND}uint32_t hiA = 0, hiB = 0;")
    for k in range(26):
        wide = 10 <= k <= 14
        s.append(f"{IND}// column {k}")
        if wide:
            s.append(f"{IND}hiA = 0;")
            s.append(f"{IND}hiB = 0;")
        s.append(column_asm(chain_terms(sqr, k, True, *args[0]), chain_terms(sqr, k, True, *args[1])))
        if k < 13:
            s.append(f"{IND}FQ30_PAIR_DIGIT({k});")
        else:
            s.append(f"{IND}{res[0]}.v[{k - 13}] = (uint32_t)accA & FQ30_MASK;")
            s.append(f"{IND}{res[1]}.v[{k - 13}] = (uint32_t)accB & FQ30_MASK;")
        s.append(f"{IND}FQ30_PAIR_SHIFT({'true' if wide else 'false'});")
    s.append("}")
    return "\n".join(s) + "\n"


def wide_pair() -> str:
    s = ["// the 26 digit sums of a*b and c*d, not reduced (fq30_mul2_add); the same digits as two fq30_mul_wide added",
         "__device__ __forceinline__ void fq30_mul_wide_pair_dev(const Fq30& a, const Fq30& b, const Fq30& c, const Fq30& d, uint32_t (&T)[26]) {",
         f"{IND}uint64_t accA = 0, accB = 0;"]
    for k in range(25):
        s.append(f"{IND}// column {k}")
        s.append(column_asm(chain_terms(False, k, False, "a", "b", "", ""), chain_terms(False, k, False, "c", "d", "", "")))
        s.append(f"{IND}T[{k}] = ((uint32_t)accA & FQ30_MASK) + ((uint32_t)accB & FQ30_MASK);")
        s.append(f"{IND}accA >>= 30;")
        s.append(f"{IND}accB >>= 30;")
    s.append(f"{IND}T[25] = (uint32_t)accA + (uint32_t)accB;")
    s.append("}")
    return "\n".join(s) + "\n"


HEADER = """// GENERATED by tools/gen_fq30_pair.py -- edit the generator, not this file.
//
// Device bodies of the paired Fq30 products (fq30.hpp: fq30_mul_pair, fq30_sqr_pair, fq30_mul2_add).  One inline-asm
// statement per column holds the mads of both chains, alternating, each chain accumulating in place from its shifted
// carry; the Montgomery digit, the carry shift and the capture word are C++ between the statements.  Included by
// fq30.hpp inside namespace ty, in the device pass only.
#pragma once

// m_k of both chains, then m_k * p_0 (captured into the third word in columns 10..12: fq30_fused_cap_last)
#define FQ30_PAIR_DIGIT(k)                                              \\
    do {                                                                \\
        mA[k] = ((uint32_t)accA * FQ30_NINV) & FQ30_MASK;               \\
        mB[k] = ((uint32_t)accB * FQ30_NINV) & FQ30_MASK;               \\
        if (fq30_fused_cap_last(k)) {                                   \\
            FQ30_MAC_CC_VS(accA, hiA, mA[k], fq30_kp(1, 0));            \\
            FQ30_MAC_CC_VS(accB, hiB, mB[k], fq30_kp(1, 0));            \\
        } else {                                                        \\
            accA += (uint64_t)mA[k] * fq30_kp(1, 0);                    \\
            accB += (uint64_t)mB[k] * fq30_kp(1, 0);                    \\
        }                                                               \\
    } while (0)
// the carry into the next column, with the third word of a wide column (fq30_fused_wide_col)
#define FQ30_PAIR_SHIFT(wide)                                           \\
    do {                                                                \\
        accA >>= 30;                                                    \\
        accB >>= 30;                                                    \\
        if (wide) {                                                     \\
            accA |= (uint64_t)hiA << 34;                                \\
            accB |= (uint64_t)hiB << 34;                                \\
        }                                                               \\
    } while (0)

"""

FOOTER = """
#undef FQ30_PAIR_DIGIT
#undef FQ30_PAIR_SHIFT
"""


def main():
    with open(OUT, "w") as f:
        f.write(HEADER + reduced_pair(False) + "\n" + reduced_pair(True) + "\n" + wide_pair() + FOOTER)
    print(OUT)


if __name__ == "__main__":
    main()
