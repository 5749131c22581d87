// Host build of csrc/fq30_rows.hpp over RowsHost, the array-of-64 wave: a program of its own (no HIP include) that runs the
// commands it reads, one per line, and prints one line per command (tests/test_fq30_rows_host.py).  Numbers are hex.
//   mul  a[13] b[13]            -> 13 limbs of fqr_mul
//   add  a[13] b[13]            -> fqr_add_lazy
//   mulk K a[13]                -> fqr_mulk_lazy<K>, K = 2, 3
//   sub  K a[13] b[13]          -> fqr_sub_lazy<K>, K = 2, 4, 6
//   sub2 K a[13] b[13] c[13]    -> fqr_sub2_lazy<K>, K = 4
//   sel  c a[13] b[13]          -> fqr_select
//   zero a[13]                  -> fqr_is_zero_mod, fqr_maybe_zero_mod on lane 0 (two numbers)
//   load w[12]                  -> 13 limbs of fqr_load, then the 13 of fq30_unpack
//   store a[13]                 -> 12 words of fqr_store_rows, then the 12 of fq30_pack of the same digits
//   gadd A[52] B[52]            -> 52 limbs of g1_add_rows (X, Y, ZZ, ZZZ), then 1 if the slow path ran
// The operands of the field commands go to all four rows; a line ends with " !" if the rows disagree, if a lane above 12
// is not zero, or if a 64-bit accumulator wrapped (RowsHost::overflow).  Exit code 2: a line that does not parse.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../typlonk_amd/csrc/fq30_rows.hpp"

using namespace ty;
using W = RowsHost;

static bool read_hex(std::istringstream& in, uint32_t* out, int n) {
    for (int i = 0; i < n; ++i) {
        std::string tok;
        if (!(in >> tok)) return false;
        char* end = nullptr;
        const unsigned long long v = strtoull(tok.c_str(), &end, 16);
        if (*end != 0 || v > 0xffffffffull) return false;
        out[i] = (uint32_t)v;
    }
    return true;
}
static W::U32 rows_of(const uint32_t* l13) {
    W::U32 r;
    for (int i = 0; i < 64; ++i) r.l[i] = (i & 15) < 13 ? l13[i & 15] : 0u;
    return r;
}
static bool bad = false;
static void print_rows(const W::U32& r, int n = 13) {
    for (int i = 0; i < n; ++i) printf("%s%x", i ? " " : "", r.l[i]);
    for (int i = 0; i < 64; ++i) {
        if (r.l[i] != r.l[i & 15]) bad = true;
        if ((i & 15) >= n && r.l[i] != 0) bad = true;
    }
}
static void end_line() {
    if (bad || W::overflow()) printf(" !");
    printf("\n");
    bad = false;
    W::overflow() = false;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        uint32_t a[64], b[64], c[13], k = 0;
        if (cmd == "mul" || cmd == "add") {
            if (!read_hex(in, a, 13) || !read_hex(in, b, 13)) return 2;
            print_rows(cmd == "mul" ? fqr_mul<W>(rows_of(a), rows_of(b)) : fqr_add_lazy<W>(rows_of(a), rows_of(b)));
        } else if (cmd == "mulk") {
            if (!read_hex(in, &k, 1) || !read_hex(in, a, 13) || (k != 2 && k != 3)) return 2;
            print_rows(k == 2 ? fqr_mulk_lazy<W, 2>(rows_of(a)) : fqr_mulk_lazy<W, 3>(rows_of(a)));
        } else if (cmd == "sub") {
            if (!read_hex(in, &k, 1) || !read_hex(in, a, 13) || !read_hex(in, b, 13) || (k != 2 && k != 4 && k != 6)) return 2;
            print_rows(k == 2   ? fqr_sub_lazy<W, 2>(rows_of(a), rows_of(b))
                       : k == 4 ? fqr_sub_lazy<W, 4>(rows_of(a), rows_of(b))
                                : fqr_sub_lazy<W, 6>(rows_of(a), rows_of(b)));
        } else if (cmd == "sub2") {
            if (!read_hex(in, &k, 1) || !read_hex(in, a, 13) || !read_hex(in, b, 13) || !read_hex(in, c, 13) || k != 4) return 2;
            print_rows(fqr_sub2_lazy<W, 4>(rows_of(a), rows_of(b), rows_of(c)));
        } else if (cmd == "sel") {
            if (!read_hex(in, &k, 1) || !read_hex(in, a, 13) || !read_hex(in, b, 13)) return 2;
            W::Mask m;
            for (int i = 0; i < 64; ++i) m.l[i] = k != 0;
            print_rows(fqr_select<W>(m, rows_of(a), rows_of(b)));
        } else if (cmd == "zero") {
            if (!read_hex(in, a, 13)) return 2;
            const W::Mask z = fqr_is_zero_mod<W>(rows_of(a)), mz = fqr_maybe_zero_mod<W>(rows_of(a));
            for (int i = 0; i < 64; ++i)
                if (z.l[i] != z.l[0]) bad = true;
            printf("%d %d", (int)z.l[0], (int)mz.l[0]);
        } else if (cmd == "load") {
            uint32_t w[12];
            if (!read_hex(in, w, 12)) return 2;
            print_rows(fqr_load<W>(w));
            const Fq30 u = fq30_unpack(w);
            for (int i = 0; i < 13; ++i) {
                printf(" %x", u.v[i]);
                if (fqr_limb_of_words(w, (uint32_t)i) != u.v[i]) bad = true;
            }
        } else if (cmd == "store") {
            if (!read_hex(in, a, 13)) return 2;
            uint32_t w[48], v[12];
            memset(w, 0, sizeof w);
            fqr_store_rows<W>(w, rows_of(a));
            for (int j = 0; j < 12; ++j) printf("%s%x", j ? " " : "", w[j]);
            for (int j = 12; j < 48; ++j)
                if (w[j] != w[j % 12]) bad = true;
            fq30_pack(fqr_to_fq30(a), v);
            for (int j = 0; j < 12; ++j) printf(" %x", v[j]);
        } else if (cmd == "gadd") {
            uint32_t la[52], lb[52], out[64];
            if (!read_hex(in, la, 52) || !read_hex(in, lb, 52)) return 2;
            memset(a, 0, sizeof a);
            memset(b, 0, sizeof b);
            for (int cc = 0; cc < 4; ++cc)
                for (int i = 0; i < 13; ++i) {
                    a[cc * 16 + i] = la[cc * 13 + i];
                    b[cc * 16 + i] = lb[cc * 13 + i];
                }
            for (int i = 0; i < 64; ++i) out[i] = 0xdeadbeefu;
            const bool slow = g1_add_rows<W>(a, b, out);
            for (int cc = 0; cc < 4; ++cc)
                for (int i = 0; i < 16; ++i) {
                    if (i < 13) printf("%s%x", cc + i ? " " : "", out[cc * 16 + i]);
                    else if (out[cc * 16 + i] != 0) bad = true;
                }
            printf(" %d", (int)slow);
        } else {
            return 2;
        }
        std::string rest;
        if (in >> rest) return 2;
        end_line();
    }
    return 0;
}
