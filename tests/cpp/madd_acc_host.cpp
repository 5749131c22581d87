// g1_madd_acc / g1_acc_finish (csrc/g1.hpp), the mixed addition of the MSM's accumulation loops, as the host compiles
// them, without any HIP header (tests/test_madd_acc_host.py).  Reads cases from stdin or from the file named by the first
// argument.  A case is
//   <stored> [X Y ZZ ZZZ] <n>  then n times  <x> <y> <neg>
// stored = 1 starts from the given XYZZ point (a later chunk's ld_xyzz), 0 from the empty accumulator; field values are
// hexadecimal integers below 2^390 in the Montgomery form the kernels hold (value * 2^390 mod p, lazily reduced where the
// invariants allow); (0, 0) is the identity of an SRS.  Prints one line per case: the flags word after every addition,
// then the 4 x 13 limbs of g1_acc_finish, all in hexadecimal.
#include <cstdio>
#include <cstring>

#include "../../typlonk_amd/csrc/g1.hpp"

using namespace ty;

// hexadecimal integer -> 13 limbs of 30 bits; false when it does not fit 390 bits or is no hexadecimal number
static bool parse_fq(const char* s, Fq30& r) {
    r = fq30_zero();
    const size_t n = strlen(s);
    if (n == 0 || n > 98) return false;
    for (size_t k = 0; k < n; ++k) {
        const char ch = s[n - 1 - k];
        uint32_t d;
        if (ch >= '0' && ch <= '9') d = (uint32_t)(ch - '0');
        else if (ch >= 'a' && ch <= 'f') d = (uint32_t)(ch - 'a') + 10u;
        else return false;
        for (int b = 0; b < 4; ++b) {
            const size_t bit = 4 * k + (size_t)b;
            if (!((d >> b) & 1u)) continue;
            if (bit >= 390) return false;
            r.v[bit / 30] |= 1u << (bit % 30);
        }
    }
    return true;
}

static bool read_fq(FILE* in, Fq30& r) {
    char buf[128];
    return fscanf(in, "%127s", buf) == 1 && parse_fq(buf, r);
}

static void print_fq(const Fq30& a) {
    for (int i = 0; i < 13; ++i) printf(" %x", a.v[i]);
}

int main(int argc, char** argv) {
    FILE* in = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!in) return 2;
    for (;;) {
        int stored;
        if (fscanf(in, "%d", &stored) != 1) return 0;
        G1Acc acc = g1_acc_empty();
        if (stored) {
            G1Xyzz p;
            if (!read_fq(in, p.x) || !read_fq(in, p.y) || !read_fq(in, p.zz) || !read_fq(in, p.zzz)) return 2;
            acc = g1_acc_from(p);
        }
        int n;
        if (fscanf(in, "%d", &n) != 1 || n < 0) return 2;   // a case cut short is an error
        printf("%x", acc.flags);
        for (int i = 0; i < n; ++i) {
            G1Affine q;
            int neg;
            if (!read_fq(in, q.x) || !read_fq(in, q.y) || fscanf(in, "%d", &neg) != 1) return 2;
            g1_madd_acc(acc, q, neg != 0);
            printf(" %x", acc.flags);
        }
        const G1Xyzz r = g1_acc_finish(acc);
        printf(" |");
        print_fq(r.x);
        print_fq(r.y);
        print_fq(r.zz);
        print_fq(r.zzz);
        printf("\n");
    }
}
