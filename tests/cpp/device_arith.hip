// Test-only device harness over the shipped arithmetic headers (tests/test_gpu_arith.py).
//
// The headers are included exactly as the library's units include them, with no extra defines, so what runs here is the
// device code the kernels run (the fused fq30_mul / fq30_sqr, the merged g1_y3, divsteps inversion, the inline-asm Fr carry
// chains).  Every entry point takes host arrays in the RAW internal form of its family -- 8 x u32 for Fr (arkworks
// Montgomery words), 9 x 30-bit limbs for Fr30, 13 x 30-bit limbs for Fq30, 4 x 13 for an XYZZ point, 3 x 13 for a
// Jacobian one, 2 x 13 for an affine one -- runs one thread per case in 64-thread blocks, and returns the HIP error code.
// da_wave runs the cross-lane additions of msm_common.hpp (butterfly_add, butterfly_add4, butterfly_reduce) on whole
// wavefronts of chosen points, one wavefront per block, and returns EVERY lane's result.
// Tests build operands at the exact limits of each function's contract and check results against Python integers.
// Not linked into libtyplonk_hip.so.
#include "../../typlonk_amd/csrc/g1.hpp"
#include "../../typlonk_amd/csrc/fr30.hpp"
#include "../../typlonk_amd/csrc/fr_inv.hpp"
#include "../../typlonk_amd/csrc/msm_common.hpp"

using namespace ty;

namespace {

constexpr int FR_W = 8, FQ_W = 13, FR30_W = 9, G1_W = 52;

// ---- Fr (ff.hpp, N = 8) ----------------------------------------------------------------------------------------------
enum { FR_ADD, FR_SUB, FR_NEG, FR_MUL, FR_SQR, FR_REDUCE_ONCE, FR_FROM_MONT, FR_INV_DIVSTEPS };

__device__ Fr ld_fr(const uint32_t* p) {
    Fr r;
    for (int i = 0; i < FR_W; ++i) r.v[i] = p[i];
    return r;
}

__global__ __launch_bounds__(64) void fr_kernel(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int32_t* aux, int n) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n) return;
    const Fr x = ld_fr(a + (size_t)t * FR_W), y = ld_fr(b + (size_t)t * FR_W);
    Fr r = Fr::zero();
    int32_t k = 0;
    switch (op) {
        case FR_ADD: r = fe_add(x, y); break;
        case FR_SUB: r = fe_sub(x, y); break;
        case FR_NEG: r = fe_neg(x); break;
        case FR_MUL: r = fe_mul(x, y); break;
        case FR_SQR: r = fe_sqr(x); break;
        case FR_REDUCE_ONCE: r = x; fe_reduce_once(r); break;
        case FR_FROM_MONT: r = fe_from_mont(x); break;
        case FR_INV_DIVSTEPS: { int rounds = 0; r = fr_inv_divsteps(x, &rounds); k = rounds; break; }
        default: k = -1;
    }
    for (int i = 0; i < FR_W; ++i) out[(size_t)t * FR_W + i] = r.v[i];
    aux[t] = k;
}

// ---- Fq30 (fq30.hpp) -------------------------------------------------------------------------------------------------
enum {
    FQ_MUL, FQ_SQR, FQ_MUL2_ADD, FQ_ADD_LAZY, FQ_MULK2, FQ_MULK3, FQ_SUB2, FQ_SUB3, FQ_SUB4, FQ_SUB5, FQ_SUB6, FQ_SUB2_4, FQ_NEG1,
    FQ_NEG4, FQ_CSUB1, FQ_CSUB2, FQ_CSUB4, FQ_CANON, FQ_IS_ZERO_MOD, FQ_IS_ZERO_EXACT, FQ_PACK, FQ_UNPACK, FQ_FROM_ARK, FQ_TO_ARK,
    FQ_INV, FQ_INV_DIVSTEPS, FQ_INV_FERMAT
};

__device__ Fq30 ld_fq30(const uint32_t* p) {
    Fq30 r;
    for (int i = 0; i < FQ_W; ++i) r.v[i] = p[i];
    return r;
}
__device__ void st_fq30(uint32_t* p, const Fq30& x) {
    for (int i = 0; i < FQ_W; ++i) p[i] = x.v[i];
}

__global__ __launch_bounds__(64) void fq30_kernel(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d,
                                                  uint32_t* out, int32_t* aux, int n) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n) return;
    const size_t o = (size_t)t * FQ_W;
    const Fq30 x = ld_fq30(a + o), y = ld_fq30(b + o), z = ld_fq30(c + o), w = ld_fq30(d + o);
    Fq30 r = fq30_zero();
    int32_t k = 0;
    uint32_t words[12];
    switch (op) {
        case FQ_MUL: r = fq30_mul(x, y); break;
        case FQ_SQR: r = fq30_sqr(x); break;
        case FQ_MUL2_ADD: r = fq30_mul2_add(x, y, z, w); break;
        case FQ_ADD_LAZY: r = fq30_add_lazy(x, y); break;
        case FQ_MULK2: r = fq30_mulk_lazy<2>(x); break;
        case FQ_MULK3: r = fq30_mulk_lazy<3>(x); break;
        case FQ_SUB2: r = fq30_sub_lazy<2>(x, y); break;
        case FQ_SUB3: r = fq30_sub_lazy<3>(x, y); break;
        case FQ_SUB4: r = fq30_sub_lazy<4>(x, y); break;
        case FQ_SUB5: r = fq30_sub_lazy<5>(x, y); break;
        case FQ_SUB6: r = fq30_sub_lazy<6>(x, y); break;
        case FQ_SUB2_4: r = fq30_sub2_lazy<4>(x, y, z); break;
        case FQ_NEG1: r = fq30_neg_lazy<1>(x); break;
        case FQ_NEG4: r = fq30_neg_lazy<4>(x); break;
        case FQ_CSUB1: r = x; fq30_cond_sub<1>(r); break;
        case FQ_CSUB2: r = x; fq30_cond_sub<2>(r); break;
        case FQ_CSUB4: r = x; fq30_cond_sub<4>(r); break;
        case FQ_CANON: r = fq30_canon(x); break;
        case FQ_IS_ZERO_MOD: k = fq30_is_zero_mod(x) ? 1 : 0; break;
        case FQ_IS_ZERO_EXACT: k = fq30_is_zero_exact(x) ? 1 : 0; break;
        case FQ_PACK:
            fq30_pack(x, words);
            for (int i = 0; i < 12; ++i) r.v[i] = words[i];
            break;
        case FQ_UNPACK:
        case FQ_FROM_ARK:
            for (int i = 0; i < 12; ++i) words[i] = x.v[i];
            r = op == FQ_UNPACK ? fq30_unpack(words) : fq30_from_ark(words);
            break;
        case FQ_TO_ARK:
            fq30_to_ark(x, words);
            for (int i = 0; i < 12; ++i) r.v[i] = words[i];
            break;
        case FQ_INV: r = fq30_inv(x); break;
        case FQ_INV_DIVSTEPS: { int rounds = 0; r = fq30_inv_divsteps(x, &rounds); k = rounds; break; }
        case FQ_INV_FERMAT: r = fq30_inv_fermat(x); break;
        default: k = -1;
    }
    st_fq30(out + o, r);
    aux[t] = k;
}

// ---- Fr30 (fr30.hpp) -------------------------------------------------------------------------------------------------
enum { FR30_MUL, FR30_UNPACK, FR30_PACK, FR30_NORM, FR30_ADD, FR30_SUB, FR30_TO_CANONICAL, FR30_SUB_QR, FR30_REDUCE_LAZY, FR30_CONST_ONE };

__global__ __launch_bounds__(64) void fr30_kernel(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int32_t* aux, int n) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n) return;
    const size_t o = (size_t)t * FR30_W;
    Fr30 x, y, r;
    for (int i = 0; i < FR30_W; ++i) {
        x.v[i] = a[o + i];
        y.v[i] = b[o + i];
        r.v[i] = 0;
    }
    int32_t k = 0;
    Fr f;
    switch (op) {
        case FR30_MUL: r = fr30_mul(x, y); break;
        case FR30_UNPACK:
            for (int i = 0; i < 8; ++i) f.v[i] = x.v[i];
            r = fr30_unpack(f);
            break;
        case FR30_PACK:
        case FR30_TO_CANONICAL:
            f = op == FR30_PACK ? fr30_pack(x) : fr30_to_canonical(x);
            for (int i = 0; i < 8; ++i) r.v[i] = f.v[i];
            break;
        case FR30_NORM: r = fr30_norm(x); break;
        case FR30_ADD: r = fr30_add(x, y); break;
        case FR30_SUB: r = fr30_sub(x, y); break;
        case FR30_SUB_QR: r = fr30_sub_qr(x, y.v[0]); break;
        case FR30_REDUCE_LAZY: r = fr30_reduce_lazy(x); break;
        case FR30_CONST_ONE: r = fr30_const_one(); break;
        default: k = -1;
    }
    for (int i = 0; i < FR30_W; ++i) out[o + i] = r.v[i];
    aux[t] = k;
}

// ---- G1 (g1.hpp) -----------------------------------------------------------------------------------------------------
// a, b: 52 words each (XYZZ: x, y, zz, zzz; Jacobian: x, y, z; affine: x, y -- leading coordinates); flag: one word
enum { G1_MADD, G1_MADD_XY, G1_ADD, G1_DBL, G1_DBL_AFFINE, G1_TO_AFFINE, G1_JAC_DBL, G1_JAC_TO_XYZZ, G1_JAC_TO_AFFINE_WITH, G1_MUL_SMALL };

__device__ G1Xyzz ld_xyzz(const uint32_t* p) {
    G1Xyzz r;
    r.x = ld_fq30(p);
    r.y = ld_fq30(p + 13);
    r.zz = ld_fq30(p + 26);
    r.zzz = ld_fq30(p + 39);
    return r;
}
__device__ void st_xyzz(uint32_t* p, const G1Xyzz& r) {
    st_fq30(p, r.x);
    st_fq30(p + 13, r.y);
    st_fq30(p + 26, r.zz);
    st_fq30(p + 39, r.zzz);
}

__global__ __launch_bounds__(64) void g1_kernel(int op, const uint32_t* a, const uint32_t* b, const uint32_t* flag, uint32_t* out, int32_t* aux,
                                                int n) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n) return;
    const uint32_t* pa = a + (size_t)t * G1_W;
    const uint32_t* pb = b + (size_t)t * G1_W;
    uint32_t* po = out + (size_t)t * G1_W;
    for (int i = 0; i < G1_W; ++i) po[i] = 0;
    G1Xyzz acc = ld_xyzz(pa);
    G1Affine q;
    q.x = ld_fq30(pb);
    q.y = ld_fq30(pb + 13);
    G1Jac j;
    j.x = acc.x;
    j.y = acc.y;
    j.z = acc.zz;
    int32_t k = 0;
    switch (op) {
        case G1_MADD: g1_madd(acc, q, flag[t] != 0); st_xyzz(po, acc); break;
        case G1_MADD_XY: g1_madd_xy(acc, q.x, q.y); st_xyzz(po, acc); break;
        case G1_ADD: st_xyzz(po, g1_add(acc, ld_xyzz(pb))); break;
        case G1_DBL: st_xyzz(po, g1_dbl(acc)); break;
        case G1_DBL_AFFINE: st_xyzz(po, g1_dbl_affine(q.x, q.y)); break;
        case G1_TO_AFFINE: {
            const G1Affine r = g1_to_affine(acc);
            st_fq30(po, r.x);
            st_fq30(po + 13, r.y);
            break;
        }
        case G1_JAC_DBL: {
            const G1Jac r = g1_jac_dbl(j);
            st_fq30(po, r.x);
            st_fq30(po + 13, r.y);
            st_fq30(po + 26, r.z);
            break;
        }
        case G1_JAC_TO_XYZZ: st_xyzz(po, g1_jac_to_xyzz(j)); break;
        case G1_JAC_TO_AFFINE_WITH: {
            const G1Affine r = g1_jac_to_affine_with(j, q.x);
            st_fq30(po, r.x);
            st_fq30(po + 13, r.y);
            break;
        }
        case G1_MUL_SMALL: st_xyzz(po, g1_mul_small(acc, flag[t])); break;
        default: k = -1;
    }
    aux[t] = k;
}

// ---- wavefront butterflies (msm_common.hpp) ------------------------------------------------------------------------------
// Lane t of a wavefront loads point t of `in` as raw limbs (no ld_xyzz: lazily reduced operands stay as given) and stores
// its own result, so that the caller sees what every lane holds after the step, not only the lane a kernel would store.
enum { WAVE_ADD, WAVE_ADD4, WAVE_REDUCE };

__global__ __launch_bounds__(64) void wave_kernel(int op, int param, const uint32_t* in, uint32_t* out, int32_t* aux) {
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    G1Xyzz v = ld_xyzz(in + t * G1_W);
    int32_t k = 0;
    switch (op) {   // op and param are kernel arguments: the whole wavefront takes the same branch
        case WAVE_ADD: v = butterfly_add(v, param); break;
        case WAVE_ADD4: v = butterfly_add4(v, param); break;
        case WAVE_REDUCE: v = butterfly_reduce(v, (uint32_t)param); break;
        default: k = -1;
    }
    st_xyzz(out + t * G1_W, v);
    aux[t] = k;
}

// ---- host side: allocate, copy, launch, synchronise, copy back, free ---------------------------------------------------
struct DevBufs {
    void* p[8] = {};
    int used = 0;
    hipError_t err = hipSuccess;
    template <class T>
    T* in(const T* host, size_t count) {
        void* d = nullptr;
        if (err == hipSuccess) err = hipMalloc(&d, count * sizeof(T));
        if (err == hipSuccess) p[used++] = d;
        if (err == hipSuccess) err = hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice);
        return static_cast<T*>(d);
    }
    template <class T>
    T* zeros(size_t count) {
        void* d = nullptr;
        if (err == hipSuccess) err = hipMalloc(&d, count * sizeof(T));
        if (err == hipSuccess) p[used++] = d;
        if (err == hipSuccess) err = hipMemset(d, 0, count * sizeof(T));
        return static_cast<T*>(d);
    }
    template <class T>
    void out(T* host, const T* dev, size_t count) {
        if (err == hipSuccess) err = hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost);
    }
    void launched() {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    ~DevBufs() {
        for (int i = 0; i < used; ++i) (void)hipFree(p[i]);
    }
};

dim3 grid_of(int n) { return dim3((unsigned)((n + 63) / 64)); }

}  // namespace

// Every entry point: n cases; arrays of n * width words (width per family, above); aux: n ints (inversion round counts,
// predicate results; -1 for an unknown op).  Returns the HIP error code (0 on success).
extern "C" int da_fr(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int32_t* aux, int n) {
    if (n <= 0) return 0;
    DevBufs m;
    const size_t w = (size_t)n * FR_W;
    const uint32_t *da = m.in(a, w), *db = m.in(b, w);
    uint32_t* dout = m.zeros<uint32_t>(w);
    int32_t* daux = m.zeros<int32_t>(n);
    if (m.err == hipSuccess) hipLaunchKernelGGL(fr_kernel, grid_of(n), dim3(64), 0, 0, op, da, db, dout, daux, n);
    m.launched();
    m.out(out, dout, w);
    m.out(aux, daux, n);
    return (int)m.err;
}

extern "C" int da_fq30(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, int32_t* aux, int n) {
    if (n <= 0) return 0;
    DevBufs m;
    const size_t w = (size_t)n * FQ_W;
    const uint32_t *da = m.in(a, w), *db = m.in(b, w), *dc = m.in(c, w), *dd = m.in(d, w);
    uint32_t* dout = m.zeros<uint32_t>(w);
    int32_t* daux = m.zeros<int32_t>(n);
    if (m.err == hipSuccess) hipLaunchKernelGGL(fq30_kernel, grid_of(n), dim3(64), 0, 0, op, da, db, dc, dd, dout, daux, n);
    m.launched();
    m.out(out, dout, w);
    m.out(aux, daux, n);
    return (int)m.err;
}

extern "C" int da_fr30(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int32_t* aux, int n) {
    if (n <= 0) return 0;
    DevBufs m;
    const size_t w = (size_t)n * FR30_W;
    const uint32_t *da = m.in(a, w), *db = m.in(b, w);
    uint32_t* dout = m.zeros<uint32_t>(w);
    int32_t* daux = m.zeros<int32_t>(n);
    if (m.err == hipSuccess) hipLaunchKernelGGL(fr30_kernel, grid_of(n), dim3(64), 0, 0, op, da, db, dout, daux, n);
    m.launched();
    m.out(out, dout, w);
    m.out(aux, daux, n);
    return (int)m.err;
}

extern "C" int da_g1(int op, const uint32_t* a, const uint32_t* b, const uint32_t* flag, uint32_t* out, int32_t* aux, int n) {
    if (n <= 0) return 0;
    DevBufs m;
    const size_t w = (size_t)n * G1_W;
    const uint32_t *da = m.in(a, w), *db = m.in(b, w), *df = m.in(flag, (size_t)n);
    uint32_t* dout = m.zeros<uint32_t>(w);
    int32_t* daux = m.zeros<int32_t>(n);
    if (m.err == hipSuccess) hipLaunchKernelGGL(g1_kernel, grid_of(n), dim3(64), 0, 0, op, da, db, df, dout, daux, n);
    m.launched();
    m.out(out, dout, w);
    m.out(aux, daux, n);
    return (int)m.err;
}

// One wavefront per block over n = 64 * waves points of 52 words.  op 0: butterfly_add(v, param), param = the lane mask 1..32;
// op 1: butterfly_add4(v, param), mask 2..32 (the caller keeps lanes l and l ^ 1 identical); op 2: butterfly_reduce(v, param),
// param = lanes 1..64.  A param outside those (or not a power of two), or n not a multiple of 64: hipErrorInvalidValue.
extern "C" int da_wave(int op, int param, const uint32_t* in, uint32_t* out, int32_t* aux, int n) {
    if (n <= 0) return 0;
    const int lo = op == WAVE_ADD4 ? 2 : 1, hi = op == WAVE_REDUCE ? 64 : 32;
    if (n % 64 != 0 || param < lo || param > hi || (param & (param - 1)) != 0) return (int)hipErrorInvalidValue;
    DevBufs m;
    const size_t w = (size_t)n * G1_W;
    const uint32_t* din = m.in(in, w);
    uint32_t* dout = m.zeros<uint32_t>(w);
    int32_t* daux = m.zeros<int32_t>(n);
    if (m.err == hipSuccess) hipLaunchKernelGGL(wave_kernel, dim3((unsigned)(n / 64)), dim3(64), 0, 0, op, param, din, dout, daux);
    m.launched();
    m.out(out, dout, w);
    m.out(aux, daux, n);
    return (int)m.err;
}
