// knn_filter_dev.h — what knn_filter.hip and knn_cells.hip share (gfx950 only): fragment vector types, the
// monotone-atomic helpers, the error-bound constants and the per-query threshold, small host macros.
#pragma once

#include "knn_common.h"

#include <math.h>
#include <string.h>

// Device buffers of an index come from the library's pool (knn_api.cpp): a one-shot cudaCallback that
// builds the filter layouts makes ~20 allocations, and hipMalloc + hipFree (a device-wide sync and
// ~0.2 ms each) cost more than its kernels.  Stand-alone tools that include this file define KNN_NO_POOL.
#ifdef KNN_NO_POOL
#define KNN_DEV_ALLOC(p, bytes) hipMalloc(p, bytes)
#define KNN_DEV_FREE(p) hipFree(p)
#else
#define KNN_DEV_ALLOC(p, bytes) knn_dev_alloc((void **)(p), bytes)
#define KNN_DEV_FREE(p) knn_dev_free((void *)(p))
#endif

#include <math.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <vector>

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f4v __attribute__((ext_vector_type(4)));

#define FILTER_BLOCK 256

// order-preserving map float -> uint (for atomic min/max over signed floats)
__device__ __forceinline__ unsigned f2ord(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned o)
{
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
static inline float ord2f_host(unsigned o)
{
    const unsigned u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// Monotone accumulators on a few hot words: a plain (possibly stale) read first.  The target only
// moves one way, so a stale value can cost a spare atomic, never lose an update; without the
// guard half a million atomics on one word serialise at ~88/us (6 ms on a 2^24-row shard).
__device__ __forceinline__ void guarded_atomic_max(unsigned *p, unsigned v)
{
    if (v > __builtin_nontemporal_load(p))
        atomicMax(p, v);
}
__device__ __forceinline__ void guarded_atomic_min(unsigned *p, unsigned v)
{
    if (v < __builtin_nontemporal_load(p))
        atomicMin(p, v);
}

__device__ __forceinline__ float wave_max_f(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = fmaxf(v, __shfl_xor(v, off, KNN_WAVE));
    return v;
}


// ------------------------------------------------------------------------------------------
// Per-query pruning threshold (double arithmetic; see the header comment for the derivation).
// ------------------------------------------------------------------------------------------
struct BoundConsts {
    double eta, eta2, rho, g2, tau, gam, sigma2;
};

__host__ __device__ inline BoundConsts knn_bound_consts(int k, int kt, double sigma, double amax,
                                                        double bmax, double nmax)
{
    const double u = 0x1p-24;
    const double theta = 0x1p-11 + 0x1p-23;          // fp32 centring + fp16 rounding, relative
    const double thp = theta / (1.0 - theta);
    const double nu0 = 0x1p-14 * 1.001;               // fp16 subnormal rounding or flush-to-zero
    const double kp = 16.0 * kt;
    const double emax = thp * (amax + bmax) + 2.0 * nu0;
    BoundConsts c;
    c.eta2 = k * emax * emax;
    c.eta = sqrt(c.eta2);
    // MFMA internal accumulation of one score, relative to the sum of the magnitudes it adds (norm + k products), per chained
    // K-step.  The matrix core's adder tree is not documented, so kt 2^-18 is an allowance, not a derivation; it is pinned by
    // MEASURED WORST CASES on gfx950 (tests/test_parity_gpu.py::test_mfma_accumulation_error_on_adversarial_operands, round 5:
    // operands exactly representable in fp16, float64 reference exact): one product per K-step 2^10 times the others
    // 2^-22.6 (kt 1) .. 2^-20.0 (kt 256); fp16-subnormal operands 2^-21.9 (kt 1: they are NOT flushed); magnitudes 2^0..2^-12
    // mixed 2^-22.9 (kt 1) .. 2^-19.9 (kt 256); alternating +P, -P products: exact; gaussian data <= 2^-20 (kt <= 64).
    // The worst of all, 2^-19.9 at k = 4096, is 2^9.9 inside its allowance (2^-10); at kt = 1 the margin is 2^3.9.
    const double omega = kt * 0x1p-18;
    c.gam = (kp + 2.0) * u;
    const double mmax = kp * amax * amax;
    c.rho = (omega + 2.0 * c.gam) * 2.0 * (nmax + mmax) + kp * 0x1p-27;
    // the cell-pruned scan takes the C operand from norms kept as two fp16 halves (knn_cells.hip): off by at most
    // 2^-22 N, or 2^-25 where the low half is flushed; twice that is allowed for (always: it is a 2^-4 of omega's share)
    c.rho += 0x1p-21 * nmax + 0x1p-24;
    c.g2 = (k + 3.0) * u * 1.0001;
    c.tau = k * 0x1p-125;
    c.sigma2 = sigma * sigma;
    return c;
}

// 8-bit rows in a cell's frame (option `cells_rows`, knn_cells_recentre_kernel): one rounding of the fp32 value v of a coordinate
// in the cell's frame to a multiple of 2^-7 in [-1, 127/128] — rh, exact in fp16 and fp32 — and its byte, 128 + 128 rh.
// err = |v - rh| + 2^-22 |v| + 2^-100 (each term exact, the sums rounded once each) bounds, taken 10^-6 larger, the coordinate's
// distance from the row's exact value in the frame, v_exact: the centring made v with |v - v_exact| <= 2^-24 |v_exact| (fp32
// subtract, exact power-of-two scale) — or, where the product falls below fp32's normal range (or is flushed), within 2^-126.  Inside the cell's box (|v| <= 1) err <= 2^-8 + 2^-22; the clamp at 127/128 makes it at most 2^-7 + 2^-22.
__host__ __device__ inline unsigned knn_u8_code(float v, float &rh, float &err)
{
#pragma clang fp contract(off)
    const float q = fminf(fmaxf(rintf(v * 128.0f), -128.0f), 127.0f);   // (v * 128: exact)
    rh = q * 0.0078125f;
    err = fabsf(v - rh) + 0x1p-22f * fabsf(v) + 0x1p-100f;
    return (unsigned)((int)q + 128);
}

// knn_bound_consts for 8-bit rows: the row's part of the per-coordinate error is ABSOLUTE — er, the cell's largest knn_u8_code
// err (10^-6 added) — instead of the fp16 rounding thp bmax; the query's fp16 rounding thp amax, the subnormal allowance 2 nu0
// and every other constant (omega, gamma, rho, g2, tau) are knn_bound_consts' own:
//     emax = thp amax + er + 2 nu0,  eta = sqrt(k) emax
// (a coordinate of (q~ - r^) - (q - r) is off by at most the query's rounding plus the row's quantisation).  nmax is the
// largest norm of the DEQUANTISED rows, |r^|^2, which is what the C operand holds — exactly (knn_cells_recentre_kernel).
__host__ __device__ inline BoundConsts knn_bound_consts_u8(int k, int kt, double sigma, double amax, double er, double nmax)
{
    BoundConsts c = knn_bound_consts(k, kt, sigma, amax, 0.0, nmax);
    const double theta = 0x1p-11 + 0x1p-23;
    const double emax = theta / (1.0 - theta) * amax + er * (1.0 + 1e-6) + 2.0 * (0x1p-14 * 1.001);
    c.eta2 = k * emax * emax;
    c.eta = sqrt(c.eta2);
    return c;
}

// 8-bit rows in per-dimension BIN frames (option `cells_u8_frame`, knn_cells_bin_rows_kernel).  One shard-wide scale s = sigma 2^e
// (power of two, the shard's fp16 frame times 2^e, e <= 4), and per (dimension d, bin b) an offset w[d][b], a multiple of 2^-6
// below 32 in s units — exact in fp16.  A row x of cell c (bin b_d of every dimension) is stored as the code of
//     u = fl(x_d - centre_d) s,   v = fl(u - w_c,d),   r^ = knn_u8_code(v)      (w_c,d = w[d][b_d])
// so the row in the shard's frame at scale s is w_c + r, r its exact offset; r^ within err of r per coordinate, err = knn_u8_code's
// (|v - r^| + 2^-22 |v| + 2^-100: covers the rounding of v) + 2^-22 |u| (the fp32 centring of u, <= 2^-24 |u| (1 + 2^-24)).
// The scan scores  S = N'' + B.r^  with  N'' = |w_c + r^|^2 (double sum, rounded once to fp32: 2^-24 N'') and B = -2 p~, the
// prep kernel's fp16 B operand times 2^e (exact): p~ is the query in the shard's frame, rounded.  Then
//     S + B.w_c = |w_c + r^|^2 - 2 p~.(w_c + r^) = |p~ - (w_c + r^)|^2 - |p~|^2
// is the ONE-FRAME score of the row w_c + r^ against p~: knn_threshold's derivation holds word for word with
//     emax = thp amax + er + 2 nu0 2^e      (amax = max |p~_d| in s units — the query's rounding is relative to |p~|, made in
//                                           sigma units where nu0 is absolute; er = the shard's largest err, 10^-6 larger)
//     eta = sqrt(k) emax,  Dup (s units) = Dup_q (sigma units) 4^e,  mq = the computed |p~|^2 (exact products, fp32 sum)
//     rho: the matrix core's accumulation of S relative to |N''| + sum |B_d r^_d| <= nmax + 2 k amax (|r^_d| <= 1), and
//          nmax + 2k + 16 amax^2 >= that for k <= 16 — knn_bound_consts' (omega + 2 gamma) 2 (...) with nmax + 2k for nmax —,
//          plus 2^-21 nmax for N''s rounding and kp 2^-27 + 2^-24 as there.
// knn_u8_bin_threshold is that line, thr = Dup + 2 eta sqrt(Dup) + eta^2 + rho - mq (1 - gamma), in fp32 rounded towards "pass"
// exactly as cell_centred_operand evaluates it (P within 2^-20 of exact, taken 10^-5 larger; the square root of max(Dup, 2^-100)
// taken 10^-6 larger: a few ulp).
// The pair term B.w_c is per (query, cell): the scan computes it in fp32 (products of two fp16 numbers of <= 11 significant
// bits: exact; eight additions of magnitude <= A = sum |B_d w_c,d| <= 2 amax W1, W1 = the shard's largest sum |w_c,d|:
// <= 2^-21 A; an fp16 subnormal B flushed: <= 2^-14 W1) and passes S < thr - B.w_c.  That subtraction rounds by
// 2^-24 (|thr| + A); all of it is covered by adding  2^-18 (|thr| + 2 amax W1) + 2^-14 W1  to thr here, once per query.
__host__ __device__ inline unsigned knn_u8_bin_code(float x, float centre, float scale, float w, float &rh, float &err)
{
#pragma clang fp contract(off)
    const float u = (x - centre) * scale;   // fp32 subtract, exact power-of-two scale
    const float v = u - w;
    float e;
    const unsigned b = knn_u8_code(v, rh, e);
    err = e + 0x1p-22f * fabsf(u);
    return b;
}

// b0, b1: the query's B operand in s units (dimensions 0-7, 8-15); dup: Dup_q in sigma units (-INF: a query the batch cannot
// bound — nothing passes); ratio = 2^e; er, nmax, w1: the shard's largest err, N'' and sum |w_c,d|.
__host__ __device__ inline float knn_u8_bin_threshold(int k, const h8 &b0, const h8 &b1, float dup, float ratio, float er, float nmax, float w1)
{
#pragma clang fp contract(off)
    float a = 0.0f, mq = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const float h = (float)(j < 8 ? b0[j & 7] : b1[j & 7]) * -0.5f;   // p~_d, exact
        a = fmaxf(a, fabsf(h));
        mq = mq + h * h;
    }
    if (!(dup > -INFINITY))
        return -INFINITY;
    const float kf = (float)k;
    const float emax = 4.8865e-4f * a + er * 1.000001f + 1.2220e-4f * ratio;   // theta' amax + er + 2 nu0 2^e
    const float sqk = k <= 1 ? 1.0f : k <= 4 ? 2.0f : k <= 9 ? 3.0f : 4.0f;   // >= sqrt(k), k <= 16
    const float eta = sqk * emax, eta2 = kf * emax * emax;
    const float rho = 1.1921e-5f * (nmax + 2.0f * kf + 16.0f * a * a) + 1.79e-7f + 4.77e-7f * nmax;
    const float dupc = dup * ratio * ratio;
#ifdef __HIP_DEVICE_COMPILE__
    const float sqdc = __builtin_amdgcn_sqrtf(fmaxf(dupc, 0x1p-100f)) * 1.000001f;   // (v_sqrt_f32: 1 ulp, no FMA; a normal argument)
#else
    const float sqdc = sqrtf(fmaxf(dupc, 0x1p-100f)) * 1.000001f;
#endif
    const float P = dupc + 2.0f * eta * sqdc + eta2 + rho;
    const float th = (P * 1.00001f + (P + mq) * 2.4e-7f + 1e-30f) - mq * 0.999996f;
    return th + (0x1p-18f * (fabsf(th) + 2.0f * a * w1) + 0x1p-14f * w1);
}

// Threshold implied by a filter score `u` = S of SOME real reference j0 of the shard (the minimum
// over the sample pass), for a query whose fp16 row has computed squared norm mq:
//   D~_j0 <= u + mq(1+g) + rho;  (sqrt(D_j0) - eta)^2 <= D~_j0 + 2 eta^2  =>  D_j0 <= D0up
//   the winner j* has E_j* <= E_j0 (v0 values), hence D_j* <= D0up (1+g2)^2 + sigma^2 tau =: Dup
//   and its own score obeys S_j* <= Dup + 2 eta sqrt(Dup) + eta^2 + rho - mq(1-g).
// Monotone in u, so any upper bound of the true sample minimum is safe too.
__host__ __device__ inline float knn_threshold(const BoundConsts &c, double u, double mq, double *dup_out = nullptr)
{
    double dt = u + mq * (1.0 + 1.01 * c.gam) + c.rho;
    if (dt < 0.0)
        dt = 0.0;
    const double sq0 = c.eta + sqrt(dt + 2.0 * c.eta2);
    const double dup = sq0 * sq0 * (1.0 + c.g2) * (1.0 + c.g2) + c.sigma2 * c.tau;
    if (dup_out)
        *dup_out = dup;  // real scaled squared distance no candidate for the answer can exceed (cell pruning)
    double thr = dup + 2.0 * c.eta * sqrt(dup) + c.eta2 + c.rho - mq * (1.0 - c.gam);
    thr += fabs(thr) * 1e-6 + 1e-30;                  // slack for the double arithmetic above
    float tf = (float)thr;
    if ((double)tf < thr)
        tf = nextafterf(tf, INFINITY);
    return nextafterf(tf, INFINITY);                  // the kernel tests S < thr (strict)
}

// The same for a radius-bounded top-K (knn_index_query_topk_within) on a one-frame layout.  C = the shard's rows with v0 distance
// E <= max_dist2; wanted: the K smallest keys of C.  For a row c among them:
//   (a) E_c <= max_dist2, hence — the line the derivation above rests on, D <= sigma^2 (E (1+g2) + tau) —
//       D_c <= dup_r = sigma^2 (max_dist2 (1+g2) + tau);
//   (b) with u = u_(K) finite (K distinct seed rows j0 scoring <= u, knn_seed_kth.h): E_c <= max E_j0.  Otherwise all K seed rows
//       had E_j0 < E_c <= max_dist2: they were in C and before c in key order, so c were not among C's K smallest (nor in C at all
//       when C holds fewer than K rows).  Then D_c <= Dup(u) by knn_threshold's own argument, however many rows C holds.
// So D_c <= min(Dup(u), dup_r) in every case, and with u = +INF (no or fewer than K finite seed scores) (a) alone stands: a finite
// radius bounds the query by itself.  Under KNN_QUERY_TOPK_PARTIAL read "the global set" for "the shard" in (b).
// The score bound is knn_threshold's last line — monotone in Dup —, with the same slack and the same rounding up;
// max_dist2 = +INF gives knn_threshold's values exactly.
__host__ __device__ inline float knn_threshold_within(const BoundConsts &c, double u, double mq, double max_dist2, double *dup_out = nullptr)
{
    double dt = u + mq * (1.0 + 1.01 * c.gam) + c.rho;   // (u = +INF: +INF from here to dup)
    if (dt < 0.0)
        dt = 0.0;
    const double sq0 = c.eta + sqrt(dt + 2.0 * c.eta2);
    double dup = sq0 * sq0 * (1.0 + c.g2) * (1.0 + c.g2) + c.sigma2 * c.tau;
    const double dup_r = c.sigma2 * (max_dist2 * (1.0 + c.g2) + c.tau);
    dup = dup_r < dup ? dup_r : dup;
    if (dup_out)
        *dup_out = dup;
    double thr = dup + 2.0 * c.eta * sqrt(dup) + c.eta2 + c.rho - mq * (1.0 - c.gam);
    thr += fabs(thr) * 1e-6 + 1e-30;
    float tf = (float)thr;
    if ((double)tf < thr)
        tf = nextafterf(tf, INFINITY);
    return nextafterf(tf, INFINITY);
}

__device__ __forceinline__ float min3f(float a, float b, float c)
{
    return __builtin_fminf(__builtin_fminf(a, b), c);
}

#define FTRY(call)                       \
    do {                                 \
        hipError_t e_ = (call);          \
        if (e_ != hipSuccess)            \
            return e_;                   \
    } while (0)

static const float kAmaxLimit = 1024.0f;           // queries far outside the references' box
