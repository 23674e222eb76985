// knn_exact.hip — exact fused distance + argmin kernels for gfx950 (MI355X).
//
// Every kernel here evaluates the squared L2 distance with the arithmetic of the reference's
// serial path v0 (sources/src/core.cu:44-49): d = q - r; p = d * d; acc = acc + p for
// dimension 0..k-1, each operation rounded once to binary32 (the file is compiled with
// -ffp-contract=off and tests/test_build.py checks the code object holds no fused
// multiply-add), and folds (distance, global index) into a packed 64-bit key with an unsigned
// min, which reproduces v0's "first strict minimum" (core.cu:50-54) for any visiting order.
//
// Two shapes of kernel, chosen by m (host side: knn_exact_launch):
//   * qreg  — many queries: each lane keeps 2*QP queries' coordinates in VGPRs (packed in
//             float2 so sub/mul/add issue as v_pk_*_f32 on two queries at once) and every
//             wave streams its block's slice of references through SGPRs (wave-uniform
//             s_load of one AoS row = one k-vector).  The (min, argmin) pair lives in the
//             lane, so no cross-lane reduction; one 64-bit atomic min per query per block.
//             VALU-bound: 3k+3 lane-ops per (query, reference) pair.
//   * rlane — few queries: each lane owns one reference row per step (read once from HBM),
//             query coordinates are wave-uniform; wave64 shuffle reduction of the packed
//             key at the end.  HBM-bound for m <~ 10.
//
// This is not a translation of the reference's one-block-per-query kernels (core.cu:808-855):
// no SoA transpose pass, no per-block result array, no host second-level reduce.
#include "knn_exact_dev.h"
#include "knn_slice_launch.h"

#include <math.h>
#include <stdlib.h>



// ------------------------------------------------------------------------------------------
// qreg: queries in VGPRs (pairs packed as float2), references streamed as wave-uniform rows.
//   grid.x = reference slices, grid.y = groups of KNN_WAVES * 128 * QP queries, block = 256.
// ------------------------------------------------------------------------------------------
template <int K, int QP>
__global__ __launch_bounds__(KNN_BLOCK) void knn_exact_qreg(const float *__restrict__ Q,
                                                            const float *__restrict__ R, int m,
                                                            long long n, long long base,
                                                            u64 *__restrict__ keys,
                                                            long long refs_per_block,
                                                            const unsigned *__restrict__ gate)
{
    if (gate && *gate == 0u)
        return;
    exact_qreg_body<K, QP>(Q, R, m, n, base, keys, refs_per_block, blockIdx.x, gridDim.x, blockIdx.y);
}

// Any k up to 16*KC without a compile-time K: the same scheme (queries in VGPRs, rows through
// wave-uniform scalar loads), dimensions in chunks of 16 with the last chunk guarded by uniform
// branches.  PACK = two queries per lane as a float2 (KC <= 4), else one (KC <= 8, k <= 128).  The
// generic row-per-lane kernel runs ~10x below this for m >= 48.
template <bool PACK> struct QregLane;
template <> struct QregLane<true> {
    typedef f2 T;
    static __device__ __forceinline__ f2 make(float a, float b) { return (f2){a, b}; }
    static __device__ __forceinline__ float second(const f2 &v) { return v.y; }
    static __device__ __forceinline__ float first(const f2 &v) { return v.x; }
};
template <> struct QregLane<false> {
    typedef float T;
    static __device__ __forceinline__ float make(float a, float) { return a; }
    static __device__ __forceinline__ float second(const float &) { return INFINITY; }
    static __device__ __forceinline__ float first(const float &v) { return v; }
};

template <int KC, bool PACK>
__global__ __launch_bounds__(KNN_BLOCK) void knn_exact_qregn(const float *__restrict__ Q,
                                                             const float *__restrict__ R, int k, int m,
                                                             long long n, long long base,
                                                             u64 *__restrict__ keys,
                                                             long long refs_per_block,
                                                             const unsigned *__restrict__ gate)
{
#pragma clang fp contract(off)
    if (gate && *gate == 0u)
        return;
    typedef QregLane<PACK> L;
    typedef typename L::T T;
    constexpr int KM = 16 * KC;
    constexpr int QL = PACK ? 2 : 1;  // queries per lane
    const int lane = threadIdx.x & (KNN_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int q0 = (blockIdx.y * KNN_WAVES + wave) * (QL * KNN_WAVE);
    if (q0 >= m)
        return;
    const int qa = min(q0 + lane, m - 1);
    const int qb = min(q0 + KNN_WAVE + lane, m - 1);
    T q[KM];
#pragma unroll
    for (int d = 0; d < KM; ++d)
        q[d] = L::make(d < k ? Q[(size_t)qa * k + d] : 0.0f, PACK && d < k ? Q[(size_t)qb * k + d] : 0.0f);
    float best0 = INFINITY, best1 = INFINITY;
    unsigned bidx0 = 0u, bidx1 = 0u;

    // Slices are strided over: an ordinary launch has one block per slice; the GATED launch (the filter's
    // device-side fallback, almost always a no-op) has at most ~5 resident blocks per CU, so looking at
    // the flag costs a few hundred blocks instead of a full grid queued on every query.
    for (long long i0 = (long long)blockIdx.x * refs_per_block; i0 < n; i0 += (long long)gridDim.x * refs_per_block) {
    const long long i1 = min(n, i0 + refs_per_block);
    unsigned gidx = (unsigned)(base + i0);  // global index of the current reference (low 32 bits)
    const float *__restrict__ r = R + (size_t)i0 * k;
    for (long long i = i0; i < i1; ++i, ++gidx, r += k) {
        T acc = L::make(0.0f, 0.0f);
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            const int rem = k - 16 * c;  // wave-uniform
            if (rem >= 16) {
                float rv[16];
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    rv[j] = r[16 * c + j];  // wave-uniform address -> scalar loads
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const T diff = q[16 * c + j] - L::make(rv[j], rv[j]);
                    const T sq = diff * diff;
                    acc = acc + sq;
                }
            } else if (rem > 0) {
#pragma unroll
                for (int j = 0; j < 15; ++j)
                    if (j < rem) {
                        const float rj = r[16 * c + j];
                        const T diff = q[16 * c + j] - L::make(rj, rj);
                        const T sq = diff * diff;
                        acc = acc + sq;
                    }
            }
        }
        if (best0 > L::first(acc)) {
            best0 = L::first(acc);
            bidx0 = gidx;
        }
        if (PACK && best1 > L::second(acc)) {
            best1 = L::second(acc);
            bidx1 = gidx;
        }
    }
    }  // slices
    if (q0 + lane < m && best0 < INFINITY) {
        const u64 key = pack_key(best0, bidx0);
        if (key < keys[q0 + lane])
            key_atomic_min(&keys[q0 + lane], key);
    }
    if (PACK && q0 + KNN_WAVE + lane < m && best1 < INFINITY) {
        const u64 key = pack_key(best1, bidx1);
        if (key < keys[q0 + KNN_WAVE + lane])
            key_atomic_min(&keys[q0 + KNN_WAVE + lane], key);
    }
}

// One query per lane, no packing: m in [~48, 128*KNN_WAVES) where pairs would idle lanes.
template <int K>
__global__ __launch_bounds__(KNN_BLOCK) void knn_exact_qreg1(const float *__restrict__ Q,
                                                             const float *__restrict__ R, int m,
                                                             long long n, long long base,
                                                             u64 *__restrict__ keys,
                                                             long long refs_per_block,
                                                             const unsigned *__restrict__ gate)
{
#pragma clang fp contract(off)
    if (gate && *gate == 0u)
        return;
    const int lane = threadIdx.x & (KNN_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int q0 = (blockIdx.y * KNN_WAVES + wave) * KNN_WAVE;
    if (q0 >= m)
        return;
    const int qi = q0 + lane;
    const int qc = min(qi, m - 1);
    float q[K];
#pragma unroll
    for (int d = 0; d < K; ++d)
        q[d] = Q[(size_t)qc * K + d];
    float best = INFINITY;
    unsigned bidx = 0u;

    // Slices are strided over: an ordinary launch has one block per slice; the GATED launch (the filter's
    // device-side fallback, almost always a no-op) has at most ~5 resident blocks per CU, so looking at
    // the flag costs a few hundred blocks instead of a full grid queued on every query.
    for (long long i0 = (long long)blockIdx.x * refs_per_block; i0 < n; i0 += (long long)gridDim.x * refs_per_block) {
    const long long i1 = min(n, i0 + refs_per_block);
    unsigned gidx = (unsigned)(base + i0);  // global index of the current reference (low 32 bits)
    const float *__restrict__ r = R + (size_t)i0 * K;
#pragma unroll 4
    for (long long i = i0; i < i1; ++i, ++gidx, r += K) {
        float acc = 0.0f;
#pragma unroll
        for (int d = 0; d < K; ++d) {
            const float diff = q[d] - r[d];
            const float sq = diff * diff;
            acc = acc + sq;
        }
        if (best > acc) {
            best = acc;
            bidx = gidx;
        }
    }
    }  // slices
    if (qi < m && best < INFINITY) {
        const u64 key = pack_key(best, bidx);
        if (key < keys[qi])
            key_atomic_min(&keys[qi], key);
    }
}

// ------------------------------------------------------------------------------------------
// rlane: one reference row per lane per step, QT wave-uniform queries per pass.
//   grid.x = blocks striding over the references, grid.y = ceil(m / QT), block = 256.
//   K > 0: compile-time dimension (rows read with the widest aligned loads the compiler
//   finds); K == 0: run-time k.
// ------------------------------------------------------------------------------------------

template <int K, int QT>
__global__ __launch_bounds__(KNN_BLOCK) void knn_exact_rlane(const float *__restrict__ Q,
                                                             const float *__restrict__ R, int krt,
                                                             int m, long long n, long long base,
                                                             u64 *__restrict__ keys,
                                                             const unsigned *__restrict__ gate,
                                                             const unsigned *__restrict__ gather)
{
#pragma clang fp contract(off)
    // gather != null: scan only the listed rows (the filter's outlier references), n = list length
    if (gate && *gate == 0u)
        return;
    const int k = K > 0 ? K : krt;
    const int nqt = (m + QT - 1) / QT;
    // grid.y may be smaller than the number of query tiles (the launch caps the grid so that a
    // gated no-op launch stays cheap): stride over them
    for (int qt = blockIdx.y; qt < nqt; qt += gridDim.y) {
    const int q0 = qt * QT;
    float best[QT];
    unsigned bidx[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        best[t] = INFINITY;
        bidx[t] = 0u;
    }
    const float *__restrict__ qrow[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t)
        qrow[t] = Q + (size_t)min(q0 + t, m - 1) * k;  // wave-uniform

    const long long stride = (long long)gridDim.x * KNN_BLOCK;
    for (long long i = (long long)blockIdx.x * KNN_BLOCK + threadIdx.x; i < n; i += stride) {
        const long long row = gather ? (long long)gather[i] : i;
        const float *__restrict__ r = R + (size_t)row * k;
        float acc[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t)
            acc[t] = 0.0f;
        if (K > 0) {
            float rv[K > 0 ? K : 1];
#pragma unroll
            for (int d = 0; d < K; ++d)
                rv[d] = r[d];
#pragma unroll
            for (int t = 0; t < QT; ++t) {
#pragma unroll
                for (int d = 0; d < K; ++d) {
                    const float diff = qrow[t][d] - rv[d];
                    const float sq = diff * diff;
                    acc[t] = acc[t] + sq;
                }
            }
        } else {
            for (int d = 0; d < k; ++d) {
                const float rv = r[d];
#pragma unroll
                for (int t = 0; t < QT; ++t) {
                    const float diff = qrow[t][d] - rv;
                    const float sq = diff * diff;
                    acc[t] = acc[t] + sq;
                }
            }
        }
        const unsigned gidx = (unsigned)(base + row);
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            if (best[t] > acc[t]) {
                best[t] = acc[t];
                bidx[t] = gidx;
            }
        }
    }

    const int lane = threadIdx.x & (KNN_WAVE - 1);
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        // A lane that never updated carries (+INF, 0) == kKeyInit, neutral under min.
        const u64 key = wave_min_u64(pack_key(best[t], bidx[t]));
        if (lane == 0 && q0 + t < m && key < kKeyInit && key < keys[q0 + t])
            key_atomic_min(&keys[q0 + t], key);
    }
    }  // query tiles
}

// ------------------------------------------------------------------------------------------
// rlane16: the k = 16, few-queries (HBM-bound) case with LDS-staged reference tiles.  A block
// reads 256 rows = 16 KiB as fully coalesced 16-byte chunks (lane l of a wave takes chunk l: one
// 1 KiB burst per wave-instruction instead of 64 partial lines), parks them in LDS with an XOR
// swizzle of the chunk index, and every lane reads back its own row with four conflict-free
// ds_read_b128.  The next tile's global loads are issued before the current tile is consumed.
// Arithmetic, tie-break and reduction are those of knn_exact_rlane.
// ------------------------------------------------------------------------------------------
typedef float f4x __attribute__((ext_vector_type(4)));

template <int QT>
__global__ __launch_bounds__(KNN_BLOCK) void knn_exact_rlane16(const float *__restrict__ Q,
                                                               const f4x *__restrict__ R4, int m,
                                                               long long n, long long base,
                                                               u64 *__restrict__ keys,
                                                               const unsigned *__restrict__ gate)
{
#pragma clang fp contract(off)
    constexpr int K = 16;
    __shared__ f4x s_x[KNN_BLOCK * 4];
    if (gate && *gate == 0u)
        return;
    const int tid = threadIdx.x;
    const int q0 = blockIdx.y * QT;
    float qv[QT][K];
#pragma unroll
    for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int d = 0; d < K; ++d)
            qv[t][d] = Q[(size_t)min(q0 + t, m - 1) * K + d];  // wave-uniform -> SGPRs
    float best[QT];
    unsigned bidx[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        best[t] = INFINITY;
        bidx[t] = 0u;
    }
    const long long ntiles = (n + KNN_BLOCK - 1) / KNN_BLOCK;
    const long long nchunks = n * 4;  // 16-byte chunks in the shard
    const int sw = (tid >> 2) & 3;

    f4x pre[4];
    long long tile = blockIdx.x;
    if (tile < ntiles) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long c = tile * (KNN_BLOCK * 4) + tid + j * KNN_BLOCK;
            pre[j] = c < nchunks ? __builtin_nontemporal_load(&R4[c]) : (f4x){0.f, 0.f, 0.f, 0.f};
        }
    }
    for (; tile < ntiles; tile += gridDim.x) {
        __syncthreads();  // the previous tile's rows have been consumed
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = tid + j * KNN_BLOCK;
            const int rr = c >> 2, cc = c & 3;
            s_x[rr * 4 + (cc ^ ((rr >> 2) & 3))] = pre[j];
        }
        __syncthreads();
        const long long nxt = tile + gridDim.x;
        if (nxt < ntiles) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long c = nxt * (KNN_BLOCK * 4) + tid + j * KNN_BLOCK;
                pre[j] = c < nchunks ? __builtin_nontemporal_load(&R4[c]) : (f4x){0.f, 0.f, 0.f, 0.f};
            }
        }
        const long long i = tile * KNN_BLOCK + tid;
        float rv[K];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            const f4x x = s_x[tid * 4 + (cc ^ sw)];
            rv[4 * cc + 0] = x[0];
            rv[4 * cc + 1] = x[1];
            rv[4 * cc + 2] = x[2];
            rv[4 * cc + 3] = x[3];
        }
        if (i < n) {
            const unsigned gidx = (unsigned)(base + i);
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                float acc = 0.0f;
#pragma unroll
                for (int d = 0; d < K; ++d) {
                    const float diff = qv[t][d] - rv[d];
                    const float sq = diff * diff;
                    acc = acc + sq;
                }
                if (best[t] > acc) {
                    best[t] = acc;
                    bidx[t] = gidx;
                }
            }
        }
    }
    const int lane = tid & (KNN_WAVE - 1);
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const u64 key = wave_min_u64(pack_key(best[t], bidx[t]));
        if (lane == 0 && q0 + t < m && key < kKeyInit && key < keys[q0 + t])
            key_atomic_min(&keys[q0 + t], key);
    }
}

// ------------------------------------------------------------------------------------------
// Exact re-rank of the MFMA filter's candidate records.  A record names one query and the 16
// references one lane of a 32x32 MFMA tile covers: (query << 32) | (ref_tile << 1) | half, rows
// 8g + 4*half + i (g, i in 0..3) of that tile.  One (record, row) pair per thread, v0 arithmetic.
// ------------------------------------------------------------------------------------------
template <int K, bool LPW = false>  // K > 0: compile-time dimension (all row loads issue before the first use)
__global__ __launch_bounds__(KNN_BLOCK) void knn_rerank_kernel(const float *__restrict__ Q,
                                                               const float *__restrict__ R, int krt,
                                                               long long n, long long base,
                                                               const u64 *__restrict__ rec,
                                                               const unsigned short *__restrict__ rec_rows,
                                                               const unsigned *__restrict__ counts, unsigned nlists,
                                                               unsigned slice, unsigned *__restrict__ ctl,
                                                               u64 *__restrict__ keys, RerankPieces pieces,
                                                               const unsigned *__restrict__ perm,
                                                               unsigned ovf_base, unsigned ovf_cap)
{
    // LPW = true (the cell-pruned path: ~3000 records over 6144 lists, most of them empty): one WAVE per record list, four
    // lists per block — a quarter of the blocks and of the registers the launch holds while the next batch's kernels
    // wait for room; else one block per list (= per filter wave).  The list's piece gives its first query.
    const unsigned list_id = LPW ? blockIdx.x * (KNN_BLOCK / KNN_WAVE) + (threadIdx.x >> 6) : blockIdx.x;
    const unsigned tid_l = LPW ? (threadIdx.x & 63u) : threadIdx.x;       // thread inside the group that owns the list
    constexpr unsigned GROUP = LPW ? KNN_WAVE : KNN_BLOCK;
    unsigned qrow_base = pieces.qrow_base[0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (list_id >= pieces.list_base[i])
            qrow_base = pieces.qrow_base[i];
    if (ctl[KNN_CTL_FALLBACK] != 0u)
        return;  // the exact scan is going to run anyway: do not re-rank a truncated candidate set
    if (ovf_cap != 0u && ctl[KNN_CTL_RECORDS] > ovf_cap) {
        // (cell-pruned path) more candidates than the buffers hold: the fp16 scores do not separate this batch's rows (a
        // cluster tighter than the fp16 step).  Its listed (cell, query) pairs are evaluated exactly instead
        // (knn_cells_exact_kernel) — not the whole shard, as round 2 did — and the records are left alone
        if (blockIdx.x == 0 && threadIdx.x == 0)
            ctl[KNN_CTL_EXACT_CELLS] = 1u;
        return;
    }
    const int k = K > 0 ? K : krt;
    if (list_id < nlists) {
        const unsigned want = counts[list_id];
        const unsigned nrec = min(want, slice);
        // (no shared record counter here: 2048 blocks adding to one word cost ~23 us; the host sums
        // counts[] when statistics are asked for)
        if (tid_l == 0 && want > slice)
            ctl[KNN_CTL_FALLBACK] = 1u;  // candidates were dropped: the gated exact scan takes over
        const u64 *__restrict__ list = rec + (size_t)list_id * slice;
        // 16 consecutive lanes share one record (one query): their keys are min-folded with shuffles
        // and ONE guarded atomic is issued per record (the keys sit on a handful of cache lines; the
        // unguarded 16-per-record form spent ~1 ms in atomic contention at 270k records).
        const unsigned total = (nrec * 16u + GROUP - 1) / GROUP * GROUP;
        // Four chunks of pairs per trip: a pair is a chain of dependent loads (record -> perm -> rows), and a wave that owns a
        // long list (skewed data: 136k records over 6144 lists, the longest in the thousands) walked it one round trip at a
        // time — 0.084 ms for that batch's re-rank, 0.072 with four in flight (a block of four waves per list: 0.062 — it is
        // the few very long lists, not the width).  Short lists (the usual case) make one trip either way.
        constexpr unsigned U = LPW ? 4u : 1u;
        for (unsigned c0 = tid_l; c0 < total; c0 += GROUP * U) {
            u64 key[U];
            unsigned qi[U];
#pragma unroll
            for (unsigned u = 0; u < U; ++u) {
                const unsigned c = c0 + u * GROUP;
                key[u] = ~0ull;
                qi[u] = 0u;
                if (c < nrec * 16u) {
                    const unsigned rmask = rec_rows ? rec_rows[(size_t)list_id * slice + (c >> 4)] : 0xFFFFu;
                    key[u] = rerank_pair<K>(Q, R, k, n, base, list[c >> 4], c & 15u, rmask, qrow_base, perm, qi[u]);
                }
            }
#pragma unroll
            for (unsigned u = 0; u < U; ++u) {
#pragma unroll
                for (int off = 8; off > 0; off >>= 1) {
                    const u64 o = __shfl_xor(key[u], off, KNN_WAVE);
                    key[u] = o < key[u] ? o : key[u];
                }
                // keys[] only ever decreases, so a stale (larger) read can only cause a spare atomic
                if ((threadIdx.x & 15u) == 0u && key[u] != ~0ull && key[u] < keys[qi[u]])
                    key_atomic_min(&keys[qi[u]], key[u]);
            }
        }
    }
    // the shared overflow area (cell-pruned path: what did not fit a wave's slice), all blocks striding over it
    if (ovf_cap != 0u) {
        const unsigned have = ctl[KNN_CTL_RECORDS];
        if (have != 0u) {   // block-uniform
            const u64 *__restrict__ ovf = rec + ovf_base;
            const unsigned pairs = have * 16u;
            const unsigned padded = (pairs + KNN_BLOCK - 1) / KNN_BLOCK * KNN_BLOCK;
            for (unsigned c = blockIdx.x * KNN_BLOCK + threadIdx.x; c < padded; c += gridDim.x * KNN_BLOCK) {
                u64 key = ~0ull;
                unsigned qi = 0u;
                if (c < pairs)
                    key = rerank_pair<K>(Q, R, k, n, base, ovf[c >> 4], c & 15u, 0xFFFFu, 0u, perm, qi);
#pragma unroll
                for (int off = 8; off > 0; off >>= 1) {
                    const u64 o = __shfl_xor(key, off, KNN_WAVE);
                    key = o < key ? o : key;
                }
                if ((threadIdx.x & 15u) == 0u && key != ~0ull && key < keys[qi])
                    key_atomic_min(&keys[qi], key);
            }
        }
    }
}

// Re-rank for records that carry a row mask (deep-K filter): ONE THREAD per record walks the set bits
// of its mask.  With the 16-lanes-per-record form above only ~1 lane in 16 had a row to evaluate
// (the mask usually has a single bit), and at k = 128 a row is a serial chain of 128 subtract /
// multiply / add steps: 0.33 ms for C5's 640k records, most lanes idle.
template <int K>
__device__ __forceinline__ float v0_row_distance(const float *__restrict__ q, const float *__restrict__ r, int krt)
{
#pragma clang fp contract(off)
    const int k = K > 0 ? K : krt;
    float acc = 0.0f;
    int d = 0;
    for (; d + 16 <= k; d += 16) {  // chunks of 16 with all 32 loads in flight; order stays d = 0..k-1
        float qv[16], rv[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            qv[j] = q[d + j];
            rv[j] = r[d + j];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float diff = qv[j] - rv[j];
            const float sq = diff * diff;
            acc = acc + sq;
        }
    }
    for (; d < k; ++d) {
        const float diff = q[d] - r[d];
        const float sq = diff * diff;
        acc = acc + sq;
    }
    return acc;
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_rerank_rows_kernel(const float *__restrict__ Q,
                                                                    const float *__restrict__ R, int k,
                                                                    long long n, long long base,
                                                                    const u64 *__restrict__ rec,
                                                                    const unsigned short *__restrict__ rec_rows,
                                                                    const unsigned *__restrict__ counts,
                                                                    unsigned slice, unsigned *__restrict__ ctl,
                                                                    u64 *__restrict__ keys)
{
    if (ctl[KNN_CTL_FALLBACK] != 0u)
        return;
    const unsigned want = counts[blockIdx.x];
    const unsigned nrec = min(want, slice);
    if (threadIdx.x == 0 && want > slice)
        ctl[KNN_CTL_FALLBACK] = 1u;
    const u64 *__restrict__ list = rec + (size_t)blockIdx.x * slice;
    const unsigned short *__restrict__ rows = rec_rows + (size_t)blockIdx.x * slice;
    for (unsigned c = threadIdx.x; c < nrec; c += KNN_BLOCK) {
        const u64 e = list[c];
        unsigned rm = rows[c];
        const unsigned qi = (unsigned)(e >> 32);
        const unsigned lo = (unsigned)(e & 0xFFFFFFFFull);
        const float *__restrict__ q = Q + (size_t)qi * k;
        u64 key = ~0ull;
        while (rm) {
            const unsigned reg = (unsigned)__builtin_ctz(rm);
            rm &= rm - 1u;
            const long long ri = (long long)(lo >> 1) * 32 + 8 * (reg >> 2) + 4 * (lo & 1u) + (reg & 3u);
            if (ri < n) {
                const float acc = v0_row_distance<0>(q, R + (size_t)ri * k, k);
                if (acc < INFINITY) {  // false for NaN too: v0 never selects those
                    const u64 cand = pack_key(acc, (unsigned)(base + ri));
                    key = cand < key ? cand : key;
                }
            }
        }
        if (key != ~0ull && key < keys[qi])
            key_atomic_min(&keys[qi], key);
    }
}

// ------------------------------------------------------------------------------------------
// Small utility kernels.
// ------------------------------------------------------------------------------------------
__global__ void knn_keys_fill_kernel(u64 *keys, int m)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m)
        keys[i] = kKeyInit;
}

__global__ void knn_keys_unpack_kernel(const u64 *__restrict__ keys, int m, int *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m)
        out[i] = (int)(unsigned)(keys[i] & 0xFFFFFFFFull);
}

__global__ void knn_synth_fill_kernel(float *__restrict__ dst, long long count, u64 seed,
                                      long long first)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        u64 z = seed + ((u64)(first + i) + 1ull) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z = z ^ (z >> 31);
        dst[i] = (float)(unsigned)(z >> 40) * 0x1.0p-24f;  // < 2^24: exact
    }
}

// ------------------------------------------------------------------------------------------
// Host-side dispatch.
// ------------------------------------------------------------------------------------------
namespace {

struct SliceGeom {
    long long refs_per_block;
    unsigned nslices;
};

// Slice the references so the grid has ~20 blocks per CU (each block 4 waves) but a slice is
// never shorter than `min_refs` rows.  32 rows, not more: a block walks its slice serially at
// ~0.6 us per row (4 queries per lane), so 512-row slices put a 0.3 ms floor under every launch
// with n <= 2.6M — (16, 1024, 1024) took 0.42 ms, 0.10 ms with 32-row slices.
SliceGeom slice_refs(long long n, unsigned qgroups, int num_cu, long long min_refs)
{
    long long want = (long long)num_cu * 20 / (qgroups ? qgroups : 1);  // 4-5 rounds of blocks: small tail
    if (want < 1)
        want = 1;
    long long per = (n + want - 1) / want;
    if (per < min_refs)
        per = min_refs;
    SliceGeom g;
    g.refs_per_block = per;
    g.nslices = (unsigned)((n + per - 1) / per);
    return g;
}

// Blocks along the slice axis: one per slice, except for a gated (almost always no-op) launch, which
// gets what is resident at once (5 blocks per CU at these kernels' register counts) and strides.
unsigned slice_grid(const SliceGeom &g, unsigned qgroups, int num_cu, const unsigned *gate)
{
    if (!gate)
        return g.nslices;
    unsigned cap = (unsigned)num_cu * 5u / (qgroups ? qgroups : 1u);
    if (cap < 1u)
        cap = 1u;
    return g.nslices < cap ? g.nslices : cap;
}

template <int K>
hipError_t launch_qreg_k(int m, long long n, long long base, const float *q, const float *r,
                         u64 *keys, int num_cu, const unsigned *gate, hipStream_t s)
{
    // queries per block: 1024 (QP=2) when m fills most of it, else 512 (QP=1), else 256 (unpacked)
    if (m > 3 * KNN_WAVE * KNN_WAVES) {
        const unsigned qg = (unsigned)knn_divup(m, KNN_WAVES * 4 * KNN_WAVE);
        const SliceGeom g = slice_refs(n, qg, num_cu, 32);
        hipLaunchKernelGGL((knn_exact_qreg<K, 2>), dim3(slice_grid(g, qg, num_cu, gate), qg), dim3(KNN_BLOCK), 0, s, q, r,
                           m, n, base, keys, g.refs_per_block, gate);
    } else if (m > KNN_WAVE * KNN_WAVES) {
        const unsigned qg = (unsigned)knn_divup(m, KNN_WAVES * 2 * KNN_WAVE);
        const SliceGeom g = slice_refs(n, qg, num_cu, 32);
        hipLaunchKernelGGL((knn_exact_qreg<K, 1>), dim3(slice_grid(g, qg, num_cu, gate), qg), dim3(KNN_BLOCK), 0, s, q, r,
                           m, n, base, keys, g.refs_per_block, gate);
    } else {
        const unsigned qg = (unsigned)knn_divup(m, KNN_WAVES * KNN_WAVE);
        const SliceGeom g = slice_refs(n, qg, num_cu, 32);
        hipLaunchKernelGGL((knn_exact_qreg1<K>), dim3(slice_grid(g, qg, num_cu, gate), qg), dim3(KNN_BLOCK), 0, s, q, r, m,
                           n, base, keys, g.refs_per_block, gate);
    }
    return hipGetLastError();
}

template <int K>
hipError_t launch_rlane_k(int k, int m, long long n, long long base, const float *q, const float *r,
                          u64 *keys, int num_cu, const unsigned *gate, hipStream_t s)
{
    constexpr int QT = 4;
    if (K == 16 && m <= 2 * QT && n >= 4096 && ((uintptr_t)r & 15u) == 0) {
        // HBM-bound shape: LDS-staged, fully coalesced reference tiles
        // query tile sized to the batch: a lone query should not pay for four (the spare VALU work
        // costs power, hence clock, hence bandwidth)
        const int qt16 = m == 1 ? 1 : m == 2 ? 2 : QT;
        const unsigned gy = (unsigned)knn_divup(m, qt16);
        long long gx = (n + KNN_BLOCK - 1) / KNN_BLOCK;
        const long long capx = (long long)num_cu * 8 / gy;
        if (gx > capx)
            gx = capx;
        if (qt16 == 1)
            hipLaunchKernelGGL((knn_exact_rlane16<1>), dim3((unsigned)gx, gy), dim3(KNN_BLOCK), 0, s, q,
                               (const f4x *)r, m, n, base, keys, gate);
        else if (qt16 == 2)
            hipLaunchKernelGGL((knn_exact_rlane16<2>), dim3((unsigned)gx, gy), dim3(KNN_BLOCK), 0, s, q,
                               (const f4x *)r, m, n, base, keys, gate);
        else
            hipLaunchKernelGGL((knn_exact_rlane16<QT>), dim3((unsigned)gx, gy), dim3(KNN_BLOCK), 0, s, q,
                               (const f4x *)r, m, n, base, keys, gate);
        return hipGetLastError();
    }
    unsigned qt = (unsigned)knn_divup(m, QT);
    if (qt > 64u)
        qt = 64u;  // the kernel strides over the remaining query tiles
    long long blocks = (n + KNN_BLOCK - 1) / KNN_BLOCK;
    long long cap = (long long)num_cu * 8 / qt;
    if (cap < 4)
        cap = 4;
    if (blocks > cap)
        blocks = cap;
    if (blocks < 1)
        blocks = 1;
    hipLaunchKernelGGL((knn_exact_rlane<K, QT>), dim3((unsigned)blocks, qt), dim3(KNN_BLOCK), 0, s, q,
                       r, k, m, n, base, keys, gate, (const unsigned *)nullptr);
    return hipGetLastError();
}

}  // namespace

hipError_t knn_exact_launch(int k, int m, long long n, long long base, const float *q,
                            const float *r, u64 *keys, int num_cu, const unsigned *gate, hipStream_t s)
{
    if (n <= 0 || m <= 0)
        return hipSuccess;
    // Few queries: stream references once per 4 queries (HBM-bound).  Many: qreg (VALU-bound).
    const bool many = m >= 48;
    if (many) {
        switch (k) {
        case 1: return launch_qreg_k<1>(m, n, base, q, r, keys, num_cu, gate, s);
        case 2: return launch_qreg_k<2>(m, n, base, q, r, keys, num_cu, gate, s);
        case 3: return launch_qreg_k<3>(m, n, base, q, r, keys, num_cu, gate, s);
        case 4: return launch_qreg_k<4>(m, n, base, q, r, keys, num_cu, gate, s);
        case 8: return launch_qreg_k<8>(m, n, base, q, r, keys, num_cu, gate, s);
        case 16: return launch_qreg_k<16>(m, n, base, q, r, keys, num_cu, gate, s);
        default: break;
        }
        if (k <= 128 && n >= 2048) {  // no compile-time K: chunked run-time-k form of the same kernel
            // (below ~2k rows its query prologue, 16*KC loads per lane, costs more than the scan)
            const int kc = (k + 15) / 16;
            const bool pack = kc <= 4;
            const unsigned qg = (unsigned)knn_divup(m, KNN_WAVES * (pack ? 2 : 1) * KNN_WAVE);
            const SliceGeom g = slice_refs(n, qg, num_cu, 32);
            const dim3 grid(slice_grid(g, qg, num_cu, gate), qg), block(KNN_BLOCK);
#define KNN_QREGN(KCV, PK)                                                                                  \
    hipLaunchKernelGGL((knn_exact_qregn<KCV, PK>), grid, block, 0, s, q, r, k, m, n, base, keys, g.refs_per_block, gate)
            switch (kc) {
            case 1: KNN_QREGN(1, true); break;
            case 2: KNN_QREGN(2, true); break;
            case 3: KNN_QREGN(3, true); break;
            case 4: KNN_QREGN(4, true); break;
            case 5: KNN_QREGN(5, false); break;
            case 6: KNN_QREGN(6, false); break;
            case 7: KNN_QREGN(7, false); break;
            default: KNN_QREGN(8, false); break;
            }
#undef KNN_QREGN
            return hipGetLastError();
        }
    }
    switch (k) {
    case 1: return launch_rlane_k<1>(k, m, n, base, q, r, keys, num_cu, gate, s);
    case 2: return launch_rlane_k<2>(k, m, n, base, q, r, keys, num_cu, gate, s);
    case 3: return launch_rlane_k<3>(k, m, n, base, q, r, keys, num_cu, gate, s);
    case 4: return launch_rlane_k<4>(k, m, n, base, q, r, keys, num_cu, gate, s);
    case 8: return launch_rlane_k<8>(k, m, n, base, q, r, keys, num_cu, gate, s);
    case 16: return launch_rlane_k<16>(k, m, n, base, q, r, keys, num_cu, gate, s);
    default: return launch_rlane_k<0>(k, m, n, base, q, r, keys, num_cu, gate, s);
    }
}

hipError_t knn_exact_gather_launch(int k, int m, unsigned count, long long base, const float *q, const float *r,
                                   const unsigned *list, u64 *keys, int num_cu, const unsigned *gate, hipStream_t s)
{
    // exact scan of an explicit row list (listed rows in any order: the packed-key min does not care)
    if (count == 0 || m <= 0)
        return hipSuccess;
    constexpr int QT = 4;
    unsigned qt = (unsigned)knn_divup(m, QT);
    if (qt > 256u)
        qt = 256u;
    long long blocks = ((long long)count + KNN_BLOCK - 1) / KNN_BLOCK;
    long long cap = (long long)num_cu * 8 / qt;
    if (cap < 1)
        cap = 1;
    if (blocks > cap)
        blocks = cap;
    const dim3 grid((unsigned)blocks, qt);
    switch (k) {
    case 3: hipLaunchKernelGGL((knn_exact_rlane<3, QT>), grid, dim3(KNN_BLOCK), 0, s, q, r, k, m, (long long)count, base, keys, gate, list); break;
    case 8: hipLaunchKernelGGL((knn_exact_rlane<8, QT>), grid, dim3(KNN_BLOCK), 0, s, q, r, k, m, (long long)count, base, keys, gate, list); break;
    case 16: hipLaunchKernelGGL((knn_exact_rlane<16, QT>), grid, dim3(KNN_BLOCK), 0, s, q, r, k, m, (long long)count, base, keys, gate, list); break;
    default: hipLaunchKernelGGL((knn_exact_rlane<0, QT>), grid, dim3(KNN_BLOCK), 0, s, q, r, k, m, (long long)count, base, keys, gate, list); break;
    }
    return hipGetLastError();
}

hipError_t knn_rerank_launch(int k, long long n, const float *q, const float *r, long long base,
                             const u64 *rec, const unsigned short *rec_rows, const unsigned *counts,
                             unsigned nlists, unsigned slice, unsigned *ctl, u64 *keys, RerankPieces pieces,
                             hipStream_t s, const unsigned *perm, unsigned ovf_base, unsigned ovf_cap)
{
    if (nlists == 0)
        return hipSuccess;
    if (rec_rows && perm)
        return hipErrorInvalidValue;  // row masks belong to the deep-K scan, cell-sorted layouts to k <= 16
    if (rec_rows) {  // deep-K scans are never cut into pieces
        hipLaunchKernelGGL(knn_rerank_rows_kernel, dim3(nlists), dim3(KNN_BLOCK), 0, s, q, r, k, n, base, rec, rec_rows,
                           counts, slice, ctl, keys);
        return hipGetLastError();
    }
#define KNN_RERANK(KK)                                                                                     \
    hipLaunchKernelGGL(knn_rerank_kernel<KK>, dim3(nlists), dim3(KNN_BLOCK), 0, s, q, r, k, n, base, rec, rec_rows, \
                       counts, nlists, slice, ctl, keys, pieces, perm, ovf_base, ovf_cap)
#define KNN_RERANK_LPW(KK)                                                                                 \
    hipLaunchKernelGGL((knn_rerank_kernel<KK, true>), dim3((nlists + KNN_WAVES - 1) / KNN_WAVES), dim3(KNN_BLOCK), 0, s, q, r, k, n, \
                       base, rec, rec_rows, counts, nlists, slice, ctl, keys, pieces, perm, ovf_base, ovf_cap)
    if (perm) {   // cell-sorted layout = the pruned scan's records: few, spread thin
        switch (k) {
        case 3: KNN_RERANK_LPW(3); break;
        case 4: KNN_RERANK_LPW(4); break;
        case 8: KNN_RERANK_LPW(8); break;
        case 16: KNN_RERANK_LPW(16); break;
        default: KNN_RERANK_LPW(0); break;
        }
        return hipGetLastError();
    }
    switch (k) {
    case 3: KNN_RERANK(3); break;
    case 4: KNN_RERANK(4); break;
    case 8: KNN_RERANK(8); break;
    case 16: KNN_RERANK(16); break;
    default: KNN_RERANK(0); break;
    }
#undef KNN_RERANK
#undef KNN_RERANK_LPW
    return hipGetLastError();
}

hipError_t knn_keys_fill_launch(u64 *keys, int m, hipStream_t s)
{
    if (m <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(knn_keys_fill_kernel, dim3(knn_divup(m, 256)), dim3(256), 0, s, keys, m);
    return hipGetLastError();
}

hipError_t knn_keys_unpack_launch(const u64 *keys, int m, int *out, hipStream_t s)
{
    if (m <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(knn_keys_unpack_kernel, dim3(knn_divup(m, 256)), dim3(256), 0, s, keys, m, out);
    return hipGetLastError();
}

hipError_t knn_synth_fill_launch(float *dst, long long count, u64 seed, long long first, hipStream_t s)
{
    if (count <= 0)
        return hipSuccess;
    long long blocks = (count + 255) / 256;
    if (blocks > 8192)
        blocks = 8192;
    hipLaunchKernelGGL(knn_synth_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, s, dst, count, seed,
                       first);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Top-K (knn_index_query_topk): the K smallest packed keys per query, sorted ascending.
//
// knn_exact_topk_kernel<KC> — the exact scan with v0's arithmetic.  One wave per block, lanes = queries (coordinates in
// VGPRs), rows streamed as wave-uniform scalar loads over the block's slice of the shard: the qregn scheme unpacked.  Each
// lane keeps its query's K best (distance, LOCAL row) keys as a sorted column of LDS ([K][64] u64: 32 KiB at K = 64) and
// its K-th key in a register; a row costs the 1-NN loop plus one 64-bit compare, and the rare accepted row is inserted
// by shifting the larger keys down one place.  Rows whose distance is not finite never get in: their key is >= (+INF, 0),
// the K-th key never exceeds it.  At the end the column goes to part[slice][query][K] with the global row numbers (base +
// row, or gids[row]: both ascending in the local row, so the order the scan decided is kept).
// KC = chunks of 16 dimensions held in VGPRs (k <= 128); KC = 0: any k, the query's coordinates re-read from memory.
// LIM (knn_index_query_topk_within): a row is a candidate only when its key is below `lim` = (bits(max_dist2) + 1) << 32, i.e.
// its v0 distance is <= max_dist2.  The K-th key a row is compared with is min(column[K - 1], lim) — the column's last place is
// KNN_KEY_INIT until K rows are in, and read back bare it would let rows beyond the radius in after the first insertion.  The
// plain form (LIM = false) never reads `lim`.
// ------------------------------------------------------------------------------------------
template <int KC, bool LIM = false>
__global__ __launch_bounds__(KNN_WAVE) void knn_exact_topk_kernel(const float *__restrict__ Q, const float *__restrict__ R,
                                                                 int k, int m, long long n, int K, long long rows_per_slice,
                                                                 long long base, const unsigned *__restrict__ gids,
                                                                 u64 *__restrict__ part, const unsigned *__restrict__ gate,
                                                                 u64 lim)
{
#pragma clang fp contract(off)
    extern __shared__ u64 topk_lst[];   // [K][KNN_WAVE]
    if (gate && *gate == 0u)   // gated form: the filter top-K's fallback (runs only when the batch raised FALLBACK)
        return;
    constexpr int KM = KC > 0 ? 16 * KC : 1;
    const int lane = threadIdx.x;
    const int q = blockIdx.y * KNN_WAVE + lane;
    const int qa = min(q, m - 1);
    float qv[KM];
#pragma unroll
    for (int d = 0; d < KM; ++d)
        qv[d] = KC > 0 && d < k ? Q[(size_t)qa * k + d] : 0.0f;
    for (int t = 0; t < K; ++t)
        topk_lst[t * KNN_WAVE + lane] = kKeyInit;
    u64 kth = LIM && lim < kKeyInit ? lim : kKeyInit;
    const long long i0 = (long long)blockIdx.x * rows_per_slice;
    const long long i1 = min(n, i0 + rows_per_slice);
    const float *__restrict__ r = R + (size_t)i0 * k;
    const float *__restrict__ qp = Q + (size_t)qa * k;
    for (long long i = i0; i < i1; ++i, r += k) {
        float acc = 0.0f;   // (lane_row_dist2's arithmetic, knn_exact_dev.h, in this kernel's own text: a call schedules the prologue differently)
        if (KC > 0) {
#pragma unroll
            for (int c = 0; c < (KC > 0 ? KC : 1); ++c) {
                const int rem = k - 16 * c;   // wave-uniform
                if (rem >= 16) {
                    float rv[16];
#pragma unroll
                    for (int j = 0; j < 16; ++j)
                        rv[j] = r[16 * c + j];   // wave-uniform address -> scalar loads
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const float diff = qv[16 * c + j] - rv[j];
                        const float sq = diff * diff;
                        acc = acc + sq;
                    }
                } else if (rem > 0) {
#pragma unroll
                    for (int j = 0; j < 15; ++j)
                        if (j < rem) {
                            const float diff = qv[16 * c + j] - r[16 * c + j];
                            const float sq = diff * diff;
                            acc = acc + sq;
                        }
                }
            }
        } else {
            for (int d = 0; d < k; ++d) {
                const float diff = qp[d] - r[d];
                const float sq = diff * diff;
                acc = acc + sq;
            }
        }
        const u64 key = pack_key(acc, (unsigned)i);
        if (key < kth) {
            int p = K - 1;
            while (p > 0) {
                const u64 prev = topk_lst[(p - 1) * KNN_WAVE + lane];
                if (prev < key)
                    break;
                topk_lst[p * KNN_WAVE + lane] = prev;
                --p;
            }
            topk_lst[p * KNN_WAVE + lane] = key;
            kth = topk_lst[(K - 1) * KNN_WAVE + lane];
            if (LIM)
                kth = kth < lim ? kth : lim;
        }
    }
    if (q >= m)
        return;
    u64 *__restrict__ out = part + ((size_t)blockIdx.x * m + q) * K;
    for (int t = 0; t < K; ++t) {
        const u64 key = topk_lst[t * KNN_WAVE + lane];
        const unsigned row = (unsigned)key;
        const bool real = (key >> 32) < 0x7F800000ull;
        const unsigned g = gids ? (real ? gids[row] : 0u) : (unsigned)(base + (long long)row);
        out[t] = real ? ((key & 0xFFFFFFFF00000000ull) | (u64)g) : kKeyInit;
    }
}

// One wave: a (its lane t < K holds a[t], the others ~0) <- the K smallest of a and b (same form), both sorted.  The
// output place of a[t] is t + #{b < a[t]}, of b[t] is t + #{a <= b[t]}: distinct places, a stable merge.  sa / sb / so:
// the wave's three 64-key LDS rows.
__device__ __forceinline__ u64 topk_wave_merge(u64 a, u64 b, int K, int lane, u64 *sa, u64 *sb, u64 *so)
{
    const u64 b0 = __shfl(b, 0, KNN_WAVE);
    const u64 alast = __shfl(a, K - 1, KNN_WAVE);
    if (b0 >= alast)   // nothing of b gets in (wave-uniform)
        return a;
    sa[lane] = a;
    sb[lane] = b;
    __syncthreads();
    if (lane < K) {
        int lo = 0, hi = K;   // #{b < a[lane]}
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sb[mid] < a)
                lo = mid + 1;
            else
                hi = mid;
        }
        if (lane + lo < K)
            so[lane + lo] = a;
        lo = 0;
        hi = K;   // #{a <= b[lane]}
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sa[mid] <= b)
                lo = mid + 1;
            else
                hi = mid;
        }
        if (lane + lo < K)
            so[lane + lo] = b;
    }
    __syncthreads();
    const u64 r = lane < K ? so[lane] : ~0ull;
    __syncthreads();
    return r;
}

// One wave (block) per query: keys[q][0..K) <- the K smallest of (keys[q] unless init, lists[0][q], ..., lists[nl-1][q]),
// sorted.  lists = [nl][m][K], every list sorted.  The fold of the scan's slices and knn_keys_topk_merge.
__global__ __launch_bounds__(KNN_WAVE) void knn_topk_select_kernel(const u64 *__restrict__ lists, int nl, int m, int K,
                                                                  u64 *__restrict__ keys, int init,
                                                                  const unsigned *__restrict__ gate)
{
    __shared__ u64 sa[KNN_WAVE], sb[KNN_WAVE], so[KNN_WAVE];
    if (gate && *gate == 0u)
        return;
    const int q = blockIdx.x;
    const int lane = threadIdx.x;
    u64 cur = lane < K ? (init ? kKeyInit : keys[(size_t)q * K + lane]) : ~0ull;
    for (int l = 0; l < nl; ++l) {
        const u64 b = lane < K ? lists[((size_t)l * m + q) * K + lane] : ~0ull;
        cur = topk_wave_merge(cur, b, K, lane, sa, sb, so);
    }
    if (lane < K)
        keys[(size_t)q * K + lane] = cur;
}

namespace {
constexpr size_t kTopkPartBytes = (size_t)128 << 20;   // most bytes of the scan's per-slice lists of one query chunk

// Slices of the shard the exact top-K scan splits one chunk of mc queries into: >= 1024 rows each, lists within
// kTopkPartBytes (at least one), and ~32 waves per CU for K <= 16 (the scalar row loads need the occupancy: K 8 at C3's shape
// 68 -> 22 ms) but ~8 for larger K (every slice fills its K-list from scratch and the fold reads every slice's list: K 64
// 241 ms at 8, 334 at 32).
}  // namespace

long long knn_topk_slices(int mc, int K, long long n, int num_cu)
{
    const unsigned qg = (unsigned)knn_divup(mc, KNN_WAVE);
    long long slices = (long long)num_cu * (K <= 16 ? 32 : 8) / qg;
    const long long by_rows = (n + 1023) / 1024;
    const long long by_room = (long long)(kTopkPartBytes / ((size_t)mc * (size_t)K * sizeof(u64)));
    if (slices > by_rows)
        slices = by_rows;
    if (slices > by_room)
        slices = by_room;
    if (slices > 65535)
        slices = 65535;
    if (slices < 1)
        slices = 1;
    const long long per = (n + slices - 1) / slices;
    return (n + per - 1) / per;
}

hipError_t knn_topk_select_launch(const u64 *lists, int nl, int m, int K, u64 *keys, int init, hipStream_t s)
{
    if (m <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(knn_topk_select_kernel, dim3((unsigned)m), dim3(KNN_WAVE), 0, s, lists, nl, m, K, keys, init,
                       (const unsigned *)nullptr);
    return hipGetLastError();
}

size_t knn_topk_part_bytes(int m, int K, long long n, int num_cu)
{
    if (n <= 0 || m <= 0)
        return 0;
    const SliceChunk first = knn_slice_chunk(0, m, n, num_cu, KnnTopkSlices{K});
    return KnnTopkSlices{K}.part_bytes(first.slices, first.mc);
}

hipError_t knn_exact_topk_launch(const TopkCall &c, const unsigned *gate, bool limit)
{
    const u64 lim = limit ? c.limit_key() : kKeyInit;
    const bool within = lim < kKeyInit;   // (a limit at or above (+INF, 0) admits what the plain form admits)
    const int K = c.K;
    hipStream_t s = c.stream;
    if (c.m <= 0 || K < 1 || K > KNN_TOPK_MAX)
        return c.m <= 0 ? hipSuccess : hipErrorInvalidValue;
    if (c.n <= 0) {   // nothing to add: the keys stay (or start at (+INF, 0))
        if (c.init && !gate)
            return knn_keys_fill_launch(c.keys, (int)((long long)c.m * K), s);
        return hipSuccess;
    }
    return knn_slice_chunks(c.m, c.n, c.num_cu, KnnTopkSlices{K}, [&](const SliceChunk &ch) {
        const int mc = ch.mc;
        const long long per = ch.per;
        if (KnnTopkSlices{K}.part_bytes(ch.slices, mc) > c.part_bytes)
            return hipErrorInvalidValue;
        const dim3 grid = ch.grid, block(KNN_WAVE);
        const size_t lds = KnnTopkSlices{K}.lds_bytes();
        const float *qc = c.q + (size_t)ch.c0 * c.k;
#define KNN_TOPK_SCAN(KCV)                                                                                                       \
    if (within)                                                                                                                  \
        hipLaunchKernelGGL((knn_exact_topk_kernel<KCV, true>), grid, block, lds, s, qc, c.r, c.k, mc, c.n, K, per, c.base, c.gids,  \
                           c.part, gate, lim);                                                                                   \
    else                                                                                                                         \
        hipLaunchKernelGGL((knn_exact_topk_kernel<KCV>), grid, block, lds, s, qc, c.r, c.k, mc, c.n, K, per, c.base, c.gids, c.part, \
                           gate, lim)
        KNN_KC_SWITCH(c.k, KNN_TOPK_SCAN)
#undef KNN_TOPK_SCAN
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
        hipLaunchKernelGGL(knn_topk_select_kernel, dim3((unsigned)mc), dim3(KNN_WAVE), 0, s, (const u64 *)c.part, (int)ch.slices, mc,
                           K, c.keys + (size_t)ch.c0 * K, c.init, gate);
        return hipGetLastError();
    });
}

hipError_t knn_topk_merge_launch(int m, int K, const u64 *a, u64 *b, hipStream_t s)
{
    if (m <= 0)
        return hipSuccess;
    if (K < 1 || K > KNN_TOPK_MAX)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(knn_topk_select_kernel, dim3((unsigned)m), dim3(KNN_WAVE), 0, s, a, 1, m, K, b, 0, (const unsigned *)nullptr);
    return hipGetLastError();
}

// knn_index_query_topk_within on the ways whose kernels carry no radius: one wave (block) per query.  lists[q][0..K) is a sorted
// top-K list; every key >= lim becomes KNN_KEY_INIT — a sorted top-K list clipped at a key is the top-K of the clipped set, and
// the clipped places are the list's tail, so it stays sorted — and the list is written to keys[q] (init) or folded into it.
__global__ __launch_bounds__(KNN_WAVE) void knn_topk_clip_kernel(const u64 *__restrict__ lists, int K, u64 lim,
                                                                u64 *__restrict__ keys, int init)
{
    __shared__ u64 sa[KNN_WAVE], sb[KNN_WAVE], so[KNN_WAVE];
    const int q = blockIdx.x;
    const int lane = threadIdx.x;
    u64 b = ~0ull;
    if (lane < K) {
        b = lists[(size_t)q * K + lane];
        b = b < lim ? b : kKeyInit;
    }
    const u64 cur = init ? b : topk_wave_merge(lane < K ? keys[(size_t)q * K + lane] : ~0ull, b, K, lane, sa, sb, so);
    if (lane < K)
        keys[(size_t)q * K + lane] = cur;
}

hipError_t knn_topk_clip_launch(int m, int K, const u64 *lists, u64 lim, u64 *keys, int init, hipStream_t s)
{
    if (m <= 0)
        return hipSuccess;
    if (K < 1 || K > KNN_TOPK_MAX)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(knn_topk_clip_kernel, dim3((unsigned)m), dim3(KNN_WAVE), 0, s, lists, K, lim, keys, init);
    return hipGetLastError();
}

// ---- top-K on the MFMA filter (knn_filter_query_topk) --------------------------------------------------------------------

// Bitonic sort of one key per lane across the wave, ascending.
__device__ __forceinline__ u64 topk_wave_sort(u64 v, int lane)
{
#pragma unroll
    for (int kk = 2; kk <= KNN_WAVE; kk <<= 1) {
#pragma unroll
        for (int j = kk >> 1; j > 0; j >>= 1) {
            const u64 o = __shfl_xor(v, j, KNN_WAVE);
            const bool up = (lane & kk) == 0;
            const bool lower = (lane & j) == 0;
            const u64 lo = o < v ? o : v, hi = o < v ? v : o;
            v = lower == up ? lo : hi;
        }
    }
    return v;
}

__device__ __forceinline__ unsigned topk_f2ord(float f)
{
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float topk_ord2f(unsigned o)
{
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

// One wave per query: umin[0][q] <- the K-th smallest FINITE per-block minimum of umin[0 .. nb)[q] (+INF when fewer than K
// blocks hold one).  The sample pass's blocks score disjoint tiles, and a padding position's or an out-of-box row's score is
// +INF (norm +INF), so K finite minima are the scores of K distinct real rows.  knn_thr_kernel then reads this one row.
__global__ __launch_bounds__(KNN_WAVE) void knn_topk_umin_kernel(float *__restrict__ umin, int nb, int m_padded, int K)
{
    __shared__ u64 sa[KNN_WAVE], sb[KNN_WAVE], so[KNN_WAVE];
    const int q = blockIdx.x, lane = threadIdx.x;
    u64 cur = ~0ull;
    for (int b0 = 0; b0 < nb; b0 += KNN_WAVE) {
        const int b = b0 + lane;
        const float u = b < nb ? umin[(size_t)b * m_padded + q] : INFINITY;
        u64 key = (u < INFINITY && u > -INFINITY) ? (((u64)topk_f2ord(u) << 32) | (u64)(unsigned)b) : ~0ull;
        key = topk_wave_sort(key, lane);
        cur = topk_wave_merge(cur, lane < K ? key : ~0ull, K, lane, sa, sb, so);
    }
    const u64 kth = __shfl(cur, K - 1, KNN_WAVE);
    __syncthreads();
    if (lane == 0)
        umin[q] = kth == ~0ull ? INFINITY : topk_ord2f((unsigned)(kth >> 32));
}

__device__ __forceinline__ void topk_cand_push(u64 key, unsigned q, u64 *__restrict__ cand, unsigned *__restrict__ ccount,
                                               unsigned ccap, unsigned *__restrict__ ctl)
{
    const unsigned slot = atomicAdd(&ccount[q], 1u);
    if (slot < ccap)
        cand[(size_t)q * ccap + slot] = key;
    else
        ctl[KNN_CTL_FALLBACK] = 1u;   // candidates dropped: the gated exact top-K answers the batch
}

// The filter's records, every row of every record with v0 arithmetic (through perm on a cell-sorted layout): each finite key
// goes to its query's candidate list.  One block per record list (= filter wave), as knn_rerank_kernel.
__global__ __launch_bounds__(KNN_BLOCK) void knn_topk_rerank_kernel(const float *__restrict__ Q, const float *__restrict__ R,
                                                                   int k, long long n, long long base,
                                                                   const u64 *__restrict__ rec,
                                                                   const unsigned short *__restrict__ rec_rows,
                                                                   const unsigned *__restrict__ counts, unsigned nlists,
                                                                   unsigned slice, unsigned *__restrict__ ctl,
                                                                   RerankPieces pieces, const unsigned *__restrict__ perm,
                                                                   u64 *__restrict__ cand, unsigned *__restrict__ ccount,
                                                                   unsigned ccap)
{
    const unsigned list_id = blockIdx.x;
    unsigned qrow_base = pieces.qrow_base[0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (list_id >= pieces.list_base[i])
            qrow_base = pieces.qrow_base[i];
    if (ctl[KNN_CTL_FALLBACK] != 0u || list_id >= nlists)
        return;
    const unsigned want = counts[list_id];
    const unsigned nrec = min(want, slice);
    if (threadIdx.x == 0 && want > slice)
        ctl[KNN_CTL_FALLBACK] = 1u;
    const u64 *__restrict__ list = rec + (size_t)list_id * slice;
    for (unsigned c = threadIdx.x; c < nrec * 16u; c += KNN_BLOCK) {
        const unsigned rmask = rec_rows ? rec_rows[(size_t)list_id * slice + (c >> 4)] : 0xFFFFu;
        unsigned qi = 0u;
        const u64 key = rerank_pair<0>(Q, R, k, n, base, list[c >> 4], c & 15u, rmask, qrow_base, perm, qi);
        if (key != ~0ull)
            topk_cand_push(key, qi, cand, ccount, ccap, ctl);
    }
}

// The same for the cell-pruned top-K (knn_cells_query_topk): a key enters its query's candidate list only when its v0 distance
// is at most gate[q] = knn_topk_gate(Dup_q) — no row of the query's top-K lies beyond it (knn_exact_dev.h) —, which turns
// "16 keys per record" into about one.  One block per list; records through perm, all 16 rows — except positions whose layout
// norm is +INF: padding, and rows outside the robust box, which sit in the layout beside rows that pass and are pushed by
// knn_topk_outlier_kernel (pushed here as well such a row stood in the list twice and the select dropped the query's K-th key).
// gids (nullable; cell-range shards, where base is 0): the key's index half becomes gids[row] BEFORE it enters the candidate list —
// the select sorts keys and a fold compares them with other ranks' —; gids ascend with the row, so v0's lowest-index tie-break stands.
__global__ __launch_bounds__(KNN_BLOCK) void knn_topk_rerank_gated_kernel(const float *__restrict__ Q, const float *__restrict__ R,
                                                                         int k, long long n, long long base,
                                                                         const u64 *__restrict__ rec,
                                                                         const unsigned *__restrict__ counts, unsigned nlists,
                                                                         unsigned slice, unsigned *__restrict__ ctl,
                                                                         const unsigned *__restrict__ perm,
                                                                         const float *__restrict__ norms,
                                                                         const float *__restrict__ dup, float inv_sigma2,
                                                                         u64 *__restrict__ cand, unsigned *__restrict__ ccount,
                                                                         unsigned ccap, const unsigned *__restrict__ gids)
{
    const unsigned list_id = blockIdx.x;
    if (ctl[KNN_CTL_FALLBACK] != 0u || list_id >= nlists)
        return;
    const unsigned want = counts[list_id];
    const unsigned nrec = min(want, slice);
    if (threadIdx.x == 0 && want > slice)
        ctl[KNN_CTL_FALLBACK] = 1u;
    const u64 *__restrict__ list = rec + (size_t)list_id * slice;
    for (unsigned c = threadIdx.x; c < nrec * 16u; c += KNN_BLOCK) {
        unsigned qi = 0u;
        const u64 e = list[c >> 4];
        const unsigned lo = (unsigned)e, reg = c & 15u;
        const long long pos = (long long)(lo >> 1) * 32 + 8 * (reg >> 2) + 4 * (lo & 1u) + (reg & 3u);   // (rerank_pair's)
        const unsigned rmask = pos < n && norms[pos] < INFINITY ? 0xFFFFu : 0u;
        const u64 key = rerank_pair<0>(Q, R, k, n, base, e, reg, rmask, 0u, perm, qi);
        if (key != ~0ull && __uint_as_float((unsigned)(key >> 32)) <= knn_topk_gate(dup[qi], inv_sigma2))
            topk_cand_push(gids ? (key & 0xFFFFFFFF00000000ull) | (u64)gids[(unsigned)key] : key, qi, cand, ccount, ccap, ctl);
    }
}

// Rows outside the filter's robust box never enter the scan: every (query, listed row) pair with v0 arithmetic, each finite
// key to the query's candidate list.  grid (row blocks, queries).  gids (nullable): as in the gated re-rank.
__global__ __launch_bounds__(KNN_BLOCK) void knn_topk_outlier_kernel(const float *__restrict__ Q, const float *__restrict__ R,
                                                                    int k, unsigned count, long long base,
                                                                    const unsigned *__restrict__ list, unsigned *__restrict__ ctl,
                                                                    u64 *__restrict__ cand, unsigned *__restrict__ ccount,
                                                                    unsigned ccap, const unsigned *__restrict__ gids)
{
#pragma clang fp contract(off)
    if (ctl[KNN_CTL_FALLBACK] != 0u)
        return;
    const unsigned q = blockIdx.y;
    const float *__restrict__ qp = Q + (size_t)q * k;
    for (unsigned j = blockIdx.x * KNN_BLOCK + threadIdx.x; j < count; j += gridDim.x * KNN_BLOCK) {
        const unsigned row = list[j];
        const float *__restrict__ r = R + (size_t)row * k;
        float acc = 0.0f;
        for (int d = 0; d < k; ++d) {
            const float diff = qp[d] - r[d];
            const float sq = diff * diff;
            acc = acc + sq;
        }
        if (acc < INFINITY)
            topk_cand_push(pack_key(acc, gids ? gids[row] : (unsigned)(base + (long long)row)), q, cand, ccount, ccap, ctl);
    }
}

// One wave per query, gated on NO fallback: keys[q] <- the K smallest of (keys[q] unless init, the query's candidates), sorted.
__global__ __launch_bounds__(KNN_WAVE) void knn_topk_select_cand_kernel(const u64 *__restrict__ cand,
                                                                       const unsigned *__restrict__ ccount, unsigned ccap,
                                                                       int K, u64 *__restrict__ keys, int init,
                                                                       const unsigned *__restrict__ fallback)
{
    __shared__ u64 sa[KNN_WAVE], sb[KNN_WAVE], so[KNN_WAVE];
    if (*fallback != 0u)
        return;
    const int q = blockIdx.x, lane = threadIdx.x;
    const unsigned c = min(ccount[q], ccap);
    u64 cur = lane < K ? (init ? kKeyInit : keys[(size_t)q * K + lane]) : ~0ull;
    for (unsigned i0 = 0; i0 < c; i0 += KNN_WAVE) {
        u64 v = i0 + lane < c ? cand[(size_t)q * ccap + i0 + lane] : ~0ull;
        v = topk_wave_sort(v, lane);
        cur = topk_wave_merge(cur, lane < K ? v : ~0ull, K, lane, sa, sb, so);
    }
    if (lane < K)
        keys[(size_t)q * K + lane] = cur;
}

hipError_t knn_topk_umin_launch(float *umin, int nb, int m_padded, int K, hipStream_t s)
{
    hipLaunchKernelGGL(knn_topk_umin_kernel, dim3((unsigned)m_padded), dim3(KNN_WAVE), 0, s, umin, nb, m_padded, K);
    return hipGetLastError();
}

hipError_t knn_topk_filter_finish(const TopkCall &c, const TopkRecords &rs)
{
    hipStream_t s = c.stream;
    if (rs.gate_dup) {   // the cell-pruned top-K: the gated re-rank over the waves' slices and over the shared overflow area
        if (rs.rec_rows || !rs.perm || !rs.pos_norms || (c.gids && c.base != 0))
            return hipErrorInvalidValue;
        if (rs.nlists)
            hipLaunchKernelGGL(knn_topk_rerank_gated_kernel, dim3(rs.nlists), dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, c.base,
                               rs.rec, rs.counts, rs.nlists, rs.slice, rs.ctl, rs.perm, rs.pos_norms, rs.gate_dup, rs.inv_sigma2, c.cand,
                               c.ccount, c.ccap, c.gids);
        if (rs.ovf_rec && rs.ovf_count)   // (its `want > slice` rule raises FALLBACK for an over-full area)
            hipLaunchKernelGGL(knn_topk_rerank_gated_kernel, dim3(1), dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, c.base,
                               rs.ovf_rec, rs.ovf_count, 1u, rs.ovf_slice, rs.ctl, rs.perm, rs.pos_norms, rs.gate_dup, rs.inv_sigma2,
                               c.cand, c.ccount, c.ccap, c.gids);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    } else if (c.gids) {   // (the ungated re-rank of the filter's full scan pushes base + row: not for cell-range shards)
        return hipErrorInvalidValue;
    } else if (rs.nlists) {
        hipLaunchKernelGGL(knn_topk_rerank_kernel, dim3(rs.nlists), dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, c.base, rs.rec,
                           rs.rec_rows, rs.counts, rs.nlists, rs.slice, rs.ctl, rs.pieces, rs.perm, c.cand, c.ccount, c.ccap);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    if (rs.n_outliers) {
        const unsigned gx = (rs.n_outliers + KNN_BLOCK - 1) / KNN_BLOCK < 64u ? (rs.n_outliers + KNN_BLOCK - 1) / KNN_BLOCK : 64u;
        hipLaunchKernelGGL(knn_topk_outlier_kernel, dim3(gx, (unsigned)c.m), dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.n_outliers, c.base,
                           rs.outliers, rs.ctl, c.cand, c.ccount, c.ccap, c.gids);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    hipLaunchKernelGGL(knn_topk_select_cand_kernel, dim3((unsigned)c.m), dim3(KNN_WAVE), 0, s, (const u64 *)c.cand,
                       (const unsigned *)c.ccount, c.ccap, c.K, c.keys, c.init, (const unsigned *)(rs.ctl + KNN_CTL_FALLBACK));
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Counts within a radius (knn_index_count_within; DESIGN §4.6 "Counts within a radius").
//
// knn_exact_count_kernel<KC> — the skeleton of knn_exact_topk_kernel without its list: one wave per block, lanes = queries
// (coordinates in VGPRs), rows of the block's slice as wave-uniform scalar loads, v0's arithmetic.  A row counts for a lane when
// its distance E is finite and E <= max_dist2 (fp32 compare, equality inside: the candidate rule of knn_index_query_topk_within).
// Each lane keeps ONE counter register and adds it to counts[q] once, at the end of the slice, when it is not zero: no LDS, no
// list, no atomic per hit.  Integer adds: the result does not depend on the order the slices arrive in.
// KC = chunks of 16 dimensions held in VGPRs (k <= 128); KC = 0: any k, the query's coordinates re-read from memory.
// gate (nullable): returns at once when *gate == 0 (the fallback of the grid way and of a cell-pruned pass).
// ------------------------------------------------------------------------------------------
template <int KC>
__global__ __launch_bounds__(KNN_WAVE) void knn_exact_count_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                  int m, long long n, long long rows_per_slice, float max_dist2,
                                                                  unsigned *__restrict__ counts, const unsigned *__restrict__ gate)
{
#pragma clang fp contract(off)
    if (gate && *gate == 0u)
        return;
    constexpr int KM = KC > 0 ? 16 * KC : 1;
    const int lane = threadIdx.x;
    const int q = blockIdx.y * KNN_WAVE + lane;
    const int qa = min(q, m - 1);
    float qv[KM];
#pragma unroll
    for (int d = 0; d < KM; ++d)
        qv[d] = KC > 0 && d < k ? Q[(size_t)qa * k + d] : 0.0f;
    unsigned cnt = 0u;
    const long long i0 = (long long)blockIdx.x * rows_per_slice;
    const long long i1 = min(n, i0 + rows_per_slice);
    const float *__restrict__ r = R + (size_t)i0 * k;
    const float *__restrict__ qp = Q + (size_t)qa * k;
    for (long long i = i0; i < i1; ++i, r += k) {
        float acc = 0.0f;   // (lane_row_dist2's arithmetic, knn_exact_dev.h, in this kernel's own text)
        if (KC > 0) {
#pragma unroll
            for (int c = 0; c < (KC > 0 ? KC : 1); ++c) {
                const int rem = k - 16 * c;   // wave-uniform
                if (rem >= 16) {
                    float rv[16];
#pragma unroll
                    for (int j = 0; j < 16; ++j)
                        rv[j] = r[16 * c + j];   // wave-uniform address -> scalar loads
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const float diff = qv[16 * c + j] - rv[j];
                        const float sq = diff * diff;
                        acc = acc + sq;
                    }
                } else if (rem > 0) {
#pragma unroll
                    for (int j = 0; j < 15; ++j)
                        if (j < rem) {
                            const float diff = qv[16 * c + j] - r[16 * c + j];
                            const float sq = diff * diff;
                            acc = acc + sq;
                        }
                }
            }
        } else {
            for (int d = 0; d < k; ++d) {
                const float diff = qp[d] - r[d];
                const float sq = diff * diff;
                acc = acc + sq;
            }
        }
        cnt += acc < INFINITY && acc <= max_dist2 ? 1u : 0u;   // (NaN fails both compares)
    }
    if (q < m && cnt != 0u)
        atomicAdd(&counts[q], cnt);
}

// counts[j] += scratch[j] unless *giveup != 0: what the grid way or a cell-pruned pass counted is committed only when nothing
// handed the batch to the exact count, which runs under the opposite gate on the same word — one of the two adds, never both.
__global__ __launch_bounds__(KNN_BLOCK) void knn_count_commit_kernel(const unsigned *__restrict__ scratch, int m,
                                                                    unsigned *__restrict__ counts, const unsigned *__restrict__ giveup)
{
    if (*giveup != 0u)
        return;
    const int j = blockIdx.x * KNN_BLOCK + threadIdx.x;
    if (j < m)
        counts[j] += scratch[j];
}

// The cell-pruned count's re-rank and out-of-box rows, scalar radius: knn_rec_count_rerank_body.inc, knn_rec_count_outlier_body.inc
// (the walks the each-forms, knn_each.hip, and the self forms, knn_self_routed.hip, include too).  What a scalar form lacks:
#define KNN_REC_SCALAR_FORM                  \
    constexpr int FORM = KNN_REC_SCALAR;     \
    constexpr const float *radii = nullptr;  \
    constexpr unsigned first = 0u;           \
    constexpr const unsigned *mask = nullptr; \
    const float cap = max_dist2
__global__ __launch_bounds__(KNN_BLOCK) void knn_count_rerank_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                    long long n, const u64 *__restrict__ rec,
                                                                    const unsigned *__restrict__ counts, unsigned nlists,
                                                                    unsigned slice, unsigned *__restrict__ ctl,
                                                                    const unsigned *__restrict__ perm, const float *__restrict__ norms,
                                                                    float max_dist2, unsigned *__restrict__ qcount)
{
    KNN_REC_SCALAR_FORM;
#include "knn_rec_count_rerank_body.inc"
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_count_outlier_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                     unsigned count, const unsigned *__restrict__ list,
                                                                     const unsigned *__restrict__ ctl, float max_dist2,
                                                                     unsigned *__restrict__ qcount)
{
#pragma clang fp contract(off)
    KNN_REC_SCALAR_FORM;
#include "knn_rec_count_outlier_body.inc"
}

long long knn_count_slices(int mc, long long n, int num_cu)
{
    const unsigned qg = (unsigned)knn_divup(mc, KNN_WAVE);
    long long slices = (long long)num_cu * 32 / qg;
    const long long by_rows = (n + 1023) / 1024;
    if (slices > by_rows)
        slices = by_rows;
    if (slices > 65535)
        slices = 65535;
    if (slices < 1)
        slices = 1;
    const long long per = (n + slices - 1) / slices;
    return (n + per - 1) / per;
}

// (knn_exact_count_launch and knn_exact_list_launch: at the end of this file, behind the each-forms of their kernels)

hipError_t knn_count_commit_launch(int m, const unsigned *scratch, unsigned *counts, const unsigned *giveup, hipStream_t s)
{
    if (m <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(knn_count_commit_kernel, dim3((unsigned)knn_divup(m, KNN_BLOCK)), dim3(KNN_BLOCK), 0, s, scratch, m, counts, giveup);
    return hipGetLastError();
}

hipError_t knn_count_records_finish(const CountCall &c, const TopkRecords &rs, unsigned *qcount)
{
    hipStream_t s = c.stream;
    if (rs.rec_rows || !rs.perm || !rs.pos_norms || !qcount)
        return hipErrorInvalidValue;
    if (c.mask)
        return knn_count_masked_records_finish(c, rs, qcount);   // (knn_masked_routed.hip)
    if (c.self_first >= 0)
        return knn_count_self_records_finish(c, rs, qcount);   // (knn_self_routed.hip)
    if (c.radii)
        return knn_count_each_records_finish(c, rs, qcount);   // (knn_each.hip)
    return knn_records_finish_launches(
        rs, c.m,
        [&](dim3 grid, const u64 *rec, const unsigned *counts, unsigned nlists, unsigned slice) {
            hipLaunchKernelGGL(knn_count_rerank_kernel, grid, dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, rec, counts, nlists, slice,
                               rs.ctl, rs.perm, rs.pos_norms, c.max_dist2, qcount);
        },
        [&](dim3 grid) {
            hipLaunchKernelGGL(knn_count_outlier_kernel, grid, dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.n_outliers, rs.outliers,
                               (const unsigned *)rs.ctl, c.max_dist2, qcount);
        },
        [&] { return knn_count_commit_launch(c.m, qcount, c.counts, rs.ctl + KNN_CTL_FALLBACK, s); });
}

// ------------------------------------------------------------------------------------------
// Lists within a radius (knn_index_list_within; DESIGN §4.6 "Lists within a radius"): the second pass of count -> offsets -> fill.
//
// A hit — a row whose v0 distance E is finite and E <= max_dist2, knn_exact_count_kernel's rule — reserves place p of its query's
// segment with one atomicAdd on the query's cursor and, when p is below the segment's room, stores its packed key at
// keys[offsets[q] + p]: one 8-byte vector store.  The cursor counts every hit, stored or not, so a cursor above the room is how the
// caller sees an overflow; nothing is stored outside [offsets[q], offsets[q + 1]).  (list_room, list_put: knn_exact_dev.h, shared
// with the list scan over a subset of the rows, knn_masked_lists.hip.)
// ------------------------------------------------------------------------------------------
// knn_exact_list_kernel<KC> — knn_exact_count_kernel's skeleton: one wave per block, lanes = queries (coordinates in VGPRs), rows
// of the block's slice as wave-uniform scalar loads, v0's arithmetic; KC and gate as there.  On a hit the lane reserves and stores
// (list_put) instead of adding to a register: hits are sparse at the radii the call is meant for, so no staging in LDS.
// gids (nullable; cell-range shards, where base is 0): the key's index half is gids[row], else base + row.
template <int KC>
__global__ __launch_bounds__(KNN_WAVE) void knn_exact_list_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                 int m, long long n, long long rows_per_slice, float max_dist2,
                                                                 long long base, const unsigned *__restrict__ gids,
                                                                 const u64 *__restrict__ offsets, unsigned *__restrict__ fill,
                                                                 u64 *__restrict__ keys, const unsigned *__restrict__ gate)
{
#pragma clang fp contract(off)
    if (gate && *gate == 0u)
        return;
    constexpr int KM = KC > 0 ? 16 * KC : 1;
    const int lane = threadIdx.x;
    const int q = blockIdx.y * KNN_WAVE + lane;
    const int qa = min(q, m - 1);
    float qv[KM];
#pragma unroll
    for (int d = 0; d < KM; ++d)
        qv[d] = KC > 0 && d < k ? Q[(size_t)qa * k + d] : 0.0f;
    u64 off;
    const unsigned room = list_room(offsets, (unsigned)qa, off);
    const long long i0 = (long long)blockIdx.x * rows_per_slice;
    const long long i1 = min(n, i0 + rows_per_slice);
    const float *__restrict__ r = R + (size_t)i0 * k;
    const float *__restrict__ qp = Q + (size_t)qa * k;
    for (long long i = i0; i < i1; ++i, r += k) {
        float acc = 0.0f;   // (lane_row_dist2's arithmetic, knn_exact_dev.h, in this kernel's own text)
        if (KC > 0) {
#pragma unroll
            for (int c = 0; c < (KC > 0 ? KC : 1); ++c) {
                const int rem = k - 16 * c;   // wave-uniform
                if (rem >= 16) {
                    float rv[16];
#pragma unroll
                    for (int j = 0; j < 16; ++j)
                        rv[j] = r[16 * c + j];   // wave-uniform address -> scalar loads
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const float diff = qv[16 * c + j] - rv[j];
                        const float sq = diff * diff;
                        acc = acc + sq;
                    }
                } else if (rem > 0) {
#pragma unroll
                    for (int j = 0; j < 15; ++j)
                        if (j < rem) {
                            const float diff = qv[16 * c + j] - r[16 * c + j];
                            const float sq = diff * diff;
                            acc = acc + sq;
                        }
                }
            }
        } else {
            for (int d = 0; d < k; ++d) {
                const float diff = qp[d] - r[d];
                const float sq = diff * diff;
                acc = acc + sq;
            }
        }
        if (q < m && acc < INFINITY && acc <= max_dist2)   // (NaN fails both compares)
            list_put(&fill[q], keys, off, room, pack_key(acc, gids ? gids[i] : (unsigned)(base + i)));
    }
}

// fill[j] = cursor[j] unless *giveup != 0: the places the grid way or a cell-pruned pass reserved in the scratch cursor become the
// caller's only when nothing handed the batch to the exact list, which runs under the opposite gate from the untouched fill over
// the same places — one of the two moves the caller's cursor, never both.
__global__ __launch_bounds__(KNN_BLOCK) void knn_list_commit_kernel(const unsigned *__restrict__ cursor, int m,
                                                                   unsigned *__restrict__ fill, const unsigned *__restrict__ giveup)
{
    if (*giveup != 0u)
        return;
    const int j = blockIdx.x * KNN_BLOCK + threadIdx.x;
    if (j < m)
        fill[j] = cursor[j];
}

// The cell-pruned list's re-rank and out-of-box rows, scalar radius: knn_rec_list_rerank_body.inc, knn_rec_list_outlier_body.inc.
__global__ __launch_bounds__(KNN_BLOCK) void knn_list_rerank_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                   long long n, long long base, const u64 *__restrict__ rec,
                                                                   const unsigned *__restrict__ counts, unsigned nlists,
                                                                   unsigned slice, unsigned *__restrict__ ctl,
                                                                   const unsigned *__restrict__ perm, const float *__restrict__ norms,
                                                                   float max_dist2, const unsigned *__restrict__ gids,
                                                                   const u64 *__restrict__ offsets, unsigned *__restrict__ cursor,
                                                                   u64 *__restrict__ keys)
{
    KNN_REC_SCALAR_FORM;
#include "knn_rec_list_rerank_body.inc"
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_list_outlier_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                    unsigned count, long long base, const unsigned *__restrict__ list,
                                                                    const unsigned *__restrict__ ctl, float max_dist2,
                                                                    const unsigned *__restrict__ gids, const u64 *__restrict__ offsets,
                                                                    unsigned *__restrict__ cursor, u64 *__restrict__ keys)
{
#pragma clang fp contract(off)
    KNN_REC_SCALAR_FORM;
#include "knn_rec_list_outlier_body.inc"
}
#undef KNN_REC_SCALAR_FORM

// offsets[0] = 0, offsets[j + 1] = offsets[j] + counts[j]: ONE block walks the counts in chunks of 8 per thread and carries a 64-bit
// running sum from chunk to chunk (m is small next to n: no multi-block scan).  Per chunk: a thread sums its 8 counts, the waves
// scan the thread sums by shuffles, the wave totals meet in LDS.
__global__ __launch_bounds__(KNN_BLOCK) void knn_counts_to_offsets_kernel(const unsigned *__restrict__ counts, int m,
                                                                         u64 *__restrict__ offsets)
{
#include "knn_counts_to_offsets_body.inc"
}

// One block per segment: the first cnt = min(fill, room) keys ascending, by a bitonic network whose comparators all put the smaller
// key at the lower place (a merge of 2h keys opens with the mirror step i <-> i ^ (2h - 1), then halves as usual).  With every
// comparator pointing the same way the places from cnt up to the next power of two behave as +INF padding that never moves, so a
// comparator whose upper place is >= cnt is simply skipped: any length sorts, nothing beyond cnt is read or written.  Equal keys are
// never exchanged.  cnt <= KNN_SORT_LDS_KEYS: in LDS (32 KB); beyond: the same network on the segment in global memory, the block's
// barriers ordering its own stores and loads.  (sort_network: knn_exact_dev.h — the large top-K sorts its lists with it too.)
__global__ __launch_bounds__(KNN_BLOCK) void knn_keys_sort_segments_kernel(const u64 *__restrict__ offsets,
                                                                          const unsigned *__restrict__ fill, u64 *keys)
{
    __shared__ u64 lds[KNN_SORT_LDS_KEYS];
    const unsigned seg = blockIdx.x;
    u64 off;
    const unsigned room = list_room(offsets, seg, off);
    const unsigned cnt = min(fill[seg], room);   // block-uniform
    if (cnt < 2u)
        return;
    u64 *a = keys + off;
    if (cnt <= KNN_SORT_LDS_KEYS) {
        for (unsigned i = threadIdx.x; i < cnt; i += KNN_BLOCK)
            lds[i] = a[i];
        __syncthreads();
        sort_network(lds, cnt);
        for (unsigned i = threadIdx.x; i < cnt; i += KNN_BLOCK)
            a[i] = lds[i];
    } else {
        sort_network(a, cnt);
    }
}

hipError_t knn_list_commit_launch(int m, const unsigned *cursor, unsigned *fill, const unsigned *giveup, hipStream_t s)
{
    if (m <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(knn_list_commit_kernel, dim3((unsigned)knn_divup(m, KNN_BLOCK)), dim3(KNN_BLOCK), 0, s, cursor, m, fill, giveup);
    return hipGetLastError();
}

hipError_t knn_list_records_finish(const ListCall &c, const TopkRecords &rs)
{
    hipStream_t s = c.stream;
    if (rs.rec_rows || !rs.perm || !rs.pos_norms || !c.scratch)
        return hipErrorInvalidValue;
    if (c.mask)
        return knn_list_masked_records_finish(c, rs);   // (knn_masked_routed.hip)
    if (c.self_first >= 0)
        return knn_list_self_records_finish(c, rs);   // (knn_self_routed.hip)
    if (c.radii)
        return knn_list_each_records_finish(c, rs);   // (knn_each.hip)
    return knn_records_finish_launches(
        rs, c.m,
        [&](dim3 grid, const u64 *rec, const unsigned *counts, unsigned nlists, unsigned slice) {
            hipLaunchKernelGGL(knn_list_rerank_kernel, grid, dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, c.base, rec, counts, nlists,
                               slice, rs.ctl, rs.perm, rs.pos_norms, c.max_dist2, c.gids, c.offsets, c.scratch, c.keys);
        },
        [&](dim3 grid) {
            hipLaunchKernelGGL(knn_list_outlier_kernel, grid, dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.n_outliers, c.base, rs.outliers,
                               (const unsigned *)rs.ctl, c.max_dist2, c.gids, c.offsets, c.scratch, c.keys);
        },
        [&] { return knn_list_commit_launch(c.m, c.scratch, c.fill, rs.ctl + KNN_CTL_FALLBACK, s); });
}

hipError_t knn_counts_to_offsets_launch(const unsigned *counts, int m, u64 *offsets, hipStream_t s)
{
    if (m <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(knn_counts_to_offsets_kernel, dim3(1), dim3(KNN_BLOCK), 0, s, counts, m, offsets);
    return hipGetLastError();
}

hipError_t knn_keys_sort_segments_launch(int m, const u64 *offsets, const unsigned *fill, u64 *keys, hipStream_t s)
{
    if (m <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(knn_keys_sort_segments_kernel, dim3((unsigned)m), dim3(KNN_BLOCK), 0, s, offsets, fill, keys);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// A radius per query (include/knn_mi355x.h 2j; DESIGN §4.6 "A radius per query"): the each-forms of the count and list kernels.
// A row is a hit for query j when its v0 distance E is finite, E <= radii[j] and E <= cap — two fp32 compares, equality inside; a
// NaN or negative radius fails the first for every row.  The kernels are their scalar twins with the radius read per query;
// the launchers behind them launch these for a call that carries radii (CountCall::radii, ListCall::radii; max_dist2 is then the cap).
// ------------------------------------------------------------------------------------------
// knn_exact_count_each_kernel<KC> — knn_exact_count_kernel<KC>'s skeleton (lane_row_dist2, knn_exact_dev.h, holds its row lines):
// the lanes ARE the queries, so the lane loads its own radius once and the compare reads a VGPR where the twin reads an SGPR.  gate as there.
template <int KC>
__global__ __launch_bounds__(KNN_WAVE) void knn_exact_count_each_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                       int m, long long n, long long rows_per_slice,
                                                                       const float *__restrict__ radii, float cap,
                                                                       unsigned *__restrict__ counts, const unsigned *__restrict__ gate)
{
#pragma clang fp contract(off)
    if (gate && *gate == 0u)
        return;
    constexpr int KM = KC > 0 ? 16 * KC : 1;
    const int lane = threadIdx.x;
    const int q = blockIdx.y * KNN_WAVE + lane;
    const int qa = min(q, m - 1);
    const float *__restrict__ qp = Q + (size_t)qa * k;
    float qv[KM];
#pragma unroll
    for (int d = 0; d < KM; ++d)
        qv[d] = KC > 0 && d < k ? qp[d] : 0.0f;
    const float rad = radii[qa];
    unsigned cnt = 0u;
    const long long i0 = (long long)blockIdx.x * rows_per_slice;
    const long long i1 = min(n, i0 + rows_per_slice);
    const float *__restrict__ r = R + (size_t)i0 * k;
    for (long long i = i0; i < i1; ++i, r += k) {
        const float acc = lane_row_dist2<KC>(qv, qp, r, k);
        cnt += acc < INFINITY && acc <= rad && acc <= cap ? 1u : 0u;   // (NaN — the distance or the radius — fails)
    }
    if (q < m && cnt != 0u)
        atomicAdd(&counts[q], cnt);
}

// knn_exact_list_each_kernel<KC> — knn_exact_list_kernel<KC> with the lane's own radius, as the count form.
template <int KC>
__global__ __launch_bounds__(KNN_WAVE) void knn_exact_list_each_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                      int m, long long n, long long rows_per_slice,
                                                                      const float *__restrict__ radii, float cap, long long base,
                                                                      const unsigned *__restrict__ gids,
                                                                      const u64 *__restrict__ offsets, unsigned *__restrict__ fill,
                                                                      u64 *__restrict__ keys, const unsigned *__restrict__ gate)
{
#pragma clang fp contract(off)
    if (gate && *gate == 0u)
        return;
    constexpr int KM = KC > 0 ? 16 * KC : 1;
    const int lane = threadIdx.x;
    const int q = blockIdx.y * KNN_WAVE + lane;
    const int qa = min(q, m - 1);
    const float *__restrict__ qp = Q + (size_t)qa * k;
    float qv[KM];
#pragma unroll
    for (int d = 0; d < KM; ++d)
        qv[d] = KC > 0 && d < k ? qp[d] : 0.0f;
    const float rad = radii[qa];
    u64 off;
    const unsigned room = list_room(offsets, (unsigned)qa, off);
    const long long i0 = (long long)blockIdx.x * rows_per_slice;
    const long long i1 = min(n, i0 + rows_per_slice);
    const float *__restrict__ r = R + (size_t)i0 * k;
    for (long long i = i0; i < i1; ++i, r += k) {
        const float acc = lane_row_dist2<KC>(qv, qp, r, k);
        if (q < m && acc < INFINITY && acc <= rad && acc <= cap)   // (NaN — the distance or the radius — fails)
            list_put(&fill[q], keys, off, room, pack_key(acc, gids ? gids[i] : (unsigned)(base + i)));
    }
}

// The count scan and the list scan: the queries in chunks, the rows in the count rule's slices.  A call with radii takes the each
// kernel, its radii advancing with the queries chunk by chunk; gate: both forms carry it.
hipError_t knn_exact_count_launch(const CountCall &c, const unsigned *gate)
{
    if (c.m <= 0 || c.n <= 0)
        return hipSuccess;
    hipStream_t s = c.stream;
    return knn_slice_chunks(c.m, c.n, c.num_cu, KnnCountSlices{}, [&](const SliceChunk &ch) {
        const int mc = ch.mc;
        const long long c0 = ch.c0, per = ch.per;
        const dim3 grid = ch.grid, block(KNN_WAVE);
        const float *qc = c.q + (size_t)c0 * c.k;
#define KNN_COUNT_SCAN(KCV)                                                                                                           \
    if (c.radii)                                                                                                                      \
        hipLaunchKernelGGL(knn_exact_count_each_kernel<KCV>, grid, block, 0, s, qc, c.r, c.k, mc, c.n, per, c.radii + c0, c.max_dist2, \
                           c.counts + c0, gate);                                                                                      \
    else                                                                                                                              \
        hipLaunchKernelGGL(knn_exact_count_kernel<KCV>, grid, block, 0, s, qc, c.r, c.k, mc, c.n, per, c.max_dist2, c.counts + c0, gate)
        KNN_KC_SWITCH(c.k, KNN_COUNT_SCAN)
#undef KNN_COUNT_SCAN
        return hipGetLastError();
    });
}

hipError_t knn_exact_list_launch(const ListCall &c, const unsigned *gate)
{
    if (c.m <= 0 || c.n <= 0)
        return hipSuccess;
    hipStream_t s = c.stream;
    return knn_slice_chunks(c.m, c.n, c.num_cu, KnnCountSlices{}, [&](const SliceChunk &ch) {
        const int mc = ch.mc;
        const long long c0 = ch.c0, per = ch.per;
        const dim3 grid = ch.grid, block(KNN_WAVE);
        const float *qc = c.q + (size_t)c0 * c.k;
#define KNN_LIST_SCAN(KCV)                                                                                                           \
    if (c.radii)                                                                                                                     \
        hipLaunchKernelGGL(knn_exact_list_each_kernel<KCV>, grid, block, 0, s, qc, c.r, c.k, mc, c.n, per, c.radii + c0, c.max_dist2, \
                           c.base, c.gids, c.offsets + c0, c.fill + c0, c.keys, gate);                                               \
    else                                                                                                                             \
        hipLaunchKernelGGL(knn_exact_list_kernel<KCV>, grid, block, 0, s, qc, c.r, c.k, mc, c.n, per, c.max_dist2, c.base, c.gids,    \
                           c.offsets + c0, c.fill + c0, c.keys, gate)
        KNN_KC_SWITCH(c.k, KNN_LIST_SCAN)
#undef KNN_LIST_SCAN
        return hipGetLastError();
    });
}
