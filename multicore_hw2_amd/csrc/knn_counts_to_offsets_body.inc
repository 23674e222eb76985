// knn_counts_to_offsets_body.inc — the one block of knn_counts_to_offsets_kernel (knn_exact.hip; the description is there) and of
// its gated twin knn_mask_prefix_gated_kernel (knn_masked.hip).  The including kernel provides counts, m and offsets by their names
// and runs as ONE block of KNN_BLOCK threads, every thread of which arrives here.
    __shared__ u64 wave_total[KNN_WAVES];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    u64 running = 0ull;
    if (threadIdx.x == 0)
        offsets[0] = 0ull;
    for (long long c0 = 0; c0 < m; c0 += (long long)KNN_BLOCK * KNN_OFFSETS_PER_THREAD) {
        const long long j0 = c0 + (long long)threadIdx.x * KNN_OFFSETS_PER_THREAD;
        unsigned v[KNN_OFFSETS_PER_THREAD];
        u64 mine = 0ull;
#pragma unroll
        for (int t = 0; t < KNN_OFFSETS_PER_THREAD; ++t) {
            v[t] = j0 + t < m ? counts[j0 + t] : 0u;
            mine += v[t];
        }
        u64 incl = mine;   // inclusive scan of the thread sums within the wave
#pragma unroll
        for (int d = 1; d < KNN_WAVE; d <<= 1) {
            const u64 o = __shfl_up(incl, d, KNN_WAVE);
            if (lane >= (unsigned)d)
                incl += o;
        }
        if (lane == KNN_WAVE - 1)
            wave_total[wave] = incl;
        __syncthreads();
        u64 before = running, total = 0ull;
#pragma unroll
        for (unsigned w = 0; w < KNN_WAVES; ++w) {
            before += w < wave ? wave_total[w] : 0ull;
            total += wave_total[w];
        }
        u64 sum = before + incl - mine;   // everything ahead of this thread's first count
#pragma unroll
        for (int t = 0; t < KNN_OFFSETS_PER_THREAD; ++t) {
            sum += v[t];
            if (j0 + t < m)
                offsets[j0 + t + 1] = sum;
        }
        running += total;
        __syncthreads();   // (wave_total is rewritten by the next chunk)
    }
