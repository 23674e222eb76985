// knn_grid_topk_body.inc — the body of the grid's top-K kernels (knn_grid.hip has the description): included into
// knn_grid_topk_kernel<KD> (WR = false) and into knn_grid_within_kernel<KD>, its radius form (WR = true, max_dist2 >= 0, finite or
// +INF), which takes one argument more.  The including kernel provides KD, the arguments of knn_grid_topk_kernel by their names,
// and the constants WR and max_dist2.
    if (blockIdx.x == 0 && threadIdx.x == 0)
        *giveup_next = 0u;   // (the slot's other word, as the 1-NN kernel)
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * (GRID_BLOCK / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (qi >= m)
        return;
    u64 *__restrict__ o = out + (size_t)qi * KK;
    u64 list = lane < KK ? kKeyInit : ~0ull;
    float q[4] = {0.f, 0.f, 0.f, 0.f};
    bool finite = true;
#pragma unroll
    for (int d = 0; d < KD; ++d) {
        q[d] = Q[(size_t)qi * KD + d];
        finite = finite && fabsf(q[d]) < INFINITY;
    }
    if (!finite) {   // every distance is NaN or +INF: no row is a candidate (and nothing to give up on)
        if (lane < KK)
            o[lane] = kKeyInit;
        return;
    }
    int c[4];
    (void)grid_cell_of(gg, q, c);
    int gmax = 1;
#pragma unroll
    for (int d = 0; d < KD; ++d)
        gmax = gg.g[d] > gmax ? gg.g[d] : gmax;

    u64 kth = kKeyInit;
    const u64 lim = WR ? ((u64)__float_as_uint(max_dist2) + 1ull) << 32 : ~0ull;   // (WR: max_dist2 >= 0, finite or +INF)
    bool done = false;
    bool first = true;
    for (int r = gmax > 1 ? 1 : 0; r < gmax && r <= rmax; ++r) {
        const int side = 2 * r + 1;
        int total = 1;
#pragma unroll
        for (int d = 0; d < KD; ++d)
            total *= side;
        int shift = 0;   // split = 1 << shift lanes per cell
        while ((total << (shift + 1)) <= KNN_WAVE)
            ++shift;
        const int sub = lane & ((1 << shift) - 1), step = 1 << shift, per = KNN_WAVE >> shift;
        for (int idx0 = 0; idx0 < total; idx0 += per) {
            const int idx = idx0 + (lane >> shift);
            unsigned p = 0u, p1 = 0u, cell;
            if (idx < total && grid_ring_cell<KD>(gg, c, r, side, idx, first, &cell)) {
                p = start[cell] + (unsigned)sub;
                p1 = start[cell + 1];
            }
            while (__ballot(p < p1) != 0ull) {
                u64 key = ~0ull;
                if (p < p1) {
                    const f4g x = pts[p];
                    float acc = 0.0f;
#pragma unroll
                    for (int d = 0; d < KD; ++d) {
                        const float diff = q[d] - x[d];   // v0: search - reference, squared, summed in order
                        const float sq = diff * diff;
                        acc = acc + sq;
                    }
                    if (acc < INFINITY)                   // NaN / +INF never beat +INF (v0's strict >)
                        key = ((u64)__float_as_uint(acc) << 32) | (u64)(unsigned)(base + orig[p]);
                }
                p += (unsigned)step;
                u64 pend = __ballot(key < kth && (!WR || key < lim));
                while (pend != 0ull) {
                    const int src = __builtin_ctzll(pend);
                    pend &= pend - 1ull;
                    const u64 cand = grid_readlane64(key, src);
                    if (cand < kth) {   // (the K-th key may have come down since the ballot; the limit does not move)
                        const int pos = __popcll(__ballot(list < cand));
                        const u64 up = __shfl_up(list, 1, KNN_WAVE);
                        if (lane < KK)
                            list = lane < pos ? list : lane == pos ? cand : up;
                        kth = grid_readlane64(list, KK - 1);
                    }
                }
            }
        }
        first = false;
        bool covers_all;
        const double lb = grid_face_bound<KD>(gg, c, q, r, &covers_all);
        if (covers_all) {   // (the list may hold fewer than KK real keys: the rest stay KNN_KEY_INIT)
            done = true;
            break;
        }
        if (lb > 0.0 && kth < kKeyInit) {
            const float kd = __uint_as_float((unsigned)(kth >> 32));
            if ((double)kd < lb * lb * (1.0 - 1e-6)) {
                done = true;
                break;
            }
        }
        if (WR && lb > 0.0 && (double)max_dist2 < lb * lb * (1.0 - 1e-6)) {   // no unseen row is within the radius
            done = true;
            break;
        }
    }
    if (lane < KK)
        o[lane] = list;
    if (lane == 0 && !done && gmax > rmax + 1)
        *giveup = 1u;      // benign race: every writer stores 1
