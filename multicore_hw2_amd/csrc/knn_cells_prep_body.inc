// knn_cells_prep_body.inc — the body of the cell-pruned path's preparation kernel (knn_cells.hip has the description), included
// into knn_cells_prep_kernel<PW, SD, KT, CTR, TK> and into knn_cells_prep_within_kernel<PW, SD, KT>, the radius form of the top-K
// prep kernel, which takes one argument more.  The including kernel provides the template parameters PW, SD, KT, the arguments of
// knn_cells_prep_kernel by their names, and the constants CTR, TK, WR, CNT and max_dist2 (WR only: finite, >= 0).  CNT (with WR:
// knn_index_count_within, knn_cells_prep_count_kernel): the count form, which scores no seed tile at all.  EACH (with CNT:
// knn_index_count_within_each, knn_cells_prep_each_kernel): max_dist2 is the block's OWN query's bound (knn_each_radius.h), or
// negative when the query has no candidates — it is then listed for no cell and sends nothing to the exact count.
    static_assert(!WR || (TK && !CTR), "the radius form is a top-K form of the one-frame layouts");
    static_assert(!CNT || WR, "the count form is a radius form");
    static_assert(!EACH || CNT, "the form with a radius per query is a count form");
    constexpr int SEEDS = 1 << SD, NS = SEEDS / PW;   // seed cells in all, per wave
    // seed tiles a wave requests at once (KT KiB each); TK: fewer — the selection network's registers come on top of the tiles in
    // flight, and the form must stay within its 1-NN twin's registers without scratch (a top-K call is worth milliseconds: the
    // extra round trips of its prep kernel are not what it is made of)
    constexpr int PREP_TILES = TK ? (KT == 1 ? 4 : 3) : KT == 1 ? CELL_PREP_TILES : 6;
    __shared__ float s_gap[16][CELL_MAX_BINS];
    __shared__ float s_red[PW];
    // WR: the radius waits in LDS for the thread that makes the threshold at the very end — kept in a register across the whole
    // kernel it cost the form scratch its twin does not have
    __shared__ float s_radius;
    if (WR && threadIdx.x == 0)
        s_radius = max_dist2;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qi = blockIdx.x;
    // housekeeping folded in here to save launches: the record counters of the scan, the control words of the NEXT
    // batch on this slot (calls on a slot are stream-ordered; this batch's own words were cleared by the previous one)
    for (unsigned i = blockIdx.x * (64u * PW) + (unsigned)tid; i < nlists; i += gridDim.x * (64u * PW))
        counts[i] = 0u;
    if (blockIdx.x == 0 && tid == 0) {
        ctl_next[KNN_CTL_FALLBACK] = 0u;
        ctl_next[KNN_CTL_RECORDS] = 0u;
        ctl_next[KNN_CTL_WIDE_SEEDS] = 0u;
        ctl_next[KNN_CTL_DENSE_CELLS] = 0u;
        ctl_next[KNN_CTL_EXACT_CELLS] = 0u;
        ctl_next[KNN_CTL_SCAN_DONE] = 0u;
        ctl_next[KNN_CTL_DEFERRED] = 0u;
        ctl_next[KNN_CTL_TAIL_DONE] = 0u;
        ctl_next[KNN_CTL_TOTAL] = 0u;
    }
    const int half = lane >> 5;
    const size_t frag_at = (size_t)(qi >> 5) * 64 * KT + (size_t)half * 32 + (size_t)(qi & 31);   // (+ 64 per K-step)
    if (qi >= m) {   // padding query of the last tile (block-uniform): never listed, never passes
        if (wib == 0 && (lane & 31) == 0) {
#pragma unroll
            for (int t = 0; t < KT; ++t)
                qfg[frag_at + 64 * t] = (h8){0, 0, 0, 0, 0, 0, 0, 0};
        }
        if (tid == 0) {
            thr[qi] = -INFINITY;
            dup_out[qi] = -INFINITY;
        }
        return;
    }
    if (keys_init && tid == 0)
        keys_init[qi] = kKeyInit;

    // ---- the query as an fp16 B operand (what knn_frag_kernel writes for a query row: centred, scaled, rounded,
    // times -2), its norm and largest coordinate.  Every lane does the whole row: the loads are wave-uniform.
    const float *__restrict__ qrow = Q + (size_t)qi * g.k;
    float nrm = 0.0f, amax = 0.0f;
    bool qbad = false;
    h8 bq[KT];
#pragma unroll
    for (int d = 0; d < 16 * KT; ++d) {
        float sc = 0.0f;
        if (d < g.k)
            sc = (qrow[d] - center[d]) * sigma;   // fp32 subtract, exact power-of-two scale
        const _Float16 hval = (_Float16)sc;       // round to nearest even
        const float back = (float)hval;
        qbad = qbad || !(fabsf(back) < INFINITY);
        amax = fmaxf(amax, fabsf(back));
        nrm = nrm + back * back;                  // exact products, fp32 sum in dimension order
        const _Float16 v = (_Float16)(back * -2.0f);
        qbad = qbad || !(fabsf((float)v) < INFINITY);
        if (((d >> 3) & 1) == half)
            bq[d >> 4][d & 7] = v;
    }
    if (wib == 0 && (lane & 31) == 0) {
#pragma unroll
        for (int t = 0; t < KT; ++t)
        {
            h8 o = bq[t];
            if (KT == 2 && t == 1 && half == 1 && g.k <= KNN_NIF_MAX_K) {   // K-slots 30, 31 of the scan's B operand: 1, 2^-11 (x the norm's halves)
                o[6] = (_Float16)1.0f;
                o[7] = __builtin_bit_cast(_Float16, (unsigned short)0x1000u);
            }
            qfg[frag_at + 64 * t] = o;   // for the scan (lanes 0 and 32 hold the two halves of every K-step)
        }
    }

    // ---- squared gaps to every bin of every dimension (scaled units, rounded down): 256 entries over the block's threads
    for (int e = tid; e < 256; e += 64 * PW) {
        const int d = e >> 4, b = e & 15;
        float v = 0.0f;
        if (d < g.k && g.nb[d] && b < (1 << g.nb[d])) {   // (d < 16: e < 256)
            const int nbins = 1 << g.nb[d];
            const float *__restrict__ bnd = bounds + d * (CELL_MAX_BINS - 1);
            const double q = (double)qrow[d];
            double gap = 0.0;
            if (b > 0 && (double)bnd[b - 1] > q)
                gap = (double)bnd[b - 1] - q;        // rows of the bin have x >= bnd[b-1] > q
            if (b < nbins - 1 && q > (double)bnd[b])
                gap = q - (double)bnd[b];            // rows of the bin have x < bnd[b] < q
            v = __double2float_rd(gap * gap * sigma2);
        }
        s_gap[d][b] = v;
    }
    // ---- seed cells (every wave works them out; wave w then takes cells w, w + PW, ...): dimensions on the lanes — the
    // query's own bin and the neighbouring bin nearest to it
    unsigned bin = 0u, alt = 0xFFFFFFFFu, nbl = 0u, shl = 0u;
    float ag = INFINITY;
    if (lane < g.k && lane < 16) {   // (the cells cut the first 16 dimensions)
        nbl = g.nb[lane];
        shl = g.shift[lane];
    }
    if (nbl) {
        const int nbins = 1 << nbl;
        const float *__restrict__ bnd = bounds + lane * (CELL_MAX_BINS - 1);
        const float q = qrow[lane];
        bin = cell_bin(bnd, nbins, q);
        if (bin > 0u) {
            alt = bin - 1u;
            ag = q - bnd[bin - 1];
        }
        if (bin + 1u < (unsigned)nbins && !(bnd[bin] - q >= ag)) {
            alt = bin + 1u;
            ag = bnd[bin] - q;
        }
        if (!(ag >= 0.0f))
            ag = 0.0f;
    }
    unsigned own = bin << shl;
#pragma unroll
    for (int off = 8; off > 0; off >>= 1)
        own |= (unsigned)__shfl_xor((int)own, off, KNN_WAVE);
    own = (unsigned)__shfl((int)own, 0, KNN_WAVE);
    int pick[SD];
    u64 key = alt != 0xFFFFFFFFu ? ((u64)__float_as_uint(ag) << 32) | (u64)lane : ~0ull;
#pragma unroll
    for (int j = 0; j < SD; ++j) {
        u64 best = key;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const u64 o = __shfl_xor(best, off, KNN_WAVE);
            best = o < best ? o : best;
        }
        pick[j] = best == ~0ull ? -1 : (int)(best & 0xFFFFFFFFull);
        if (lane == pick[j])
            key = ~0ull;
    }
    unsigned code = own;   // lane s < SEEDS: the code of seed cell s (bit j of s = across the j-th nearest cut)
    bool ok = lane < SEEDS;
#pragma unroll
    for (int j = 0; j < SD; ++j) {
        const int pj = pick[j] < 0 ? 0 : pick[j];
        const unsigned pa = (unsigned)__shfl((int)alt, pj, KNN_WAVE), pn = (unsigned)__shfl((int)nbl, pj, KNN_WAVE),
                       ps = (unsigned)__shfl((int)shl, pj, KNN_WAVE);
        if ((lane >> j) & 1) {
            if (pick[j] < 0)
                ok = false;
            else
                code = (code & ~(((1u << pn) - 1u) << ps)) | (pa << ps);
        }
    }
    // the tiles of seed cell `lane` (requested now, used after the tables): its first fragment, its first norm word, how many.
    // A cell of this index: all its tiles, out of the layout; a cell of another rank (cell-range shards): the few tiles of
    // the replicated seed layer.
    unsigned long long v_fa = 0ull, v_na = 0ull;
    unsigned v_nt = 0u, v_cell = 0u;
    if (!CNT && ok) {   // (the count form reads no seed tile: rf, rn2 and the layer are null there)
        const unsigned l = code - g.cell_base;
        if (code >= g.cell_base && l < g.ncells) {
            const unsigned tb = tile_start[l];
            v_cell = l;
            v_nt = tile_start[l + 1u] - tb;
            // (a shard's OUTER seeds — beyond the own cell and the cells across the two nearest cuts — give what the layer
            // would: their first tiles.  Whole, the 16 local seed cells of a query that lives on this rank were 136 tiles
            // against the 32 of everybody else's, and the launch lasted as long as those blocks: 36 us against 15)
            if (SD > 2 && lane >= 4)
                v_nt = min(v_nt, (unsigned)CELL_OUTER_SEED_TILES);
            v_fa = (unsigned long long)(rf + (size_t)tb * 64 * KT);
            v_na = (unsigned long long)(rn2 + (size_t)tb * 32);
        } else if (KT == 1 && layer.base) {
            // (TK, a top-K pass of a cell-range shard: these positions enter the K-th seed selection beside the own cells'.  What
            // knn_seed_kth.h asks of them — K finite scores are K distinct real rows — holds: a code outside this index's range
            // belongs to ANOTHER rank's part, so layer positions and positions of the own layout never name the same row, and the
            // four seed codes differ, so no layer position is read twice.  A finite norm is a real in-box row: the export
            // (knn_cells_seed_export_kernel) copies the owner's split norms word for word for the tiles the cell has and writes
            // 0x00007C00 = (+INF, 0) for the rest of its depth and for cells beyond the owner's range; the owner's placement kernels
            // write pack_norm22(+INF) = the same word on padding positions and on rows outside the robust box; a rank without rows
            // exports that word everywhere (knn_index_seed_export).  Checked by reading those three writers.)
            unsigned part = 0u;   // the rank whose range holds the cell (a table walk: no 64-bit divisions in here)
            for (unsigned r = 1u; r < layer.nranks; ++r)
                part += code >= layer.first[r] ? 1u : 0u;
            const unsigned cl = code - layer.first[part];
            const unsigned char *pb = layer.base + (size_t)part * layer.part_bytes + KNN_SEED_HEADER_BYTES;
            v_nt = layer.tiles;
            v_fa = (unsigned long long)(pb + (size_t)cl * layer.tiles * 1024u);
            v_na = (unsigned long long)(pb + (size_t)layer.cpr * layer.tiles * 1024u + (size_t)cl * layer.tiles * 128u);
        }
    }
    float fv_seed[NS];   // CTR: the frames of this wave's seed cells, word w on lane w (in flight while the tables are made)
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        fv_seed[c] = 0.0f;
        if constexpr (CTR) {
            const unsigned cell = (unsigned)__builtin_amdgcn_readlane((int)v_cell, wib + PW * c);
            if (lane < KNN_CELL_FRAME_WORDS)
                fv_seed[c] = frame[(size_t)cell * KNN_CELL_FRAME_WORDS + lane];
        }
    }
    __syncthreads();   // s_gap is complete
    // ---- the tables: double sums of the rounded-down gaps, rounded down again.  (Bits and positions of the dimensions
    // come from the lanes that hold them — nbl, shl above — as wave-uniform values: indexing the geometry struct with a
    // run-time d is a dependent scalar load from the kernel arguments per dimension and entry.)
    // Entry e of the high table belongs to local cells [e 2^sa, (e + 1) 2^sa): codes cell_base + that (cell_base is a
    // multiple of 2^sa; 0 unless the index is a cell-range shard).
    const int nl = 1 << g.sa, nh = (int)g.nh;   // nl >= 64: a wave's entries are all low or all high
    for (int e0 = 64 * wib; e0 < nl + nh; e0 += 64 * PW) {
        const int e = e0 + lane;
        const bool low = e0 < nl;   // wave-uniform
        const unsigned ecode = low ? (unsigned)e : ((g.cell_base >> g.sa) + (unsigned)(e - nl)) << g.sa;
        double sum = 0.0;
#pragma unroll
        for (int d = 0; d < 16; ++d) {
            const unsigned nbd = (unsigned)__builtin_amdgcn_readlane((int)nbl, d);
            const unsigned shd = (unsigned)__builtin_amdgcn_readlane((int)shl, d);
            if (nbd != 0u && ((int)shd < g.sa) == low)   // wave-uniform
                sum += (double)s_gap[d][(ecode >> shd) & ((1u << nbd) - 1u)];
        }
        const float v = __double2float_rd(sum);
        if (e < nl + nh) {
            if (low)
                lo_tab[!TK && lo_by_entry ? (size_t)e * m_padded + qi : (size_t)qi * nl + e] = v;
            else
                hi_tab[(size_t)(e - nl) * m_padded + qi] = v;
        }
        // the smallest of a group of 64 low entries AS STORED (no new sum), [group][query]: the wave's 64 entries are one group —
        // the 64 cells of one block of the match kernel, whose pass 1 queues the query iff that smallest entry passes.  Lists made
        // by the scan's own waves (1-NN, lo_by_entry) have no match launch and no reader of it.
        if (low && (TK || !lo_by_entry)) {   // wave-uniform
            float vmin = v;                  // (nl is a multiple of 64: every lane of a low wave holds an entry)
#pragma unroll
            for (int off = 32; off > 0; off >>= 1)
                vmin = fminf(vmin, __shfl_xor(vmin, off, KNN_WAVE));
            if (lane == 0)
                lo_min[(size_t)(e0 >> 6) * m_padded + qi] = vmin;
        }
    }
    // ---- seed scores.  A wave's seed tiles — those of its NS cells, a cell of many tiles sampled (every stride-th,
    // at most CELL_SEED_MAX_TILES: any real row's score bounds the answer, and one query per MFMA against the thousands of
    // tiles of a cluster would cost more than the scan it prepares) — are ONE list, requested CELL_PREP_TILES at a time.
    float um = INFINITY;
    // (all wave-uniform) run c: `cnt[c]` tiles fa[c] + v stride[c] KiB, norm words na[c] + v stride[c] 128 B
    auto score_runs = [&](const unsigned long long (&fa)[NS], const unsigned long long (&na)[NS], const unsigned (&cnt)[NS],
                          const unsigned (&stride)[NS], const h8 (&bqx)[KT]) __attribute__((always_inline)) {
        unsigned start[NS + 1];   // run c holds positions [start[c], start[c + 1]) of the list (constant indices only: these
        start[0] = 0u;            // arrays must stay in registers — indexed by a run-time c they went to scratch memory)
#pragma unroll
        for (int c = 0; c < NS; ++c)
            start[c + 1] = start[c] + cnt[c];
        const unsigned total = start[NS];
        for (unsigned v0 = 0u; v0 < total; v0 += PREP_TILES) {
            h8 ar[PREP_TILES][KT];
            unsigned nw[PREP_TILES];
#pragma unroll
            for (int p = 0; p < PREP_TILES; ++p) {
                const unsigned v = v0 + (unsigned)p;   // position in the list -> (run, tile of the run)
                nw[p] = 0u;
                if (v < total) {
                    unsigned long long f = fa[0], nn = na[0];
                    unsigned st = stride[0], vv = v;
#pragma unroll
                    for (int c = 1; c < NS; ++c)
                        if (v >= start[c]) {   // (start[] ascends: the last run that matches is the one)
                            f = fa[c];
                            nn = na[c];
                            st = stride[c];
                            vv = v - start[c];
                        }
                    const size_t t = (size_t)vv * st;
#pragma unroll
                    for (int kk = 0; kk < KT; ++kk)
                        ar[p][kk] = ((const h8 *)f)[(t * KT + kk) * 64 + lane];
                    if (lane < 32)
                        nw[p] = ((const unsigned *)nn)[t * 32 + lane];
                }
            }
#pragma unroll
            for (int p = 0; p < PREP_TILES; ++p)
                if (v0 + (unsigned)p < total) {
                    f16v d = __builtin_amdgcn_mfma_f32_32x32x16_f16(norm_a_operand(nw[p]), norm_b_operand(), zero_acc(), 0, 0, 0);
#pragma unroll
                    for (int kk = 0; kk < KT; ++kk)
                        d = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar[p][kk], bqx[kk], d, 0, 0, 0);
                    um = min_tree16(d, um);
                }
        }
    };
    if constexpr (CTR && TK) {
        // A top-K batch on per-cell frames (KNN_QUERY_TOPK_FRAMES; DESIGN §4.6 "Per-cell frames", knn_frame_dup.h): scores of cells in
        // different frames do not compare, the frame-free bounds they imply do.  Per seed cell: the query rounded in the cell's frame,
        // the K smallest finite per-row scores of its (sampled) tiles by knn_seed_kth.h's selection, each converted to Dup_c(u) in the
        // shard's units — lane t converts list entry t; Dup_c is non-decreasing in u, so the list stays sorted — and, as keys, merged
        // across the wave's cells, then across the block's waves.  Dup_(K), the K-th smallest, bounds the K-th smallest true distance:
        // K finite scores of distinct positions are K distinct real in-box rows, each within its own Dup_c(u) <= Dup_(K).  The far
        // branch gives every finite position of the cell the triangle inequality's bound.  Fewer than K: the 64 tiles spread over
        // the layout, each in its own cell's frame, minus those inside a seed cell; still fewer: +INF, FALLBACK.
        const int topk = lo_by_entry;
        unsigned v_tb = 0u, v_own = 0u;   // the tiles of the layout seed cell `lane` stands for (the wide sample leaves them out)
        {
            const unsigned l = code - g.cell_base;
            if (ok && code >= g.cell_base && l < g.ncells) {
                v_tb = tile_start[l];
                v_own = v_nt;
            }
        }
        // (The tile walk — request PREP_TILES tiles, norm MFMA + score MFMA, lane select — exists three times in this kernel: score_runs,
        // score_runs_tk and here; each form's text is kept apart so that the others compile as they did.  A change to the seed
        // scoring goes into all three.)
        // fv: the cell's frame, word w on lane w -> the cell's 64 smallest Dup keys, ascending over the lanes (cnt0 tiles f0 + v
        // stride0 KiB, norm words n0 + v stride0 128 B; all wave-uniform)
        auto cell_dups = [&](float fv, unsigned long long f0, unsigned long long n0, unsigned cnt0,
                             unsigned stride0) __attribute__((always_inline)) -> unsigned {
            float fr[KNN_CELL_FRAME_WORDS];
#pragma unroll
            for (int w_ = 0; w_ < KNN_CELL_FRAME_WORDS; ++w_)
                fr[w_] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, fv), w_));
            _Float16 bv[16];
            const KnnFrameQuery fq = knn_frame_query(g.k, fr, qrow, bv);
            h8 bqc;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                bqc[j] = half ? bv[8 + j] : bv[j];
            unsigned cur = KNN_SEED_NONE;
            for (unsigned v0 = 0u; v0 < cnt0; v0 += PREP_TILES) {
                h8 ar[PREP_TILES];
                unsigned nw[PREP_TILES];
                unsigned sel[PREP_TILES];   // the tiles' score keys, one per lane
#pragma unroll
                for (int p = 0; p < PREP_TILES; ++p) {
                    nw[p] = 0u;
                    if (v0 + (unsigned)p < cnt0) {
                        const size_t t = (size_t)(v0 + (unsigned)p) * stride0;
                        ar[p] = ((const h8 *)f0)[t * 64 + lane];
                        if (lane < 32)
                            nw[p] = ((const unsigned *)n0)[t * 32 + lane];
                    }
                }
#pragma unroll
                for (int p = 0; p < PREP_TILES; ++p)
                    if (v0 + (unsigned)p < cnt0) {
                        f16v d = __builtin_amdgcn_mfma_f32_32x32x16_f16(norm_a_operand(nw[p]), norm_b_operand(), zero_acc(), 0, 0, 0);
                        d = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar[p], bqc, d, 0, 0, 0);
                        float sc = d[0];
#pragma unroll
                        for (int i = 1; i < 16; ++i)
                            sc = (lane & 15) == i ? d[i] : sc;
                        sel[p] = knn_seed_lane_holds_row(lane) ? knn_seed_key(sc) : KNN_SEED_NONE;
                    }
#pragma unroll
                for (int p = 0; p < PREP_TILES; ++p)
                    if (v0 + (unsigned)p < cnt0) {
                        const unsigned kth = (unsigned)__shfl((int)cur, topk - 1, KNN_WAVE);
                        if (__ballot(sel[p] < kth) != 0ull)   // wave-uniform: a tile with nothing below the K-th changes nothing
                            cur = seed_merge64(cur, seed_sort64(sel[p], lane), lane);
                    }
            }
            const float s = knn_seed_score(cur);   // lane t: list entry t (+INF: none)
            return knn_seed_key(s < INFINITY ? knn_frame_dup(g.k, fr[16], fr[17], fr[18], fr[19], fq, s) : INFINITY);
        };
        unsigned cur = KNN_SEED_NONE;
#pragma unroll
        for (int c = 0; c < NS; ++c) {   // this wave's seed cells
            const int sl = wib + PW * c;
            const unsigned nt = (unsigned)__builtin_amdgcn_readlane((int)v_nt, sl);
            if (nt != 0u) {   // wave-uniform
                const unsigned long long f0 = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v_fa >> 32), sl) << 32) |
                                              (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)v_fa, sl);
                const unsigned long long n0 = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v_na >> 32), sl) << 32) |
                                              (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)v_na, sl);
                // a fat cell: the per-cell-frame form's strided sample (strided positions are distinct)
                const unsigned scap = min(CELL_SEED_MAX_TILES_CTR, max(CELL_SEED_MAX_TILES, (nt * 9u) >> 9));
                const unsigned st0 = (nt + scap - 1u) / scap;
                cur = seed_merge64(cur, cell_dups(fv_seed[c], f0, n0, (nt + st0 - 1u) / st0, st0), lane);
            }
        }
        // the block's K-th smallest: every wave merges all the waves' lists (the same value everywhere: block-uniform below)
        __shared__ unsigned s_topf[PW][64];
        s_topf[wib][lane] = cur;
        __syncthreads();
        unsigned all = s_topf[0][lane];
#pragma unroll
        for (int i = 1; i < PW; ++i)
            all = seed_merge64(all, s_topf[i][lane], lane);
        if ((unsigned)__shfl((int)all, topk - 1, KNN_WAVE) == KNN_SEED_NONE && ntiles > 0) {   // block-uniform
            __syncthreads();   // s_topf has been read by everybody
            const unsigned total = (unsigned)(ntiles > 64 ? 64 : ntiles);
            const unsigned wstride = (unsigned)(ntiles > 64 ? ntiles / 64 : 1);
            cur = KNN_SEED_NONE;
            for (unsigned i = (unsigned)wib * (64u / PW); i < min(((unsigned)wib + 1u) * (64u / PW), total); ++i) {
                const unsigned t = i * wstride;
                if (__ballot(lane < SEEDS && v_own != 0u && t >= v_tb && t - v_tb < v_own) != 0ull)   // inside a seed cell: counted already
                    continue;
                const float fv = lane < KNN_CELL_FRAME_WORDS ? frame[(size_t)tile_cell[t] * KNN_CELL_FRAME_WORDS + lane] : 0.0f;
                cur = seed_merge64(cur, cell_dups(fv, (unsigned long long)(rf + (size_t)t * 64), (unsigned long long)(rn2 + (size_t)t * 32), 1u, 1u),
                                   lane);
            }
            s_topf[wib][lane] = cur;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < PW; ++i)
                all = seed_merge64(all, s_topf[i][lane], lane);
            if (tid == 0)
                atomicAdd(&ctl[KNN_CTL_WIDE_SEEDS], 1u);   // rare; statistics only
        }
        const float u = knn_seed_score((unsigned)__shfl((int)all, topk - 1, KNN_WAVE));   // Dup_(K), the shard's units
        if (tid == 0) {
            const bool bad = qbad || !(amax <= amax_limit) || !(u < INFINITY);
            float sq = sqrtf(u);
            sq = nextafterf(nextafterf(sq, INFINITY), INFINITY);
            thr[qi] = bad ? -INFINITY : sq;
            dup_out[qi] = bad ? -INFINITY : u;
            if (bad)
                ctl[KNN_CTL_FALLBACK] = 1u;  // benign race: every writer stores 1
        }
        return;
    } else if constexpr (CTR) {
        // One seed cell (or sampled tile) at a time: the query rounded in the cell's frame — what knn_frag_kernel would write
        // for it with (centre_c, scale_c) —, the cell's tiles scored against it, the bound on the answer's distance they give
        // in the SHARD's scaled units (the two frames differ by the power of two frame[17]).  All lanes do all of it.
        // fv: the cell's frame, word w on lane w (requested early — before the tables — for the seed cells)
        auto cell_bound = [&](float fv, unsigned long long f0, unsigned long long n0, unsigned cnt0,
                              unsigned stride0) __attribute__((always_inline)) -> float {
            float fr[KNN_CELL_FRAME_WORDS];
#pragma unroll
            for (int w_ = 0; w_ < KNN_CELL_FRAME_WORDS; ++w_)
                fr[w_] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, fv), w_));
            const float scale = fr[16], ratio = fr[17];
            float nrmc = 0.0f, amaxc = 0.0f, n32 = 0.0f;
            bool badc = false;
            h8 bqc[KT];
#pragma unroll
            for (int d = 0; d < 16; ++d) {
                float sc = 0.0f;
                if (d < g.k)
                    sc = (qrow[d] - fr[d]) * scale;
                n32 = n32 + sc * sc;
                const _Float16 hval = (_Float16)sc;
                const float back = (float)hval;
                badc = badc || !(fabsf(back) < INFINITY);
                amaxc = fmaxf(amaxc, fabsf(back));
                nrmc = nrmc + back * back;
                const _Float16 v = (_Float16)(back * -2.0f);
                badc = badc || !(fabsf((float)v) < INFINITY);
                if (((d >> 3) & 1) == half)
                    bqc[0][d & 7] = v;
            }
            // A query that does not fit this cell's frame (beyond CELL_FRAME_AMAX cell units: far from a tight cell): no fp16 scores — a
            // zero B operand leaves the rows' norms, finite iff the tiles hold a real row — and the bound is the triangle
            // inequality's: every row of the cell is within sqrt(k) bmax_c (1 + 2^-10) of its centre.
            const bool far = badc || !(amaxc <= CELL_FRAME_AMAX);
            if (far)
                bqc[0] = (h8){0, 0, 0, 0, 0, 0, 0, 0};
            unsigned long long fa[NS], na[NS];
            unsigned cnt[NS], stride[NS];
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                fa[c] = na[c] = 0ull;
                cnt[c] = 0u;
                stride[c] = 1u;
            }
            fa[0] = f0;
            na[0] = n0;
            cnt[0] = cnt0;
            stride[0] = stride0;
            um = INFINITY;
            score_runs(fa, na, cnt, stride, bqc);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1)
                um = fminf(um, __shfl_xor(um, off, KNN_WAVE));
            if (!(um < INFINITY))
                return INFINITY;
            KnnFrameQuery fq;
            fq.amax = amaxc;
            fq.nrm = nrmc;
            fq.n32 = n32;
            fq.far = far;
            return knn_frame_dup(g.k, scale, ratio, fr[18], fr[19], fq, um);
        };
        float best = INFINITY;
#pragma unroll
        for (int c = 0; c < NS; ++c) {   // this wave's seed cells
            const int sl = wib + PW * c;
            const unsigned nt = (unsigned)__builtin_amdgcn_readlane((int)v_nt, sl);
            if (nt != 0u) {   // wave-uniform
                const unsigned long long f0 = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v_fa >> 32), sl) << 32) |
                                              (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)v_fa, sl);
                const unsigned long long n0 = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v_na >> 32), sl) << 32) |
                                              (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)v_na, sl);
                // (a fat cell — a whole cluster — leaves about (its rows / the rows sampled here) candidates per query: 1/56 of its
                // tiles, between 36 and 144, keeps a batch of 1024 near 16 records per scan wave.  n 2^24, 64 clusters: 36 tiles
                // 0.318 ms per step, 248 k records; 144 tiles 0.208, 60 k.  n 2^22: 36 tiles 0.105; 144 tiles 0.121 — the prep
                // kernel's extra 16 us buy nothing there)
                const unsigned scap = min(CELL_SEED_MAX_TILES_CTR, max(CELL_SEED_MAX_TILES, (nt * 9u) >> 9));
                const unsigned st0 = (nt + scap - 1u) / scap;
                best = fminf(best, cell_bound(fv_seed[c], f0, n0, (nt + st0 - 1u) / st0, st0));
            }
        }
        if (lane == 0)
            s_red[wib] = best;
        __syncthreads();
        float u = s_red[0];
#pragma unroll
        for (int i = 1; i < PW; ++i)
            u = fminf(u, s_red[i]);
        if (!(u < INFINITY) && ntiles > 0) {   // block-uniform: nothing in the seed cells — 64 tiles spread over the layout, each in its cell's frame
            __syncthreads();
            const unsigned total = (unsigned)(ntiles > 64 ? 64 : ntiles);
            const unsigned wstride = (unsigned)(ntiles > 64 ? ntiles / 64 : 1);
            best = INFINITY;
            for (unsigned i = (unsigned)wib * (64u / PW); i < min(((unsigned)wib + 1u) * (64u / PW), total); ++i) {
                const size_t t = (size_t)i * wstride;
                const float fv = lane < KNN_CELL_FRAME_WORDS ? frame[(size_t)tile_cell[t] * KNN_CELL_FRAME_WORDS + lane] : 0.0f;
                best = fminf(best, cell_bound(fv, (unsigned long long)(rf + t * 64), (unsigned long long)(rn2 + t * 32), 1u, 1u));
            }
            if (lane == 0)
                s_red[wib] = best;
            __syncthreads();
            u = s_red[0];
#pragma unroll
            for (int i = 1; i < PW; ++i)
                u = fminf(u, s_red[i]);
            if (tid == 0)
                atomicAdd(&ctl[KNN_CTL_WIDE_SEEDS], 1u);   // rare; statistics only
        }
        if (tid == 0) {
            const bool bad = qbad || !(amax <= amax_limit) || !(u < INFINITY);
            float sq = sqrtf(u);
            sq = nextafterf(nextafterf(sq, INFINITY), INFINITY);
            thr[qi] = bad ? -INFINITY : sq;
            dup_out[qi] = bad ? -INFINITY : u;
            if (bad)
                ctl[KNN_CTL_FALLBACK] = 1u;  // benign race: every writer stores 1
        }
        return;
    }
    float u;
    if constexpr (CNT) {
        // the count form (knn_cells_prep_count_kernel): no seed tile is scored — the radius alone bounds the query, knn_threshold_within
        // at u = +INF (its case (a)); everything above that only the seed scores read is dead here
        u = INFINITY;
    } else if constexpr (TK) {
        const int topk = lo_by_entry;
        unsigned cur = KNN_SEED_NONE;   // the wave's 64 smallest score keys so far, ascending over the lanes
        unsigned wide_first = 0xFFFFFFFFu, wide_stride = 0u;   // the wide sample: list position v is tile (wide_first + v) wide_stride
        // the tiles [v_tb, v_tb + v_own) of the layout that seed cell `lane` has put into the selection (the wide sample leaves them
        // out).  Cells of THIS index only: a seed of another rank came out of the seed layer (v_nt = its depth there), no tile of
        // this layout stands for it — taken for tiles 0 .. depth - 1 it cost the wide sample its first tiles (safe, a looser bound)
        unsigned v_tb = 0u, v_own = 0u;
        {
            const unsigned l = code - g.cell_base;
            if (ok && code >= g.cell_base && l < g.ncells) {
                v_tb = tile_start[l];
                v_own = v_nt;
            }
        }
        // score_runs' walk over the wave's list of tiles, with the selection of knn_seed_kth.h in place of the minimum.  (A lambda of
        // its own inside the TK branch: with the selection as a branch of score_runs, or this lambda where the other forms see it, what
        // it captures changed the order of the per-cell-frame forms' instructions.)
        auto score_runs_tk = [&](const unsigned long long (&fa)[NS], const unsigned long long (&na)[NS], const unsigned (&cnt)[NS],
                              const unsigned (&stride)[NS], const h8 (&bqx)[KT]) __attribute__((always_inline)) {
            unsigned start[NS + 1];   // run c holds positions [start[c], start[c + 1]) of the list (constant indices only: these
            start[0] = 0u;            // arrays must stay in registers — indexed by a run-time c they went to scratch memory)
#pragma unroll
            for (int c = 0; c < NS; ++c)
                start[c + 1] = start[c] + cnt[c];
            const unsigned total = start[NS];
            for (unsigned v0 = 0u; v0 < total; v0 += PREP_TILES) {
                h8 ar[PREP_TILES][KT];
                unsigned nw[PREP_TILES];
                unsigned sel[PREP_TILES];   // the tiles' score keys, one per lane
#pragma unroll
                for (int p = 0; p < PREP_TILES; ++p) {
                    const unsigned v = v0 + (unsigned)p;   // position in the list -> (run, tile of the run)
                    nw[p] = 0u;
                    if (v < total) {
                        unsigned long long f = fa[0], nn = na[0];
                        unsigned st = stride[0], vv = v;
#pragma unroll
                        for (int c = 1; c < NS; ++c)
                            if (v >= start[c]) {   // (start[] ascends: the last run that matches is the one)
                                f = fa[c];
                                nn = na[c];
                                st = stride[c];
                                vv = v - start[c];
                            }
                        const size_t t = (size_t)vv * st;
#pragma unroll
                        for (int kk = 0; kk < KT; ++kk)
                            ar[p][kk] = ((const h8 *)f)[(t * KT + kk) * 64 + lane];
                        if (lane < 32)
                            nw[p] = ((const unsigned *)nn)[t * 32 + lane];
                    }
                }
#pragma unroll
                for (int p = 0; p < PREP_TILES; ++p)
                    if (v0 + (unsigned)p < total) {
                        f16v d = __builtin_amdgcn_mfma_f32_32x32x16_f16(norm_a_operand(nw[p]), norm_b_operand(), zero_acc(), 0, 0, 0);
#pragma unroll
                        for (int kk = 0; kk < KT; ++kk)
                            d = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar[p][kk], bqx[kk], d, 0, 0, 0);
                        // this tile's 32 row scores on lanes 0..15 and 32..47 (accumulator lane & 15) as keys (knn_seed_kth.h); a
                        // wide-sample tile that lies in one of the seed cells is left out
                        bool skip = false;
                        if (wide_first != 0xFFFFFFFFu) {   // wave-uniform
                            const unsigned t = (wide_first + v0 + (unsigned)p) * wide_stride;
                            skip = __ballot(lane < SEEDS && v_own != 0u && t >= v_tb && t - v_tb < v_own) != 0ull;
                        }
                        float sc = d[0];
#pragma unroll
                        for (int i = 1; i < 16; ++i)
                            sc = (lane & 15) == i ? d[i] : sc;
                        sel[p] = knn_seed_lane_holds_row(lane) && !skip ? knn_seed_key(sc) : KNN_SEED_NONE;
                    }
                // sorted and merged into `cur` behind the MFMAs, when the tiles' registers are free (inside the loop above the
                // network's temporaries came on top of the tiles in flight: scratch)
#pragma unroll
                for (int p = 0; p < PREP_TILES; ++p)
                    if (v0 + (unsigned)p < total) {
                        const unsigned kth = (unsigned)__shfl((int)cur, topk - 1, KNN_WAVE);
                        if (__ballot(sel[p] < kth) != 0ull)   // wave-uniform: a tile with nothing below the K-th changes nothing
                            cur = seed_merge64(cur, seed_sort64(sel[p], lane), lane);
                    }
            }
        };
        {
            unsigned long long fa[NS], na[NS];
            unsigned cnt[NS], stride[NS];
#pragma unroll
            for (int c = 0; c < NS; ++c) {   // this wave's seed cells
                const int sl = wib + PW * c;
                const unsigned nt = (unsigned)__builtin_amdgcn_readlane((int)v_nt, sl);
                fa[c] = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v_fa >> 32), sl) << 32) |
                        (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)v_fa, sl);
                na[c] = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v_na >> 32), sl) << 32) |
                        (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)v_na, sl);
                stride[c] = (nt + CELL_SEED_MAX_TILES - 1u) / CELL_SEED_MAX_TILES;   // 1 up to the cap
                cnt[c] = nt == 0u ? 0u : (nt + stride[c] - 1u) / stride[c];
            }
            score_runs_tk(fa, na, cnt, stride, bq);
        }
        // the block's K-th smallest: every wave merges all the waves' lists (the same value everywhere: block-uniform below)
        __shared__ unsigned s_top[PW][64];
        s_top[wib][lane] = cur;
        __syncthreads();
        unsigned all = s_top[0][lane];
#pragma unroll
        for (int i = 1; i < PW; ++i)
            all = seed_merge64(all, s_top[i][lane], lane);
        if ((unsigned)__shfl((int)all, topk - 1, KNN_WAVE) == KNN_SEED_NONE && ntiles > 0) {   // block-uniform
            // fewer than K real rows in the seed cells: the 64 tiles spread over the layout are merged in, 64 / PW per wave
            __syncthreads();   // s_top has been read by everybody
            const unsigned total = (unsigned)(ntiles > 64 ? 64 : ntiles);
            const unsigned wstride = (unsigned)(ntiles > 64 ? ntiles / 64 : 1);
            const unsigned mine_first = (unsigned)wib * (64u / PW);
            cur = KNN_SEED_NONE;
            if (mine_first < total) {
                unsigned long long fa[NS], na[NS];
                unsigned cnt[NS], stride[NS];
#pragma unroll
                for (int c = 0; c < NS; ++c) {
                    fa[c] = na[c] = 0ull;
                    cnt[c] = 0u;
                    stride[c] = 1u;
                }
                fa[0] = (unsigned long long)(rf + (size_t)mine_first * wstride * 64 * KT);
                na[0] = (unsigned long long)(rn2 + (size_t)mine_first * wstride * 32);
                cnt[0] = min(64u / PW, total - mine_first);
                stride[0] = wstride;
                wide_first = mine_first;
                wide_stride = wstride;
                score_runs_tk(fa, na, cnt, stride, bq);
            }
            s_top[wib][lane] = cur;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < PW; ++i)
                all = seed_merge64(all, s_top[i][lane], lane);
            if (tid == 0)
                atomicAdd(&ctl[KNN_CTL_WIDE_SEEDS], 1u);   // rare; statistics only
        }
        u = knn_seed_score((unsigned)__shfl((int)all, topk - 1, KNN_WAVE));
    } else {
    {
        unsigned long long fa[NS], na[NS];
        unsigned cnt[NS], stride[NS];
#pragma unroll
        for (int c = 0; c < NS; ++c) {   // this wave's seed cells
            const int sl = wib + PW * c;
            const unsigned nt = (unsigned)__builtin_amdgcn_readlane((int)v_nt, sl);
            fa[c] = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v_fa >> 32), sl) << 32) |
                    (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)v_fa, sl);
            na[c] = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v_na >> 32), sl) << 32) |
                    (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)v_na, sl);
            stride[c] = (nt + CELL_SEED_MAX_TILES - 1u) / CELL_SEED_MAX_TILES;   // 1 up to the cap
            cnt[c] = nt == 0u ? 0u : (nt + stride[c] - 1u) / stride[c];
        }
        score_runs(fa, na, cnt, stride, bq);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)   // (every column is this query; the halves hold different rows)
        um = fminf(um, __shfl_xor(um, off, KNN_WAVE));
    if (lane == 0)
        s_red[wib] = um;
    __syncthreads();
    u = s_red[0];
#pragma unroll
    for (int i = 1; i < PW; ++i)
        u = fminf(u, s_red[i]);
    if (!(u < INFINITY) && ntiles > 0) {   // block-uniform
        // nothing in the seed cells (a query in an empty corner of a clustered set): any real row gives a valid, if
        // loose, bound — look at 64 tiles spread over the whole layout, 64 / PW per wave
        __syncthreads();   // s_red has been read by everybody
        const unsigned total = (unsigned)(ntiles > 64 ? 64 : ntiles);
        const unsigned wstride = (unsigned)(ntiles > 64 ? ntiles / 64 : 1);
        const unsigned mine_first = (unsigned)wib * (64u / PW);
        um = INFINITY;
        if (mine_first < total) {
            unsigned long long fa[NS], na[NS];
            unsigned cnt[NS], stride[NS];
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                fa[c] = na[c] = 0ull;
                cnt[c] = 0u;
                stride[c] = 1u;
            }
            fa[0] = (unsigned long long)(rf + (size_t)mine_first * wstride * 64 * KT);
            na[0] = (unsigned long long)(rn2 + (size_t)mine_first * wstride * 32);
            cnt[0] = min(64u / PW, total - mine_first);
            stride[0] = wstride;
            score_runs(fa, na, cnt, stride, bq);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            um = fminf(um, __shfl_xor(um, off, KNN_WAVE));
        if (lane == 0)
            s_red[wib] = um;
        __syncthreads();
        u = s_red[0];
#pragma unroll
        for (int i = 1; i < PW; ++i)
            u = fminf(u, s_red[i]);
        if (tid == 0)
            atomicAdd(&ctl[KNN_CTL_WIDE_SEEDS], 1u);   // rare; statistics only
    }
    }
    if (tid == 0) {
        bool bad = qbad || !(amax <= amax_limit);
        float t = -INFINITY, dupf = -INFINITY;
        if (!WR && !bad && !(u < INFINITY))
            bad = true;        // no row of the filter seen: cannot bound (WR: the radius bounds the query)
        if (!bad) {
            const BoundConsts cst = knn_bound_consts(g.k, KT, sigma, amax, bmax, nmax);
            double dup = 0.0;
            t = WR ? knn_threshold_within(cst, u, nrm, s_radius, &dup) : knn_threshold(cst, u, nrm, &dup);
            if (!(t < INFINITY))
                bad = true;
            else {
                dup *= 1.0 + 1e-6;
                dupf = (float)dup;
                if ((double)dupf < dup)
                    dupf = nextafterf(dupf, INFINITY);
            }
        }
        if (EACH && !(s_radius >= 0.0f)) {   // no candidates: a padding query's threshold, and no fallback — the count is 0
            bad = false;
            t = dupf = -INFINITY;
        }
        thr[qi] = bad ? -INFINITY : t;
        dup_out[qi] = bad ? -INFINITY : dupf;
        if (bad)
            ctl[KNN_CTL_FALLBACK] = 1u;  // benign race: every writer stores 1
    }
