// knn_cells_scan_body.inc — the body of knn_cells_scan_kernel and of knn_cells_records_kernel (knn_cells.hip), included
// inside each: the template parameters DYN, K, SELF, KT, CTR, NIF, U8 and the constant TOPK are those of the including kernel.
// TOPK = true (with KNN_CELLS_SCAN_RECORD_ONLY defined, which leaves the 1-NN epilogue out of the text) is the record-only form of
// a top-K pass: it ends behind the item loop, once the wave's record count is written.
// (Included text, not a __device__ function the two kernels call: behind a call the compiler schedules the 1-NN forms
// differently and they spill under their register caps.)
    extern __shared__ __attribute__((aligned(128))) unsigned char s_dyn[];   // (aligned: static LDS of the kernel sits in front of it, and the b128 reads below want 16-byte addresses)
    constexpr int TPP = CELL_TILES_PER_PASS;                         // reference tiles a wave holds in registers at a time
    constexpr int SW = KT == 1 && !CTR ? CELL_SCAN_WAVES : CELL_SCAN_WAVES_KT2;   // waves of a block
    constexpr int QB = CTR ? 64 : 32 * KT;                              // bytes of a query in LDS (CTR: its fp32 row, 16 dimensions)
    // the bin-frame 8-bit scan with the counter deal: an item's list words and w_c are requested with its tiles and first
    // waited for behind them — one round trip per item (see l0 below)
    constexpr bool ONE_TRIP = DYN && U8 && !CTR && !SELF && KT == 1;
    h8 *s_qf = (h8 *)s_dyn;                                             // [m_padded / 32][KT][64]; CTR: float s_q32[m_padded][16]
    float *s_thr = (float *)(s_dyn + (size_t)m_padded * QB);            // [m_padded]
    f4v *s_nrm = (f4v *)(s_dyn + (size_t)m_padded * (QB + 4));          // [waves][TPP * 8]
    // SELF: the batch's Dup values and one list room per wave behind the norm windows (knn_cells_scan_plan sizes it)
    float *s_dup = (float *)(s_dyn + (size_t)m_padded * (QB + 4) + (size_t)SW * TPP * 8 * sizeof(f4v));   // [m_padded]
    unsigned short *s_lists = (unsigned short *)(s_dup + m_padded);     // [waves][CELL_SELF_CAP]
    __shared__ unsigned s_flag;
    SCAN_STAMP(0);
    if (threadIdx.x == 0)
        s_flag = ctl[KNN_CTL_FALLBACK];   // read once per block: see knn_cells_match_kernel
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned wave = blockIdx.x * (unsigned)SW + (unsigned)wib, nwaves = gridDim.x * (unsigned)SW;
    __shared__ unsigned s_next, s_imeta[DYN ? CELL_SCAN_CHUNK : 1], s_itb[DYN ? CELL_SCAN_CHUNK : 1], s_inq[DYN ? CELL_SCAN_CHUNK : 1];
    const unsigned per_wave = (nitems + nwaves - 1u) / nwaves;
    // DYN: a block's share is one RUN of CELL_SCAN_RUN consecutive items out of every stripe of gridDim.x runs, not one
    // contiguous stretch of the item order.  Round 4, from the per-wave stamps of tools/scan_timeline.py at C3
    // (profiles/r04_scan_timeline.txt): with contiguous shares the blocks finished their items 71 to 109 us after the launch
    // began, later the further along the cell order their stretch lay (+14 us from the first to the last block of either half
    // of the grid: the work per cell drifts along the order — the side of a cut that got a percent more rows has more cells
    // that spill into a ninth tile).  A share that samples the whole order carries the average: the launch alone 0.1133 ->
    // 0.1085 ms, one batch at a time 0.1500 -> 0.1450 (three A/B pairs on one box); batches in flight fill the gaps either
    // way (0.1186-0.1237 / 0.1179-0.1204 per step).  All blocks still move through the layout together.
    // Which run of a stripe: rotated from stripe to stripe by a golden-ratio step — with the b-th run of every stripe a
    // block's cells would all share the code bits that number the run inside a stripe, and the drift follows the code bits.
    // Slot s of a share = item (stripe * gridDim.x + (blockIdx.x + stripe * rot) % gridDim.x) * RUN + s % RUN, stripe = s / RUN;
    // slots past the last item are holes.
    // (What is left after this: the 256 blocks placed second on their CUs finish 15 us behind the 256 placed first whatever
    // they are given — 87 against 102 us — and the XCDs differ by +-6 %.  A pool of items behind the shares that waves drain
    // through ONE counter in memory was tried for that: an agent-scope atomic on one address costs ~26 ns and they queue up —
    // 10 % of the items in the pool doubled the launch, 0.107 -> 0.190 ms.  tools/arms/scan_item_pool.patch.)
    // (everything derived from the arguments is recomputed where it is used — the fills, twice a launch: values kept across
    // the item loop for them went to scratch under the 80-register cap)
    const unsigned i0 = 0u;
    const unsigned i1 = DYN ? (((nitems + (unsigned)CELL_SCAN_RUN - 1u) / (unsigned)CELL_SCAN_RUN + gridDim.x - 1u) / gridDim.x) *
                                  (unsigned)CELL_SCAN_RUN
                            : 0u;   // the share, in slots
    auto slot_item = [&](unsigned s) {
        const unsigned nruns = (nitems + (unsigned)CELL_SCAN_RUN - 1u) / (unsigned)CELL_SCAN_RUN;
        const unsigned rot = __umulhi(gridDim.x, 2654435769u) | 1u;   // gridDim.x * 0.618...
        const unsigned stripe = s / (unsigned)CELL_SCAN_RUN;
        const unsigned run = stripe * gridDim.x + (blockIdx.x + stripe * rot) % gridDim.x;
        const unsigned it = run * (unsigned)CELL_SCAN_RUN + s % (unsigned)CELL_SCAN_RUN;
        return run < nruns && it < nitems ? it : 0xFFFFFFFFu;
    };
    // DYN: the first chunk's descriptors — two dependent round trips (item -> its cell's list length) — are requested BEFORE
    // the block fills its LDS (36 KiB of B operands and thresholds, one more round trip and a barrier): they overlap instead
    // of queueing up in front of the first tile load, and one barrier pair goes (round 4: 114.4 -> 112.5 us at C3, rocprofv3).
    // (The same for the fixed deal kept two more values alive across the fill: 16 bytes of scratch under the 80-register
    // cap, and a kernel that uses scratch at all ran 7 % slower — 0.1197 -> 0.1283 ms on one box.  Left as it was.)
    if constexpr (DYN) {
        const unsigned nc0 = min((unsigned)CELL_SCAN_CHUNK, i1 - i0);
        for (unsigned i = threadIdx.x; i < nc0; i += 64 * SW) {
            const unsigned it = slot_item(i0 + i);
            const u64 item = it != 0xFFFFFFFFu ? items[it] : 0ull;
            s_imeta[i] = (unsigned)(item >> 40);
            s_itb[i] = (unsigned)item;
            if constexpr (SELF)
                s_inq[i] = it != 0xFFFFFFFFu ? 1u : 0u;   // (the list is made when the item is taken)
            else
                s_inq[i] = it != 0xFFFFFFFFu ? cell_counts[(unsigned)(item >> 48)] : 0u;   // (a hole: nobody lists it)
        }
        if (threadIdx.x == 0)
            s_next = (unsigned)SW;   // the first item of every wave is its own number
    }
    // (LDS-DMA for this fill — no staging registers — measured: C3 -0.5 %, a rank of 8 +5 % per pipelined step.  Not taken.)
    if constexpr (CTR) {   // the batch's fp32 rows, padded to 16 dimensions (and to m_padded queries) with zeros
        const int kq = K > 0 ? K : krt;
        for (int i = threadIdx.x; i < m_padded * 16; i += 64 * SW)
            ((float *)s_dyn)[i] = (i >> 4) < m && (i & 15) < kq ? Q[(size_t)(i >> 4) * kq + (i & 15)] : 0.0f;
    } else if constexpr (U8) {   // bin frames: the B operands at the bins' scale (x 2^e: exact) and every query's threshold
        const _Float16 rt = (_Float16)self.bin_ratio;
        for (int i = threadIdx.x; i < m_padded * 2; i += 64 * SW)
            s_qf[i] = qfg[i] * rt;
        const int kq = K > 0 ? K : krt;
        for (int i = threadIdx.x; i < m_padded; i += 64 * SW) {
            const size_t at = (size_t)(i >> 5) * 64 + (size_t)(i & 31);
            s_thr[i] = knn_u8_bin_threshold(kq, qfg[at] * rt, qfg[at + 32] * rt, self.dup[i], self.bin_ratio, self.bin_er,
                                            self.bin_nmax, self.bin_w1);
        }
    } else {
        for (int i = threadIdx.x; i < m_padded * 2 * KT; i += 64 * SW)
            s_qf[i] = qfg[i];
    }
    if constexpr (CTR || !U8)
        for (int i = threadIdx.x; i < m_padded; i += 64 * SW)
            s_thr[i] = thrg[i];
    if constexpr (SELF || CTR)
        for (int i = threadIdx.x; i < m_padded; i += 64 * SW)
            s_dup[i] = self.dup[i];
    __syncthreads();
    if (s_flag != 0u)
        return;
    SCAN_STAMP(1);
    f4v *my_nrm = s_nrm + wib * (TPP * 8);
    unsigned short *my_list = s_lists + (SELF ? wib * (int)CELL_SELF_CAP : 0);

    u64 *__restrict__ my_rec = rec + (size_t)wave * slice;
    unsigned cnt = 0u;
    bool dead = false;                  // the shared area is over-full: stop scanning (wave-uniform)
    const int col = lane & 31, half = lane >> 5;
    // DYN = false: wave w takes items w, w + W, ... (an item = a run of tiles of one cell; uniform data: one item per cell):
    // all waves read one moving window of the layout (contiguous ranges per wave: +6 %).
    // DYN = true: the block owns a share of the items (see above) and its waves take them
    // one by one from a counter in LDS — with the fixed deal the busiest wave of a 2^21-row shard had 115 tile steps against
    // 48.5 on average (lists of 76..160 queries, cells of 5..9 tiles) and the launch lasted as long as that wave.
    // DYN: the chunk of the block's run whose tables are in LDS (the first one was filled above), this wave's item in it
    unsigned c0 = i0, nc = min((unsigned)CELL_SCAN_CHUNK, i1 - i0), mine_dyn = (unsigned)wib;
    for (unsigned g0 = 0u;; g0 += 64u) {
        unsigned v_meta = 0u, v_tb = 0u, v_nq = 0u;
        if constexpr (DYN) {
            if (g0 == 0u && c0 >= i1)
                break;
            if (g0 != 0u && mine_dyn >= nc) {   // block-uniform in effect: every wave runs dry before the barrier lets anyone on
                c0 += CELL_SCAN_CHUNK;
                if (c0 >= i1)
                    break;
                nc = min((unsigned)CELL_SCAN_CHUNK, i1 - c0);
                __syncthreads();   // everybody is done with the previous chunk's tables
                for (unsigned i = threadIdx.x; i < nc; i += 64 * SW) {
                    const unsigned it = slot_item(c0 + i);
                    const u64 item = it != 0xFFFFFFFFu ? items[it] : 0ull;
                    s_imeta[i] = (unsigned)(item >> 40);
                    s_itb[i] = (unsigned)item;
                    if constexpr (SELF)
                        s_inq[i] = it != 0xFFFFFFFFu ? 1u : 0u;
                    else
                        s_inq[i] = it != 0xFFFFFFFFu ? cell_counts[(unsigned)(item >> 48)] : 0u;
                }
                if (threadIdx.x == 0)
                    s_next = (unsigned)SW;   // the first item of every wave is its own number
                __syncthreads();
                mine_dyn = (unsigned)wib;
            }
            if (mine_dyn < nc && lane == 0 && !dead) {
                v_meta = s_imeta[mine_dyn];
                v_tb = s_itb[mine_dyn];
                v_nq = s_inq[mine_dyn];
            }
        } else {
            if (g0 >= per_wave || dead)
                break;
            // cells, list lengths and tile ranges of up to 64 items, one per lane
            // (measured and not kept, round 3: handing the cells out through an odd multiplier — cells w, w + W, ... share their
            // low bits and with them the queries that list them, the busiest wave has twice the average number of tile steps —
            // left the 2^21-row shard where it was and cost C3 4 %: the moving window over the layout is worth more than the balance)
            const unsigned mine = (g0 + (unsigned)lane) * nwaves + wave;
            const bool in = g0 + (unsigned)lane < per_wave && mine < nitems;
            const u64 item = in ? items[mine] : 0ull;
            v_meta = (unsigned)(item >> 40);   // cell << 8 | tiles
            v_tb = (unsigned)item;
            if constexpr (SELF)
                v_nq = in ? 1u : 0u;   // (the list is made when the item is taken)
            else
                v_nq = in ? cell_counts[v_meta >> 8] : 0u;
        }
        for (u64 todo = __ballot(v_nq != 0u); todo != 0ull && !dead; todo &= todo - 1ull) {
            const int j = (int)__builtin_ctzll(todo);
            const unsigned tb = (unsigned)__builtin_amdgcn_readlane((int)v_tb, j);
            const unsigned meta = (unsigned)__builtin_amdgcn_readlane((int)v_meta, j);
            const unsigned te = tb + (meta & 0xFFu);
            const unsigned cellj = meta >> 8;
            unsigned nq;
            if constexpr (SELF) {
                __builtin_amdgcn_wave_barrier();   // the previous item's reads of the list room are done
                nq = cell_self_list(self.lo_t, self.hi, self.sa, m_padded, cellj, m, s_dup, my_list, lane);
                wave_lds_sync();
                if (nq == 0u)   // (wave-uniform) nobody wants this cell
                    continue;
            } else {
                nq = (unsigned)__builtin_amdgcn_readlane((int)v_nq, j);
            }
            // a list longer than its room (a thousand copies of one query all want the same cells) is cut short by the
            // match kernel: the cell is then scored `dense`, against every query of the batch — what a list that long
            // asks for anyway — instead of sending the batch to the exact scan as round 2 did
            const bool dense = nq > cap;
            const unsigned nq_room = min(nq, cap);   // entries of the list's room that hold queries (>= 1)
            if (dense) {
                nq = (unsigned)m;
                if (lane == 0)
                    atomicAdd(&ctl[KNN_CTL_DENSE_CELLS], 1u);   // rare; statistics only
            }
            const unsigned short *__restrict__ list = SELF ? my_list : lists + (size_t)cellj * cap;
            // the first two blocks of the list travel with the tiles (one round trip per cell)
            // (SELF: the list is in LDS — every block of 32 is read from there)
            // (ONE_TRIP: read whether dense or not, inside the room, and the dense case taken where the words are used: a select
            // here made the wave wait for l0 before it asked for l1, w_c and the tiles — three round trips per item, not one)
            unsigned l0 = SELF ? 0u : ONE_TRIP ? (unsigned)list[min((unsigned)lane, nq_room - 1u)] : dense ? (unsigned)lane : (unsigned)list[min((unsigned)lane, nq - 1u)];
            // (round 3: blocks three and four of the list too — lists average 120 entries on the 2^21-row shards of an
            // 8-GPU run, and every block beyond the second was a dependent read from memory)
            unsigned l1 = SELF ? 0u : ONE_TRIP ? (unsigned)list[min(64u + (unsigned)lane, nq_room - 1u)] : dense ? 64u + (unsigned)lane : (unsigned)list[min(64u + (unsigned)lane, nq - 1u)];
            float ccv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, c_scale = 0.f, c_ratio = 0.f, c_bmax = 0.f, c_nmax = 0.f, c_er = 0.f, th_kept = 0.f;
            h8 b_kept = {0, 0, 0, 0, 0, 0, 0, 0};
            h8 wc = {0, 0, 0, 0, 0, 0, 0, 0};   // bin frames: this lane's half of the cell's offset w_c
            if constexpr (U8 && !CTR) {
                if constexpr (TOPK) {   // (the record-only form hoists this lane's part of the address out of the item loop and
                    unsigned hw = (unsigned)half;   //  spills it under the 80-register cap: made here, per item)
                    __asm__ volatile("" : "+v"(hw));
                    wc = ((const h8 *)self.binw)[(size_t)cellj * 2 + hw];
                } else {
                    wc = ((const h8 *)self.binw)[(size_t)cellj * 2 + half];
                }
            }
            if constexpr (CTR) {   // the cell's frame: this lane's half of the centre, the scale, the cell's bounds
                const float *__restrict__ fr = self.frame + (size_t)cellj * KNN_CELL_FRAME_WORDS;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    ccv[j] = fr[8 * half + j];
                c_scale = fr[16];
                c_ratio = fr[17];
                c_bmax = fr[18];
                c_nmax = fr[19];
                if constexpr (U8) {   // the 8-bit rows' error and norm bounds
                    c_er = self.cell_u8[(size_t)cellj * 2];
                    c_nmax = self.cell_u8[(size_t)cellj * 2 + 1];
                }
            }
            for (unsigned t0 = tb; t0 < te && !dead; t0 += TPP) {
                const int nt = (int)min((unsigned)TPP, te - t0);   // wave-uniform
                h8 ar[U8 ? 1 : TPP][KT];
                u2v a8[U8 ? TPP : 1];   // (U8: widened at every step — two registers per tile held instead of four)
#pragma unroll
                for (int p = 0; p < TPP; ++p)
                    if (p < nt) {
                        if constexpr (U8) {
                            a8[p] = __builtin_nontemporal_load(&((const u2v *)rf)[(size_t)(t0 + (unsigned)p) * 64 + lane]);
                        } else {
#pragma unroll
                            for (int kk = 0; kk < KT; ++kk)
                                ar[U8 ? 0 : p][kk] = __builtin_nontemporal_load(&rf[((size_t)(t0 + (unsigned)p) * KT + kk) * 64 + lane]);
                        }
                    }
                if constexpr (!NIF) {
                    const f4v *__restrict__ rn4 = (const f4v *)rn + (size_t)t0 * 8;
                    const f4v n0 = lane < nt * 8 ? __builtin_nontemporal_load(&rn4[lane]) : (f4v){0.f, 0.f, 0.f, 0.f};
                    f4v n1 = {0.f, 0.f, 0.f, 0.f};
                    if constexpr (TPP * 8 > 64)
                        n1 = 64 + lane < nt * 8 ? __builtin_nontemporal_load(&rn4[64 + lane]) : (f4v){0.f, 0.f, 0.f, 0.f};
                    if constexpr (ONE_TRIP)   // first used here, behind the pass's loads: nothing hoists a use (the w_c widening,
                        __asm__ volatile("" : "+v"(l0), "+v"(l1), "+v"(wc));   // a lane select) in front of them
                    __builtin_amdgcn_wave_barrier();   // the previous pass's reads of the window are done
                    if (TPP * 8 >= 64 || lane < TPP * 8)
                        my_nrm[lane] = n0;
                    if constexpr (TPP * 8 > 64)
                        if (lane < TPP * 8 - 64)
                            my_nrm[64 + lane] = n1;
                    wave_lds_sync();
                }
                for (unsigned q0 = 0u; q0 < nq && !dead; q0 += 32u) {
                    const unsigned idx = q0 + (unsigned)col;
                    const bool valid = idx < nq;
                    unsigned qid;
                    if constexpr (SELF) {
                        qid = dense ? (valid ? idx : 0u) : (unsigned)my_list[valid ? idx : 0u];
                    } else if (q0 < 64u) {
                        const unsigned from = __shfl(l0, (int)idx, KNN_WAVE);
                        qid = valid ? from : __shfl(l0, 0, KNN_WAVE);
                    } else if (q0 < 128u) {
                        const unsigned from = __shfl(l1, (int)(idx - 64u), KNN_WAVE);
                        qid = valid ? from : __shfl(l0, 0, KNN_WAVE);
                    } else {
                        qid = dense ? (valid ? idx : 0u) : (unsigned)list[valid ? idx : 0u];
                    }
                    if constexpr (ONE_TRIP)   // (l0 / l1 are list words even for a dense cell)
                        qid = dense ? (valid ? idx : 0u) : qid;
                    h8 b[KT];
                    float th;
                    if constexpr (CTR) {
                        // (an item of several passes whose list is one block of queries — 16 queries per cluster cell on 64 tight
                        // clusters — keeps the block's operand from its first pass)
                        if (t0 == tb || nq > 32u)
                            cell_centred_operand<U8>((const float *)s_dyn, K > 0 ? K : krt, qid, half, valid, ccv, c_scale, c_ratio, c_bmax, c_nmax, c_er,
                                                 s_dup[qid], s_thr[qid], b_kept, th_kept);
                        b[0] = b_kept;
                        th = th_kept;
                    } else {
#pragma unroll
                        for (int kk = 0; kk < KT; ++kk)
                            b[kk] = s_qf[((qid >> 5) * KT + (unsigned)kk) * 64u + (unsigned)half * 32u + (qid & 31u)];
                        th = valid ? s_thr[qid] : -INFINITY;
                        if constexpr (U8) {   // bin frames: the pair term B.w_c (exact fp32 products, fp32 sums in dimension order —
                                              // no FMA or dot instruction in this kernel; the rounding is in s_thr)
                            float dw = (float)b[0][0] * (float)wc[0];
#pragma unroll
                            for (int i = 1; i < 8; ++i)
                                dw = dw + (float)b[0][i] * (float)wc[i];
                            dw = dw + __shfl_xor(dw, 32, KNN_WAVE);
                            th = th - dw;
                        }
                    }
                    // (a hit is recorded right behind its tile: parking the nine masks of a pass until its end, as round 2
                    // did, kept 18 registers busy with them — the allocator put the mask pairs in VGPRs)
#pragma unroll
                    for (int p = 0; p < TPP; ++p) {
                        if (p < nt) {
                            u64 mask;
                            if constexpr (U8) {
                                if constexpr (!CTR)   // (else the widened tiles, invariant over the blocks of queries, are hoisted
                                    __asm__ volatile("" : "+v"(a8[p]));   //  out of that loop: 36 registers under the 80-register cap)
                                const h8 a1[1] = {cell_widen_u8(a8[p])};
                                mask = cell_tile_step<1>(a1, my_nrm, p, half, b, th);
                            } else {
                                mask = NIF ? cell_tile_step_nif<KT>(ar[p], b, th) : cell_tile_step<KT>(ar[p], my_nrm, p, half, b, th);
                            }
                            if (__builtin_expect(mask != 0ull, 0)) {
                                const bool hit = (mask >> lane) & 1ull;
                                const unsigned pos = cnt + __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                                                                     __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                                unsigned hh = (unsigned)half;
                                if constexpr (U8 && !CTR)   // (else the nine tiles' record words are made ahead of the query loop:
                                    __asm__ volatile("" : "+v"(hh));   //  18 registers, spilled under the 80-register cap)
                                const u64 r = ((u64)qid << 32) | ((u64)(t0 + (unsigned)p) << 1) | (u64)hh;
                                if (hit && pos < slice)
                                    my_rec[pos] = r;
                                const unsigned total = cnt + (unsigned)__popcll(mask);
                                if (total > slice && ovf_cap != 0u) {   // wave-uniform
                                    // this wave's slice is full (many queries of the batch want the same tile — copies of one
                                    // query): what does not fit goes to the area all waves share, ONE atomic per step for the
                                    // lanes that need room there, none once the area is over-full
                                    const unsigned first_over = max(cnt, slice);
                                    unsigned obase = ovf_cap;
                                    if (lane == 0 && !dead)
                                        obase = atomicAdd(&ctl[KNN_CTL_RECORDS], total - first_over);
                                    obase = (unsigned)__builtin_amdgcn_readfirstlane((int)obase);
                                    if (hit && pos >= slice) {
                                        const unsigned op = obase + (pos - first_over);
                                        if (op < ovf_cap)
                                            rec[(size_t)ovf_base + op] = r;   // (beyond: the re-rank sees the count and falls back)
                                    }
                                    // Slice full AND the shared area over-full (what the atomic returned says so; a plain read
                                    // of a word other XCDs are adding to can stay stale in this XCD's L2): the fp16 scores do not
                                    // separate this batch's rows (a cluster tighter than the fp16 step — every row of a query's
                                    // cells is a candidate).  The re-rank will see the count and hand the batch's listed pairs to
                                    // knn_cells_exact_kernel; nothing this wave still finds is needed.  The loops around the
                                    // steps look at `dead`; a jump out of the unrolled steps cost every step of every batch six
                                    // instructions of exec bookkeeping.
                                    dead = obase + (total - first_over) > ovf_cap;
                                }
                                const unsigned steps_new = (total / CELL_PUBLISH_STEP - cnt / CELL_PUBLISH_STEP) * CELL_PUBLISH_STEP;
                                cnt = total;
                                // Is this a batch the fp16 scores cannot separate (rows of a cluster tighter than the fp16 step:
                                // millions of candidates)?  Then it goes to the exact evaluation of its listed pairs, which costs
                                // the same whatever was recorded, and every record and tile step from here on is wasted — round 4
                                // noticed only when a wave's own slice AND the shared area were full, i.e. when all 6144 slices
                                // were (64 tight clusters: 3.6 M records, scan 69 -> 183 us).  Now: every 64th wave publishes its
                                // count in steps of CELL_PUBLISH_STEP records (a SAMPLE of the batch's total: a returning atomic on
                                // one word costs ~26 ns and they queue — all waves publishing took the scan to 0.4 ms); when the
                                // sample says CELL_BATCH_RECORD_LIMIT is passed, the publisher marks the shared area over-full, and
                                // every wave looks at that word (an agent-scope load, no atomic) whenever its own count crosses a
                                // step.  A clean batch — a few records per wave — never gets here.
                                // (not in the self-listing variant: its registers are all taken — 8 bytes of scratch with this in —
                                // and it serves shards of <= 2^13 cells one batch at a time, where the slices are large)
                                if (!SELF && steps_new != 0u && ovf_cap != 0u) {   // wave-uniform
                                    if ((wave & 63u) == 0u) {
                                        unsigned seen = 0u;
                                        if (lane == 0)
                                            seen = atomicAdd(&ctl[KNN_CTL_TOTAL], steps_new) + steps_new;
                                        seen = (unsigned)__builtin_amdgcn_readfirstlane((int)seen);
                                        if (seen > (TOPK ? CELL_TOPK_RECORD_LIMIT : CELL_BATCH_RECORD_LIMIT) / 64u) {
                                            unsigned full = ovf_cap;
                                            if constexpr (TOPK && CTR)   // (the record-only per-cell-frame forms: ovf_cap + 1 is made here, in this
                                                __asm__ volatile("" : "+s"(full));   //  rare branch — hoisted out of the item loop as a vector register it was spilled: 8 bytes of scratch in the 8-bit form)
                                            if (lane == 0)
                                                atomicMax(&ctl[KNN_CTL_RECORDS], full + 1u);   // what the tail kernel reads as "over-full"
                                            dead = true;
                                        }
                                    } else if (__hip_atomic_load(&ctl[KNN_CTL_RECORDS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > ovf_cap) {
                                        dead = true;
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
        if constexpr (DYN) {   // the next item of the chunk (an index past its end: the chunk is done for this wave)
            unsigned nx = 0u;
            if (lane == 0)
                nx = dead ? nc : atomicAdd(&s_next, 1u);
            mine_dyn = (unsigned)__builtin_amdgcn_readfirstlane((int)nx);
        }
    }
    SCAN_STAMP(2);
    const unsigned nrec = min(cnt, slice);   // what is IN the slice; the rest went to the shared area (wave-uniform)
    if (lane == 0)
        counts[wave] = nrec;                  // (statistics: knn_index_last_stats sums them)
#ifndef KNN_CELLS_SCAN_RECORD_ONLY   // (defined by knn_cells_records_kernel around its include: the record-only form ends here —
                                    //  knn_topk_rerank_gated_kernel reads counts[] and the slices; R, perm, keys, fin do not exist there)
    // ---- this wave's records, re-ranked on the spot (round 4; rounds 1-3 launched knn_rerank_kernel behind the scan: one
    // wave per list, 8-9 us for ~3000 records spread over 6144 lists).  16 lanes per record: its 16 rows with v0's
    // arithmetic on the fp32 rows, min-folded, ONE guarded atomic per record.  The loop above is over: its registers are free.
    // A LONG list is not re-ranked here: it is left where it is and the tail kernel, which sees the whole batch, either
    // re-ranks it with every CU or — when the shared area ended up over-full — drops it for the exact evaluation of the
    // batch's listed pairs.  (Round 4's first form re-ranked whatever a wave had: on 64 tight clusters (n 2^22) every wave
    // filled its slice of 586 records while the shared area was still filling, re-ranked them for 270 us on average — and the
    // batch then went to the exact evaluation anyway: scan 69 -> 566 us, step 0.32 -> 0.78 ms, profiles/r04_distribution_check.txt.)
    if (nrec > CELL_INLINE_RERANK_MAX && !dead && lane == 0)
        __hip_atomic_store(&ctl[KNN_CTL_DEFERRED], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (every writer stores 1)
    if (nrec != 0u && nrec <= CELL_INLINE_RERANK_MAX && !dead) {
        // the records were stored by other lanes of this wave: wait for the stores, no more — workgroup scope is this CU's own
        // cache.  (An agent-scope fence here, __threadfence(), is a write-back AND an invalidate of the XCD's whole L2 — one per
        // wave with records: the scan took 261 us instead of 110 at C3 with it.)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const int k = K > 0 ? K : krt;
        for (unsigned c0 = 0u; c0 < nrec * 16u; c0 += 64u) {
            const unsigned c = c0 + (unsigned)lane;
            const bool live = c < nrec * 16u;
            // one dependent chain per pair — record -> position -> row number -> row — with everything that does not hang on
            // it (the query's row, its current key) requested up front
            const u64 e = live ? __hip_atomic_load(&my_rec[c >> 4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0ull;
            const unsigned qi = (unsigned)(e >> 32), lo = (unsigned)e, reg = c & 15u;
            const long long pos = (long long)(lo >> 1) * 32 + 8 * (reg >> 2) + 4 * (lo & 1u) + (reg & 3u);
            const unsigned row = live && pos < npos ? perm[pos] : 0xFFFFFFFFu;   // ~0u: padding position
            const float *__restrict__ qp = Q + (size_t)qi * k;
            constexpr int KD = K > 0 ? K : 16;
            const u64 cur = keys[qi];   // (may be stale: keys[] only ever decreases, a stale read costs a spare atomic)
            const float *__restrict__ rp = R + (size_t)(row != 0xFFFFFFFFu ? row : 0u) * k;
            float acc = 0.0f;
#pragma unroll
            for (int ch = 0; ch < KT; ++ch) {   // (KT = 2: dimensions 16 .. 31 behind 0 .. 15, the same registers again)
                float qv[KD], rv[KD];
#pragma unroll
                for (int d = 0; d < KD; ++d)
                    qv[d] = 16 * ch + d < k ? qp[16 * ch + d] : 0.0f;
#pragma unroll
                for (int d = 0; d < KD; ++d)
                    rv[d] = 16 * ch + d < k ? rp[16 * ch + d] : 0.0f;
#pragma unroll
                for (int d = 0; d < KD; ++d)
                    if (16 * ch + d < k) {   // v0's order and operations: diff, square, add (no contraction)
                        const float diff = qv[d] - rv[d];
                        const float sq = diff * diff;
                        acc = acc + sq;
                    }
            }
            u64 key = row != 0xFFFFFFFFu && acc < INFINITY ? pack_key(acc, (unsigned)(base + (long long)row)) : ~0ull;
            // (ds_swizzle's xor mode, not __shfl_xor: that one wants every lane's number in a register, computed at the top of
            // the kernel and kept across the item loop — 4 bytes of scratch under the 80-register cap)
#define KNN_SWZ_MIN(OFF)                                                                                   \
            {                                                                                              \
                const unsigned olo = (unsigned)__builtin_amdgcn_ds_swizzle((int)(unsigned)key, ((OFF) << 10) | 0x1F);         \
                const unsigned ohi = (unsigned)__builtin_amdgcn_ds_swizzle((int)(unsigned)(key >> 32), ((OFF) << 10) | 0x1F); \
                const u64 o = ((u64)ohi << 32) | (u64)olo;                                                 \
                key = o < key ? o : key;                                                                   \
            }
            KNN_SWZ_MIN(8)
            KNN_SWZ_MIN(4)
            KNN_SWZ_MIN(2)
            KNN_SWZ_MIN(1)
#undef KNN_SWZ_MIN
            if ((lane & 15) == 0 && key < cur)   // (key == ~0: never below a key)
                key_atomic_min(&keys[qi], key);
        }
    }
    // ---- end of the batch: the block that finishes last finalises it, unless something is still to fold into the keys
    // (records in the shared area, an over-full area, rows outside the box) — then the tail kernel does, which sees the
    // same two words and returns at once in the case handled here.
    // (What the finaliser reads from other blocks are words they changed with agent-scope ATOMICS — the keys, the record
    // counter, the DEFERRED flag: those are performed at the memory side, no cache to write back.  Every wave waits for its
    // own atomics to have been PERFORMED before the block counts itself done — cells_wait_own_atomics: the workgroup-scope
    // release fence alone compiles to `s_waitcnt lgkmcnt(0)` on gfx950 and leaves the no-return atomics in flight (ADVICE
    // r04; tests/test_host_logic.py reads the ISA for the vmcnt(0)) — and the finaliser reads with agent-scope loads.)
    __shared__ unsigned s_last;
    SCAN_STAMP(3);
    cells_wait_own_atomics();
    __syncthreads();
    if (threadIdx.x == 0)
        s_last = __hip_atomic_fetch_add(&ctl[KNN_CTL_SCAN_DONE], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u ? 1u : 0u;
    __syncthreads();
    if (s_last != 0u && !fin.defer) {   // block-uniform
        const unsigned have = __hip_atomic_load(&ctl[KNN_CTL_RECORDS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) |
                              __hip_atomic_load(&ctl[KNN_CTL_DEFERRED], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (have == 0u)
            cells_finalize(keys, m, fin, threadIdx.x, 64u * SW);
    }
    SCAN_STAMP(4);
#endif
