// knn_grid_radius_body.inc — the one walk of the grid's radius kernels (KNN_QUERY_COUNT_GRID): included into knn_grid_count_kernel,
// knn_grid_list_kernel, their each-forms, their self forms and their masked forms (knn_grid.hip), which fix four compile-time
// switches —
//   LIST    a hit reserves a place and stores its key; else it bumps the lane's register;
//   EACH    the wave's own radius radii[qi] under cap (include/knn_mi355x.h 2j); else the scalar radius cap, radii not read;
//   SELF    query qi is the shard's LOCAL row first + qi, and that row is no hit (2k);
//   MASKED  a row is a hit only when the bit of its LOCAL number is set in mask (2l)
// — and provide KD, the arguments Q, m, gg, start, pts, rmax, giveup, giveup_next by their names, and every one of orig, first,
// base, out, offsets, cursor, keys, radii, cap, mask: as its argument, or as a constant null / zero stand-in where the form has none.
//
// One wave per query on grid_walk (knn_grid.hip): lanes take the cells of ring r, and a row is a hit when its v0 distance E is finite,
// E <= rad and E <= cap (fp32 compares, equality inside; the scalar forms' rad is cap, so theirs is one compare).  One wave per
// query, so radii[qi] is wave-uniform as the scalar radius is.
// Stop rule, after ring r: the block of rings 0..r is the whole grid, or bound < lb^2 (1 - 1e-6) — the radius clause of
// knn_grid_within_kernel: every unseen row's computed distance is strictly above that bound, so none is within the radius; the test
// is wave-uniform (the query, its cell and r decide it).  The clause takes the query's bound (knn_each_radius.h; the scalar forms'
// is cap): every hit lies within it, and rmax is made from cap's rings, so a query whose bound is below cap stops no later than the
// scalar call at cap would.  Past rmax rings the query raises the give-up word (the slot's two words alternate as in the other grid
// kernels).  No LDS, no block barrier.
// Every cell of rings 0..r is visited once (grid_ring_cell: a position of the (2r+1)^K block belongs to exactly one ring), every row
// sits in one cell: no row is counted or listed twice.
// Counts: one wave reduction at the end, lane 0 stores the query's count to out[q] — the slot's scratch, never the caller's counts: a
// batch that gives up is answered again by the exact count behind this kernel, and knn_count_commit_kernel adds the scratch only when
// nobody gave up.
// Lists: a hit reserves place p of its query's segment with one atomicAdd on cursor[q] and, when p is below the segment's room,
// stores its key — the distance's bits and base + orig[position] — at keys[offsets[q] + p].  cursor is the slot's scratch, on entry
// a copy of the caller's fill, never the caller's fill itself: a batch that gives up is answered again by the exact list behind
// this kernel from the untouched fill, over the same places, and knn_list_commit_kernel copies the cursor to fill only when nobody
// gave up.
// A query without candidates — a non-finite coordinate (every distance is NaN or +INF), or with EACH a NaN or negative radius —
// walks nothing, counts 0 / leaves its cursor where it was, and never raises the give-up word: there is nothing to give up on.
// SELF: Q = R + first * k, the rows themselves, and the row at position p is no hit when orig[p] == first + qi — identity by local
// row number: another copy of the row stays a hit at distance 0.  The compare sits on the hit side, behind the distance; the walk,
// the stop clause, the give-up word and what the commit sees are the twins'.  (The self list reads orig[p] once, before the
// reservation; the other lists read it only at the store.)
// MASKED: the row at position p is a hit only when bit orig[p] & 31 of mask[orig[p] >> 5] is set — the caller's mask, in the shard's
// local row order, read by the rows inside the radius alone: the test sits behind the distance compare, as SELF's, and nothing
// else of the walk knows of the mask (a cell is never skipped for it).  orig[p] < n, so no word beyond (n + 31) / 32 is read and
// the bits at and beyond n in the last word belong to no row.  The masked list reads orig[p] once, before the reservation.
    if (blockIdx.x == 0 && threadIdx.x == 0)
        *giveup_next = 0u;   // (the slot's other word, as the 1-NN kernel)
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * (GRID_BLOCK / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (qi >= m)
        return;
    float q[4];
    const bool finite = grid_query_load<KD>(Q, qi, q);
    const float rad = EACH ? radii[qi] : cap;
    if (!finite || (EACH && !knn_each_has(rad))) {   // no row can be a hit (and nothing to give up on)
        if (!LIST && lane == 0)
            out[qi] = 0u;
        return;
    }
    const float bound = EACH ? knn_each_bound(rad, cap) : cap;
    const unsigned own = first + (unsigned)qi;
    const u64 off = LIST ? offsets[qi] : 0ull, end = LIST ? offsets[qi + 1] : 0ull;
    const u64 room64 = end > off ? end - off : 0ull;
    const unsigned room = room64 < 0xFFFFFFFFull ? (unsigned)room64 : 0xFFFFFFFFu;   // (the cursor is 32-bit)

    unsigned cnt = 0u;
    const bool gave_up = grid_walk<KD>(
        gg, start, pts, q, lane, rmax,
        [&](float acc, unsigned p) {
            if (acc < INFINITY && acc <= rad && acc <= cap) {
                if (!LIST && MASKED) {
                    const unsigned row = orig[p];
                    cnt += (mask[row >> 5] >> (row & 31u)) & 1u;
                } else if (!LIST) {
                    cnt += !SELF || orig[p] != own ? 1u : 0u;
                } else if (SELF || MASKED) {
                    const unsigned row = orig[p];
                    if (SELF ? row != own : ((mask[row >> 5] >> (row & 31u)) & 1u) != 0u) {
                        const unsigned place = atomicAdd(&cursor[qi], 1u);
                        if (place < room)
                            keys[off + place] = ((u64)__float_as_uint(acc) << 32) | (u64)(unsigned)(base + (long long)row);
                    }
                } else {
                    const unsigned place = atomicAdd(&cursor[qi], 1u);
                    if (place < room)
                        keys[off + place] = ((u64)__float_as_uint(acc) << 32) | (u64)(unsigned)(base + (long long)orig[p]);
                }
            }
        },
        [] {}, [&](double reach) { return (double)bound < reach; });   // no unseen row is within the query's bound
    if (!LIST) {
#pragma unroll
        for (int step = 32; step > 0; step >>= 1)
            cnt += (unsigned)__shfl_xor((int)cnt, step, KNN_WAVE);
    }
    if (lane == 0) {
        if (!LIST)
            out[qi] = cnt;
        if (gave_up)
            *giveup = 1u;      // benign race: every writer stores 1
    }
