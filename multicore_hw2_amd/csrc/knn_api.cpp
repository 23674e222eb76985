// knn_api.cpp — host side of libknn_mi355x.so: the C-ABI of include/knn_mi355x.h.
//
// Mirrors the orchestration of the reference's v8::cudaCallback (sources/src/core.cu:856-958)
// for ONE purpose — same inputs, same outputs, same error behaviour — without its structure:
// one host thread per GPU like core.cu:873, but shard offsets are folded into packed keys on
// the GPU (instead of the host-side `+= offset`, core.cu:932-933) and the final reduction is an
// unsigned min over m keys per GPU (instead of the distance-recomputing CPU loop,
// core.cu:935-957, whose indexing is wrong for m > 1 — SURVEY.md §8 a2').
#include "../../include/knn_mi355x.h"
#include "knn_common.h"
#include "knn_radix_pick.h"
#include "knn_slice_launch.h"
#include "knn_mask_split.h"
#include "knn_self_window.h"
#include "knn_each_radius.h"
#include "knn_cluster_uf.h"
#include "knn_cluster_pair.h"
#include "knn_forest_pick.h"

#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <mutex>
#include <unordered_map>
#include <string>
#include <thread>
#include <vector>

namespace {

thread_local std::string g_err;

int fail(int code, const char *what, const char *detail = nullptr)
{
    g_err = what;
    if (detail) {
        g_err += ": ";
        g_err += detail;
    }
    return code;
}

// "<who>: <what>[: <detail>]" — the text of a step that several entry points share
int fail_in(int code, const char *who, const char *what, const char *detail = nullptr)
{
    const std::string text = std::string(who) + ": " + what;
    return fail(code, text.c_str(), detail);
}

#define HIP_TRY(call)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            char buf_[256];                                                                \
            snprintf(buf_, sizeof buf_, "%s:%d, code:%d, reason: %s", __FILE__, __LINE__,  \
                     (int)e_, hipGetErrorString(e_));                                      \
            g_err = buf_;                                                                  \
            return KNN_EHIP;                                                               \
        }                                                                                  \
    } while (0)

// Abort-on-error for the void drop-in entry (reference core.h:77-87: print and exit(1)).
[[noreturn]] void die(const char *file, int line, int code, const char *reason)
{
    printf("Error: %s:%d, code:%d, reason: %s \n", file, line, code, reason);
    fflush(stdout);
    exit(1);
}
#define DIE_IF(rc)                                                \
    do {                                                          \
        int rc_ = (rc);                                           \
        if (rc_ != KNN_OK)                                        \
            die(__FILE__, __LINE__, rc_, g_err.c_str());          \
    } while (0)

std::atomic<long long> g_opt_path{0};
std::atomic<long long> g_opt_shards{0};
std::atomic<long long> g_opt_filter_qt{0};
std::atomic<long long> g_opt_filter_rounds{0};
std::atomic<long long> g_opt_filter_chain{0};
std::atomic<long long> g_opt_stream{0};
std::atomic<long long> g_opt_scan_blocks{0};     // pruned scan, blocks per CU: 0 auto, 1, 2
std::atomic<long long> g_last_cells{0};          // read-only: shards of the most recent cudaCallback that were served by the pruned scan
std::atomic<long long> g_opt_sample_stride{0};   // deep-K scans: stride of the sample pass in tiles, 0 = policy
std::atomic<long long> g_opt_run_thresholds{0};  // deep-K scan: 0 / 1 running thresholds, 2 off (A/B)
std::atomic<long long> g_opt_cells_lists{0};     // pruned scan, who lists a cell's queries: 0 auto, 1 the match launch, 2 the scan's own waves
std::atomic<long long> g_opt_scan_deal{0};       // pruned scan, how waves get their items: 0 auto, 1 fixed deal, 2 block counter
std::atomic<long long> g_opt_cells_build{0};     // cell-sorted layout: 0 fast two-pass build (counted one if a bucket overflows), 1 the one-pass placement, 2 the counted two-pass build (A/B, tests)
std::atomic<long long> g_opt_topk_cells{0};      // top-K on the pruned scan: 0 policy (knn_cells_topk_plan), 1 wherever the layout allows it, 2 never
std::atomic<long long> g_opt_cells{0};       // cell-sorted layouts (k <= 16): 0 resident indexes large enough to prune (knn_index_build_plan), 1 from 2^17 rows, 2 never
std::atomic<long long> g_opt_ingest{0};      // indexes created from host rows: 0 layouts built under the copy, 1 copy then build
std::atomic<long long> g_opt_rccl{0};        // 0 auto (several GPUs, one shard each), 1 always, 2 never
std::atomic<long long> g_rccl_reductions{0}; // cudaCallback merges done by the RCCL all-reduce
std::atomic<long long> g_last_shards{0};     // shards of the most recent cudaCallback (tests, KNN_MI355X_TRACE_CALL)

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess)
            prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (prev >= 0)
            (void)hipSetDevice(prev);
    }
};

// Staging buffers of the host-input entry points (cudaCallback, knn_index_query_host, indexes created
// from host rows).  A one-shot call otherwise spends 0.3-0.5 ms in hipMalloc + hipFree (hipFree
// alone 0.22 ms) around a 0.1-0.4 ms scan at TA scale; the pool keeps up to kPoolSlots freed buffers
// per device (at most kPoolBytes in total) and hands one back when it is at least as large as, and
// at most twice, the size asked for.  Buffers are only returned to it after the stream work that
// used them has been waited for.
constexpr int kPoolDevices = 64;
constexpr size_t kPoolSlots = 64;
constexpr size_t kPoolBytes = 4ull << 30;
struct PoolEntry {
    void *p;
    size_t bytes;
};
std::mutex g_pool_mu;
std::vector<PoolEntry> g_pool[kPoolDevices];

// device `dev` must be current
hipError_t pool_get(int dev, size_t bytes, void **out)
{
    *out = nullptr;
    if (bytes == 0)
        bytes = 1;
    if (dev >= 0 && dev < kPoolDevices) {
        std::lock_guard<std::mutex> lock(g_pool_mu);
        std::vector<PoolEntry> &v = g_pool[dev];
        size_t best = v.size();
        for (size_t i = 0; i < v.size(); ++i)
            if (v[i].bytes >= bytes && v[i].bytes / 2 <= bytes && (best == v.size() || v[i].bytes < v[best].bytes))
                best = i;
        if (best != v.size()) {
            *out = v[best].p;
            v.erase(v.begin() + (long)best);
            return hipSuccess;
        }
    }
    return hipMalloc(out, bytes);
}

// `bytes` = the size the buffer was asked for with (its real size may be larger: that is fine, the
// pool then under-estimates what it holds by at most 2x)
void pool_put(int dev, void *p, size_t bytes)
{
    if (!p)
        return;
    if (bytes == 0)
        bytes = 1;
    std::vector<void *> drop;
    if (dev >= 0 && dev < kPoolDevices && bytes <= kPoolBytes) {
        std::lock_guard<std::mutex> lock(g_pool_mu);
        std::vector<PoolEntry> &v = g_pool[dev];
        size_t held = bytes;
        for (const PoolEntry &e : v)
            held += e.bytes;
        while (!v.empty() && (v.size() >= kPoolSlots || held > kPoolBytes)) {  // oldest first
            held -= v.front().bytes;
            drop.push_back(v.front().p);
            v.erase(v.begin());
        }
        v.push_back(PoolEntry{p, bytes});
    } else {
        drop.push_back(p);
    }
    for (void *d : drop)
        (void)hipFree(d);
}

// Owner of staging buffers taken from the pool on one device: they go back when it leaves scope or on release().  It
// keeps the pool's rule: unless its user has said waited() — all work that used the buffers has been waited for, by a
// blocking copy or a synchronised stream — it waits for the whole device first.
class Staging {
    int dev_;
    bool waited_ = false;
    std::vector<PoolEntry> held_;
public:
    explicit Staging(int dev) : dev_(dev) {}
    Staging(Staging &&o) noexcept : dev_(o.dev_), waited_(o.waited_) { held_.swap(o.held_); }
    ~Staging() { release(); }
    // device `dev` must be current
    template <class T> hipError_t get(T **out, size_t bytes)
    {
        const hipError_t e = pool_get(dev_, bytes, (void **)out);
        held_.push_back(PoolEntry{*out, bytes});   // (null after a failure: pool_put skips it)
        waited_ = false;
        return e;
    }
    void waited() { waited_ = true; }
    void release()
    {
        if (!waited_ && !held_.empty()) {
            DeviceGuard guard(dev_);
            (void)hipDeviceSynchronize();
        }
        for (const PoolEntry &e : held_)
            pool_put(dev_, e.p, e.bytes);
        held_.clear();
    }
};

// What one shard of a cudaCallback leaves: its m packed keys, on the host or (RCCL exchange) in `owner`'s buffer `dev`, or an error.
struct ShardKeys {
    std::vector<u64> host;
    Staging owner;
    u64 *dev = nullptr;   // (complete when rc is KNN_OK)
    int rc = 0;
    std::string err;
    explicit ShardKeys(int device) : owner(device) {}
};

std::unordered_map<void *, std::pair<int, size_t>> g_live;  // pooled buffers handed to the filter code

}  // namespace

hipError_t knn_dev_alloc(void **p, size_t bytes)
{
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess)
        return e;
    e = pool_get(dev, bytes, p);
    if (e == hipSuccess && *p) {
        std::lock_guard<std::mutex> lock(g_pool_mu);
        g_live[*p] = std::make_pair(dev, bytes);
    }
    return e;
}

// One device-wide wait covers any number of frees that follow it on this thread (knn_index_destroy gives ~15
// buffers back; a wait per buffer was 15 device-wide syncs).
static thread_local bool g_free_synced = false;
void knn_dev_free_begin_synced()
{
    (void)hipDeviceSynchronize();
    g_free_synced = true;
}
void knn_dev_free_end_synced() { g_free_synced = false; }

hipError_t knn_dev_free(void *p)
{
    if (!p)
        return hipSuccess;
    std::pair<int, size_t> info(-1, 0);
    {
        std::lock_guard<std::mutex> lock(g_pool_mu);
        auto it = g_live.find(p);
        if (it != g_live.end()) {
            info = it->second;
            g_live.erase(it);
        }
    }
    if (info.first < 0)
        return hipFree(p);
    if (!g_free_synced)
        (void)hipDeviceSynchronize();  // hipFree's implicit wait: nothing may still be using the buffer
    pool_put(info.first, p, info.second);
    return hipSuccess;
}

namespace {

// Two non-blocking streams per device for the streamed one-shot path (created once: a stream costs
// ~0.1 ms to create, more than a TA-scale call).
struct DeviceStreams {
    hipStream_t copy = nullptr, compute = nullptr;
};
DeviceStreams g_streams[kPoolDevices];

// device `dev` must be current
hipError_t streams_get(int dev, DeviceStreams *out)
{
    if (dev < 0 || dev >= kPoolDevices)
        return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(g_pool_mu);
    DeviceStreams &d = g_streams[dev];
    if (!d.copy) {
        hipError_t e = hipStreamCreateWithFlags(&d.copy, hipStreamNonBlocking);
        if (e != hipSuccess)
            return e;
    }
    if (!d.compute) {
        hipError_t e = hipStreamCreateWithFlags(&d.compute, hipStreamNonBlocking);
        if (e != hipSuccess)
            return e;
    }
    *out = d;
    return hipSuccess;
}

}  // namespace

struct knn_index {
    int device = 0;
    int k = 0;
    long long n = 0;
    long long base = 0;
    int num_cu = 256;
    const float *refs = nullptr;  // device, AoS [n][k]
    float *owned_refs = nullptr;  // set when the index copied the references itself (pooled)
    size_t owned_bytes = 0;
    long long stats[4] = {0, 0, 0, 0};
    FilterState filter;           // MFMA filter layouts + workspace (usable == false: exact only)
    GridState *grid = nullptr;    // k <= 4: uniform-grid spatial index (null: not built / ruled out)
    // the device word behind the last call's stats[2] (knn_index_last_stats): a call on the grid — its give-up word; a large
    // top-K (way 1) — the word that says the index word's passes ran
    const unsigned *grid_topk_gate = nullptr;
    int timing = 0;            // 0 off, N > 0: bracket every N-th dominant-kernel launch with events
    unsigned long long timing_seq = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;  // one pair per timed launch
    size_t events_used = 0;
    int last_slot = 0;
    bool filter_wanted = false;  // the creator asked for the filter layouts explicitly (one-shot cost model)
    unsigned long long recent_slots = 0;   // the workspace slots of the last eight calls, one byte each (newest lowest)
    int recent_calls = 0;
    bool sharded = false;        // a cell-range shard (knn_index_create_sharded): always served by the cell-pruned path
    ShardGeom geom;              // its copy of the global grid (filter.cells->geom points here)
    int rank = 0;
    // per slot, grown on first use to what knn_topk_scratch_plan says (never shrunk): the exact top-K scan's per-slice lists; the
    // filter ways' candidate lists and counters (the grid way: a folding call's lists); a radius call's unclipped lists
    struct TopkSlot {
        u64 *part = nullptr, *cand = nullptr, *lists = nullptr;
        size_t part_bytes = 0, cand_bytes = 0, lists_bytes = 0;
        u64 *count = nullptr;      // knn_index_count_within on the grid and cell ways: the per-query count scratch [m] unsigned
        size_t count_bytes = 0;
        u64 *large = nullptr;      // knn_index_query_topk_large: what knn_topk_large_plan says (histograms, select state, a fold's lists)
        size_t large_bytes = 0;
        u64 *mask = nullptr;       // the masked calls: what knn_masked_plan says (the prefix of the granules' admitted rows, their counts)
        size_t mask_bytes = 0;
        u64 *self = nullptr;       // knn_index_self_topk's through way: what knn_self_plan says (the plain call's K + 1 keys per row, a fold's K)
        size_t self_bytes = 0;
        u64 *cluster = nullptr;    // knn_index_self_cluster_within: what knn_cluster_plan says (best [n_local], the core mask when the caller keeps none)
        size_t cluster_bytes = 0;
        u64 *forest = nullptr;     // knn_index_self_forest_within: what knn_forest_plan says (candidates, picks, done bits, gate words)
        size_t forest_bytes = 0;
    } topk[KNN_SLOTS];
    // Calls on one index from several host threads are serialised (enqueueing a batch is ~20 us of host work; the GPU
    // work of different slots still overlaps): the workspaces' lazily grown buffers, the event list, the statistics and
    // the chain events are plain members.  Recursive: knn_index_query_host calls the keyed entry points.
    std::recursive_mutex mu;
};

extern "C" {

const char *knn_last_error(void) { return g_err.c_str(); }

const char *knn_version(void) { return "knn_mi355x 0.1 (gfx950)"; }

long long knn_trim(void)
{
    long long released = 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess)
        ndev = 0;
    for (int dev = 0; dev < kPoolDevices && dev < ndev; ++dev) {
        std::vector<PoolEntry> take;
        {
            std::lock_guard<std::mutex> lock(g_pool_mu);
            take.swap(g_pool[dev]);
        }
        if (take.empty())
            continue;
        DeviceGuard guard(dev);
        for (const PoolEntry &e : take) {
            (void)hipFree(e.p);
            released += (long long)e.bytes;
        }
    }
    return released;
}

int knn_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

}  // extern "C"

namespace {

// The options, one row each: name, range (and, where the range has holes, the set of values as a bit mask), where the value
// lives, and the message a value outside gets.  knn_set_option and knn_get_option both walk this table.
struct OptionRow {
    const char *name;
    long long lo, hi;
    unsigned long long allowed;          // 0: every value in [lo, hi]; else bit v set = v allowed
    std::atomic<long long> *wide;        // the value's home: one of the two
    std::atomic<int> *narrow;
    const char *message;
};
const OptionRow kOptions[] = {
    {"path", 0, 3, 0, &g_opt_path, nullptr, "knn_set_option: path must be 0, 1, 2 or 3"},
    {"shards", 0, 1024, 0, &g_opt_shards, nullptr, "knn_set_option: shards must be in [0, 1024]"},
    {"filter_qt", 0, 32, 1ull | 1ull << 2 | 1ull << 8 | 1ull << 16 | 1ull << 32, &g_opt_filter_qt, nullptr, "knn_set_option: filter_qt must be 0, 2, 8, 16 or 32"},
    {"filter_chain", 0, 2, 0, &g_opt_filter_chain, nullptr, "knn_set_option: filter_chain must be 0 (auto), 1 (chained) or 2 (free)"},
    {"stream", 0, 2, 0, &g_opt_stream, nullptr, "knn_set_option: stream must be 0 (auto), 1 (never) or 2 (whenever the shard is >= 32 MiB)"},
    {"scan_blocks", 0, 2, 0, &g_opt_scan_blocks, nullptr, "knn_set_option: scan_blocks must be 0 (auto), 1 or 2"},
    {"cells_build", 0, 2, 0, &g_opt_cells_build, nullptr, "knn_set_option: cells_build must be 0 (fast two-pass), 1 (one-pass placement) or 2 (counted two-pass)"},
    {"sample_stride", 0, 1024, 0, &g_opt_sample_stride, nullptr, "knn_set_option: sample_stride must be in [0, 1024]"},
    {"run_thresholds", 0, 2, 0, &g_opt_run_thresholds, nullptr, "knn_set_option: run_thresholds must be 0 (auto), 1 (on) or 2 (off)"},
    {"cells_centre", 0, 2, 0, nullptr, &g_knn_cells_centre, "knn_set_option: cells_centre must be 0 (auto: per-cell frames for clustered data), 1 (always) or 2 (never)"},
    {"cells_rows", 0, 2, 0, nullptr, &g_knn_cells_rows, "knn_set_option: cells_rows must be 0 (auto), 1 (fp16 fragments) or 2 (8-bit rows in per-cell frames)"},
    {"cells_u8_frame", 0, 2, 0, nullptr, &g_knn_cells_u8_frame, "knn_set_option: cells_u8_frame must be 0 (auto), 1 (per-cell frames) or 2 (per-dimension bin frames)"},
    {"topk_cells", 0, 2, 0, &g_opt_topk_cells, nullptr, "knn_set_option: topk_cells must be 0 (policy), 1 (pruned top-K wherever the layout allows it) or 2 (never)"},
    {"cells_lists", 0, 2, 0, &g_opt_cells_lists, nullptr, "knn_set_option: cells_lists must be 0 (auto), 1 (match launch) or 2 (the scan lists its own items)"},
    {"scan_deal", 0, 2, 0, &g_opt_scan_deal, nullptr, "knn_set_option: scan_deal must be 0 (auto), 1 (fixed deal) or 2 (block counter)"},
    {"cells", 0, 2, 0, &g_opt_cells, nullptr, "knn_set_option: cells must be 0 (library policy), 1 (always) or 2 (never)"},
    {"ingest", 0, 1, 0, &g_opt_ingest, nullptr, "knn_set_option: ingest must be 0 (layouts built under the copy) or 1 (copy, then build)"},
    {"rccl", 0, 2, 0, &g_opt_rccl, nullptr, "knn_set_option: rccl must be 0 (auto), 1 (always) or 2 (never: host merge)"},
    {"filter_rounds", 0, 64, 0, &g_opt_filter_rounds, nullptr, "knn_set_option: filter_rounds must be in [0, 64]"},
};
// What knn_get_option reads besides: counters nobody sets.
struct CounterRow {
    const char *name;
    long long (*read)();
};
const CounterRow kCounters[] = {
    {"cells_centred_builds", [] { return g_knn_cells_centred_builds.load(); }},   // cell-sorted layouts moved into per-cell frames so far
    {"cells_u8_bin_builds", [] { return g_knn_cells_u8_bin_builds.load(); }},     // 8-bit-row layouts built in bin frames so far
    {"cells_u8_builds", [] { return g_knn_cells_u8_builds.load(); }},             // cell-sorted layouts given 8-bit rows so far
    {"rccl_reductions", [] { return g_rccl_reductions.load(); }},                 // cudaCallback merges done by RCCL so far
    {"rccl_comm_sets", [] { return (long long)knn_rccl_comm_sets(); }},           // RCCL communicator sets created by this process (at most one)
    {"last_shards", [] { return g_last_shards.load(); }},                         // GPUs / shards the most recent cudaCallback was split over
    {"last_cells", [] { return g_last_cells.load(); }},                           // how many of them the pruned scan served
    {"rccl_version", [] { return (long long)knn_rccl_version(); }},               // NCCL_VERSION_CODE of the loaded RCCL, 0 if none
};

}  // namespace

extern "C" {

int knn_set_option(const char *name, long long value)
{
    if (!name)
        return fail(KNN_EINVAL, "knn_set_option: null name");
    for (const OptionRow &o : kOptions) {
        if (strcmp(name, o.name))
            continue;
        if (value < o.lo || value > o.hi || (o.allowed && !(o.allowed >> value & 1ull)))
            return fail(KNN_EINVAL, o.message);
        if (o.wide)
            *o.wide = value;
        else
            *o.narrow = (int)value;
        return KNN_OK;
    }
    return fail(KNN_EINVAL, "knn_set_option: unknown option", name);
}

long long knn_get_option(const char *name)
{
    if (!name)
        return -1;
    for (const OptionRow &o : kOptions)
        if (!strcmp(name, o.name))
            return o.wide ? o.wide->load() : (long long)o.narrow->load();
    for (const CounterRow &c : kCounters)
        if (!strcmp(name, c.name))
            return c.read();
    return -1;
}

}  // extern "C"

// What an index is built with (knn_common.h; tests/test_route_logic.py restates it through knn_debug_index_build_plan).
IndexBuildPlan knn_index_build_plan(const IndexBuildInputs &in)
{
    IndexBuildPlan p;
    const int k = in.k;
    const long long n = in.n_local;
    // MFMA filter layouts (skipped for small shards and when the exact path is forced)
    p.filter_wanted = in.build_filter > 0;
    // cell-sorted layout for the pruned scan: indexes the caller keeps (library policy) or on request; the
    // one-shot cudaCallback asks for explicit layouts and answers one batch, which does not repay the sort.
    // Pruning needs enough cells for the dimension: measured on uniform data at m = 1024 (profiles/r02_cells_policy.txt)
    // the pruned scan wins from 2^19 rows for k <= 12 and from 2^20 rows for k = 13..16; below that the lists
    // hold most of the batch and the full scan's register-resident loop is the faster way to score them.
    // (16 < k <= 32, round 5: the cells cut the first 16 dimensions; policy from the measurements in profiles/r05_cells_k17_32.txt:
    // uniform data, m = 1024, ms per step pruned / full scan on one box — n = 2^24: k 17 0.211 / 0.94, 20 0.265 / 0.96, 22 0.424 / 0.962,
    // 24 0.625 / 0.976, 25 0.716 / 0.980, 26 1.06 / 0.99 (loses); n = 2^23: k 21 0.238 / 0.465, 23 0.354 / 0.476, 24 0.445 / 0.477 (a wash),
    // 25 0.579 / 0.480 (loses); n = 2^22: k 20 0.143 / 0.25, 21 0.174 / 0.236, 22 0.220 / 0.240 and 23 0.219 / 0.243 (a wash), 24 loses)
    p.want_cells = k <= 32 && n >= (1ll << 17) &&
                   (in.cells == 1 || (in.cells == 0 && in.build_filter == 2) ||
                    (in.cells == 0 && in.build_filter < 0 && n >= knn_cells_size_rule(k)));
    p.build_filter = in.build_filter;
    if (in.build_filter < 0) {
        // library policy: shards of >= 65536 rows; for 32 < k <= 4096 (3k+3 exact lane-ops per pair,
        // one query per lane above k = 64, row-per-lane kernels above 128) the MFMA filter pays off from 4096 rows already
        p.build_filter = in.path == 2 || n >= 65536 || (k > 32 && k <= KNN_FILTER_MAX_K && n >= 4096);
        p.filter_wanted = p.build_filter && n < 65536 && in.path != 2;
    }
    // k <= 4: the uniform-grid index — resident shards of >= 16384 rows, or whenever forced
    p.grid_planned = k <= 4 && (in.path == 3 || (in.path == 0 && in.build_grid != 0 && (in.build_grid > 0 || n >= 16384)));
    // (a shard the grid index will serve gets no MFMA layouts unless the grid turns out to be ruled out)
    p.want_layouts = n > 0 && in.path != 1 && in.path != 3 && p.build_filter;
    // host rows: the layouts are built under the copy (the cell sort: its fast build's bucket pass) unless option `ingest` says
    // copy first or the grid index comes first
    if (n > 0 && !in.refs_on_device && p.want_layouts && !p.grid_planned && in.ingest != 1) {
        if (!p.want_cells)
            p.ingest = IngestForm::LayoutsUnderCopy;
        else if (in.cells_build == 0)
            p.ingest = IngestForm::CellsUnderCopy;
    }
    return p;
}

namespace {
// build_filter: 1 build the MFMA filter layouts, 2 build them cell-sorted (the pruned scan), 0 do not, -1 library policy
// build_grid (k <= 4): 1 build the grid index, 0 do not, -1 library policy
int index_create_impl(knn_index **out, int device, int k, long long n_local, const float *refs,
                      int refs_on_device, long long base_index, void *stream, int build_filter, int build_grid = -1)
{
    if (!out)
        return fail(KNN_EINVAL, "knn_index_create: null out");
    *out = nullptr;
    if (k < 1 || n_local < 0 || base_index < 0 || (n_local > 0 && !refs))
        return fail(KNN_EINVAL, "knn_index_create: bad k, n_local, base_index or refs");
    if (base_index + n_local > 0x7FFFFFFFll + 1)
        return fail(KNN_EINVAL, "knn_index_create: global index exceeds int32 (results are int)");
    int ndev = knn_device_count();
    if (ndev < 1)
        return fail(KNN_ENODEV, "knn_index_create: no HIP device visible");
    if (device < 0 || device >= ndev)
        return fail(KNN_EINVAL, "knn_index_create: device out of range");
    DeviceGuard guard(device);
    if (!guard.ok)
        return fail(KNN_EHIP, "knn_index_create: hipSetDevice failed");

    knn_index *idx = new (std::nothrow) knn_index();
    if (!idx)
        return fail(KNN_ENOMEM, "knn_index_create: out of host memory");
    idx->device = device;
    idx->k = k;
    idx->n = n_local;
    idx->base = base_index;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        idx->num_cu = prop.multiProcessorCount;

    hipStream_t s = (hipStream_t)stream;
    const IndexBuildPlan plan = knn_index_build_plan({k, n_local, refs_on_device != 0, build_filter, build_grid, (int)g_opt_path,
                                                      (int)g_opt_cells, (int)g_opt_ingest, (int)g_opt_cells_build});
    idx->filter_wanted = plan.filter_wanted;
    const bool want_cells = plan.want_cells;
    bool want_layouts = plan.want_layouts;   // (until the grid index turns out to serve the shard)
    bool layouts_done = false;
    if (n_local > 0) {
        if (refs_on_device) {
            idx->refs = refs;
        } else {
            const size_t bytes = (size_t)n_local * (size_t)k * sizeof(float);
            hipError_t e = pool_get(device, bytes, (void **)&idx->owned_refs);
            idx->owned_bytes = bytes;
            if (e != hipSuccess) {
                delete idx;
                return fail(KNN_ENOMEM, "knn_index_create: hipMalloc(refs)", hipGetErrorString(e));
            }
            DeviceStreams ds;
            // (an ingest without its two streams: copy, then build)
            const IngestForm ingest = plan.ingest != IngestForm::CopyThenBuild && streams_get(device, &ds) == hipSuccess
                                          ? plan.ingest : IngestForm::CopyThenBuild;
            if (ingest == IngestForm::LayoutsUnderCopy) {
                // ingest: rows and filter layouts in one pass over PCIe (knn_filter_build_from_host)
                e = hipStreamSynchronize(s);   // work the caller queued ahead of this call
                if (e == hipSuccess)
                    e = knn_filter_build_from_host(idx->filter, k, n_local, idx->owned_refs, refs, ds.copy, ds.compute);
                layouts_done = e == hipSuccess;
            } else if (ingest == IngestForm::CellsUnderCopy) {
                // ingest into a cell-sorted index: the fast build's bucket pass under the copy (round 5)
                e = hipStreamSynchronize(s);   // work the caller queued ahead of this call
                if (e == hipSuccess)
                    e = knn_filter_build_cells_from_host(idx->filter, k, n_local, idx->owned_refs, refs, ds.copy, ds.compute);
                layouts_done = e == hipSuccess && idx->filter.usable;   // (else: the rows are there, the build below sorts them)
                if (e == hipSuccess && !layouts_done)
                    knn_filter_free(idx->filter);
            } else {
                e = hipMemcpyAsync(idx->owned_refs, refs, bytes, hipMemcpyHostToDevice, s);
                if (e == hipSuccess)
                    e = hipStreamSynchronize(s);  // the host buffer may be freed right after return
            }
            if (e != hipSuccess) {
                (void)hipDeviceSynchronize();
                knn_filter_free(idx->filter);
                pool_put(device, idx->owned_refs, bytes);
                delete idx;
                return fail(KNN_EHIP, "knn_index_create: H2D copy of refs", hipGetErrorString(e));
            }
            idx->refs = idx->owned_refs;
        }
    }
    if (n_local > 0 && plan.grid_planned) {
        const hipError_t e = knn_grid_build(&idx->grid, k, n_local, idx->refs, s);
        if (e != hipSuccess) {
            knn_index_destroy(idx);
            return fail(KNN_EHIP, "knn_index_create: building the grid index", hipGetErrorString(e));
        }
        if (idx->grid)
            want_layouts = false;
    }
    if (want_layouts && !layouts_done) {
        hipError_t e = knn_filter_build(idx->filter, k, n_local, idx->refs, s, want_cells, (int)g_opt_cells_build);
        if (e == hipErrorOutOfMemory) {
            // no room for the fp16 layouts beside the rows: the index still works, exact kernels only
            (void)hipGetLastError();
            knn_filter_free(idx->filter);
            e = hipSuccess;
        }
        if (e != hipSuccess) {
            knn_index_destroy(idx);
            return fail(KNN_EHIP, "knn_index_create: building the filter layouts", hipGetErrorString(e));
        }
    }
    *out = idx;
    return KNN_OK;
}
}  // namespace

extern "C" int knn_index_create(knn_index **out, int device, int k, long long n_local, const float *refs,
                                int refs_on_device, long long base_index, void *stream)
{
    return index_create_impl(out, device, k, n_local, refs, refs_on_device, base_index, stream, -1);
}

// ---------------------------------------------------------------------------------------------
// Cell-range shards (round 4): one global grid, every rank holds a contiguous range of its cell codes.
// ---------------------------------------------------------------------------------------------
struct knn_geom {
    ShardGeom g;
};

extern "C" {

int knn_geom_create(knn_geom **out, int k, long long n_global, int nranks, const float *sample_host, long long samples,
                    int seed_tiles)
{
    if (!out)
        return fail(KNN_EINVAL, "knn_geom_create: null out");
    *out = nullptr;
    if (k < 1 || n_global < 1 || nranks < 1 || !sample_host || samples < 1 || seed_tiles < 0)
        return fail(KNN_EINVAL, "knn_geom_create: bad arguments");
    knn_geom *g = new (std::nothrow) knn_geom();
    if (!g)
        return fail(KNN_ENOMEM, "knn_geom_create: out of host memory");
    if (!knn_geom_from_sample(g->g, k, n_global, nranks, sample_host, samples, seed_tiles == 0 ? 2 : seed_tiles)) {
        delete g;
        return fail(KNN_EINVAL, "knn_geom_create: the set does not suit cell-range shards (k > 16, fewer than 512 cells of >= 144 "
                                "rows per rank, fewer than 64 sample rows, or a sample that is not finite / has no extent): "
                                "shard by index range instead (knn_index_create with base_index)");
    }
    *out = g;
    return KNN_OK;
}

void knn_geom_destroy(knn_geom *g) { delete g; }

int knn_geom_info(const knn_geom *g, long long out[8])
{
    if (!g || !out)
        return fail(KNN_EINVAL, "knn_geom_info: bad arguments");
    out[0] = g->g.bits;
    out[1] = g->g.ncells;
    out[2] = g->g.cells_per_rank;
    out[3] = g->g.seed_tiles;
    out[4] = (long long)g->g.part_bytes();
    out[5] = (long long)g->g.part_bytes() * g->g.nranks;
    out[6] = g->g.sa;
    out[7] = g->g.nranks;
    return KNN_OK;
}

long long knn_geom_first_cell(const knn_geom *g, int rank)
{
    if (!g || rank < 0)
        return fail(KNN_EINVAL, "knn_geom_first_cell: bad arguments");
    return (long long)g->g.first_cell(rank);   // (rank >= ranks: the number of cells)
}

int knn_geom_assign(const knn_geom *g, int device, const float *rows_dev, long long n, int *owner_dev, void *stream)
{
    if (!g || n < 0 || (n > 0 && (!rows_dev || !owner_dev)))
        return fail(KNN_EINVAL, "knn_geom_assign: bad arguments");
    DeviceGuard guard(device);
    if (!guard.ok)
        return fail(KNN_EHIP, "knn_geom_assign: hipSetDevice failed");
    HIP_TRY(knn_geom_assign_launch(g->g, rows_dev, n, owner_dev, (hipStream_t)stream));
    return KNN_OK;
}

int knn_index_create_sharded(knn_index **out, int device, const knn_geom *g, int rank, long long n_local, const float *refs_dev,
                             const unsigned *gids_dev, void *stream)
{
    if (!out)
        return fail(KNN_EINVAL, "knn_index_create_sharded: null out");
    *out = nullptr;
    if (!g || rank < 0 || rank >= g->g.nranks || n_local < 0 || (n_local > 0 && (!refs_dev || !gids_dev)))
        return fail(KNN_EINVAL, "knn_index_create_sharded: bad geometry, rank, n_local or pointers");
    const int ndev = knn_device_count();
    if (ndev < 1)
        return fail(KNN_ENODEV, "knn_index_create_sharded: no HIP device visible");
    if (device < 0 || device >= ndev)
        return fail(KNN_EINVAL, "knn_index_create_sharded: device out of range");
    DeviceGuard guard(device);
    if (!guard.ok)
        return fail(KNN_EHIP, "knn_index_create_sharded: hipSetDevice failed");
    hipStream_t s = (hipStream_t)stream;
    if (n_local > 0) {
        // the rows' global numbers: strictly ascending (ties between equal distances are decided by LOCAL row order inside
        // the shard, which then is global order) and inside int32 (results are int)
        unsigned bad = 0u, last = 0u;
        HIP_TRY(knn_gids_check(gids_dev, n_local, &bad, s));
        HIP_TRY(hipMemcpy(&last, gids_dev + (n_local - 1), sizeof last, hipMemcpyDeviceToHost));
        if (bad != 0u || last > 0x7FFFFFFFu)
            return fail(KNN_EINVAL, "knn_index_create_sharded: gids must be strictly ascending and below 2^31");
    }
    knn_index *idx = new (std::nothrow) knn_index();
    if (!idx)
        return fail(KNN_ENOMEM, "knn_index_create_sharded: out of host memory");
    idx->device = device;
    idx->k = g->g.k;
    idx->n = n_local;
    idx->base = 0;   // keys carry LOCAL rows until the batch's last kernel translates them through gids
    idx->sharded = true;
    idx->geom = g->g;
    idx->rank = rank;
    idx->refs = refs_dev;
    idx->filter_wanted = true;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        idx->num_cu = prop.multiProcessorCount;
    if (n_local > 0) {
        unsigned bad_rows = 0u;
        const hipError_t e = knn_filter_build(idx->filter, idx->k, n_local, refs_dev, s, true, (int)g_opt_cells_build, &idx->geom, rank,
                                              &bad_rows);
        if (e != hipSuccess || !idx->filter.usable || !idx->filter.cells) {
            char why[160];
            if (bad_rows != 0u)
                snprintf(why, sizeof why, "%u row(s) lie outside rank %d's cell range of this geometry (knn_geom_assign says where rows belong)",
                         bad_rows, rank);
            else
                snprintf(why, sizeof why, "%s", e != hipSuccess ? hipGetErrorString(e) : "the rows do not suit the layouts (mostly outside the global box, or not finite)");
            knn_index_destroy(idx);
            return fail(e != hipSuccess ? KNN_EHIP : KNN_EINVAL, "knn_index_create_sharded", why);
        }
        idx->filter.cells->gids = gids_dev;
        idx->filter.cells->geom = &idx->geom;
    }
    *out = idx;
    return KNN_OK;
}

int knn_index_seed_export(knn_index *idx, void *layer_dev, void *stream)
{
    if (!idx || !idx->sharded || !layer_dev)
        return fail(KNN_EINVAL, "knn_index_seed_export: needs a cell-range shard and the layer buffer");
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    DeviceGuard guard(idx->device);
    if (idx->n == 0) {   // a rank without rows: its part is all padding (zero fragments never score: +INF norms)
        const size_t pb = idx->geom.part_bytes();
        unsigned char *part = (unsigned char *)layer_dev + (size_t)idx->rank * pb;
        const size_t frag_bytes = (size_t)idx->geom.cells_per_rank * idx->geom.seed_tiles * 1024u;
        HIP_TRY(hipMemsetAsync(part, 0, KNN_SEED_HEADER_BYTES + frag_bytes, (hipStream_t)stream));
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(part + KNN_SEED_HEADER_BYTES + frag_bytes), 0x00007C00,
                                  (size_t)idx->geom.cells_per_rank * idx->geom.seed_tiles * 32u, (hipStream_t)stream));
        return KNN_OK;
    }
    HIP_TRY(knn_cells_seed_export(idx->filter, idx->rank, (unsigned char *)layer_dev, (hipStream_t)stream));
    return KNN_OK;
}

int knn_index_seed_attach(knn_index *idx, const void *layer_dev)
{
    if (!idx || !idx->sharded || !layer_dev)
        return fail(KNN_EINVAL, "knn_index_seed_attach: needs a cell-range shard and the complete layer");
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    if (idx->n == 0)
        return KNN_OK;
    DeviceGuard guard(idx->device);
    // the bound constants must cover every rank's fragments: largest coordinate and norm over all parts' headers
    float bmax = idx->filter.bmax, nmax = idx->filter.nmax;
    for (int r = 0; r < idx->geom.nranks; ++r) {
        float hdr[2] = {0.0f, 0.0f};
        HIP_TRY(hipMemcpy(hdr, (const unsigned char *)layer_dev + (size_t)r * idx->geom.part_bytes(), sizeof hdr, hipMemcpyDeviceToHost));
        if (!(hdr[0] >= 0.0f) || !(hdr[1] >= 0.0f) || !(hdr[0] < INFINITY) || !(hdr[1] < INFINITY))
            return fail(KNN_EINVAL, "knn_index_seed_attach: a part of the layer has no valid header (was every rank's part exported and gathered?)");
        bmax = fmaxf(bmax, hdr[0]);
        nmax = fmaxf(nmax, hdr[1]);
    }
    idx->filter.bmax = bmax;
    idx->filter.nmax = nmax;
    idx->filter.cells->seed_layer = (const unsigned char *)layer_dev;
    return KNN_OK;
}

}  // extern "C"

extern "C" {

void knn_index_destroy(knn_index *idx)
{
    if (!idx)
        return;
    {
        DeviceGuard guard(idx->device);
        // the pool must never hand out memory a kernel may still be reading: ONE device-wide wait, then
        // every buffer of the index goes back
        knn_dev_free_begin_synced();
        if (idx->owned_refs)
            pool_put(idx->device, idx->owned_refs, idx->owned_bytes);
        knn_filter_free(idx->filter);
        knn_grid_free(idx->grid);
        for (auto &t : idx->topk) {
            (void)knn_dev_free(t.part);
            (void)knn_dev_free(t.cand);
            (void)knn_dev_free(t.lists);
            (void)knn_dev_free(t.count);
            (void)knn_dev_free(t.large);
            (void)knn_dev_free(t.mask);
            (void)knn_dev_free(t.self);
            (void)knn_dev_free(t.cluster);
            (void)knn_dev_free(t.forest);
        }
        knn_dev_free_end_synced();
        for (auto &ev : idx->events) {
            (void)hipEventDestroy(ev.first);
            (void)hipEventDestroy(ev.second);
        }
    }
    delete idx;
}

int knn_keys_init(int device, unsigned long long *keys_dev, int m, void *stream)
{
    if (m < 0 || (m > 0 && !keys_dev))
        return fail(KNN_EINVAL, "knn_keys_init: bad arguments");
    DeviceGuard guard(device);
    if (!guard.ok)
        return fail(KNN_EHIP, "knn_keys_init: hipSetDevice failed");
    HIP_TRY(knn_keys_fill_launch((u64 *)keys_dev, m, (hipStream_t)stream));
    return KNN_OK;
}

int knn_index_query_keys(knn_index *idx, int m, const float *queries_dev,
                         unsigned long long *keys_dev, void *stream)
{
    return knn_index_query_keys_slot(idx, 0, m, queries_dev, keys_dev, stream);
}

int knn_index_query_keys_slot(knn_index *idx, int slot, int m, const float *queries_dev,
                              unsigned long long *keys_dev, void *stream)
{
    return knn_index_query_keys_ex(idx, slot, m, queries_dev, keys_dev, stream, 0u);
}

int knn_index_query_keys_ex(knn_index *idx, int slot, int m, const float *queries_dev,
                            unsigned long long *keys_dev, void *stream, unsigned flags)
{
    return knn_index_query(idx, slot, m, queries_dev, keys_dev, nullptr, stream, flags);
}

}  // extern "C"

// Which path answers a call: the one place it is chosen (DESIGN, "which path answers a call").  n > 0 here: the entry points
// answer an empty shard before they ask.
// A cell-range shard is always served by its cell-sorted layout (it has no other, and never a grid index).
// A known oddity, kept: under option `cells` = 2 a layout in per-cell frames (centred) has no full scan to go to, so a 1-NN call
// that reaches the filter stays on the pruned scan — but `cells_live` is then false, so the filter is reached from m >= 5 only:
// m < 5 takes the exact scan, m >= 5 the pruned one.
QueryRoute knn_query_route(const QueryRouteInputs &in)
{
    QueryRoute r;
    CellTopkInputs t = in.t;
    const int m = t.q.m, path = in.path;
    const bool grid_serves = in.has_grid && (path == 0 || path == 3);
    // (with a cell-sorted layout even one query is served faster by the pruned scan than by reading the shard)
    const bool cells_live = t.has_cells && (t.cells_option != 2 || t.sharded);
    const bool sized = t.n >= 65536 || in.filter_wanted;
    if (t.K == 0) {
        const bool use_filter = t.sharded || (in.filter_usable && (path == 2 || (path == 0 && (m >= 5 || cells_live) && sized)));
        if (grid_serves)
            r.way = QueryWay::Grid;
        else if (use_filter)
            r.way = t.has_cells && t.q.kt <= 2 && (t.sharded || t.cells_option != 2 || t.q.centred) ? QueryWay::Cells : QueryWay::Filter;
        // the filter ways start the keys themselves when asked to (the cell-pruned one inside its first kernel)
        r.fill_keys_first = in.init_keys && (r.way == QueryWay::Exact || r.way == QueryWay::Grid);
        return r;
    }
    // Top-K: the cell-pruned top-K where knn_cells_topk_plan takes the call; else the MFMA filter for the dense
    // layouts and for a cell-sorted fp16 layout in the shard's frame (scanned in full), under the 1-NN rule's options and sizes;
    // exact top-K for per-cell frames (centred) the plan declines (it takes them only with KNN_QUERY_TOPK_FRAMES), 8-bit rows it declines, grid indexes (unless the call carries
    // KNN_QUERY_TOPK_GRID: then the grid's own top-K, DESIGN §4.6 "Grid top-K"), cell-range shards whose call does not
    // carry KNN_QUERY_TOPK_PARTIAL (the pruned form's lists are not the shard's own top-K: include/knn_mi355x.h §2c), tiny
    // shards, few queries, and outlier lists longer than half a query's candidate room.
    t.ccap = r.ccap = knn_topk_ccap(t.K, m);
    if (grid_serves && in.topk_grid) {   // KNN_QUERY_TOPK_GRID: on request, until it is measured against the exact top-K
        r.way = QueryWay::Grid;
        return r;
    }
    t.other_path = grid_serves || path == 1 || path == 3;
    r.topk = knn_cells_topk_plan(t);
    if (r.topk.use)
        r.way = QueryWay::Cells;
    else if (!t.sharded && in.filter_usable && !grid_serves && !(t.has_cells && (t.q.centred || t.q.rows_u8)) &&
             t.n_outliers <= r.ccap / 2 && r.ccap >= 64 && (path == 2 || (path == 0 && m >= 5 && sized)))
        r.way = QueryWay::Filter;
    return r;
}

// Which way answers a count call (knn_index_count_within; DESIGN §4.0, §4.6 "Counts within a radius"): the one place it is chosen.
// The exact count scan is the default — a path becomes a default only once it is measured faster than what it replaces —, the grid
// index and the cell-pruned scan answer on request, by flag; on an index that lacks the structure a flag changes nothing.
CountPlan knn_count_route(const CountRouteInputs &in)
{
    CountPlan p;
    p.slices = knn_slice_plan(in.m, in.n, in.num_cu, KnnCountSlices{}).slices;
    const int path = in.path;
    if (in.has_grid && in.flag_grid && (path == 0 || path == 3)) {
        // rmax: the radius-bounded top-K's rule at K = 1, the 2^15-cell budget included (chosen, not measured)
        const GridTopkPlan g = knn_grid_topk_plan(in.k, 1, in.m, true, path, true, in.radius_finite ? in.radius_rings : 0);
        p.way = QueryWay::Grid;
        p.rmax = g.rmax;
        p.blocks = g.blocks;
        p.waves = g.waves;
        p.scratch_bytes = (size_t)in.m * sizeof(unsigned);
        return p;
    }
    // a cell-sorted layout in the shard's ONE frame: fp16 rows without per-cell frames, or 8-bit rows in bin frames.  Cell-range
    // shards as they are: the ranks' counts add, so no seed layer and no PARTIAL contract.  +INF has no cap to prune with.
    const bool one_frame = in.has_cells && !in.centred && (!in.rows_u8 || in.bins);
    if (in.flag_cells && in.radius_finite && one_frame && in.k <= 32 && in.m >= 5 && (path == 0 || path == 2) && in.cells_option != 2) {
        p.way = QueryWay::Cells;
        p.passes = (in.m + KNN_CELL_BATCH - 1) / KNN_CELL_BATCH;
        p.pass_m = std::min(in.m, KNN_CELL_BATCH);
        p.scratch_bytes = (size_t)in.m * sizeof(unsigned);
    }
    return p;
}

// What a slot's top-K buffers must hold for a call: the one place their sizes are decided (tests/test_topk_scratch_logic.py
// restates the rules through knn_debug_topk_scratch).
TopkScratchPlan knn_topk_scratch_plan(const TopkScratchInputs &in)
{
    TopkScratchPlan p;
    const bool filter_way = in.way == QueryWay::Filter || in.way == QueryWay::Cells;
    p.part_bytes = knn_topk_part_bytes(in.m, in.K, in.n, in.num_cu);
    if (in.way == QueryWay::Cells) {   // the gated exact top-K of a pass sizes its lists by the pass's queries
        p.part_bytes = std::max(p.part_bytes, knn_topk_part_bytes(in.pass_m, in.K, in.n, in.num_cu));
        if (in.m % KNN_CELL_BATCH)
            p.part_bytes = std::max(p.part_bytes, knn_topk_part_bytes(in.m % KNN_CELL_BATCH, in.K, in.n, in.num_cu));
    }
    if (filter_way)   // candidate lists [m][ccap], then the counters [m]
        p.cand_bytes = (size_t)in.m * knn_topk_ccap(in.K, in.m) * sizeof(u64) + (size_t)in.m * sizeof(unsigned);
    else if (in.way == QueryWay::Grid && !in.init)
        p.cand_bytes = in.grid_scratch_bytes;
    if (filter_way && in.within)
        p.lists_bytes = (size_t)in.m * (size_t)in.K * sizeof(u64);
    return p;
}

namespace {

// The route's inputs for a call on idx: the index's facts and the option globals, read here and nowhere else on the query side.
QueryRouteInputs route_inputs(const knn_index *idx, int m, int K, unsigned flags)
{
    QueryRouteInputs in;
    const FilterState &f = idx->filter;
    const CellIndex *c = f.usable ? f.cells : nullptr;
    CellTopkInputs &t = in.t;
    // (several_slots false: a top-K call does not feed the index's record of recent slots; one batch at a time shapes)
    t.q = CellQueryInputs{idx->k, f.kt, c && c->centred, c && c->rows_u8, c ? c->ncells : 0u, c ? c->nitems : 0u, c ? c->cap : 0u, false,
                          (int)g_opt_scan_blocks, (int)g_opt_scan_deal, 1, m, idx->num_cu, KNN_RECORD_CAPACITY};
    t.has_cells = c != nullptr;
    t.bins = c && c->bins;
    t.K = K;
    t.n = idx->n;
    t.topk_cells = (int)g_opt_topk_cells;
    t.cells_option = (int)g_opt_cells;
    t.sharded = idx->sharded;
    t.shard_partial = idx->sharded && (flags & KNN_QUERY_TOPK_PARTIAL) != 0u;
    t.frames_flag = K > 0 && (flags & KNN_QUERY_TOPK_FRAMES) != 0u;
    t.n_outliers = f.n_outliers;
    in.filter_usable = f.usable;
    in.has_grid = idx->grid != nullptr;
    in.filter_wanted = idx->filter_wanted;
    in.init_keys = (flags & KNN_QUERY_INIT_KEYS) != 0u;
    in.path = (int)g_opt_path;
    in.topk_grid = K > 0 && (flags & KNN_QUERY_TOPK_GRID) != 0u;
    return in;
}

// The options of a filter call from the globals (several_slots: the 1-NN entry's, slots_differ).
FilterCallOptions filter_call_options()
{
    FilterCallOptions opt;
    opt.force_qt = (int)g_opt_filter_qt;
    opt.force_rounds = (int)g_opt_filter_rounds;
    opt.chain_policy = (int)g_opt_filter_chain;
    opt.run_thresholds = (int)g_opt_run_thresholds;
    opt.sample_stride = (int)g_opt_sample_stride;
    opt.scan_blocks = (int)g_opt_scan_blocks;
    opt.scan_deal = (int)g_opt_scan_deal;
    opt.cells_lists = (int)g_opt_cells_lists;
    return opt;
}

// Notes the call's workspace slot; true when the last eight calls named more than one.  Batches in flight on several
// workspace slots = a caller after throughput: the pruned scan of a small shard then takes ONE block per CU, so that the next
// batch's preparation kernels find registers beside it (knn_cells_query).  Derived from the last eight calls (the
// flag used to stick for the life of the index once any call had named a slot other than 0 — a caller that went back to one
// batch at a time kept the throughput shapes).
bool slots_differ(knn_index *idx, int slot)
{
    idx->recent_slots = (idx->recent_slots << 8) | (unsigned long long)(unsigned)slot;
    if (idx->recent_calls < 8)
        ++idx->recent_calls;
    bool several = false;
    for (int i = 1; i < idx->recent_calls; ++i)
        several = several || ((idx->recent_slots >> (8 * i)) & 0xFFull) != (unsigned long long)(unsigned)slot;
    return several;
}

typedef std::pair<hipEvent_t, hipEvent_t> EventPair;

// *out = the pair that brackets this call's dominant kernel, null when the call is not a timed one.  make_more: when the pairs
// knn_index_timing made are used up, create one (the 1-NN entry: every N-th batch is timed however long the run); else the
// call goes untimed (the top-K entry: its callers read the timing long before 64 calls).
int next_event_pair(knn_index *idx, bool make_more, EventPair **out)
{
    *out = nullptr;
    if (idx->timing <= 0 || idx->timing_seq++ % (unsigned long long)idx->timing != 0)
        return KNN_OK;
    if (idx->events_used == idx->events.size()) {
        if (!make_more)
            return KNN_OK;
        EventPair fresh;
        HIP_TRY(hipEventCreate(&fresh.first));
        HIP_TRY(hipEventCreate(&fresh.second));
        idx->events.push_back(fresh);
    }
    *out = &idx->events[idx->events_used++];
    return KNN_OK;
}

// A per-slot scratch buffer of at least `need` bytes: one too small is freed (which waits for the device: it may be in use)
// and allocated anew.
int slot_buffer_grow(u64 *&buf, size_t &bytes, size_t need)
{
    if (bytes >= need)
        return KNN_OK;
    HIP_TRY(knn_dev_free(buf));
    buf = nullptr;
    bytes = 0;
    HIP_TRY(knn_dev_alloc((void **)&buf, need));
    bytes = need;
    return KNN_OK;
}

#define KNN_TRY(call)           \
    do {                        \
        const int rc_ = (call); \
        if (rc_ != KNN_OK)      \
            return rc_;         \
    } while (0)

// The global numbers of a cell-range shard's rows, which its keys carry (gids); null: an index-range shard's keys carry base + row.
const unsigned *shard_gids(const knn_index *idx)
{
    return idx->sharded && idx->filter.cells ? idx->filter.cells->gids : nullptr;
}

// What every index call that consults no layout, or none yet, leaves for knn_index_last_stats: way 1, nothing counted.
void begin_call(knn_index *idx, int slot)
{
    idx->stats[0] = 1;
    idx->stats[1] = 0;
    idx->stats[2] = 0;
    idx->stats[3] = 0;
    idx->grid_topk_gate = nullptr;
    idx->last_slot = slot;
}

// call.ev0 / ev1 = the pair that brackets the call's dominant kernel, null when the call is not a timed one.
template <class Call>
int take_events(knn_index *idx, Call &call)
{
    EventPair *ev = nullptr;
    KNN_TRY(next_event_pair(idx, false, &ev));
    call.ev0 = ev ? ev->first : nullptr;
    call.ev1 = ev ? ev->second : nullptr;
    return KNN_OK;
}

}  // namespace

extern "C" {

int knn_index_query(knn_index *idx, int slot, int m, const float *queries_dev, unsigned long long *keys_dev,
                    int *indices_dev, void *stream, unsigned flags)
{
    if (!idx || m < 0 || slot < 0 || slot >= KNN_SLOTS || (m > 0 && (!queries_dev || !keys_dev)) ||
        (flags & ~(unsigned)KNN_QUERY_INIT_KEYS) != 0u)
        return fail(KNN_EINVAL, "knn_index_query_keys: bad arguments");
    if (m == 0)
        return KNN_OK;
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    DeviceGuard guard(idx->device);
    if (!guard.ok)
        return fail(KNN_EHIP, "knn_index_query_keys: hipSetDevice failed");
    const bool init_keys = (flags & KNN_QUERY_INIT_KEYS) != 0u;
    if (idx->sharded && !init_keys)
        return fail(KNN_EINVAL, "knn_index_query: a cell-range shard WRITES its keys (pass KNN_QUERY_INIT_KEYS): they carry local "
                                "rows until the batch's last kernel, so they cannot fold into keys other shards have written");
    hipStream_t s = (hipStream_t)stream;
    u64 *keys = (u64 *)keys_dev;
    if (idx->n == 0) {   // an empty shard leaves (+INF, 0)
        if (init_keys)
            HIP_TRY(knn_keys_fill_launch(keys, m, s));
        if (indices_dev)
            HIP_TRY(knn_keys_unpack_launch(keys, m, indices_dev, s));
        return KNN_OK;
    }
    EventPair *ev = nullptr;
    KNN_TRY(next_event_pair(idx, true, &ev));
    const QueryRoute route = knn_query_route(route_inputs(idx, m, 0, flags));
    idx->stats[0] = (long long)route.way;
    idx->stats[1] = 0;
    idx->stats[2] = 0;
    idx->grid_topk_gate = nullptr;
    if (route.fill_keys_first)
        HIP_TRY(knn_keys_fill_launch(keys, m, s));
    switch (route.way) {
    case QueryWay::Grid: {
        // k <= 4 spatial index: one wave per query walks the grid rings; the brute-force scan behind it is
        // gated on the "some query gave up" word (far-outside queries, empty regions)
        idx->last_slot = slot;
        if (ev)
            HIP_TRY(hipEventRecord(ev->first, s));
        const unsigned *gate = nullptr;
        HIP_TRY(knn_grid_query(idx->grid, slot, m, queries_dev, idx->base, keys, &gate, s));
        if (ev)
            HIP_TRY(hipEventRecord(ev->second, s));
        HIP_TRY(knn_exact_launch(idx->k, m, idx->n, idx->base, queries_dev, idx->refs, keys, idx->num_cu, gate, s));
        break;
    }
    case QueryWay::Filter:
    case QueryWay::Cells: {
        // the event pair brackets the MFMA filter kernel alone (the dominant kernel); the indices come from the path's own launches
        FilterCallOptions opt = filter_call_options();
        opt.several_slots = slots_differ(idx, slot);
        idx->last_slot = slot;
        HIP_TRY(knn_filter_query(idx->filter, opt, route.way == QueryWay::Cells, slot, m, queries_dev, idx->refs, idx->base, keys,
                                 idx->num_cu, s, ev ? ev->first : nullptr, ev ? ev->second : nullptr, init_keys, indices_dev));
        return KNN_OK;
    }
    case QueryWay::Exact:
        if (ev)
            HIP_TRY(hipEventRecord(ev->first, s));
        HIP_TRY(knn_exact_launch(idx->k, m, idx->n, idx->base, queries_dev, idx->refs, keys, idx->num_cu, nullptr, s));
        if (ev)
            HIP_TRY(hipEventRecord(ev->second, s));
        break;
    }
    if (indices_dev)
        HIP_TRY(knn_keys_unpack_launch(keys, m, indices_dev, s));
    return KNN_OK;
}

}  // extern "C"

namespace {

// The index's side of a TopkCall: the shard's rows, the numbers their keys carry and the device's size.
void topk_index_side(const knn_index *idx, TopkCall &call)
{
    call.k = idx->k;
    call.n = idx->n;
    call.base = idx->base;
    call.gids = shard_gids(idx);
    call.r = idx->refs;
    call.num_cu = idx->num_cu;
}

// knn_index_query_topk and knn_index_query_topk_within behind their argument checks.  max_dist2 = +INF: the plain call, launch
// for launch.  A finite radius changes no route (knn_query_route never sees it): the exact top-K and the grid way carry the limit
// key in their kernels, the cell-pruned scan of a one-frame layout caps its bound with it, and the filter ways — whose lists may
// hold rows just beyond it, or come from a fallback — make their top-K into the slot's list scratch, which one clip launch turns
// into the caller's keys.
int query_topk(knn_index *idx, int slot, TopkCall call, int *indices_dev, unsigned flags, const char *who)
{
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    DeviceGuard guard(idx->device);
    if (!guard.ok)
        return fail_in(KNN_EHIP, who, "hipSetDevice failed");
    hipStream_t s = call.stream;
    const int m = call.m, K = call.K, mk = m * K;
    call.init = (flags & KNN_QUERY_INIT_KEYS) != 0u;
    idx->stats[0] = 1;
    idx->stats[1] = 0;
    idx->stats[2] = 0;
    idx->grid_topk_gate = nullptr;
    idx->last_slot = slot;
    if (idx->n == 0) {   // an empty shard adds nothing
        if (call.init)
            HIP_TRY(knn_keys_fill_launch(call.keys, mk, s));
        if (indices_dev)
            HIP_TRY(knn_keys_unpack_launch(call.keys, mk, indices_dev, s));
        return KNN_OK;
    }
    const QueryRoute route = knn_query_route(route_inputs(idx, m, K, flags));
    const QueryWay way = route.way;
    idx->stats[0] = (long long)way;
    // the grid way (KNN_QUERY_TOPK_GRID) — a radius call: the rings its radius spans size rmax, the kernel's face bound decides
    GridTopkPlan gp;
    if (way == QueryWay::Grid)
        gp = knn_grid_topk_plan(idx->k, K, m, true, 0, true, call.within() ? knn_grid_radius_rings(idx->grid, call.max_dist2) : 0);
    // the slot's scratch, grown before the first launch
    const TopkScratchPlan sp = knn_topk_scratch_plan({way, m, K, idx->n, idx->num_cu, call.init != 0, call.within(), route.topk.pass_m,
                                                      gp.scratch_bytes});
    knn_index::TopkSlot &ts = idx->topk[slot];
    KNN_TRY(slot_buffer_grow(ts.part, ts.part_bytes, sp.part_bytes));
    KNN_TRY(slot_buffer_grow(ts.cand, ts.cand_bytes, sp.cand_bytes));
    KNN_TRY(slot_buffer_grow(ts.lists, ts.lists_bytes, sp.lists_bytes));
    EventPair *ev = nullptr;
    KNN_TRY(next_event_pair(idx, false, &ev));
    topk_index_side(idx, call);
    call.ev0 = ev ? ev->first : nullptr;
    call.ev1 = ev ? ev->second : nullptr;
    call.part = ts.part;
    call.part_bytes = ts.part_bytes;
    call.cand = ts.cand;
    call.ccap = route.ccap;
    const bool filter_way = way == QueryWay::Filter || way == QueryWay::Cells;
    call.ccount = filter_way ? (unsigned *)(ts.cand + (size_t)m * route.ccap) : nullptr;
    // a radius call on the filter ways: the top-K starts the slot's list scratch, the clip behind writes or folds the caller's keys
    const bool clip = filter_way && call.within();
    const TopkCall way_call = clip ? call.writing(ts.lists) : call;
    switch (way) {
    case QueryWay::Grid:
        // the kernel's lists are the caller's keys, or — a folding call — the slot's scratch
        idx->stats[3] = 0;
        HIP_TRY(knn_grid_query_topk(idx->grid, gp, slot, call, &idx->grid_topk_gate));
        break;
    case QueryWay::Cells:
        // layouts in the shard's frame — or, with KNN_QUERY_TOPK_FRAMES, in per-cell frames —, in passes of KNN_CELL_BATCH queries
        // (option `topk_cells`)
        HIP_TRY(knn_filter_query_topk_cells(idx->filter, route.topk, slot, way_call));
        break;
    case QueryWay::Filter: {
        FilterCallOptions opt = filter_call_options();
        opt.run_thresholds = 2;   // running thresholds are a 1-NN argument; the non-running sample stride with them
        opt.sample_stride = 0;
        opt.topk = K;
        TopkCall plain = way_call;   // the dense scan has no use for the radius: it is handed none
        plain.max_dist2 = INFINITY;
        HIP_TRY(knn_filter_query_topk(idx->filter, opt, slot, plain));
        break;
    }
    case QueryWay::Exact:
        if (ev)
            HIP_TRY(hipEventRecord(call.ev0, s));
        HIP_TRY(knn_exact_topk_launch(call, nullptr, true));
        if (ev)
            HIP_TRY(hipEventRecord(call.ev1, s));
        break;
    }
    if (clip)
        HIP_TRY(knn_topk_clip_launch(m, K, ts.lists, call.limit_key(), call.keys, call.init, s));
    if (indices_dev)
        HIP_TRY(knn_keys_unpack_launch(call.keys, mk, indices_dev, s));
    return KNN_OK;
}

// What the caller of a top-K entry states; query_topk and topk_one_way add the index's side and the slot's scratch.
TopkCall topk_call_of(int m, int K, const float *queries_dev, unsigned long long *keys_dev, void *stream, float max_dist2)
{
    TopkCall c;
    c.m = m;
    c.K = K;
    c.q = queries_dev;
    c.keys = (u64 *)keys_dev;
    c.stream = (hipStream_t)stream;
    c.max_dist2 = max_dist2;
    return c;
}

// The arguments both top-K entries reject (the four flags they admit: values up to 15).
bool topk_args_bad(const knn_index *idx, int slot, int m, int K, const float *queries_dev, const unsigned long long *keys_dev, unsigned flags)
{
    return !idx || m < 1 || K < 1 || K > KNN_TOPK_MAX || (long long)m * K > INT_MAX || slot < 0 || slot >= KNN_SLOTS ||
        !queries_dev || !keys_dev || (flags & ~(unsigned)(KNN_QUERY_INIT_KEYS | KNN_QUERY_TOPK_PARTIAL | KNN_QUERY_TOPK_GRID | KNN_QUERY_TOPK_FRAMES)) != 0u;
}

// The way of a count or list call on idx (knn_count_route's inputs from the index's facts, the call's radius and its two flags).
CountPlan count_plan_of(const knn_index *idx, const QueryRouteInputs &ri, int m, float max_dist2, unsigned flags)
{
    CountRouteInputs ci;
    ci.k = idx->k;
    ci.m = m;
    ci.n = idx->n;
    ci.radius_finite = max_dist2 < INFINITY;
    ci.flag_grid = (flags & KNN_QUERY_COUNT_GRID) != 0u;
    ci.flag_cells = (flags & KNN_QUERY_COUNT_CELLS) != 0u;
    ci.has_grid = ri.has_grid;
    ci.has_cells = ri.t.has_cells;
    ci.centred = ri.t.q.centred;
    ci.rows_u8 = ri.t.q.rows_u8;
    ci.bins = ri.t.bins;
    ci.sharded = ri.t.sharded;
    ci.path = ri.path;
    ci.cells_option = ri.t.cells_option;
    ci.num_cu = idx->num_cu;
    ci.radius_rings = ci.has_grid && ci.radius_finite ? knn_grid_radius_rings(idx->grid, max_dist2) : 0;
    return knn_count_route(ci);
}

// ---- the radius family (include/knn_mi355x.h 2e .. 2l): one description, one argument ladder, one call front ---------------------
// What an entry of the family is, and what its caller states.  m: the queries, or the rows of a self call (queries null: they are
// the shard's rows from row_first).  max_dist2: the radius, or the cap over `radii` (nullable, device [m]).
enum : unsigned {
    kCap = 1u,      // the entry's texts speak of a cap, not of max_dist2 (the each and routed forms)
    kRouted = 2u,   // admits KNN_QUERY_COUNT_GRID / _CELLS and takes the way knn_count_route names; else way 1 on every index
    kSelf = 4u,     // about the shard's own rows: rows and row_first in m's place, a query's own row no candidate
    kMasked = 8u,   // over a subset of the rows: `mask` admits them; way 1 is the exact masked scan (never with radii or kSelf)
};
struct WithinCall {
    const char *who;
    unsigned form;
    int slot, m;
    const float *queries;
    long long row_first;
    const float *radii;
    float max_dist2;
    void *stream;
    unsigned flags;
    const unsigned *mask = nullptr;   // kMasked: device (n_local + 31) / 32 words
};
struct NullRule {
    bool broken;
    const char *what;
};
const char *const kNullLists = "null offsets, fill or keys";

// The family's argument rules, one message per rule in one order — radius or cap, flags, slot, m or rows (+ row_first), the entry's
// pointer groups, the index last —: the *_logic.py tests tell them apart without a GPU.
int within_check(const WithinCall &w, std::initializer_list<NullRule> pointers, const knn_index *idx)
{
    const bool routed = (w.form & kRouted) != 0u, self = (w.form & kSelf) != 0u;
    if (!(w.max_dist2 >= 0.0f))
        return fail_in(KNN_EINVAL, w.who, (w.form & kCap) ? "cap must be >= 0 (or +INF) and not NaN" : "max_dist2 must be >= 0 and not NaN");
    if ((w.flags & ~(routed ? KNN_QUERY_INIT_KEYS | KNN_QUERY_COUNT_GRID | KNN_QUERY_COUNT_CELLS : (unsigned)KNN_QUERY_INIT_KEYS)) != 0u)
        return fail_in(KNN_EINVAL, w.who, routed ? "unknown flag (KNN_QUERY_INIT_KEYS, KNN_QUERY_COUNT_GRID, KNN_QUERY_COUNT_CELLS)"
                                                 : "unknown flag (KNN_QUERY_INIT_KEYS alone is admitted)");
    if (w.slot < 0 || w.slot >= KNN_SLOTS)
        return fail_in(KNN_EINVAL, w.who, "slot outside 0 .. 7");
    if (w.m < 1)
        return fail_in(KNN_EINVAL, w.who, self ? "rows < 1" : "m < 1");
    if (self && w.row_first < 0)
        return fail_in(KNN_EINVAL, w.who, "row_first < 0");
    for (const NullRule &p : pointers)
        if (p.broken)
            return fail_in(KNN_EINVAL, w.who, p.what);
    if (!idx)
        return fail_in(KNN_EINVAL, w.who, "null index");
    return KNN_OK;
}

// Where a call's hits go: the two call structs as their entries start them.
CountCall counts_into(unsigned *counts_dev)
{
    CountCall c;
    c.counts = counts_dev;
    return c;
}
ListCall lists_into(const unsigned long long *offsets_dev, unsigned *fill_dev, unsigned long long *keys_dev)
{
    ListCall c;
    c.offsets = (const u64 *)offsets_dev;
    c.fill = fill_dev;
    c.keys = (u64 *)keys_dev;
    return c;
}
// What the two differ in on the host: the array every way adds to, the number a key carries, and the launchers' names.
unsigned *added_to(const CountCall &c) { return c.counts; }
unsigned *added_to(const ListCall &c) { return c.fill; }
void key_numbers(const knn_index *, CountCall &) {}
void key_numbers(const knn_index *idx, ListCall &c)
{
    c.base = idx->base;
    c.gids = shard_gids(idx);
}
hipError_t grid_within(const GridState *gs, int rmax, int slot, const CountCall &c, const unsigned **gate) { return knn_grid_query_count(gs, rmax, slot, c, gate); }
hipError_t grid_within(const GridState *gs, int rmax, int slot, const ListCall &c, const unsigned **gate) { return knn_grid_query_list(gs, rmax, slot, c, gate); }
hipError_t cells_within(FilterState &st, const CellTopkPlan &tp, int slot, const CountCall &c) { return knn_filter_query_count_cells(st, tp, slot, c); }
hipError_t cells_within(FilterState &st, const CellTopkPlan &tp, int slot, const ListCall &c) { return knn_filter_query_list_cells(st, tp, slot, c); }
hipError_t exact_within(const CountCall &c) { return knn_exact_count_launch(c, nullptr); }
hipError_t exact_within(const ListCall &c) { return knn_exact_list_launch(c, nullptr); }
hipError_t self_within(const CountCall &c, long long row_first) { return knn_self_count_launch(c, row_first); }
hipError_t self_within(const ListCall &c, long long row_first) { return knn_self_list_launch(c, row_first); }
// (the exact masked scans: they make their prefix in c.mask_scratch and record the call's events themselves, behind it)
hipError_t masked_within(const CountCall &c, bool init)
{
    return knn_masked_count_launch(c, knn_masked_plan(c.k, c.m, 0, c.n, c.num_cu, init), c.mask, c.mask_scratch);
}
hipError_t masked_within(const ListCall &c, bool init)
{
    return knn_masked_list_launch(c, knn_masked_lists_plan(c.k, c.m, 0, c.n, c.num_cu, init), c.mask, c.mask_scratch);
}

// Behind the lock and the device, every call of the family: the fields both call structs share (q: the queries as the launches
// take them), way 1 in the statistics, and — every way ADDS to the caller's counts or fill — an init call's zeroes.
template <class Call>
int within_begin(knn_index *idx, const WithinCall &w, const float *q, Call &call)
{
    call.k = idx->k;
    call.m = w.m;
    call.n = idx->n;
    call.q = q;
    call.r = idx->refs;
    call.radii = w.radii;
    call.max_dist2 = w.max_dist2 == 0.0f ? 0.0f : w.max_dist2;   // (-0 counts as 0)
    call.num_cu = idx->num_cu;
    call.stream = (hipStream_t)w.stream;
    key_numbers(idx, call);
    begin_call(idx, w.slot);
    if ((w.flags & KNN_QUERY_INIT_KEYS) != 0u)
        HIP_TRY(hipMemsetAsync(added_to(call), 0, (size_t)w.m * sizeof(unsigned), call.stream));
    return KNN_OK;
}

// A count or list call behind within_check, on the way knn_count_route names for m queries at max_dist2 (the cap of a call with
// radii: the kernels are then the each-forms) under the call's flags and the options.  A self call's queries are the resident rows:
// nothing is uploaded.  Routed (2k), call.self_first tells the grid and cell ways to drop a query's own row and to gate the
// self-scan behind them, and way 1 is the exact self-scan in the exact scan's place; not routed (2i, 2j), no layout is consulted
// and the self-scan — which reads neither call.q nor call.scratch — is launched as it always was.
// Masked (2g, 2h, 2l): way 1 is the exact masked scan in the exact scan's place; routed (2l), call.mask tells the grid and cell ways
// to drop the rows it does not admit and to gate the masked scan behind them.  The slot's mask scratch is grown before the first
// launch whichever way is taken: the host cannot know whether the scan behind a pruned way will run.
template <class Call>
int within_run(knn_index *idx, const WithinCall &w, Call call)
{
    const bool routed = (w.form & kRouted) != 0u, self = (w.form & kSelf) != 0u, masked = (w.form & kMasked) != 0u;
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    if (self && (w.row_first > idx->n || (long long)w.m > idx->n - w.row_first))
        return fail_in(KNN_EINVAL, w.who, "row_first + rows above the shard's rows");
    DeviceGuard guard(idx->device);
    if (!guard.ok)
        return fail_in(KNN_EHIP, w.who, "hipSetDevice failed");
    KNN_TRY(within_begin(idx, w, !self ? w.queries : routed ? idx->refs + (size_t)w.row_first * (size_t)idx->k : nullptr, call));
    if (idx->n == 0)   // an empty shard adds nothing (a self call's range check has failed by here)
        return KNN_OK;
    QueryRouteInputs ri;
    CountPlan plan;   // (way 1)
    if (routed) {
        call.self_first = self ? w.row_first : -1;
        ri = route_inputs(idx, w.m, 1, 0u);
        plan = count_plan_of(idx, ri, w.m, call.max_dist2, w.flags);
        idx->stats[0] = (long long)plan.way;
        // the slot's count scratch — a list's scratch cursor — of the grid and cell ways, grown before the first launch
        knn_index::TopkSlot &ts = idx->topk[w.slot];
        KNN_TRY(slot_buffer_grow(ts.count, ts.count_bytes, plan.scratch_bytes));
        call.scratch = (unsigned *)ts.count;
    }
    if (masked) {
        knn_index::TopkSlot &ts = idx->topk[w.slot];
        KNN_TRY(slot_buffer_grow(ts.mask, ts.mask_bytes, knn_masked_plan(idx->k, w.m, 0, idx->n, idx->num_cu, false).mask_bytes));
        call.mask = w.mask;
        call.mask_scratch = ts.mask;
    }
    KNN_TRY(take_events(idx, call));
    switch (plan.way) {
    case QueryWay::Grid:
        HIP_TRY(grid_within(idx->grid, plan.rmax, w.slot, call, &idx->grid_topk_gate));
        break;
    case QueryWay::Cells: {
        const CellTopkPlan tp = knn_cells_count_plan(ri.t);
        if (!tp.use)
            return fail_in(KNN_EHIP, w.who, "the cell-pruned scan has no pass shape for this layout");
        HIP_TRY(cells_within(idx->filter, tp, w.slot, call));
        break;
    }
    default:
        if (self) {   // (ungated, the self-scan records the call's events itself)
            HIP_TRY(self_within(call, w.row_first));
            break;
        }
        if (masked) {   // (ungated, the masked scan records the call's events itself)
            HIP_TRY(masked_within(call, (w.flags & KNN_QUERY_INIT_KEYS) != 0u));
            break;
        }
        if (call.ev0)
            HIP_TRY(hipEventRecord(call.ev0, call.stream));
        HIP_TRY(exact_within(call));
        if (call.ev1)
            HIP_TRY(hipEventRecord(call.ev1, call.stream));
        break;
    }
    return KNN_OK;
}

// ---- the one-way top-K forms (include/knn_mi355x.h 2f .. 2i): one description, one argument ladder, one call front ---------------
// What an entry of the forms is (kMasked and kSelf as the radius family's), and what its caller states.  m: the queries, or the rows
// of a self entry (queries null: they are the shard's rows from row_first).  A *_host entry states host arrays, names no slot (0)
// and takes no flags (0): those two rules cannot speak for it.
enum : unsigned {
    kLarge = 16u,        // K up to KNN_TOPK_LARGE_MAX (the radix select), else up to KNN_TOPK_MAX
    kSizesFirst = 32u,   // K, m and m * K are looked at before slot, radius and flags (the order the header's 2f states for its two entries)
};
struct TopkEntry {
    const char *who;
    unsigned form;
    int slot, m, K;
    const float *queries;
    long long row_first;
    float max_dist2;
    const unsigned *mask = nullptr;   // kMasked: (n_local + 31) / 32 words
    unsigned long long *keys = nullptr;
    void *stream = nullptr;
    unsigned flags = 0u, admits = KNN_QUERY_INIT_KEYS;   // admits: the flags the entry takes
};

// The forms' argument rules, one message per rule in one order — radius, flags, slot, m or rows (+ row_first), K, m * K, the entry's
// pointer groups, the index last — or, kSizesFirst, K, m, m * K, slot, radius, flags in front of the pointers: the *_logic.py tests
// and tests/golden/topk_arg_errors.json tell them apart, and which of two broken rules speaks, without a GPU.
int topk_check(const TopkEntry &t, std::initializer_list<NullRule> pointers, const knn_index *idx)
{
    enum Rule { Radius, Flags, Slot, Rows, Neighbours, Product };
    static const Rule usual[6] = {Radius, Flags, Slot, Rows, Neighbours, Product};
    static const Rule sizes_first[6] = {Neighbours, Rows, Product, Slot, Radius, Flags};
    const bool self = (t.form & kSelf) != 0u, large = (t.form & kLarge) != 0u;
    const Rule *const order = (t.form & kSizesFirst) ? sizes_first : usual;
    for (int i = 0; i < 6; ++i) {
        const char *broken = nullptr;
        switch (order[i]) {
        case Radius:
            if (!(t.max_dist2 >= 0.0f))
                broken = "max_dist2 must be >= 0 and not NaN";
            break;
        case Flags:
            if ((t.flags & ~t.admits) != 0u)
                broken = t.admits == KNN_QUERY_INIT_KEYS ? "unknown flag (KNN_QUERY_INIT_KEYS alone is admitted)"
                                                         : "unknown flag (KNN_QUERY_INIT_KEYS, KNN_QUERY_TOPK_GRID, KNN_QUERY_TOPK_FRAMES)";
            break;
        case Slot:
            if (t.slot < 0 || t.slot >= KNN_SLOTS)
                broken = "slot outside 0 .. 7";
            break;
        case Rows:
            if (t.m < 1)
                broken = self ? "rows < 1" : "m < 1";
            else if (self && t.row_first < 0)
                broken = "row_first < 0";
            break;
        case Neighbours:
            if (t.K < 1 || t.K > (large ? KNN_TOPK_LARGE_MAX : KNN_TOPK_MAX))
                broken = large ? "K outside 1 .. 4096" : "K outside 1 .. 64";
            break;
        case Product:
            if ((long long)t.m * t.K > INT_MAX)
                broken = self ? "rows * K above INT_MAX" : "m * K above INT_MAX";
            break;
        }
        if (broken)
            return fail_in(KNN_EINVAL, t.who, broken);
    }
    for (const NullRule &p : pointers)
        if (p.broken)
            return fail_in(KNN_EINVAL, t.who, p.what);
    if (!idx)
        return fail_in(KNN_EINVAL, t.who, "null index");
    return KNN_OK;
}

// A device entry of the forms behind topk_check (a self entry: behind its range rule too): one way on every index, no layout is
// consulted.  The forms differ in their plan, in the slot buffers it sizes — the mask scratch of a masked form; the per-slice
// lists (part), or the large scratch of a kLarge form, which the call is handed as call.part — and in their launcher, which
// records the call's events itself; the two large forms leave the word behind knn_index_last_stats()[2].
int topk_one_way(knn_index *idx, const TopkEntry &t, int *indices_dev)
{
    const unsigned kind = t.form & (kLarge | kMasked | kSelf);
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    DeviceGuard guard(idx->device);
    if (!guard.ok)
        return fail_in(KNN_EHIP, t.who, "hipSetDevice failed");
    // (-0 counts as 0; a self entry's queries are the resident rows: its scan reads them in place)
    TopkCall call = topk_call_of(t.m, t.K, kind == kSelf ? idx->refs + (size_t)t.row_first * (size_t)idx->k : t.queries, t.keys, t.stream,
                                 t.max_dist2 == 0.0f ? 0.0f : t.max_dist2);
    call.init = (t.flags & KNN_QUERY_INIT_KEYS) != 0u;
    const int mk = t.m * t.K;
    begin_call(idx, t.slot);
    if (idx->n > 0) {   // (an empty shard adds nothing)
        topk_index_side(idx, call);
        // the slot's scratch, grown before the first launch
        const bool init = call.init != 0;
        knn_index::TopkSlot &ts = idx->topk[t.slot];
        TopkLargePlan large;
        MaskedPlan masked;
        MaskedListsPlan both;
        size_t mask_bytes = 0, part_bytes = 0;
        switch (kind) {
        case kLarge:
            large = knn_topk_large_plan(idx->k, t.m, t.K, idx->n, idx->num_cu, init);
            part_bytes = large.scratch_bytes;
            break;
        case kMasked:
            masked = knn_masked_plan(idx->k, t.m, t.K, idx->n, idx->num_cu, init);
            mask_bytes = masked.mask_bytes;
            part_bytes = masked.part_bytes;
            break;
        case kLarge | kMasked:
            both = knn_masked_lists_plan(idx->k, t.m, t.K, idx->n, idx->num_cu, init);
            mask_bytes = both.cut.mask_bytes;
            part_bytes = both.select_bytes;
            break;
        default:   // kSelf
            part_bytes = knn_self_plan(idx->k, t.m, t.K, idx->n, idx->num_cu, init).part_bytes;
            break;
        }
        if ((kind & kMasked) != 0u)
            KNN_TRY(slot_buffer_grow(ts.mask, ts.mask_bytes, mask_bytes));
        u64 *&part = (kind & kLarge) != 0u ? ts.large : ts.part;
        size_t &held = (kind & kLarge) != 0u ? ts.large_bytes : ts.part_bytes;
        KNN_TRY(slot_buffer_grow(part, held, part_bytes));
        call.part = part;
        call.part_bytes = held;
        KNN_TRY(take_events(idx, call));
        switch (kind) {
        case kLarge:
            HIP_TRY(knn_topk_large_launch(call, large, &idx->grid_topk_gate));
            break;
        case kMasked:
            HIP_TRY(knn_masked_topk_launch(call, masked, t.mask, ts.mask));
            break;
        case kLarge | kMasked:
            HIP_TRY(knn_masked_large_launch(call, both, t.mask, ts.mask, &idx->grid_topk_gate));
            break;
        default:
            HIP_TRY(knn_self_topk_launch(call, t.row_first));
            break;
        }
    } else if (call.init) {
        HIP_TRY(knn_keys_fill_launch(call.keys, mk, call.stream));
    }
    if (indices_dev)
        HIP_TRY(knn_keys_unpack_launch(call.keys, mk, indices_dev, call.stream));
    return KNN_OK;
}

}  // namespace

extern "C" {

int knn_index_query_topk(knn_index *idx, int slot, int m, int K, const float *queries_dev, unsigned long long *keys_dev,
                         int *indices_dev, void *stream, unsigned flags)
{
    if (topk_args_bad(idx, slot, m, K, queries_dev, keys_dev, flags))
        return fail(KNN_EINVAL, "knn_index_query_topk: bad arguments (1 <= K <= 64, m >= 1, slot 0 .. 7)");
    return query_topk(idx, slot, topk_call_of(m, K, queries_dev, keys_dev, stream, INFINITY), indices_dev, flags, "knn_index_query_topk");
}

int knn_index_query_topk_within(knn_index *idx, int slot, int m, int K, const float *queries_dev, float max_dist2,
                                unsigned long long *keys_dev, int *indices_dev, void *stream, unsigned flags)
{
    if (topk_args_bad(idx, slot, m, K, queries_dev, keys_dev, flags) || !(max_dist2 >= 0.0f))
        return fail(KNN_EINVAL, "knn_index_query_topk_within: bad arguments (1 <= K <= 64, m >= 1, slot 0 .. 7, max_dist2 >= 0 and not NaN)");
    // (-0 counts as 0: the limit key is made from the bits)
    return query_topk(idx, slot, topk_call_of(m, K, queries_dev, keys_dev, stream, max_dist2 == 0.0f ? 0.0f : max_dist2), indices_dev,
                      flags, "knn_index_query_topk_within");
}

int knn_keys_topk_merge(int device, int m, int K, const unsigned long long *a_dev, unsigned long long *b_dev, void *stream)
{
    if (m < 1 || K < 1 || K > KNN_TOPK_MAX || !a_dev || !b_dev)
        return fail(KNN_EINVAL, "knn_keys_topk_merge: bad arguments (1 <= K <= 64, m >= 1)");
    DeviceGuard guard(device);
    if (!guard.ok)
        return fail(KNN_EHIP, "knn_keys_topk_merge: hipSetDevice failed");
    HIP_TRY(knn_topk_merge_launch(m, K, (const u64 *)a_dev, (u64 *)b_dev, (hipStream_t)stream));
    return KNN_OK;
}

int knn_index_count_within(knn_index *idx, int slot, int m, const float *queries_dev, float max_dist2, unsigned *counts_dev,
                           void *stream, unsigned flags)
{
    const WithinCall w = {"knn_index_count_within", kRouted, slot, m, queries_dev, 0, nullptr, max_dist2, stream, flags};
    KNN_TRY(within_check(w, {{!queries_dev || !counts_dev, "null queries or counts"}}, idx));
    return within_run(idx, w, counts_into(counts_dev));
}

int knn_debug_count_plan(const long long in[16], long long out[8])
{
    if (!in || !out || in[0] < 1 || in[0] > 4096 || in[1] < 1 || in[1] > INT_MAX || in[2] < 1 || in[12] < 0 || in[12] > 3 || in[13] < 0 ||
        in[13] > 2 || in[14] < 1 || in[14] > INT_MAX || in[15] < 0 || (in[6] != 0 && in[0] > 4) ||
        (in[6] != 0 && in[11] != 0))   // (a grid index needs k <= 4; a cell-range shard has none)
        return fail(KNN_EINVAL, "knn_debug_count_plan: bad arguments (1 <= k <= 4096, m >= 1, rows >= 1, path 0 .. 3, cells 0 .. 2, num_cu >= 1, "
                                "rings >= 0; a grid index only with k <= 4 and never on a cell-range shard)");
    for (int i = 3; i <= 11; ++i)
        if (in[i] != 0 && in[i] != 1)
            return fail(KNN_EINVAL, "knn_debug_count_plan: inputs 3 .. 11 are 0 or 1");
    CountRouteInputs ci;
    ci.k = (int)in[0];
    ci.m = (int)in[1];
    ci.n = in[2];
    ci.radius_finite = in[3] != 0;
    ci.flag_grid = in[4] != 0;
    ci.flag_cells = in[5] != 0;
    ci.has_grid = in[6] != 0;
    ci.has_cells = in[7] != 0;
    ci.centred = in[8] != 0;
    ci.rows_u8 = in[9] != 0;
    ci.bins = in[10] != 0;
    ci.sharded = in[11] != 0;
    ci.path = (int)in[12];
    ci.cells_option = (int)in[13];
    ci.num_cu = (int)in[14];
    ci.radius_rings = in[15];
    const CountPlan p = knn_count_route(ci);
    const long long v[8] = {(long long)p.way, p.passes, p.pass_m, p.rmax, p.blocks, p.waves, p.slices, (long long)p.scratch_bytes};
    memcpy(out, v, sizeof v);
    return KNN_OK;
}

int knn_counts_to_offsets(int device, const unsigned *counts_dev, int m, unsigned long long *offsets_dev, void *stream)
{
    if (m < 1)
        return fail(KNN_EINVAL, "knn_counts_to_offsets: m < 1");
    if (!counts_dev || !offsets_dev)
        return fail(KNN_EINVAL, "knn_counts_to_offsets: null counts or offsets");
    DeviceGuard guard(device);
    if (!guard.ok)
        return fail(KNN_EHIP, "knn_counts_to_offsets: hipSetDevice failed");
    HIP_TRY(knn_counts_to_offsets_launch(counts_dev, m, (u64 *)offsets_dev, (hipStream_t)stream));
    return KNN_OK;
}

int knn_keys_sort_segments(int device, int m, const unsigned long long *offsets_dev, const unsigned *fill_dev,
                           unsigned long long *keys_dev, void *stream)
{
    if (m < 1)
        return fail(KNN_EINVAL, "knn_keys_sort_segments: m < 1");
    if (!offsets_dev || !fill_dev || !keys_dev)
        return fail(KNN_EINVAL, "knn_keys_sort_segments: null offsets, fill or keys");
    DeviceGuard guard(device);
    if (!guard.ok)
        return fail(KNN_EHIP, "knn_keys_sort_segments: hipSetDevice failed");
    HIP_TRY(knn_keys_sort_segments_launch(m, (const u64 *)offsets_dev, fill_dev, (u64 *)keys_dev, (hipStream_t)stream));
    return KNN_OK;
}

int knn_index_list_within(knn_index *idx, int slot, int m, const float *queries_dev, float max_dist2,
                          const unsigned long long *offsets_dev, unsigned *fill_dev, unsigned long long *keys_dev, void *stream,
                          unsigned flags)
{
    const WithinCall w = {"knn_index_list_within", kRouted, slot, m, queries_dev, 0, nullptr, max_dist2, stream, flags};
    KNN_TRY(within_check(w, {{!queries_dev || !offsets_dev || !fill_dev || !keys_dev, "null queries, offsets, fill or keys"}}, idx));
    return within_run(idx, w, lists_into(offsets_dev, fill_dev, keys_dev));
}

int knn_index_query_topk_large(knn_index *idx, int slot, int m, int K, const float *queries_dev, float max_dist2,
                               unsigned long long *keys_dev, int *indices_dev, void *stream, unsigned flags)
{
    // (its sizes before slot, radius and flags: tests/test_topk_large_logic.py tells the rules apart without a GPU)
    const TopkEntry t = {"knn_index_query_topk_large", kLarge | kSizesFirst, slot, m, K, queries_dev, 0, max_dist2, nullptr, keys_dev, stream, flags};
    KNN_TRY(topk_check(t, {{!queries_dev || !keys_dev, "null queries or keys"}}, idx));
    return topk_one_way(idx, t, indices_dev);
}

int knn_keys_topk_merge_large(int device, int m, int K, const unsigned long long *a_dev, unsigned long long *b_dev, void *stream)
{
    if (K < 1 || K > KNN_TOPK_LARGE_MAX)
        return fail(KNN_EINVAL, "knn_keys_topk_merge_large: K outside 1 .. 4096");
    if (m < 1)
        return fail(KNN_EINVAL, "knn_keys_topk_merge_large: m < 1");
    if (!a_dev || !b_dev)
        return fail(KNN_EINVAL, "knn_keys_topk_merge_large: null list");
    DeviceGuard guard(device);
    if (!guard.ok)
        return fail(KNN_EHIP, "knn_keys_topk_merge_large: hipSetDevice failed");
    HIP_TRY(knn_topk_merge_large_launch(m, K, (const u64 *)a_dev, (u64 *)b_dev, (hipStream_t)stream));
    return KNN_OK;
}

int knn_debug_topk_large_plan(const long long in[6], long long out[8])
{
    if (!in || !out || in[0] < 1 || in[0] > INT_MAX || in[1] < 1 || in[1] > INT_MAX || in[2] < 1 || in[2] > KNN_TOPK_LARGE_MAX ||
        in[1] * in[2] > INT_MAX || in[3] < 1 || in[4] < 1 || in[4] > INT_MAX || (in[5] != 0 && in[5] != 1))
        return fail(KNN_EINVAL, "knn_debug_topk_large_plan: bad arguments (k >= 1, m >= 1, 1 <= K <= 4096, m * K <= INT_MAX, rows >= 1, "
                                "CUs >= 1, init 0 or 1)");
    const TopkLargePlan p = knn_topk_large_plan((int)in[0], (int)in[1], (int)in[2], in[3], (int)in[4], in[5] != 0);
    const long long v[8] = {p.chunks, p.slices, p.dist_passes, p.index_passes, (long long)p.lds_bytes, (long long)p.scratch_bytes,
                            p.launches_clean, p.launches_ties};
    memcpy(out, v, sizeof v);
    return KNN_OK;
}

int knn_debug_radix_kth(const unsigned long long *keys, long long n, int K, unsigned long long *kth, int *passes_run)
{
    if (!kth || !passes_run || n < 0 || (n > 0 && !keys) || K < 1 || K > KNN_TOPK_LARGE_MAX)
        return fail(KNN_EINVAL, "knn_debug_radix_kth: bad arguments (n >= 0, 1 <= K <= 4096)");
    // the device sequence for one query: per pass the histogram of the keys under the prefix, then the pick; a pass runs only
    // when the one before left the query open
    u64 prefix = 0ull;
    unsigned need = (unsigned)K;
    int passes = 0;
    bool open = true;
    for (int pass = 0; pass < KNN_RADIX_PASSES && open; ++pass, ++passes) {
        unsigned hist[KNN_RADIX_BINS] = {0u};
        for (long long i = 0; i < n; ++i)
            if (knn_radix_match(keys[i], prefix, pass))
                ++hist[knn_radix_digit(keys[i], pass)];
        open = knn_radix_pick(hist, 1ull, pass, prefix, need);
    }
    *kth = prefix;
    *passes_run = passes;
    return KNN_OK;
}

// ---- queries over a subset of the rows (include/knn_mi355x.h 2g; knn_masked.hip) ------------------------------------------------
// (tests/test_masked_logic.py tells the rules apart without a GPU)
int knn_index_query_topk_masked(knn_index *idx, int slot, int m, int K, const float *queries_dev, float max_dist2,
                                const unsigned *mask_dev, unsigned long long *keys_dev, int *indices_dev, void *stream, unsigned flags)
{
    const TopkEntry t = {"knn_index_query_topk_masked", kMasked, slot, m, K, queries_dev, 0, max_dist2, mask_dev, keys_dev, stream, flags};
    KNN_TRY(topk_check(t, {{!queries_dev || !mask_dev || !keys_dev, "null queries, mask or keys"}}, idx));
    return topk_one_way(idx, t, indices_dev);
}

int knn_index_count_within_masked(knn_index *idx, int slot, int m, const float *queries_dev, float max_dist2,
                                  const unsigned *mask_dev, unsigned *counts_dev, void *stream, unsigned flags)
{
    const WithinCall w = {"knn_index_count_within_masked", kMasked, slot, m, queries_dev, 0, nullptr, max_dist2, stream, flags, mask_dev};
    KNN_TRY(within_check(w, {{!queries_dev || !mask_dev || !counts_dev, "null queries, mask or counts"}}, idx));
    return within_run(idx, w, counts_into(counts_dev));   // (not routed: one way on every index, no layout is consulted)
}

int knn_mask_set_rows(int device, long long n_local, const unsigned *rows_dev, long long count, int value, unsigned *mask_dev,
                      void *stream)
{
    if (n_local < 0)
        return fail(KNN_EINVAL, "knn_mask_set_rows: n_local < 0");
    if (count < 0)
        return fail(KNN_EINVAL, "knn_mask_set_rows: count < 0");
    if (value != 0 && value != 1)
        return fail(KNN_EINVAL, "knn_mask_set_rows: value is 0 (clear) or 1 (set)");
    if ((count > 0 && !rows_dev) || !mask_dev)
        return fail(KNN_EINVAL, "knn_mask_set_rows: null rows or mask");
    DeviceGuard guard(device);
    if (!guard.ok)
        return fail(KNN_EHIP, "knn_mask_set_rows: hipSetDevice failed");
    HIP_TRY(knn_mask_set_rows_launch(n_local, rows_dev, count, value, mask_dev, (hipStream_t)stream));
    return KNN_OK;
}

int knn_debug_masked_plan(const long long in[6], long long out[8])
{
    if (!in || !out || in[0] < 1 || in[0] > INT_MAX || in[1] < 1 || in[1] > INT_MAX || in[2] < 0 || in[2] > KNN_TOPK_MAX ||
        in[1] * in[2] > INT_MAX || in[3] < 0 || in[3] > (1ll << 32) || in[4] < 1 || in[4] > INT_MAX || (in[5] != 0 && in[5] != 1))
        return fail(KNN_EINVAL, "knn_debug_masked_plan: bad arguments (k >= 1, m >= 1, 0 <= K <= 64, m * K <= INT_MAX, 0 <= rows <= 2^32, "
                                "CUs >= 1, init 0 or 1)");
    const MaskedPlan p = knn_masked_plan((int)in[0], (int)in[1], (int)in[2], in[3], (int)in[4], in[5] != 0);
    const long long v[8] = {p.granules, p.slices, p.chunks, (long long)p.lds_bytes, (long long)p.mask_bytes, (long long)p.part_bytes,
                            p.launches, p.chunk_m};
    memcpy(out, v, sizeof v);
    return KNN_OK;
}

int knn_debug_mask_split(const unsigned *granule_counts, long long granules, int slices, long long *first_granule)
{
    if (granules < 0 || granules > (1ll << 22) || (granules > 0 && !granule_counts) || slices < 1 || slices > 65535 || !first_granule)
        return fail(KNN_EINVAL, "knn_debug_mask_split: bad arguments (0 <= granules <= 2^22, 1 <= slices <= 65535)");
    // the device sequence: the exclusive 64-bit prefix of the counts, then every block's search over it
    std::vector<u64> P((size_t)granules + 1, 0ull);
    for (long long g = 0; g < granules; ++g)
        P[(size_t)g + 1] = P[(size_t)g] + granule_counts[g];
    if (P[(size_t)granules] >= (1ull << 48))   // (T * S must stay below 2^64; a shard's rows are far below)
        return fail(KNN_EINVAL, "knn_debug_mask_split: more than 2^48 admitted rows");
    for (int b = 0; b <= slices; ++b)
        first_granule[b] = knn_mask_split_first(P.data(), granules, (u64)slices, (u64)b);
    return KNN_OK;
}

int knn_debug_mask_split_rows(const unsigned *mask_host, long long n_local, int slices, long long *first_row)
{
    if (n_local < 0 || n_local > (1ll << 32) || (n_local > 0 && !mask_host) || slices < 1 || slices > 65535 || !first_row)
        return fail(KNN_EINVAL, "knn_debug_mask_split_rows: bad arguments (0 <= n_local <= 2^32, 1 <= slices <= 65535)");
    // the device sequence: every granule's admitted rows, their exclusive 64-bit prefix, then every block's cut
    const long long G = (n_local + KNN_MASK_GRANULE_ROWS - 1) / KNN_MASK_GRANULE_ROWS;
    std::vector<u64> P((size_t)G + 1, 0ull);
    for (long long g = 0; g < G; ++g) {
        u64 c = 0ull;
        for (int j = 0; j < KNN_MASK_GRANULE_WORDS; ++j)
            c += (unsigned)__builtin_popcount(knn_mask_word(mask_host, n_local, g * KNN_MASK_GRANULE_WORDS + j));
        P[(size_t)g + 1] = P[(size_t)g] + c;
    }
    for (int b = 0; b <= slices; ++b)
        first_row[b] = knn_mask_split_row(mask_host, n_local, P.data(), G, (u64)slices, (u64)b);
    return KNN_OK;
}

// ---- lists and top-K beyond 64 over a subset of the rows (include/knn_mi355x.h 2h; knn_masked_lists.hip) ------------------------
// (one message per rule, in the header's order, the index last: tests/test_masked_lists_logic.py tells them apart without a GPU)
int knn_index_list_within_masked(knn_index *idx, int slot, int m, const float *queries_dev, float max_dist2, const unsigned *mask_dev,
                                 const unsigned long long *offsets_dev, unsigned *fill_dev, unsigned long long *keys_dev, void *stream,
                                 unsigned flags)
{
    const WithinCall w = {"knn_index_list_within_masked", kMasked, slot, m, queries_dev, 0, nullptr, max_dist2, stream, flags, mask_dev};
    KNN_TRY(within_check(w, {{!queries_dev, "null queries"}, {!mask_dev, "null mask"}, {!offsets_dev || !fill_dev || !keys_dev, kNullLists}},
                         idx));
    return within_run(idx, w, lists_into(offsets_dev, fill_dev, keys_dev));   // (not routed: one way on every index)
}

int knn_index_query_topk_large_masked(knn_index *idx, int slot, int m, int K, const float *queries_dev, float max_dist2,
                                      const unsigned *mask_dev, unsigned long long *keys_dev, int *indices_dev, void *stream,
                                      unsigned flags)
{
    const TopkEntry t = {"knn_index_query_topk_large_masked", kLarge | kMasked, slot, m, K, queries_dev, 0, max_dist2, mask_dev, keys_dev, stream,
                         flags};
    KNN_TRY(topk_check(t, {{!queries_dev, "null queries"}, {!mask_dev, "null mask"}, {!keys_dev, "null keys"}}, idx));
    return topk_one_way(idx, t, indices_dev);
}

int knn_debug_masked_lists_plan(const long long in[6], long long out[8])
{
    if (!in || !out || in[0] < 1 || in[0] > INT_MAX || in[1] < 1 || in[1] > INT_MAX || in[2] < 0 || in[2] > KNN_TOPK_LARGE_MAX ||
        in[1] * in[2] > INT_MAX || in[3] < 0 || in[3] > (1ll << 32) || in[4] < 1 || in[4] > INT_MAX || (in[5] != 0 && in[5] != 1))
        return fail(KNN_EINVAL, "knn_debug_masked_lists_plan: bad arguments (k >= 1, m >= 1, 0 <= K <= 4096, m * K <= INT_MAX, "
                                "0 <= rows <= 2^32, CUs >= 1, init 0 or 1)");
    const MaskedListsPlan p = knn_masked_lists_plan((int)in[0], (int)in[1], (int)in[2], in[3], (int)in[4], in[5] != 0);
    const long long v[8] = {p.cut.granules, p.slices, p.slice_waves, p.cut.chunks, (long long)p.lds_bytes, (long long)p.cut.mask_bytes,
                            (long long)p.select_bytes, p.launches};
    memcpy(out, v, sizeof v);
    return KNN_OK;
}

// ---- queries about the shard's own rows (include/knn_mi355x.h 2i; knn_self.hip) -------------------------------------------------
// (one message per rule, in the header's order, the index before the one rule that needs it: tests/test_self_logic.py tells them
// apart without a GPU)
int knn_index_self_topk(knn_index *idx, int slot, long long row_first, int rows, int K, float max_dist2, unsigned long long *keys_dev,
                        int *indices_dev, void *stream, unsigned flags)
{
    const TopkEntry t = {"knn_index_self_topk", kSelf, slot, rows, K, nullptr, row_first, max_dist2, nullptr, keys_dev, stream, flags,
                         KNN_QUERY_INIT_KEYS | KNN_QUERY_TOPK_GRID | KNN_QUERY_TOPK_FRAMES};   // the three it admits
    KNN_TRY(topk_check(t, {{!keys_dev, "null keys"}}, idx));
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    if (row_first > idx->n || (long long)rows > idx->n - row_first)
        return fail(KNN_EINVAL, "knn_index_self_topk: row_first + rows above the shard's rows");
    // The way: what the one route function says for the plain call of K + 1 neighbours — self is among ITS candidates — with
    // this call's rows, flags and options.  Exact, or no room for K + 1 keys — K = 64, or rows * (K + 1) beyond the plain call's
    // own INT_MAX limit —: the self-scan with K (the header's 2i says so), on the one-way front.
    const bool through = K + 1 <= KNN_TOPK_MAX && (long long)rows * (K + 1) <= INT_MAX && knn_query_route(route_inputs(idx, rows, K + 1, flags)).way != QueryWay::Exact;
    if (!through)
        return topk_one_way(idx, t, indices_dev);
    DeviceGuard guard(idx->device);
    if (!guard.ok)
        return fail(KNN_EHIP, "knn_index_self_topk: hipSetDevice failed");
    // the plain call as it is — its queries the resident rows, handed by address; -0 counts as 0 —, K + 1 keys per row into the slot's
    // scratch; its fallbacks and statistics are its own
    const bool init = (flags & KNN_QUERY_INIT_KEYS) != 0u;
    hipStream_t s = (hipStream_t)stream;
    u64 *keys = (u64 *)keys_dev;
    knn_index::TopkSlot &ts = idx->topk[slot];
    KNN_TRY(slot_buffer_grow(ts.self, ts.self_bytes, knn_self_plan(idx->k, rows, K, idx->n, idx->num_cu, init).through_bytes));
    const TopkCall plain = topk_call_of(rows, K + 1, idx->refs + (size_t)row_first * (size_t)idx->k, ts.self, stream, max_dist2 == 0.0f ? 0.0f : max_dist2);
    KNN_TRY(query_topk(idx, slot, plain, nullptr, flags | KNN_QUERY_INIT_KEYS, "knn_index_self_topk"));
    u64 *kept = init ? keys : ts.self + (size_t)rows * (size_t)(K + 1);
    HIP_TRY(knn_self_drop_launch(rows, K, ts.self, row_first, idx->base, shard_gids(idx), kept, s));
    if (!init)
        HIP_TRY(knn_topk_merge_launch(rows, K, kept, keys, s));
    if (indices_dev)
        HIP_TRY(knn_keys_unpack_launch(keys, rows * K, indices_dev, s));
    return KNN_OK;
}

int knn_index_self_count_within(knn_index *idx, int slot, long long row_first, int rows, float max_dist2, unsigned *counts_dev,
                                void *stream, unsigned flags)
{
    const WithinCall w = {"knn_index_self_count_within", kSelf, slot, rows, nullptr, row_first, nullptr, max_dist2, stream, flags};
    KNN_TRY(within_check(w, {{!counts_dev, "null counts"}}, idx));
    return within_run(idx, w, counts_into(counts_dev));
}

int knn_index_self_list_within(knn_index *idx, int slot, long long row_first, int rows, float max_dist2,
                               const unsigned long long *offsets_dev, unsigned *fill_dev, unsigned long long *keys_dev, void *stream,
                               unsigned flags)
{
    const WithinCall w = {"knn_index_self_list_within", kSelf, slot, rows, nullptr, row_first, nullptr, max_dist2, stream, flags};
    KNN_TRY(within_check(w, {{!offsets_dev || !fill_dev || !keys_dev, kNullLists}}, idx));
    return within_run(idx, w, lists_into(offsets_dev, fill_dev, keys_dev));
}

// ---- 2j. A radius per query: max_dist2_dev the radii, cap the radius the way is chosen at -----------------------------------------
int knn_index_count_within_each(knn_index *idx, int slot, int m, const float *queries_dev, const float *max_dist2_dev, float cap,
                                unsigned *counts_dev, void *stream, unsigned flags)
{
    const WithinCall w = {"knn_index_count_within_each", kCap | kRouted, slot, m, queries_dev, 0, max_dist2_dev, cap, stream, flags};
    KNN_TRY(within_check(w, {{!queries_dev, "null queries"}, {!max_dist2_dev, "null radii"}, {!counts_dev, "null counts"}}, idx));
    return within_run(idx, w, counts_into(counts_dev));
}

int knn_index_list_within_each(knn_index *idx, int slot, int m, const float *queries_dev, const float *max_dist2_dev, float cap,
                               const unsigned long long *offsets_dev, unsigned *fill_dev, unsigned long long *keys_dev, void *stream,
                               unsigned flags)
{
    const WithinCall w = {"knn_index_list_within_each", kCap | kRouted, slot, m, queries_dev, 0, max_dist2_dev, cap, stream, flags};
    KNN_TRY(within_check(w, {{!queries_dev, "null queries"}, {!max_dist2_dev, "null radii"},
                             {!offsets_dev || !fill_dev || !keys_dev, kNullLists}}, idx));
    return within_run(idx, w, lists_into(offsets_dev, fill_dev, keys_dev));
}

int knn_index_self_count_within_each(knn_index *idx, int slot, long long row_first, int rows, const float *max_dist2_dev, float cap,
                                     unsigned *counts_dev, void *stream, unsigned flags)
{
    const WithinCall w = {"knn_index_self_count_within_each", kCap | kSelf, slot, rows, nullptr, row_first, max_dist2_dev, cap, stream, flags};
    KNN_TRY(within_check(w, {{!max_dist2_dev, "null radii"}, {!counts_dev, "null counts"}}, idx));
    return within_run(idx, w, counts_into(counts_dev));
}

int knn_index_self_list_within_each(knn_index *idx, int slot, long long row_first, int rows, const float *max_dist2_dev, float cap,
                                    const unsigned long long *offsets_dev, unsigned *fill_dev, unsigned long long *keys_dev,
                                    void *stream, unsigned flags)
{
    const WithinCall w = {"knn_index_self_list_within_each", kCap | kSelf, slot, rows, nullptr, row_first, max_dist2_dev, cap, stream, flags};
    KNN_TRY(within_check(w, {{!max_dist2_dev, "null radii"}, {!offsets_dev || !fill_dev || !keys_dev, kNullLists}}, idx));
    return within_run(idx, w, lists_into(offsets_dev, fill_dev, keys_dev));
}

// ---- 2k. The radius graph on the grid and cell-pruned ways (DESIGN §4.6 "The radius graph on the pruned ways") --------------------
// max_dist2_dev null: the scalar form, every row's radius the cap.
int knn_index_self_count_within_routed(knn_index *idx, int slot, long long row_first, int rows, const float *max_dist2_dev, float cap,
                                       unsigned *counts_dev, void *stream, unsigned flags)
{
    const WithinCall w = {"knn_index_self_count_within_routed", kCap | kRouted | kSelf, slot, rows, nullptr, row_first, max_dist2_dev, cap,
                          stream, flags};
    KNN_TRY(within_check(w, {{!counts_dev, "null counts"}}, idx));
    return within_run(idx, w, counts_into(counts_dev));
}

int knn_index_self_list_within_routed(knn_index *idx, int slot, long long row_first, int rows, const float *max_dist2_dev, float cap,
                                      const unsigned long long *offsets_dev, unsigned *fill_dev, unsigned long long *keys_dev,
                                      void *stream, unsigned flags)
{
    const WithinCall w = {"knn_index_self_list_within_routed", kCap | kRouted | kSelf, slot, rows, nullptr, row_first, max_dist2_dev, cap,
                          stream, flags};
    KNN_TRY(within_check(w, {{!offsets_dev || !fill_dev || !keys_dev, kNullLists}}, idx));
    return within_run(idx, w, lists_into(offsets_dev, fill_dev, keys_dev));
}

// ---- over a subset of the rows, on the pruned ways (include/knn_mi355x.h 2l; knn_masked_routed.hip, knn_grid.hip) ---------------
// (one message per rule, in the header's order, the index last: tests/test_masked_routed_logic.py tells them apart without a GPU)
int knn_index_count_within_masked_routed(knn_index *idx, int slot, int m, const float *queries_dev, float max_dist2,
                                         const unsigned *mask_dev, unsigned *counts_dev, void *stream, unsigned flags)
{
    const WithinCall w = {"knn_index_count_within_masked_routed", kRouted | kMasked, slot, m, queries_dev, 0, nullptr, max_dist2, stream,
                          flags, mask_dev};
    KNN_TRY(within_check(w, {{!queries_dev, "null queries"}, {!mask_dev, "null mask"}, {!counts_dev, "null counts"}}, idx));
    return within_run(idx, w, counts_into(counts_dev));
}

int knn_index_list_within_masked_routed(knn_index *idx, int slot, int m, const float *queries_dev, float max_dist2,
                                        const unsigned *mask_dev, const unsigned long long *offsets_dev, unsigned *fill_dev,
                                        unsigned long long *keys_dev, void *stream, unsigned flags)
{
    const WithinCall w = {"knn_index_list_within_masked_routed", kRouted | kMasked, slot, m, queries_dev, 0, nullptr, max_dist2, stream,
                          flags, mask_dev};
    KNN_TRY(within_check(w, {{!queries_dev, "null queries"}, {!mask_dev, "null mask"}, {!offsets_dev || !fill_dev || !keys_dev, kNullLists}},
                         idx));
    return within_run(idx, w, lists_into(offsets_dev, fill_dev, keys_dev));
}

// ---- 2m. Clusters of the radius graph (include/knn_mi355x.h 2m; knn_cluster.hip, knn_grid.hip) -----------------------
// (one message per rule, in the header's order, the index before the one rule that needs it: tests/test_cluster_logic.py tells
// them apart without a GPU)
// (the two rules the device call and the host form share word for word)
constexpr unsigned kClusterFlags = KNN_QUERY_COUNT_GRID;   // the one flag the cluster calls admit
static int cluster_check(const char *who, float max_dist2, unsigned flags)
{
    if (!(max_dist2 >= 0.0f))
        return fail_in(KNN_EINVAL, who, "max_dist2 must be >= 0 and not NaN");
    if ((flags & ~kClusterFlags) != 0u)
        return fail_in(KNN_EINVAL, who, "unknown flag (KNN_QUERY_COUNT_GRID alone is admitted: the call always writes its labels, and "
                                        "the cell-pruned way is not built for it)");
    return KNN_OK;
}

// 2n's flag rule: the two flags of the routed count, and no INIT_KEYS — the call always writes its labels.
constexpr unsigned kClusterRoutedFlags = KNN_QUERY_COUNT_GRID | KNN_QUERY_COUNT_CELLS;
static int cluster_routed_check(const char *who, float max_dist2, unsigned flags)
{
    if (!(max_dist2 >= 0.0f))
        return fail_in(KNN_EINVAL, who, "max_dist2 must be >= 0 and not NaN");
    if ((flags & ~kClusterRoutedFlags) != 0u)
        return fail_in(KNN_EINVAL, who, "unknown flag (KNN_QUERY_COUNT_GRID, KNN_QUERY_COUNT_CELLS)");
    return KNN_OK;
}

// A device cluster call behind its radius and flag rules (2m's or 2n's, which decide the flags that can reach this): the rest of
// the ladder, then degrees -> core -> the link sweep of the degree step's way -> flatten.
static int cluster_run(const char *who, knn_index *idx, int slot, float max_dist2, int min_pts, int *labels_dev, unsigned *core_dev,
                       void *stream, unsigned flags)
{
    if (slot < 0 || slot >= KNN_SLOTS)
        return fail_in(KNN_EINVAL, who, "slot outside 0 .. 7");
    if (min_pts < 1)
        return fail_in(KNN_EINVAL, who, "min_pts < 1");
    if (!labels_dev)
        return fail_in(KNN_EINVAL, who, "null labels");
    if (!idx)
        return fail_in(KNN_EINVAL, who, "null index");
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    if (idx->n > INT_MAX)
        return fail_in(KNN_EINVAL, who, "more than INT_MAX rows (labels are int row numbers)");
    DeviceGuard guard(idx->device);
    if (!guard.ok)
        return fail_in(KNN_EHIP, who, "hipSetDevice failed");
    begin_call(idx, slot);
    if (idx->n == 0)   // an empty shard has no row to label
        return KNN_OK;
    const int n = (int)idx->n;
    // the slot's scratch, grown before the first launch
    const ClusterPlan plan = knn_cluster_plan(idx->n, idx->num_cu, core_dev == nullptr);
    knn_index::TopkSlot &ts = idx->topk[slot];
    KNN_TRY(slot_buffer_grow(ts.cluster, ts.cluster_bytes, plan.scratch_bytes));
    ClusterCall c;
    c.k = idx->k;
    c.n = idx->n;
    c.r = idx->refs;
    c.max_dist2 = max_dist2 == 0.0f ? 0.0f : max_dist2;   // (-0 counts as 0)
    c.min_pts = min_pts;
    c.num_cu = idx->num_cu;
    c.stream = (hipStream_t)stream;
    c.parent = labels_dev;
    c.best = ts.cluster;
    c.core = core_dev ? core_dev : (unsigned *)(ts.cluster + (size_t)n);
    // 1. degrees: the routed self count of the whole shard at cap = max_dist2 under the call's flag, zeroed first, into the labels.
    //    It decides the way (and leaves it in the statistics); its rules have passed above, so its texts cannot be met here.
    const WithinCall w = {who, kCap | kRouted | kSelf, slot, n, nullptr, 0, nullptr, max_dist2, stream, flags | KNN_QUERY_INIT_KEYS};
    KNN_TRY(within_run(idx, w, counts_into((unsigned *)labels_dev)));
    HIP_TRY(knn_cluster_core_launch(c));
    // 2. the link sweep on the same way; the grid's is followed by the exact one, gated on its give-up word
    if (idx->stats[0] == (long long)QueryWay::Grid) {
        const CountPlan cp = count_plan_of(idx, route_inputs(idx, n, 1, 0u), n, c.max_dist2, flags);
        const unsigned *gate = nullptr;
        HIP_TRY(knn_grid_cluster_link(idx->grid, cp.rmax, slot, c, &gate));
        idx->grid_topk_gate = gate;   // (the degree batch's walks are the same walks: both words say the same)
        HIP_TRY(knn_cluster_link_launch(c, gate));
    } else if (idx->stats[0] == (long long)QueryWay::Cells) {   // (2n alone: 2m's flag rule admits no KNN_QUERY_COUNT_CELLS)
        const CellTopkPlan tp = knn_cells_count_plan(route_inputs(idx, n, 1, 0u).t);
        if (!tp.use)
            return fail_in(KNN_EHIP, who, "the cell-pruned scan has no pass shape for this layout");
        HIP_TRY(knn_filter_cluster_link_cells(idx->filter, tp, slot, c));
    } else {
        HIP_TRY(knn_cluster_link_launch(c, nullptr));
    }
    // 3. forest -> labels
    HIP_TRY(knn_cluster_flatten_launch(c));
    return KNN_OK;
}

int knn_index_self_cluster_within(knn_index *idx, int slot, float max_dist2, int min_pts, int *labels_dev, unsigned *core_dev,
                                  void *stream, unsigned flags)
{
    const char *const who = "knn_index_self_cluster_within";
    KNN_TRY(cluster_check(who, max_dist2, flags));
    return cluster_run(who, idx, slot, max_dist2, min_pts, labels_dev, core_dev, stream, flags);
}

// ---- 2n. Clusters on the routed ways: 2m's answer, the cell-pruned way on request (knn_cluster_routed.hip) -------------------------
int knn_index_self_cluster_within_routed(knn_index *idx, int slot, float max_dist2, int min_pts, int *labels_dev, unsigned *core_dev,
                                         void *stream, unsigned flags)
{
    const char *const who = "knn_index_self_cluster_within_routed";
    KNN_TRY(cluster_routed_check(who, max_dist2, flags));
    return cluster_run(who, idx, slot, max_dist2, min_pts, labels_dev, core_dev, stream, flags);
}

int knn_debug_cluster_pair(int own_core, int row_core, long long row, long long own, int *action)
{
    if ((own_core != 0 && own_core != 1) || (row_core != 0 && row_core != 1) || row < 0 || own < 0 || row > INT_MAX || own > INT_MAX || !action)
        return fail(KNN_EINVAL, "knn_debug_cluster_pair: bad arguments (core bits 0 or 1, 0 <= row, own <= INT_MAX, no null action)");
    *action = knn_cluster_pair(own_core != 0, row_core != 0, row, own);   // the kernels' own lines (knn_cluster_pair.h)
    return KNN_OK;
}

int knn_debug_cluster_routed_plan(const long long in[], long long out[])
{
    // in = knn_debug_count_plan's sixteen with m = the shard's rows, then 1 if the caller passes core_dev
    const char *const bad = "knn_debug_cluster_routed_plan: bad arguments (knn_debug_count_plan's with m = the shard's rows <= INT_MAX, "
                            "core_dev given 0 or 1)";
    if (!in || !out || in[1] != in[2] || in[2] > INT_MAX || (in[16] != 0 && in[16] != 1))
        return fail(KNN_EINVAL, bad);
    long long cnt[8];
    if (knn_debug_count_plan(in, cnt) != KNN_OK)
        return fail(KNN_EINVAL, bad);
    const long long way = cnt[0], n = in[2];
    const ClusterPlan p = knn_cluster_plan(n, (int)in[14], in[16] == 0);
    long long launches = way == 3 ? p.launches_grid : p.launches_exact, with_outliers = launches;
    if (way == 4) {
        // per pass of the degree step: prep, match, record-only scan, count re-rank of the slices and of the overflow area, commit,
        // the gated self-scan (a pass's rows are one chunk) = 7; per pass of the link sweep: the same front, the link re-rank of the
        // slices and of the overflow area, the gated twin = 6; core and flatten.  A layout with out-of-box rows: one more in each.
        const long long gated = knn_divup(std::min<long long>(n, KNN_CELL_BATCH), KNN_TOPK_CHUNK);
        launches = cnt[1] * (11 + 2 * gated) + 2;
        with_outliers = launches + 2 * cnt[1];
    }
    const long long v[8] = {way, cnt[1], cnt[2], launches, with_outliers, (long long)p.scratch_bytes,
                            way == 1 ? 0 : (long long)p.count_bytes, p.chunks};
    memcpy(out, v, sizeof v);
    return KNN_OK;
}

int knn_debug_cluster_plan(const long long in[], long long out[])
{
    // in = {k, the shard's rows, CUs, 1 if the caller passes core_dev, 1 if the grid way answers}
    if (!in || !out || in[0] < 1 || in[0] > INT_MAX || in[1] < 0 || in[1] > INT_MAX || in[2] < 1 || in[2] > INT_MAX ||
        (in[3] != 0 && in[3] != 1) || (in[4] != 0 && in[4] != 1) || (in[4] != 0 && in[0] > 4))
        return fail(KNN_EINVAL, "knn_debug_cluster_plan: bad arguments (k >= 1, 0 <= rows <= INT_MAX, CUs >= 1, core_dev given 0 or 1, "
                                "grid way 0 or 1 and only with k <= 4)");
    const ClusterPlan p = knn_cluster_plan(in[1], (int)in[2], in[3] == 0);
    const bool grid = in[4] != 0 && in[1] > 0;
    const long long v[8] = {p.chunks, p.slices, p.launches_exact, p.launches_grid, (long long)p.scratch_bytes,
                            grid ? (long long)p.count_bytes : 0, in[1] > 0 ? (grid ? 3 : 1) : 1, grid ? p.launches_grid : p.launches_exact};
    memcpy(out, v, sizeof v);
    return KNN_OK;
}

int knn_debug_cluster_unite(int *parent, long long n, const int *pairs, long long npairs)
{
    if (n < 0 || n > INT_MAX || npairs < 0 || (n > 0 && !parent) || (npairs > 0 && !pairs))
        return fail(KNN_EINVAL, "knn_debug_cluster_unite: bad arguments (0 <= n <= INT_MAX, npairs >= 0, no null array)");
    for (long long t = 0; t < 2 * npairs; ++t)
        if (pairs[t] < 0 || pairs[t] >= n)
            return fail(KNN_EINVAL, "knn_debug_cluster_unite: a pair names a row outside 0 .. n - 1");
    for (long long i = 0; i < n; ++i)
        if (parent[i] < 0 || parent[i] > i)
            return fail(KNN_EINVAL, "knn_debug_cluster_unite: parent[x] <= x does not hold on entry (start from parent[x] = x)");
    // the kernels' own lines (knn_cluster_uf.h) with the host's atomics
    for (long long t = 0; t < npairs; ++t)
        (void)knn_uf_unite<KnnUfHost>(parent, pairs[2 * t], pairs[2 * t + 1]);
    return KNN_OK;
}

// ---- 2o. Minimum spanning forest of the radius graph (include/knn_mi355x.h 2o; knn_forest.hip, knn_grid.hip) ----------
// (one message per rule, in the header's order; tests/test_forest_logic.py tells them apart without a GPU)
constexpr unsigned kForestFlags = KNN_QUERY_COUNT_GRID;   // the one flag the forest calls admit
static int forest_check(const char *who, float max_dist2, unsigned flags)
{
    if (!(max_dist2 >= 0.0f))
        return fail_in(KNN_EINVAL, who, "max_dist2 must be >= 0 and not NaN");
    if ((flags & ~kForestFlags) != 0u)
        return fail_in(KNN_EINVAL, who, "unknown flag (KNN_QUERY_COUNT_GRID alone is admitted: the call always writes its outputs, and "
                                        "the cell-pruned way is not built for it)");
    return KNN_OK;
}

int knn_index_self_forest_within(knn_index *idx, int slot, float max_dist2, int *labels_dev, unsigned long long *edge_keys_dev,
                                 unsigned *edge_hi_dev, unsigned *count_dev, void *stream, unsigned flags)
{
    const char *const who = "knn_index_self_forest_within";
    KNN_TRY(forest_check(who, max_dist2, flags));
    if (slot < 0 || slot >= KNN_SLOTS)
        return fail_in(KNN_EINVAL, who, "slot outside 0 .. 7");
    if (!labels_dev || !edge_keys_dev || !edge_hi_dev || !count_dev)
        return fail_in(KNN_EINVAL, who, "null labels, edge keys, edge hi or count");
    if (!idx)
        return fail_in(KNN_EINVAL, who, "null index");
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    if (idx->n > INT_MAX)
        return fail_in(KNN_EINVAL, who, "more than INT_MAX rows (labels and edge ends are int row numbers)");
    DeviceGuard guard(idx->device);
    if (!guard.ok)
        return fail_in(KNN_EHIP, who, "hipSetDevice failed");
    begin_call(idx, slot);
    if (idx->n == 0) {   // an empty shard has no row and no edge
        HIP_TRY(hipMemsetAsync(count_dev, 0, 2 * sizeof(unsigned), (hipStream_t)stream));
        return KNN_OK;
    }
    const int n = (int)idx->n;
    const ForestPlan plan = knn_forest_plan(idx->n, idx->num_cu);
    knn_index::TopkSlot &ts = idx->topk[slot];
    KNN_TRY(slot_buffer_grow(ts.forest, ts.forest_bytes, plan.scratch_bytes));   // the slot's scratch, grown before the first launch
    ForestCall c;
    c.k = idx->k;
    c.n = idx->n;
    c.r = idx->refs;
    c.max_dist2 = max_dist2 == 0.0f ? 0.0f : max_dist2;   // (-0 counts as 0)
    c.num_cu = idx->num_cu;
    c.stream = (hipStream_t)stream;
    c.labels = labels_dev;
    c.edge_keys = edge_keys_dev;
    c.edge_hi = edge_hi_dev;
    c.count = count_dev;
    knn_forest_layout(c, plan, ts.forest);
    // the way the routed self count takes for the shard's rows at this cap under the call's flag
    const CountPlan cp = count_plan_of(idx, route_inputs(idx, n, 1, 0u), n, c.max_dist2, flags);
    const bool grid = cp.way == QueryWay::Grid;
    idx->stats[0] = (long long)(grid ? QueryWay::Grid : QueryWay::Exact);
    HIP_TRY(knn_forest_begin_launch(c, plan));
    for (int t = 0; t < c.rounds; ++t) {
        HIP_TRY(knn_forest_flatten_launch(c, t));
        if (grid) {   // the walk, then the exact scan gated on the round's give-up word as well
            HIP_TRY(knn_grid_forest_scan(idx->grid, cp.rmax, c, t));
            HIP_TRY(knn_forest_scan_launch(c, t, c.giveup(t)));
        } else {
            HIP_TRY(knn_forest_scan_launch(c, t, nullptr));
        }
        HIP_TRY(knn_forest_pick_launch(c, t));
    }
    HIP_TRY(knn_forest_labels_launch(c));   // (the last round's hook left a forest: one more flatten when it added an edge)
    if (grid)
        idx->grid_topk_gate = c.stat();   // (the give-up word of the last round that ran)
    return KNN_OK;
}

int knn_debug_forest_plan(const long long in[], long long out[])
{
    // in = {k, the shard's rows, CUs, 1 if the grid way answers}
    if (!in || !out || in[0] < 1 || in[0] > INT_MAX || in[1] < 0 || in[1] > INT_MAX || in[2] < 1 || in[2] > INT_MAX ||
        (in[3] != 0 && in[3] != 1) || (in[3] != 0 && in[0] > 4))
        return fail(KNN_EINVAL, "knn_debug_forest_plan: bad arguments (k >= 1, 0 <= rows <= INT_MAX, CUs >= 1, grid way 0 or 1 and only "
                                "with k <= 4)");
    const ForestPlan p = knn_forest_plan(in[1], (int)in[2]);
    const bool grid = in[3] != 0 && in[1] > 0;
    const long long v[8] = {p.rounds, p.chunks, p.slices, p.launches_exact, p.launches_grid, (long long)p.scratch_bytes, grid ? 3 : 1,
                            grid ? p.launches_grid : p.launches_exact};
    memcpy(out, v, sizeof v);
    return KNN_OK;
}

int knn_debug_forest_round(long long n, int *parent, const unsigned long long *cand, unsigned long long *edge_keys, unsigned *edge_hi,
                           unsigned *count, int *added)
{
    if (n < 0 || n > INT_MAX || !count || !added || (n > 0 && (!parent || !cand || !edge_keys || !edge_hi)))
        return fail(KNN_EINVAL, "knn_debug_forest_round: bad arguments (0 <= n <= INT_MAX, no null array)");
    for (long long i = 0; i < n; ++i)
        if (parent[i] < 0 || parent[i] > i)
            return fail(KNN_EINVAL, "knn_debug_forest_round: parent[x] <= x does not hold on entry (start from parent[x] = x)");
    for (long long i = 0; i < n; ++i)
        if (cand[i] != KNN_FOREST_NONE && ((long long)(unsigned)cand[i] >= n || (long long)(unsigned)cand[i] == i))
            return fail(KNN_EINVAL, "knn_debug_forest_round: a candidate names the row itself or a row outside 0 .. n - 1");
    const int threads = std::min(16, std::max(1, *added));
    // every step over all rows, row i on thread i % threads, a join between two steps (the launches' order on the stream)
    const auto step = [&](const std::function<void(long long)> &row) {
        if (threads == 1) {
            for (long long i = 0; i < n; ++i)
                row(i);
            return;
        }
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t)
            pool.emplace_back([&, t] {
                for (long long i = t; i < n; i += threads)
                    row(i);
            });
        for (std::thread &th : pool)
            th.join();
    };
    // the kernels' own lines (knn_forest_pick.h, knn_cluster_uf.h) with the host's atomics
    std::vector<unsigned long long> pick1((size_t)n);
    std::vector<unsigned> pick2((size_t)n);
    const unsigned before = count[0];
    unsigned raised = 0u;
    step([&](long long i) {   // flatten
        knn_forest_flatten<KnnPickHost>(parent, i);
        knn_forest_clear(pick1.data(), pick2.data(), i);
    });
    step([&](long long i) { knn_forest_offer1<KnnPickHost>(parent, cand, pick1.data(), i); });
    step([&](long long i) { knn_forest_offer2<KnnPickHost>(parent, cand, pick1.data(), pick2.data(), i); });
    step([&](long long i) { (void)knn_forest_emit<KnnPickHost>(parent, pick1.data(), pick2.data(), i, n, edge_keys, edge_hi, count, &raised); });
    step([&](long long i) { knn_forest_hook<KnnPickHost>(parent, pick1.data(), pick2.data(), i); });
    *added = (int)(count[0] - before);
    return KNN_OK;
}

int knn_debug_self_routed_plan(const long long in[16], long long out[8])
{
    // knn_debug_count_plan's inputs with m = the call's rows, which lie inside the shard; its outputs, [6] from the self-scan's plan
    if (!in || !out || in[1] < 1 || in[1] > in[2] || in[2] > (1ll << 32))
        return fail(KNN_EINVAL, "knn_debug_self_routed_plan: bad arguments (knn_debug_count_plan's, and 1 <= rows <= the shard's rows <= 2^32)");
    const int rv = knn_debug_count_plan(in, out);
    if (rv != KNN_OK)
        return fail(rv, "knn_debug_self_routed_plan: bad arguments (knn_debug_count_plan's, and 1 <= rows <= the shard's rows <= 2^32)");
    out[6] = knn_self_plan((int)in[0], (int)in[1], 0, in[2], (int)in[14], true).slices;
    return KNN_OK;
}

int knn_keys_column_dist2(int device, const unsigned long long *keys_dev, int m, int K, int column, float *dist2_dev, void *stream)
{
    if (m < 1)
        return fail(KNN_EINVAL, "knn_keys_column_dist2: m < 1");
    if (K < 1 || column < 0 || column >= K)
        return fail(KNN_EINVAL, "knn_keys_column_dist2: K < 1 or column outside 0 .. K - 1");
    if (!keys_dev || !dist2_dev)
        return fail(KNN_EINVAL, "knn_keys_column_dist2: null keys or dist2");
    DeviceGuard guard(device);
    if (!guard.ok)
        return fail(KNN_EHIP, "knn_keys_column_dist2: hipSetDevice failed");
    HIP_TRY(knn_keys_column_dist2_launch((const u64 *)keys_dev, m, K, column, dist2_dev, (hipStream_t)stream));
    return KNN_OK;
}

int knn_debug_each_radius(float radius, float cap, float out[2])
{
    if (!out)
        return fail(KNN_EINVAL, "knn_debug_each_radius: null out");
    if (!(cap >= 0.0f))
        return fail(KNN_EINVAL, "knn_debug_each_radius: cap must be >= 0 (or +INF) and not NaN");
    const bool has = knn_each_has(radius);
    out[0] = has ? 1.0f : 0.0f;
    out[1] = has ? knn_each_bound(radius, cap) : 0.0f;   // (the kernels never form the bound of a query without candidates)
    return KNN_OK;
}

int knn_debug_self_plan(const long long in[6], long long out[8])
{
    if (!in || !out || in[0] < 1 || in[0] > INT_MAX || in[1] < 1 || in[1] > INT_MAX || in[2] < -1 || in[2] > KNN_TOPK_MAX ||
        (in[2] > 0 && in[1] * in[2] > INT_MAX) || in[3] < in[1] || in[3] > (1ll << 32) || in[4] < 1 || in[4] > INT_MAX ||
        (in[5] != 0 && in[5] != 1))
        return fail(KNN_EINVAL, "knn_debug_self_plan: bad arguments (k >= 1, rows >= 1, -1 <= K <= 64, rows * K <= INT_MAX, "
                                "rows <= the shard's rows <= 2^32, CUs >= 1, init 0 or 1)");
    const SelfPlan p = knn_self_plan((int)in[0], (int)in[1], (int)in[2], in[3], (int)in[4], in[5] != 0);
    const long long v[8] = {p.chunks, p.slices, p.groups, (long long)p.lds_bytes, (long long)p.part_bytes, p.launches, p.chunk_m,
                            (long long)p.through_bytes};
    memcpy(out, v, sizeof v);
    return KNN_OK;
}

int knn_debug_self_ranges(long long i0, long long i1, long long w0, long long w1, long long out[6])
{
    if (!out)
        return fail(KNN_EINVAL, "knn_debug_self_ranges: null out");
    knn_self_ranges(i0, i1, w0, w1, out);
    return KNN_OK;
}

int knn_debug_slice_chunks(const long long in[5], int cap, long long (*out)[6], int *chunks)
{
    if (!in || !out || !chunks || cap < 1 || in[0] < 1 || in[0] > INT_MAX || in[1] < 1 || in[1] > (1ll << 32) || in[2] < 1 ||
        in[2] > INT_MAX || in[4] < 0 || in[4] > 2 || (in[4] == 1 && (in[3] < 1 || in[3] > KNN_TOPK_MAX)) ||
        knn_divup(in[0], KNN_TOPK_CHUNK) > cap)
        return fail(KNN_EINVAL, "knn_debug_slice_chunks: bad arguments (1 <= queries <= INT_MAX, 1 <= rows <= 2^32, CUs >= 1, rule 0, "
                                "1 with 1 <= K <= 64, or 2, cap >= the chunks)");
    int count = 0;
    const auto put = [&](const SliceChunk &ch) {
        const long long v[6] = {ch.c0, ch.mc, ch.slices, ch.per, ch.grid.x, ch.grid.y};
        memcpy(out[count++], v, sizeof v);
        return hipSuccess;
    };
    if (in[4] == 1)
        (void)knn_slice_chunks(in[0], in[1], (int)in[2], KnnTopkSlices{(int)in[3]}, put);
    else if (in[4] == 2)
        (void)knn_slice_chunks(in[0], in[1], (int)in[2], KnnSelectSlices{}, put);
    else
        (void)knn_slice_chunks(in[0], in[1], (int)in[2], KnnCountSlices{}, put);
    *chunks = count;
    return KNN_OK;
}

int knn_debug_filter_scores(knn_index *idx, int m, const float *queries_dev, float *scores_dev,
                            float *qnorm_dev, double consts[8])
{
    if (!idx || m < 1 || !queries_dev || !scores_dev || !qnorm_dev || !consts)
        return fail(KNN_EINVAL, "knn_debug_filter_scores: bad arguments");
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    if (!idx->filter.usable)
        return fail(KNN_EINVAL, "knn_debug_filter_scores: this index has no filter layouts");
    DeviceGuard guard(idx->device);
    HIP_TRY(knn_filter_debug(idx->filter, m, queries_dev, idx->refs, scores_dev, nullptr, qnorm_dev, consts,
                             nullptr));
    return KNN_OK;
}

int knn_index_timing(knn_index *idx, int enable)
{
    if (!idx)
        return fail(KNN_EINVAL, "knn_index_timing: null index");
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    idx->timing = enable > 0 ? enable : 0;
    idx->timing_seq = 0;
    idx->events_used = 0;
    if (enable > 0) {
        // The event pairs are made HERE, not at the launches they bracket: the first bracketed launch of a run used to create
        // its pair on the spot — 0.2-0.3 ms of hipEventCreate inside the caller's timed region (a 20-step bench run read 0.141 ms
        // per step where the same 20 batches take 0.126 without the instrumentation; tools/fill_drain.py).
        DeviceGuard guard(idx->device);
        while (idx->events.size() < 64) {
            std::pair<hipEvent_t, hipEvent_t> fresh;
            HIP_TRY(hipEventCreate(&fresh.first));
            if (hipEventCreate(&fresh.second) != hipSuccess) {
                (void)hipEventDestroy(fresh.first);
                return fail(KNN_EHIP, "knn_index_timing: hipEventCreate failed");
            }
            idx->events.push_back(fresh);
        }
    }
    return KNN_OK;
}

int knn_index_timing_read(knn_index *idx, int *launches, double *total_ms)
{
    if (!idx || !launches || !total_ms)
        return fail(KNN_EINVAL, "knn_index_timing_read: bad arguments");
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    DeviceGuard guard(idx->device);
    double sum = 0.0;
    for (size_t i = 0; i < idx->events_used; ++i) {
        float ms = 0.0f;
        HIP_TRY(hipEventSynchronize(idx->events[i].second));
        HIP_TRY(hipEventElapsedTime(&ms, idx->events[i].first, idx->events[i].second));
        sum += ms;
    }
    *launches = (int)idx->events_used;
    *total_ms = sum;
    idx->events_used = 0;
    return KNN_OK;
}

int knn_index_last_stats(knn_index *idx, long long stats[4])
{
    if (!idx || !stats)
        return fail(KNN_EINVAL, "knn_index_last_stats: bad arguments");
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    const FilterWorkspace &w = idx->filter.ws[idx->last_slot];
    if ((idx->stats[0] == 2 || idx->stats[0] == 4) && w.ctl) {
        DeviceGuard guard(idx->device);
        unsigned ctl[KNN_CTL_WORDS];
        HIP_TRY(hipMemcpy(ctl, w.ctl_cur ? w.ctl_cur : w.ctl, sizeof ctl, hipMemcpyDeviceToHost));
        std::vector<unsigned> counts(w.nlists);
        if (!counts.empty())
            HIP_TRY(hipMemcpy(counts.data(), w.counts, counts.size() * sizeof(unsigned),
                              hipMemcpyDeviceToHost));
        long long records = 0;
        for (unsigned c : counts)
            records += c < w.slice ? c : w.slice;
        if (idx->stats[0] == 4)   // + the shared overflow area
            records += ctl[KNN_CTL_RECORDS] < w.ovf_cap ? ctl[KNN_CTL_RECORDS] : w.ovf_cap;
        idx->stats[1] = records;
        idx->stats[2] = ctl[KNN_CTL_FALLBACK] ? 1 : ctl[KNN_CTL_EXACT_CELLS] ? 2 : 0;   // 2: the batch's listed (cell, query) pairs were evaluated exactly
        idx->stats[3] = idx->filter.n_outliers;
    }
    if (idx->stats[0] == 3 && idx->grid_topk_gate) {   // a top-K call on the grid: 1 = some query gave up, the exact top-K answered
        DeviceGuard guard(idx->device);
        unsigned word = 0u;
        HIP_TRY(hipMemcpy(&word, idx->grid_topk_gate, sizeof word, hipMemcpyDeviceToHost));
        idx->stats[2] = word ? 1 : 0;
    }
    if (idx->stats[0] == 1 && idx->grid_topk_gate) {   // a large top-K: 1 = some query's cut fell inside a class of equal distances
        DeviceGuard guard(idx->device);
        unsigned word = 0u;
        HIP_TRY(hipMemcpy(&word, idx->grid_topk_gate, sizeof word, hipMemcpyDeviceToHost));
        idx->stats[2] = word ? 1 : 0;
    }
    memcpy(stats, idx->stats, sizeof idx->stats);
    return KNN_OK;
}

int knn_index_debug_counters(knn_index *idx, long long out[4])
{
    if (!idx || !out)
        return fail(KNN_EINVAL, "knn_index_debug_counters: bad arguments");
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    out[0] = out[1] = out[2] = out[3] = 0;
    const FilterWorkspace &w = idx->filter.ws[idx->last_slot];
    if (idx->stats[0] == 4 && w.ctl_cur) {
        DeviceGuard guard(idx->device);
        unsigned ctl[KNN_CTL_WORDS];
        HIP_TRY(hipMemcpy(ctl, w.ctl_cur, sizeof ctl, hipMemcpyDeviceToHost));
        out[0] = ctl[KNN_CTL_WIDE_SEEDS];
        out[1] = ctl[KNN_CTL_DENSE_CELLS];
        out[2] = idx->filter.cells ? idx->filter.cells->ncells : 0;
        out[3] = idx->filter.cells ? idx->filter.cells->max_cell_rows : 0;
    }
    return KNN_OK;
}

// Test hook: what the match launch of the most recent cell-pruned batch on `slot` read and wrote, copied to the host once the
// device is idle.  what 0: nothing (dims only); 1 cell_counts, unsigned [ncells]; 2 the lists, unsigned short [ncells][cap] (the first
// min(count, cap) entries of a row are its list); 3 the low table, 4 the high table, 5 the group minima, 6 Dup — floats, laid out
// for the m_padded of that batch.  dims = {ncells, cap, 2^sa, entries of the high table, m_cap, cell_base}.  At most `bytes` bytes.
int knn_debug_cells_fetch(knn_index *idx, int slot, int what, void *out, long long bytes, long long dims[6])
{
    if (!idx || slot < 0 || slot >= KNN_SLOTS || what < 0 || what > 6 || !dims || bytes < 0 || (what && !out))
        return fail(KNN_EINVAL, "knn_debug_cells_fetch: bad arguments");
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    const CellIndex *c = idx->filter.cells;
    const FilterWorkspace &w = idx->filter.ws[slot];
    if (!c || !w.cell_counts || !w.cell_lists || !w.lo_min)
        return fail(KNN_EINVAL, "knn_debug_cells_fetch: no cell-pruned batch has run on this slot");
    const size_t nl = (size_t)1 << c->sa, nh = (c->ncells + nl - 1) >> c->sa, mc = (size_t)w.cell_m_cap;
    const long long d[6] = {c->ncells, c->cap, (long long)nl, (long long)nh, (long long)mc, c->cell_base};
    memcpy(dims, d, sizeof d);
    const void *src[7] = {nullptr, w.cell_counts, w.cell_lists, w.lo_tab, w.hi_tab, w.lo_min, w.dup};
    const size_t size[7] = {0, (size_t)c->ncells * sizeof(unsigned), (size_t)c->ncells * c->cap * sizeof(unsigned short), mc * nl * sizeof(float),
                            mc * nh * sizeof(float), mc * (nl / 64) * sizeof(float), mc * sizeof(float)};
    if (what) {
        DeviceGuard guard(idx->device);
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out, src[what], std::min(size[what], (size_t)bytes), hipMemcpyDeviceToHost));
    }
    return KNN_OK;
}

// Test hook (host arithmetic, no GPU): the match kernel's two tests (knn_cell_queued, knn_cell_listed: the kernel's own lines) on
// `n` (block, query) cases — hi[i], dup[i] and 64 low entries lo[64 i ..].  queued[i] = the block's queue takes the query on the
// smallest of its 64 low entries; listed[i] = how many of the 64 cells keep it on their list.
int knn_debug_match_tests(long long n, const float *lo, const float *hi, const float *dup, unsigned char *queued, unsigned char *listed)
{
    if (n < 0 || !lo || !hi || !dup || !queued || !listed)
        return fail(KNN_EINVAL, "knn_debug_match_tests: bad arguments");
    for (long long i = 0; i < n; ++i) {
        float lo_min = lo[64 * i];
        unsigned cnt = 0;
        for (int l = 0; l < 64; ++l) {
            lo_min = fminf(lo_min, lo[64 * i + l]);
            cnt += knn_cell_listed(lo[64 * i + l], hi[i], dup[i]) ? 1u : 0u;
        }
        queued[i] = knn_cell_queued(lo_min, hi[i], dup[i]) ? 1 : 0;
        listed[i] = (unsigned char)cnt;
    }
    return KNN_OK;
}

int knn_debug_scan_plan(int num_cu, int blocks_per_cu, unsigned nitems, int m, long long out[8])
{
    return knn_debug_scan_plan_ex(num_cu, blocks_per_cu, nitems, m, 0, out);
}

int knn_debug_scan_plan_ex(int num_cu, int blocks_per_cu, unsigned nitems, int m, int self_lists, long long out[8])
{
    if (!out || num_cu < 1 || blocks_per_cu < 1 || blocks_per_cu > 2 || m < 1 || m > KNN_CELL_BATCH)
        return fail(KNN_EINVAL, "knn_debug_scan_plan: bad arguments");
    const int m_padded = (m + 31) / 32 * 32;
    const CellScanPlan p = knn_cells_scan_plan(num_cu, blocks_per_cu, nitems, KNN_RECORD_CAPACITY, m_padded, self_lists != 0);
    out[0] = p.blocks;
    out[1] = p.nlists;
    out[2] = p.slice;
    out[3] = p.ovf_base;
    out[4] = p.ovf_cap;
    out[5] = (long long)p.lds_bytes;
    out[6] = KNN_RECORD_CAPACITY;
    out[7] = KNN_MAX_LISTS;
    return KNN_OK;
}

int knn_debug_cells_query_plan(const long long in[14], long long out[28])
{
    if (!in || !out || in[0] < 1 || in[0] > 32 || in[1] < 1 || in[1] > 2 || in[4] < 1 || in[11] < 1 || in[11] > KNN_CELL_BATCH ||
        in[12] < 1)
        return fail(KNN_EINVAL, "knn_debug_cells_query_plan: bad arguments");
    CellQueryInputs ci;
    ci.k = (int)in[0];
    ci.kt = (int)in[1];
    ci.centred = in[2] != 0;
    ci.rows_u8 = in[3] != 0;
    ci.ncells = (unsigned)in[4];
    ci.nitems = (unsigned)in[5];
    ci.cap = (unsigned)in[6];
    ci.several_slots = in[7] != 0;
    ci.scan_blocks = (int)in[8];
    ci.scan_deal = (int)in[9];
    ci.cells_lists = (int)in[10];
    ci.m = (int)in[11];
    ci.num_cu = (int)in[12];
    ci.rec_cap = (unsigned)in[13];
    const CellQueryPlan p = knn_cells_query_plan(ci);
    const CellScanForm &f = p.scan;
    const long long v[28] = {p.prep_pw, p.prep_kt, p.prep_ctr, p.self_lists, p.match_waves, p.stage, (long long)p.match_lds,
                             f.dyn, f.k, f.self, f.kt, f.ctr, f.nif, f.u8,
                             p.grid.blocks, p.grid.waves, p.grid.nlists, p.grid.slice, p.grid.ovf_base, p.grid.ovf_cap,
                             (long long)p.grid.lds_bytes, p.list_cap, p.tail_k, p.tail_kt, p.tail_blocks, p.exact_launch,
                             (long long)p.scan_lds_limit, (long long)p.match_lds_limit};
    memcpy(out, v, sizeof v);
    return KNN_OK;
}

}  // extern "C"

namespace {
// in[0 .. 20) of knn_debug_cells_topk_plan and of knn_debug_query_route
CellTopkInputs topk_inputs_of(const long long in[20])
{
    CellTopkInputs ti;
    ti.q.k = (int)in[0];
    ti.q.kt = knn_kt_of(ti.q.k);
    ti.K = (int)in[1];
    ti.q.m = (int)in[2];
    ti.n = in[3];
    ti.topk_cells = (int)in[4];
    ti.has_cells = in[5] != 0;
    ti.q.rows_u8 = in[7] != 0;
    ti.bins = in[8] != 0;
    // centred: 1 = per-cell frames; 2 = per-cell frames and the call carries KNN_QUERY_TOPK_FRAMES (as `sharded` = 2 is a shard whose
    // call carries its flag).  Bin frames are the shard's one frame: 2 there is the flag alone, which changes nothing.
    ti.frames_flag = in[6] == 2;
    ti.q.centred = in[6] != 0 && !(in[6] == 2 && ti.q.rows_u8 && ti.bins);
    ti.sharded = in[9] != 0;
    ti.shard_partial = in[9] == 2;
    ti.n_outliers = (unsigned)in[10];
    ti.q.ncells = (unsigned)in[11];
    ti.q.nitems = (unsigned)in[12];
    ti.q.cap = (unsigned)in[13];
    ti.q.several_slots = in[14] != 0;
    ti.q.scan_blocks = (int)in[15];
    ti.q.scan_deal = (int)in[16];
    ti.q.num_cu = (int)in[17];
    ti.q.rec_cap = (unsigned)in[18];
    ti.cells_option = (int)in[19];
    ti.q.cells_lists = 1;
    return ti;
}
}  // namespace

extern "C" {

int knn_debug_cells_topk_plan(const long long in[20], long long out[25])
{
    if (!in || !out || in[0] < 1 || in[0] > 4096 || in[2] < 1 || in[2] > INT_MAX || in[17] < 1 || in[3] < 0)
        return fail(KNN_EINVAL, "knn_debug_cells_topk_plan: bad arguments");
    CellTopkInputs ti = topk_inputs_of(in);
    ti.ccap = knn_topk_ccap(ti.K, ti.q.m);
    const CellTopkPlan t = knn_cells_topk_plan(ti);
    const CellQueryPlan &p = t.batch;
    const long long v[25] = {t.use, p.prep_pw, p.prep_kt, p.prep_ctr, p.match_waves, p.stage,
                             t.scan.dyn, t.scan.kt, t.scan.nif, t.scan.u8, t.scan.self, t.scan.ctr,
                             p.grid.blocks, p.grid.waves, p.grid.nlists, p.grid.slice, p.grid.ovf_base, p.grid.ovf_cap,
                             (long long)p.grid.lds_bytes, p.list_cap, t.ccap, t.passes, (long long)p.scan_lds_limit,
                             (long long)p.match_lds_limit, t.pass_m};
    memcpy(out, v, sizeof v);
    return KNN_OK;
}

int knn_debug_filter_query_plan(const long long in[11], long long out[49])
{
    if (!in || !out || in[0] < 1 || in[0] > KNN_FILTER_MAX_K / 16 || in[1] < 1 || in[2] < 1 || in[2] > INT_MAX || in[3] < 1 ||
        in[3] > 4096 || in[4] < 1 || in[4] > UINT_MAX || in[5] < 0 || in[5] > KNN_TOPK_MAX ||
        (in[6] != 0 && in[6] != 2 && in[6] != 8 && in[6] != 16 && in[6] != 32) || in[7] < 0 || in[7] > 64 || in[8] < 0 ||
        in[8] > 2 || in[9] < 0 || in[9] > 2 || in[10] < 0 || in[10] > 1024)
        return fail(KNN_EINVAL, "knn_debug_filter_query_plan: bad arguments");
    FilterQueryInputs fi;
    fi.kt = (int)in[0];
    fi.ntiles = in[1];
    fi.m = (int)in[2];
    fi.num_cu = (int)in[3];
    fi.rec_cap = (unsigned)in[4];
    fi.opt.topk = (int)in[5];
    fi.opt.force_qt = (int)in[6];
    fi.opt.force_rounds = (int)in[7];
    fi.opt.chain_policy = (int)in[8];
    fi.opt.run_thresholds = (int)in[9];
    fi.opt.sample_stride = (int)in[10];
    const FilterQueryPlan p = knn_filter_query_plan(fi);
    long long v[49] = {p.ok, (long long)p.form, p.kt, p.npieces, p.nlists, p.slice, p.stride, p.sample_blocks, (long long)p.umin_floats,
                       p.topk, p.thr_nb, p.thr_running, p.scan_running, p.in_chain, p.chained, p.has_rows};
    for (int i = 0; i < 4; ++i) {
        const FilterPiece &pc = p.pieces[i];
        const long long f[6] = {pc.qt, pc.begin, pc.count, pc.gx, pc.gy, pc.list_base};
        memcpy(v + 16 + 6 * i, f, sizeof f);
        v[41 + i] = p.rerank.list_base[i];
        v[45 + i] = p.rerank.qrow_base[i];
    }
    v[40] = p.rerank.n;
    memcpy(out, v, sizeof v);
    return KNN_OK;
}

int knn_debug_query_route(const long long in[25], long long out[6])
{
    if (!in || !out || in[0] < 1 || in[0] > 4096 || in[1] < 0 || in[1] > KNN_TOPK_MAX || in[2] < 1 || in[2] > INT_MAX || in[3] < 1 ||
        in[4] < 0 || in[4] > 2 || in[9] < 0 || in[9] > 2 || in[17] < 1 || in[19] < 0 || in[19] > 2 || in[20] < 0 || in[20] > 3 ||
        (in[22] != 0 && in[9] != 0))   // (a cell-range shard has no grid index)
        return fail(KNN_EINVAL, "knn_debug_query_route: bad arguments");
    QueryRouteInputs ri;
    ri.t = topk_inputs_of(in);
    ri.path = (int)in[20];
    ri.filter_usable = in[21] != 0;
    ri.has_grid = in[22] != 0;
    ri.filter_wanted = in[23] != 0;
    ri.init_keys = in[24] != 0;
    const QueryRoute r = knn_query_route(ri);
    const long long v[6] = {(long long)r.way, r.fill_keys_first, r.ccap, r.topk.use, r.topk.passes, r.topk.pass_m};
    memcpy(out, v, sizeof v);
    return KNN_OK;
}

int knn_debug_grid_topk_plan(const long long in[6], long long out[6])
{
    if (!in || !out || in[0] < 1 || in[0] > 4 || in[1] < 1 || in[1] > KNN_TOPK_MAX || in[2] < 1 || in[2] > INT_MAX ||
        in[2] * in[1] > INT_MAX || in[3] < 0 || in[3] > 1 || in[4] < 0 || in[4] > 3 || in[5] < 0 || in[5] > 1)
        return fail(KNN_EINVAL, "knn_debug_grid_topk_plan: bad arguments (1 <= k <= 4, 1 <= K <= 64, m >= 1, path 0 .. 3)");
    const GridTopkPlan p = knn_grid_topk_plan((int)in[0], (int)in[1], (int)in[2], in[3] != 0, (int)in[4], in[5] != 0);
    const long long v[6] = {p.use, p.rmax, p.blocks, p.waves, (long long)p.scratch_bytes, p.launches};
    memcpy(out, v, sizeof v);
    return KNN_OK;
}

int knn_debug_grid_within_plan(const long long in[7], long long out[6])
{
    if (!in || !out || in[0] < 1 || in[0] > 4 || in[1] < 1 || in[1] > KNN_TOPK_MAX || in[2] < 1 || in[2] > INT_MAX ||
        in[2] * in[1] > INT_MAX || in[3] < 0 || in[3] > 1 || in[4] < 0 || in[4] > 3 || in[5] < 0 || in[5] > 1 || in[6] < 0)
        return fail(KNN_EINVAL, "knn_debug_grid_within_plan: bad arguments (1 <= k <= 4, 1 <= K <= 64, m >= 1, path 0 .. 3, rings >= 0)");
    const GridTopkPlan p = knn_grid_topk_plan((int)in[0], (int)in[1], (int)in[2], in[3] != 0, (int)in[4], in[5] != 0, in[6]);
    const long long v[6] = {p.use, p.rmax, p.blocks, p.waves, (long long)p.scratch_bytes, p.launches};
    memcpy(out, v, sizeof v);
    return KNN_OK;
}

int knn_debug_topk_scratch(const long long in[9], long long out[3])
{
    if (!in || !out || in[0] < 1 || in[0] > 4 || in[1] < 1 || in[1] > INT_MAX || in[2] < 1 || in[2] > KNN_TOPK_MAX ||
        in[1] * in[2] > INT_MAX || in[3] < 0 || in[4] < 1 || in[4] > INT_MAX || in[7] < 0 || in[7] > KNN_CELL_BATCH || in[8] < 0)
        return fail(KNN_EINVAL, "knn_debug_topk_scratch: bad arguments (way 1 .. 4, m >= 1, 1 <= K <= 64, n >= 0, num_cu >= 1, "
                                "0 <= pass_m <= 1024, grid_scratch_bytes >= 0)");
    const TopkScratchPlan p = knn_topk_scratch_plan({(QueryWay)in[0], (int)in[1], (int)in[2], in[3], (int)in[4], in[5] != 0, in[6] != 0,
                                                     (int)in[7], (size_t)in[8]});
    const long long v[3] = {(long long)p.part_bytes, (long long)p.cand_bytes, (long long)p.lists_bytes};
    memcpy(out, v, sizeof v);
    return KNN_OK;
}

int knn_debug_index_build_plan(const long long in[9], long long out[6])
{
    if (!in || !out || in[0] < 1 || in[0] > INT_MAX || in[1] < 0 || in[3] < -1 || in[3] > 2 || in[4] < -1 || in[4] > 1 || in[5] < 0 ||
        in[5] > 3 || in[6] < 0 || in[6] > 2 || in[7] < 0 || in[7] > 1 || in[8] < 0 || in[8] > 2)
        return fail(KNN_EINVAL, "knn_debug_index_build_plan: bad arguments");
    const IndexBuildPlan p = knn_index_build_plan({(int)in[0], in[1], in[2] != 0, (int)in[3], (int)in[4], (int)in[5], (int)in[6],
                                                   (int)in[7], (int)in[8]});
    const long long v[6] = {p.filter_wanted, p.want_cells, p.build_filter, p.grid_planned, p.want_layouts, (long long)p.ingest};
    memcpy(out, v, sizeof v);
    return KNN_OK;
}

int knn_debug_ingest_head_rows(const long long in[3], long long out[1])
{
    if (!in || !out || in[0] < 1 || in[0] > INT_MAX || in[1] < 0 || in[1] > (1ll << 40) || in[2] < 32 || in[2] > (1ll << 20) ||
        in[2] % 32 != 0)
        return fail(KNN_EINVAL, "knn_debug_ingest_head_rows: bad arguments");
    out[0] = knn_ingest_head_rows((int)in[0], in[1], in[2]);
    return KNN_OK;
}

int knn_keys_to_indices(int device, const unsigned long long *keys_dev, int m, int *out_dev,
                        void *stream)
{
    if (m < 0 || (m > 0 && (!keys_dev || !out_dev)))
        return fail(KNN_EINVAL, "knn_keys_to_indices: bad arguments");
    DeviceGuard guard(device);
    if (!guard.ok)
        return fail(KNN_EHIP, "knn_keys_to_indices: hipSetDevice failed");
    HIP_TRY(knn_keys_unpack_launch((const u64 *)keys_dev, m, out_dev, (hipStream_t)stream));
    return KNN_OK;
}

int knn_keys_allreduce_min(int ndev, const int *devices, unsigned long long *const *keys_dev, int m,
                           void *const *streams)
{
    if (ndev < 1 || !devices || !keys_dev || m < 0)
        return fail(KNN_EINVAL, "knn_keys_allreduce_min: bad arguments");
    const int have = knn_device_count();
    for (int g = 0; g < ndev; ++g) {
        if (devices[g] < 0 || devices[g] >= have || (m > 0 && !keys_dev[g]))
            return fail(KNN_EINVAL, "knn_keys_allreduce_min: bad device or null key array");
        for (int h = 0; h < g; ++h)
            if (devices[h] == devices[g])
                return fail(KNN_EINVAL, "knn_keys_allreduce_min: a device appears twice (one key array per GPU)");
    }
    if (have < 1)
        return fail(KNN_ENODEV, "knn_keys_allreduce_min: no HIP device visible");
    std::string err;
    static_assert(sizeof(unsigned long long) == sizeof(u64), "key type");
    if (knn_rccl_allreduce_min(ndev, devices, (u64 *const *)keys_dev, m, (const hipStream_t *)streams, err) != 0)
        return fail(KNN_EHIP, "knn_keys_allreduce_min", err.c_str());
    return KNN_OK;
}

int knn_synth_fill_device(int device, float *dst_dev, long long count, unsigned long long seed,
                          long long first, void *stream)
{
    if (count < 0 || (count > 0 && !dst_dev))
        return fail(KNN_EINVAL, "knn_synth_fill_device: bad arguments");
    DeviceGuard guard(device);
    if (!guard.ok)
        return fail(KNN_EHIP, "knn_synth_fill_device: hipSetDevice failed");
    HIP_TRY(knn_synth_fill_launch(dst_dev, count, seed, first, (hipStream_t)stream));
    return KNN_OK;
}

}  // extern "C"

namespace {

// One query with the queries on the host — K = 0: the nearest neighbour, one key per query; K >= 1: the top-K, K keys
// per query.  The queries are staged into a pooled buffer, the query runs on the null stream and the packed keys come
// back to keys_host; everything else stays on `idx->device`.  keep != nullptr: the keys stay on the device instead, in a
// buffer that keep->owner holds (keep->dev, complete on return) — the RCCL merge of cudaCallback reads them there.
// max_dist2 finite (K >= 1): knn_index_query_topk_within.
int staged_query(knn_index *idx, const char *who, int m, int K, const float *queries_host, u64 *keys_host, ShardKeys *keep = nullptr,
                 float max_dist2 = INFINITY)
{
    const std::string name(who);
    DeviceGuard guard(idx->device);
    if (!guard.ok)
        return fail(KNN_EHIP, (name + ": hipSetDevice failed").c_str());
    Staging stage(idx->device);
    float *q_dev = nullptr;
    u64 *keys_dev = nullptr;
    const size_t qbytes = (size_t)m * (size_t)idx->k * sizeof(float), kbytes = (size_t)m * (size_t)std::max(K, 1) * sizeof(u64);
    hipError_t e = stage.get(&q_dev, qbytes);
    if (e == hipSuccess)
        e = (keep ? keep->owner : stage).get(&keys_dev, kbytes);
    if (e == hipSuccess)
        e = hipMemcpy(q_dev, queries_host, qbytes, hipMemcpyHostToDevice);
    if (e != hipSuccess)
        return fail(KNN_EHIP, (name + ": staging queries").c_str(), hipGetErrorString(e));
    int rc = K > 0 && max_dist2 < INFINITY
                 ? knn_index_query_topk_within(idx, 0, m, K, q_dev, max_dist2, keys_dev, nullptr, nullptr, KNN_QUERY_INIT_KEYS)
             : K > 0 ? knn_index_query_topk(idx, 0, m, K, q_dev, keys_dev, nullptr, nullptr, KNN_QUERY_INIT_KEYS)
                     : knn_keys_init(idx->device, keys_dev, m, nullptr);
    if (rc == KNN_OK && K == 0)
        rc = knn_index_query_keys(idx, m, q_dev, keys_dev, nullptr);
    if (rc != KNN_OK)
        return rc;
    e = keep ? hipStreamSynchronize(nullptr) : hipMemcpy(keys_host, keys_dev, kbytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess)
        return fail(KNN_EHIP, (name + ": D2H keys").c_str(), hipGetErrorString(e));
    if (keep)
        keep->dev = keys_dev;
    if (K == 0)
        stage.waited();   // by the blocking copy / the synchronised null stream
    // K >= 1: not declared, so that the top-K's buffers go back after the device-wide wait `stage` then makes itself
    return KNN_OK;
}

// A packed key's halves: the row number (low word) and, dist2 non-null, the distance whose bits the high word holds.
inline void unpack_key(u64 key, int *index, float *dist2)
{
    *index = (int)(unsigned)(key & 0xFFFFFFFFull);
    if (dist2) {
        const unsigned hi = (unsigned)(key >> 32);
        memcpy(dist2, &hi, sizeof hi);
    }
}

// The host arrays of a top-K host call from its m lists of K keys: indices and (nullable) dist2 [m][K], and (nullable) counts [m],
// the real keys of a list — padding is KNN_KEY_INIT; a real key is below it.
void unpack_topk(const u64 *keys, int m, int K, int *indices, float *dist2, int *counts)
{
    for (size_t i = 0; i < (size_t)m * (size_t)K; ++i)
        unpack_key(keys[i], &indices[i], dist2 ? &dist2[i] : nullptr);
    if (counts)
        for (int j = 0; j < m; ++j) {
            int c = 0;
            while (c < K && keys[(size_t)j * K + c] < kKeyInit)
                ++c;
            counts[j] = c;
        }
}

// The tail of a list host call: the sorted keys of all segments -> malloc'd indices and (dist2_out non-null) dist2, one element of
// room for an empty result, and the offsets [offs.size()] to the caller's array.  Nothing stays allocated on failure.
int lists_to_host(const char *who, const std::vector<u64> &offs, const std::vector<u64> &keys, long long *offsets_host,
                  int **indices_out, float **dist2_out)
{
    const size_t total = keys.size(), room = total ? total : 1u;
    int *ind = (int *)malloc(room * sizeof(int));
    float *d2 = dist2_out ? (float *)malloc(room * sizeof(float)) : nullptr;
    if (!ind || (dist2_out && !d2)) {
        free(ind);
        free(d2);
        return fail_in(KNN_EHIP, who, "out of host memory");
    }
    for (size_t i = 0; i < total; ++i)
        unpack_key(keys[i], &ind[i], d2 ? &d2[i] : nullptr);
    for (size_t j = 0; j < offs.size(); ++j)
        offsets_host[j] = (long long)offs[j];
    *indices_out = ind;
    if (dist2_out)
        *dist2_out = d2;
    return KNN_OK;
}

// The synchronous top-K calls over queries on the host (2f, 2g, 2h) behind topk_check: t.queries and t.mask are host arrays.  The
// queries, the keys and a masked form's mask — max((n_local + 31) / 32, 1) words, copied unless the shard is empty — are staged,
// device_call(queries, mask, keys) is the entry's device call on the null stream, slot 0, writing its keys, and the keys come
// back through unpack_topk.
template <class DeviceCall>
int topk_host_run(knn_index *idx, const TopkEntry &t, int *indices_host, float *dist2_host, int *counts_host, DeviceCall device_call)
{
    const bool masked = (t.form & kMasked) != 0u;
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    DeviceGuard guard(idx->device);
    if (!guard.ok)
        return fail_in(KNN_EHIP, t.who, "hipSetDevice failed");
    const size_t mk = (size_t)t.m * (size_t)t.K;
    std::vector<u64> keys(mk);
    {
        Staging stage(idx->device);
        float *q_dev = nullptr;
        u64 *keys_dev = nullptr;
        unsigned *mask_dev = nullptr;
        const size_t qbytes = (size_t)t.m * (size_t)idx->k * sizeof(float);
        const size_t mbytes = std::max<size_t>((size_t)((idx->n + 31) / 32), 1) * sizeof(unsigned);   // (an empty shard: one word, unread)
        hipError_t e = stage.get(&q_dev, qbytes);
        if (e == hipSuccess)
            e = stage.get(&keys_dev, mk * sizeof(u64));
        if (e == hipSuccess && masked)
            e = stage.get(&mask_dev, mbytes);
        if (e == hipSuccess)
            e = hipMemcpy(q_dev, t.queries, qbytes, hipMemcpyHostToDevice);
        if (e == hipSuccess && masked && idx->n > 0)
            e = hipMemcpy(mask_dev, t.mask, mbytes, hipMemcpyHostToDevice);
        if (e != hipSuccess)
            return fail_in(KNN_EHIP, t.who, masked ? "staging queries and mask" : "staging queries", hipGetErrorString(e));
        KNN_TRY(device_call(q_dev, mask_dev, keys_dev));
        e = hipMemcpy(keys.data(), keys_dev, mk * sizeof(u64), hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            return fail_in(KNN_EHIP, t.who, "D2H keys", hipGetErrorString(e));
        // (not declared waited: the buffers go back after the device-wide wait `stage` then makes itself, as the top-K's)
    }
    unpack_topk(keys.data(), t.m, t.K, indices_host, dist2_host, counts_host);
    return KNN_OK;
}

// The round every synchronous list call makes once its inputs are staged: counts() issues the counts of the `segments` queries or
// rows into c_dev, lists(keys_dev) their lists into off_dev / fill_dev / keys_dev, both on the null stream.  count -> offsets, the
// one synchronisation (the total sizes the keys, staged in `stage` when it is non-zero), list -> sort, and the sorted keys to the
// caller through lists_to_host.
template <class Counts, class Lists>
int lists_host_round(knn_index *idx, const char *who, Staging &stage, int segments, const unsigned *c_dev, const unsigned *fill_dev,
                     u64 *off_dev, long long *offsets_host, int **indices_out, float **dist2_out, Counts counts, Lists lists)
{
    int rc = counts();
    if (rc == KNN_OK)
        rc = knn_counts_to_offsets(idx->device, c_dev, segments, off_dev, nullptr);
    if (rc != KNN_OK)
        return rc;
    std::vector<u64> offs((size_t)segments + 1);
    hipError_t e = hipMemcpy(offs.data(), off_dev, offs.size() * sizeof(u64), hipMemcpyDeviceToHost);
    if (e != hipSuccess)
        return fail_in(KNN_EHIP, who, "D2H offsets", hipGetErrorString(e));
    const u64 total = offs[(size_t)segments];
    std::vector<u64> keys((size_t)total);
    if (total) {
        u64 *keys_dev = nullptr;
        e = stage.get(&keys_dev, (size_t)total * sizeof(u64));
        if (e != hipSuccess)
            return fail_in(KNN_EHIP, who, "staging keys", hipGetErrorString(e));
        rc = lists(keys_dev);
        if (rc == KNN_OK)
            rc = knn_keys_sort_segments(idx->device, segments, off_dev, fill_dev, keys_dev, nullptr);
        if (rc != KNN_OK)
            return rc;
        e = hipMemcpy(keys.data(), keys_dev, (size_t)total * sizeof(u64), hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            return fail_in(KNN_EHIP, who, "D2H keys", hipGetErrorString(e));
    }
    // (not declared waited: the slot's buffers go back after the device-wide wait `stage` then makes itself, as the other host calls)
    return lists_to_host(who, offs, keys, offsets_host, indices_out, dist2_out);
}

}  // namespace

extern "C" int knn_index_query_host(knn_index *idx, int m, const float *queries_host, int *out_host)
{
    if (!idx || m < 0 || (m > 0 && (!queries_host || !out_host)))
        return fail(KNN_EINVAL, "knn_index_query_host: bad arguments");
    if (m == 0)
        return KNN_OK;
    std::vector<u64> keys((size_t)m, kKeyInit);
    if (idx->n > 0) {
        int rc = staged_query(idx, "query", m, 0, queries_host, keys.data());
        if (rc != KNN_OK)
            return rc;
    }
    for (int j = 0; j < m; ++j)
        unpack_key(keys[(size_t)j], &out_host[j], nullptr);
    return KNN_OK;
}

extern "C" int knn_index_query_topk_host(knn_index *idx, int m, int K, const float *queries_host, int *indices_host,
                                         float *dist2_host)
{
    if (!idx || m < 1 || K < 1 || K > KNN_TOPK_MAX || (long long)m * K > INT_MAX || !queries_host || !indices_host)
        return fail(KNN_EINVAL, "knn_index_query_topk_host: bad arguments (1 <= K <= 64, m >= 1)");
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    const size_t mk = (size_t)m * (size_t)K;
    std::vector<u64> keys(mk);
    const int rc = staged_query(idx, "knn_index_query_topk_host", m, K, queries_host, keys.data());
    if (rc != KNN_OK)
        return rc;
    unpack_topk(keys.data(), m, K, indices_host, dist2_host, nullptr);
    return KNN_OK;
}

extern "C" int knn_index_query_topk_within_host(knn_index *idx, int m, int K, const float *queries_host, float max_dist2,
                                                int *indices_host, float *dist2_host, int *counts_host)
{
    if (!idx || m < 1 || K < 1 || K > KNN_TOPK_MAX || (long long)m * K > INT_MAX || !queries_host || !indices_host || !(max_dist2 >= 0.0f))
        return fail(KNN_EINVAL, "knn_index_query_topk_within_host: bad arguments (1 <= K <= 64, m >= 1, max_dist2 >= 0 and not NaN)");
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    const size_t mk = (size_t)m * (size_t)K;
    std::vector<u64> keys(mk);
    const int rc = staged_query(idx, "knn_index_query_topk_within_host", m, K, queries_host, keys.data(), nullptr, max_dist2);
    if (rc != KNN_OK)
        return rc;
    unpack_topk(keys.data(), m, K, indices_host, dist2_host, counts_host);
    return KNN_OK;
}

extern "C" int knn_index_query_topk_large_host(knn_index *idx, int m, int K, const float *queries_host, float max_dist2,
                                               int *indices_host, float *dist2_host, int *counts_host)
{
    const TopkEntry t = {"knn_index_query_topk_large_host", kLarge | kSizesFirst, 0, m, K, queries_host, 0, max_dist2};
    KNN_TRY(topk_check(t, {{!queries_host || !indices_host, "null queries or indices"}}, idx));
    return topk_host_run(idx, t, indices_host, dist2_host, counts_host, [&](const float *q_dev, const unsigned *, u64 *keys_dev) {
        return knn_index_query_topk_large(idx, 0, m, K, q_dev, max_dist2, keys_dev, nullptr, nullptr, KNN_QUERY_INIT_KEYS);
    });
}

extern "C" int knn_index_query_topk_masked_host(knn_index *idx, int m, int K, const float *queries_host, float max_dist2,
                                                const unsigned *mask_host, int *indices_host, float *dist2_host, int *counts_host)
{
    const TopkEntry t = {"knn_index_query_topk_masked_host", kMasked, 0, m, K, queries_host, 0, max_dist2, mask_host};
    KNN_TRY(topk_check(t, {{!queries_host || !mask_host || !indices_host, "null queries, mask or indices"}}, idx));
    return topk_host_run(idx, t, indices_host, dist2_host, counts_host, [&](const float *q_dev, const unsigned *mask_dev, u64 *keys_dev) {
        return knn_index_query_topk_masked(idx, 0, m, K, q_dev, max_dist2, mask_dev, keys_dev, nullptr, nullptr, KNN_QUERY_INIT_KEYS);
    });
}

// The synchronous count and list calls behind their argument checks: radii_host null — the scalar calls at max_dist2 —, or the
// radii of knn_index_count_within_each_host / knn_index_list_within_each_host, max_dist2 then being the cap.
static int count_within_host_run(knn_index *idx, const char *who, int m, const float *queries_host, const float *radii_host,
                                 float max_dist2, unsigned *counts_host)
{
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    DeviceGuard guard(idx->device);
    if (!guard.ok)
        return fail_in(KNN_EHIP, who, "hipSetDevice failed");
    Staging stage(idx->device);
    float *q_dev = nullptr, *r_dev = nullptr;
    unsigned *c_dev = nullptr;
    const size_t qbytes = (size_t)m * (size_t)idx->k * sizeof(float), cbytes = (size_t)m * sizeof(unsigned);
    const size_t rbytes = (size_t)m * sizeof(float);
    hipError_t e = stage.get(&q_dev, qbytes);
    if (e == hipSuccess)
        e = stage.get(&c_dev, cbytes);
    if (e == hipSuccess && radii_host)
        e = stage.get(&r_dev, rbytes);
    if (e == hipSuccess)
        e = hipMemcpy(q_dev, queries_host, qbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && radii_host)
        e = hipMemcpy(r_dev, radii_host, rbytes, hipMemcpyHostToDevice);
    if (e != hipSuccess)
        return fail_in(KNN_EHIP, who, "staging queries", hipGetErrorString(e));
    const int rc = radii_host ? knn_index_count_within_each(idx, 0, m, q_dev, r_dev, max_dist2, c_dev, nullptr, KNN_QUERY_INIT_KEYS)
                              : knn_index_count_within(idx, 0, m, q_dev, max_dist2, c_dev, nullptr, KNN_QUERY_INIT_KEYS);
    if (rc != KNN_OK)
        return rc;
    e = hipMemcpy(counts_host, c_dev, cbytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess)
        return fail_in(KNN_EHIP, who, "D2H counts", hipGetErrorString(e));
    // (not declared waited: the slot's buffers go back after the device-wide wait `stage` then makes itself, as the top-K host calls)
    return KNN_OK;
}

static int list_within_host_run(knn_index *idx, const char *who, int m, const float *queries_host, const float *radii_host,
                                float max_dist2, long long *offsets_host, int **indices_out, float **dist2_out)
{
    *indices_out = nullptr;
    if (dist2_out)
        *dist2_out = nullptr;
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    DeviceGuard guard(idx->device);
    if (!guard.ok)
        return fail_in(KNN_EHIP, who, "hipSetDevice failed");
    Staging stage(idx->device);
    float *q_dev = nullptr, *r_dev = nullptr;
    unsigned *c_dev = nullptr, *fill_dev = nullptr;
    u64 *off_dev = nullptr;
    const size_t qbytes = (size_t)m * (size_t)idx->k * sizeof(float), cbytes = (size_t)m * sizeof(unsigned);
    const size_t obytes = ((size_t)m + 1) * sizeof(u64), rbytes = (size_t)m * sizeof(float);
    hipError_t e = stage.get(&q_dev, qbytes);
    if (e == hipSuccess)
        e = stage.get(&c_dev, cbytes);
    if (e == hipSuccess)
        e = stage.get(&fill_dev, cbytes);
    if (e == hipSuccess)
        e = stage.get(&off_dev, obytes);
    if (e == hipSuccess && radii_host)
        e = stage.get(&r_dev, rbytes);
    if (e == hipSuccess)
        e = hipMemcpy(q_dev, queries_host, qbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && radii_host)
        e = hipMemcpy(r_dev, radii_host, rbytes, hipMemcpyHostToDevice);
    if (e != hipSuccess)
        return fail_in(KNN_EHIP, who, "staging queries", hipGetErrorString(e));
    return lists_host_round(
        idx, who, stage, m, c_dev, fill_dev, off_dev, offsets_host, indices_out, dist2_out,
        [&] {
            return radii_host ? knn_index_count_within_each(idx, 0, m, q_dev, r_dev, max_dist2, c_dev, nullptr, KNN_QUERY_INIT_KEYS)
                              : knn_index_count_within(idx, 0, m, q_dev, max_dist2, c_dev, nullptr, KNN_QUERY_INIT_KEYS);
        },
        [&](u64 *keys_dev) {
            return radii_host ? knn_index_list_within_each(idx, 0, m, q_dev, r_dev, max_dist2, off_dev, fill_dev, keys_dev, nullptr,
                                                           KNN_QUERY_INIT_KEYS)
                              : knn_index_list_within(idx, 0, m, q_dev, max_dist2, off_dev, fill_dev, keys_dev, nullptr, KNN_QUERY_INIT_KEYS);
        });
}

extern "C" int knn_index_count_within_host(knn_index *idx, int m, const float *queries_host, float max_dist2, unsigned *counts_host)
{
    if (!idx || m < 1 || !queries_host || !counts_host || !(max_dist2 >= 0.0f))
        return fail(KNN_EINVAL, "knn_index_count_within_host: bad arguments (m >= 1, max_dist2 >= 0 and not NaN)");
    return count_within_host_run(idx, "knn_index_count_within_host", m, queries_host, nullptr, max_dist2, counts_host);
}

extern "C" int knn_index_list_within_host(knn_index *idx, int m, const float *queries_host, float max_dist2, long long *offsets_host,
                                          int **indices_out, float **dist2_out)
{
    if (!idx || m < 1 || !queries_host || !offsets_host || !indices_out || !(max_dist2 >= 0.0f))
        return fail(KNN_EINVAL, "knn_index_list_within_host: bad arguments (m >= 1, max_dist2 >= 0 and not NaN)");
    return list_within_host_run(idx, "knn_index_list_within_host", m, queries_host, nullptr, max_dist2, offsets_host, indices_out, dist2_out);
}

// (2j) the same two with a radius per query, host arrays in and out, this shard alone on the default way
extern "C" int knn_index_count_within_each_host(knn_index *idx, int m, const float *queries_host, const float *max_dist2_host, float cap,
                                                unsigned *counts_host)
{
    if (!idx || m < 1 || !queries_host || !max_dist2_host || !counts_host || !(cap >= 0.0f))
        return fail(KNN_EINVAL, "knn_index_count_within_each_host: bad arguments (m >= 1, cap >= 0 and not NaN)");
    return count_within_host_run(idx, "knn_index_count_within_each_host", m, queries_host, max_dist2_host, cap, counts_host);
}

extern "C" int knn_index_list_within_each_host(knn_index *idx, int m, const float *queries_host, const float *max_dist2_host, float cap,
                                               long long *offsets_host, int **indices_out, float **dist2_out)
{
    if (!idx || m < 1 || !queries_host || !max_dist2_host || !offsets_host || !indices_out || !(cap >= 0.0f))
        return fail(KNN_EINVAL, "knn_index_list_within_each_host: bad arguments (m >= 1, cap >= 0 and not NaN)");
    return list_within_host_run(idx, "knn_index_list_within_each_host", m, queries_host, max_dist2_host, cap, offsets_host, indices_out,
                                dist2_out);
}

// ---- the whole shard about its own rows (include/knn_mi355x.h 2i): the kNN graph and the radius graph, synchronous ---------------
extern "C" int knn_index_self_topk_host(knn_index *idx, int K, float max_dist2, int *indices_host, float *dist2_host, int *counts_host)
{
    // (the rows are the whole shard's: the entry states none, and one row cannot break the m * K rule)
    const TopkEntry t = {"knn_index_self_topk_host", kSelf, 0, 1, K, nullptr, 0, max_dist2};
    KNN_TRY(topk_check(t, {{!indices_host, "null indices"}}, idx));
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    if (idx->n == 0)
        return KNN_OK;
    DeviceGuard guard(idx->device);
    if (!guard.ok)
        return fail(KNN_EHIP, "knn_index_self_topk_host: hipSetDevice failed");
    const long long step = KNN_TOPK_CHUNK;   // rows per call: step * K stays far below INT_MAX
    Staging stage(idx->device);
    u64 *keys_dev = nullptr;
    hipError_t e = stage.get(&keys_dev, (size_t)std::min(step, idx->n) * (size_t)K * sizeof(u64));
    if (e != hipSuccess)
        return fail(KNN_EHIP, "knn_index_self_topk_host: staging keys", hipGetErrorString(e));
    std::vector<u64> keys((size_t)std::min(step, idx->n) * (size_t)K);
    for (long long r0 = 0; r0 < idx->n; r0 += step) {
        const int rc = (int)std::min(step, idx->n - r0);
        const int rv = knn_index_self_topk(idx, 0, r0, rc, K, max_dist2, keys_dev, nullptr, nullptr, KNN_QUERY_INIT_KEYS);
        if (rv != KNN_OK)
            return rv;
        const size_t mk = (size_t)rc * (size_t)K, at = (size_t)r0 * (size_t)K;
        e = hipMemcpy(keys.data(), keys_dev, mk * sizeof(u64), hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            return fail(KNN_EHIP, "knn_index_self_topk_host: D2H keys", hipGetErrorString(e));
        unpack_topk(keys.data(), rc, K, indices_host + at, dist2_host ? dist2_host + at : nullptr, counts_host ? counts_host + r0 : nullptr);
    }
    // (not declared waited: the buffers go back after the device-wide wait `stage` then makes itself, as the other host calls)
    return KNN_OK;
}

// The radius graph of the whole shard on the host, behind the argument checks: knn_index_self_list_within_host (routed false: the
// existing self calls, max_dist2 the radius) and knn_index_self_list_within_routed_host (routed: the 2k calls under `flags`,
// radii_host [n_local] or null, max_dist2 the cap).  Blocks of 65536 rows: count -> offsets -> list -> sort.
static int self_list_host_run(knn_index *idx, const char *who, bool routed, const float *radii_host, float max_dist2, unsigned flags,
                              long long *offsets_host, int **indices_out, float **dist2_out)
{
    *indices_out = nullptr;
    if (dist2_out)
        *dist2_out = nullptr;
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    if (idx->n > INT_MAX)
        return fail_in(KNN_EINVAL, who, "more than INT_MAX rows (use the device calls, a block of rows at a time)");
    DeviceGuard guard(idx->device);
    if (!guard.ok)
        return fail_in(KNN_EHIP, who, "hipSetDevice failed");
    const int n = (int)idx->n;
    const int step = KNN_TOPK_CHUNK;   // rows per call
    const unsigned fl = KNN_QUERY_INIT_KEYS | flags;
    Staging stage(idx->device);
    if (n == 0)   // (an empty shard: the one offset 0, one element of room)
        return lists_to_host(who, std::vector<u64>(1, 0ull), std::vector<u64>(), offsets_host, indices_out, dist2_out);
    unsigned *c_dev = nullptr, *fill_dev = nullptr;
    u64 *off_dev = nullptr;
    float *rad_dev = nullptr;
    const size_t cbytes = (size_t)n * sizeof(unsigned), obytes = ((size_t)n + 1) * sizeof(u64);
    hipError_t e = stage.get(&c_dev, cbytes);
    if (e == hipSuccess)
        e = stage.get(&fill_dev, cbytes);
    if (e == hipSuccess)
        e = stage.get(&off_dev, obytes);
    if (e == hipSuccess && radii_host)
        e = stage.get(&rad_dev, (size_t)n * sizeof(float));
    if (e != hipSuccess)
        return fail_in(KNN_EHIP, who, "staging counts", hipGetErrorString(e));
    if (radii_host) {
        e = hipMemcpy(rad_dev, radii_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess)
            return fail_in(KNN_EHIP, who, "H2D radii", hipGetErrorString(e));
    }
    // (the offsets are absolute: every block of rows stores into the one keys array)
    return lists_host_round(
        idx, who, stage, n, c_dev, fill_dev, off_dev, offsets_host, indices_out, dist2_out,
        [&] {
            int rv = KNN_OK;
            for (int r0 = 0; r0 < n && rv == KNN_OK; r0 += step)
                rv = routed ? knn_index_self_count_within_routed(idx, 0, r0, std::min(step, n - r0), rad_dev ? rad_dev + r0 : nullptr, max_dist2,
                                                                 c_dev + r0, nullptr, fl)
                            : knn_index_self_count_within(idx, 0, r0, std::min(step, n - r0), max_dist2, c_dev + r0, nullptr, fl);
            return rv;
        },
        [&](u64 *keys_dev) {
            int rv = KNN_OK;
            for (int r0 = 0; r0 < n && rv == KNN_OK; r0 += step)
                rv = routed ? knn_index_self_list_within_routed(idx, 0, r0, std::min(step, n - r0), rad_dev ? rad_dev + r0 : nullptr,
                                                                max_dist2, off_dev + r0, fill_dev + r0, keys_dev, nullptr, fl)
                            : knn_index_self_list_within(idx, 0, r0, std::min(step, n - r0), max_dist2, off_dev + r0, fill_dev + r0,
                                                         keys_dev, nullptr, fl);
            return rv;
        });
}

extern "C" int knn_index_self_list_within_host(knn_index *idx, float max_dist2, long long *offsets_host, int **indices_out,
                                               float **dist2_out)
{
    if (!(max_dist2 >= 0.0f))
        return fail(KNN_EINVAL, "knn_index_self_list_within_host: max_dist2 must be >= 0 and not NaN");
    if (!offsets_host || !indices_out)
        return fail(KNN_EINVAL, "knn_index_self_list_within_host: null offsets or indices");
    if (!idx)
        return fail(KNN_EINVAL, "knn_index_self_list_within_host: null index");
    return self_list_host_run(idx, "knn_index_self_list_within_host", false, nullptr, max_dist2, 0u, offsets_host, indices_out, dist2_out);
}

extern "C" int knn_index_self_list_within_routed_host(knn_index *idx, const float *max_dist2_host, float cap, unsigned flags,
                                                      long long *offsets_host, int **indices_out, float **dist2_out)
{
    if (!(cap >= 0.0f))
        return fail(KNN_EINVAL, "knn_index_self_list_within_routed_host: cap must be >= 0 (or +INF) and not NaN");
    constexpr unsigned kFlags = KNN_QUERY_INIT_KEYS | KNN_QUERY_COUNT_GRID | KNN_QUERY_COUNT_CELLS;   // the three it admits
    if ((flags & ~kFlags) != 0u)
        return fail(KNN_EINVAL, "knn_index_self_list_within_routed_host: unknown flag (KNN_QUERY_INIT_KEYS, KNN_QUERY_COUNT_GRID, "
                                "KNN_QUERY_COUNT_CELLS)");
    if (!offsets_host || !indices_out)
        return fail(KNN_EINVAL, "knn_index_self_list_within_routed_host: null offsets or indices");
    if (!idx)
        return fail(KNN_EINVAL, "knn_index_self_list_within_routed_host: null index");
    return self_list_host_run(idx, "knn_index_self_list_within_routed_host", true, max_dist2_host, cap, flags, offsets_host, indices_out,
                              dist2_out);
}


// The clusters of the whole shard on the host: the device call on the default stream, then the renumbering — clusters 0 .. C - 1 in
// ascending order of their representative row (the smallest core row: the label the device call gives) — and the tallies.
// (behind the entry's radius and flag rules; device_call: the entry's device twin)
typedef int (*ClusterDeviceCall)(knn_index *, int, float, int, int *, unsigned *, void *, unsigned);
static int cluster_host_run(const char *who, ClusterDeviceCall device_call, knn_index *idx, float max_dist2, int min_pts, unsigned flags,
                            int *labels_host, unsigned char *core_host, long long info[4])
{
    if (min_pts < 1)
        return fail_in(KNN_EINVAL, who, "min_pts < 1");
    if (!labels_host)
        return fail_in(KNN_EINVAL, who, "null labels");
    if (!idx)
        return fail_in(KNN_EINVAL, who, "null index");
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    if (idx->n > INT_MAX)
        return fail_in(KNN_EINVAL, who, "more than INT_MAX rows (labels are int row numbers)");
    DeviceGuard guard(idx->device);
    if (!guard.ok)
        return fail_in(KNN_EHIP, who, "hipSetDevice failed");
    const size_t n = (size_t)idx->n, words = (n + 31) / 32;
    long long tally[4] = {0, 0, 0, 0};
    if (n > 0) {
        Staging stage(idx->device);
        int *labels_dev = nullptr;
        unsigned *core_dev = nullptr;
        hipError_t e = stage.get(&labels_dev, n * sizeof(int));
        if (e == hipSuccess)
            e = stage.get(&core_dev, words * sizeof(unsigned));
        if (e != hipSuccess)
            return fail_in(KNN_EHIP, who, "staging labels", hipGetErrorString(e));
        const int rv = device_call(idx, 0, max_dist2, min_pts, labels_dev, core_dev, nullptr, flags);
        if (rv != KNN_OK)
            return rv;
        std::vector<unsigned> core(words);
        e = hipMemcpy(labels_host, labels_dev, n * sizeof(int), hipMemcpyDeviceToHost);
        if (e == hipSuccess)
            e = hipMemcpy(core.data(), core_dev, words * sizeof(unsigned), hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            return fail_in(KNN_EHIP, who, "D2H labels", hipGetErrorString(e));
        // a representative is the row that carries its own number; they are met in ascending order
        std::vector<int> number(n, -1);
        int next = 0;
        for (size_t i = 0; i < n; ++i)
            if (labels_host[i] == (int)i)
                number[i] = next++;
        for (size_t i = 0; i < n; ++i) {
            const bool is_core = ((core[i >> 5] >> (i & 31)) & 1u) != 0u;
            if (core_host)
                core_host[i] = is_core ? 1 : 0;
            const int rep = labels_host[i];
            labels_host[i] = rep < 0 ? KNN_CLUSTER_NOISE : number[(size_t)rep];
            ++tally[is_core ? 1 : rep < 0 ? 3 : 2];
        }
        tally[0] = next;
        // (not declared waited: the buffers go back after the device-wide wait `stage` then makes itself, as the other host calls)
    }
    if (info)
        memcpy(info, tally, sizeof tally);
    return KNN_OK;
}

extern "C" int knn_index_self_cluster_within_host(knn_index *idx, float max_dist2, int min_pts, unsigned flags, int *labels_host,
                                                  unsigned char *core_host, long long info[4])
{
    const char *const who = "knn_index_self_cluster_within_host";
    KNN_TRY(cluster_check(who, max_dist2, flags));
    return cluster_host_run(who, knn_index_self_cluster_within, idx, max_dist2, min_pts, flags, labels_host, core_host, info);
}

extern "C" int knn_index_self_cluster_within_routed_host(knn_index *idx, float max_dist2, int min_pts, unsigned flags, int *labels_host,
                                                         unsigned char *core_host, long long info[4])
{
    const char *const who = "knn_index_self_cluster_within_routed_host";
    KNN_TRY(cluster_routed_check(who, max_dist2, flags));
    return cluster_host_run(who, knn_index_self_cluster_within_routed, idx, max_dist2, min_pts, flags, labels_host, core_host, info);
}

// The forest of the whole shard on the host: the device call on the default stream (every round queued), copied back, the edges
// SORTED ascending by (E's bits, i, j) — the order single linkage merges in.
extern "C" int knn_index_self_forest_within_host(knn_index *idx, float max_dist2, unsigned flags, int *labels_host, int *lo_host,
                                                 int *hi_host, float *dist2_host, long long info[4])
{
    const char *const who = "knn_index_self_forest_within_host";
    KNN_TRY(forest_check(who, max_dist2, flags));
    if (!lo_host || !hi_host)
        return fail_in(KNN_EINVAL, who, "null lo or hi");
    if (!idx)
        return fail_in(KNN_EINVAL, who, "null index");
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    if (idx->n > INT_MAX)
        return fail_in(KNN_EINVAL, who, "more than INT_MAX rows (labels and edge ends are int row numbers)");
    DeviceGuard guard(idx->device);
    if (!guard.ok)
        return fail_in(KNN_EHIP, who, "hipSetDevice failed");
    const size_t n = (size_t)idx->n;
    long long tally[4] = {0, 0, 0, 0};
    if (n > 0) {
        Staging stage(idx->device);
        int *labels_dev = nullptr;
        u64 *keys_dev = nullptr;
        unsigned *his_dev = nullptr, *count_dev = nullptr;
        hipError_t e = stage.get(&labels_dev, n * sizeof(int));
        if (e == hipSuccess)
            e = stage.get(&keys_dev, n * sizeof(u64));
        if (e == hipSuccess)
            e = stage.get(&his_dev, n * sizeof(unsigned));
        if (e == hipSuccess)
            e = stage.get(&count_dev, 2 * sizeof(unsigned));
        if (e != hipSuccess)
            return fail_in(KNN_EHIP, who, "staging the forest", hipGetErrorString(e));
        const int rv = knn_index_self_forest_within(idx, 0, max_dist2, labels_dev, keys_dev, his_dev, count_dev, nullptr, flags);
        if (rv != KNN_OK)
            return rv;
        unsigned count[2] = {0u, 0u};
        e = hipMemcpy(count, count_dev, sizeof count, hipMemcpyDeviceToHost);
        const size_t edges = std::min<size_t>(count[0], n);
        std::vector<u64> keys(edges);
        std::vector<unsigned> his(edges);
        if (e == hipSuccess && edges > 0)
            e = hipMemcpy(keys.data(), keys_dev, edges * sizeof(u64), hipMemcpyDeviceToHost);
        if (e == hipSuccess && edges > 0)
            e = hipMemcpy(his.data(), his_dev, edges * sizeof(unsigned), hipMemcpyDeviceToHost);
        if (e == hipSuccess && labels_host)
            e = hipMemcpy(labels_host, labels_dev, n * sizeof(int), hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            return fail_in(KNN_EHIP, who, "D2H forest", hipGetErrorString(e));
        std::vector<size_t> order(edges);
        for (size_t t = 0; t < edges; ++t)
            order[t] = t;
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return keys[a] != keys[b] ? keys[a] < keys[b] : his[a] < his[b]; });
        for (size_t t = 0; t < edges; ++t) {
            const u64 key = keys[order[t]];
            lo_host[t] = (int)(unsigned)key;
            hi_host[t] = (int)his[order[t]];
            if (dist2_host) {
                const unsigned bits = (unsigned)(key >> 32);
                memcpy(&dist2_host[t], &bits, sizeof bits);
            }
        }
        long long stats[4] = {0, 0, 0, 0};
        KNN_TRY(knn_index_last_stats(idx, stats));
        tally[0] = (long long)edges;
        tally[1] = (long long)(n - edges);
        tally[2] = std::min<long long>(knn_forest_rounds(idx->n), (long long)count[1] + 1);   // (the first round that adds nothing ends the run)
        tally[3] = stats[2];
        // (not declared waited: the buffers go back after the device-wide wait `stage` then makes itself, as the other host calls)
    }
    if (info)
        memcpy(info, tally, sizeof tally);
    return KNN_OK;
}

extern "C" int knn_index_list_within_masked_host(knn_index *idx, int m, const float *queries_host, float max_dist2,
                                                 const unsigned *mask_host, long long *offsets_host, int **indices_out, float **dist2_out)
{
    if (!idx || m < 1 || !queries_host || !mask_host || !offsets_host || !indices_out || !(max_dist2 >= 0.0f))
        return fail(KNN_EINVAL, "knn_index_list_within_masked_host: bad arguments (m >= 1, max_dist2 >= 0 and not NaN)");
    const char *const who = "knn_index_list_within_masked_host";
    *indices_out = nullptr;
    if (dist2_out)
        *dist2_out = nullptr;
    std::lock_guard<std::recursive_mutex> lock(idx->mu);
    DeviceGuard guard(idx->device);
    if (!guard.ok)
        return fail_in(KNN_EHIP, who, "hipSetDevice failed");
    Staging stage(idx->device);
    float *q_dev = nullptr;
    unsigned *c_dev = nullptr, *fill_dev = nullptr, *mask_dev = nullptr;
    u64 *off_dev = nullptr;
    const size_t qbytes = (size_t)m * (size_t)idx->k * sizeof(float), cbytes = (size_t)m * sizeof(unsigned);
    const size_t obytes = ((size_t)m + 1) * sizeof(u64);
    const size_t mbytes = std::max<size_t>((size_t)((idx->n + 31) / 32), 1) * sizeof(unsigned);   // (an empty shard: one word, unread)
    hipError_t e = stage.get(&q_dev, qbytes);
    if (e == hipSuccess)
        e = stage.get(&c_dev, cbytes);
    if (e == hipSuccess)
        e = stage.get(&fill_dev, cbytes);
    if (e == hipSuccess)
        e = stage.get(&off_dev, obytes);
    if (e == hipSuccess)
        e = stage.get(&mask_dev, mbytes);
    if (e == hipSuccess)
        e = hipMemcpy(q_dev, queries_host, qbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && idx->n > 0)
        e = hipMemcpy(mask_dev, mask_host, mbytes, hipMemcpyHostToDevice);
    if (e != hipSuccess)
        return fail_in(KNN_EHIP, who, "staging queries and mask", hipGetErrorString(e));
    return lists_host_round(
        idx, who, stage, m, c_dev, fill_dev, off_dev, offsets_host, indices_out, dist2_out,
        [&] { return knn_index_count_within_masked(idx, 0, m, q_dev, max_dist2, mask_dev, c_dev, nullptr, KNN_QUERY_INIT_KEYS); },
        [&](u64 *keys_dev) {
            return knn_index_list_within_masked(idx, 0, m, q_dev, max_dist2, mask_dev, off_dev, fill_dev, keys_dev, nullptr, KNN_QUERY_INIT_KEYS);
        });
}

extern "C" int knn_index_query_topk_large_masked_host(knn_index *idx, int m, int K, const float *queries_host, float max_dist2,
                                                      const unsigned *mask_host, int *indices_host, float *dist2_host, int *counts_host)
{
    const TopkEntry t = {"knn_index_query_topk_large_masked_host", kLarge | kMasked, 0, m, K, queries_host, 0, max_dist2, mask_host};
    KNN_TRY(topk_check(t, {{!queries_host || !mask_host || !indices_host, "null queries, mask or indices"}}, idx));
    return topk_host_run(idx, t, indices_host, dist2_host, counts_host, [&](const float *q_dev, const unsigned *mask_dev, u64 *keys_dev) {
        return knn_index_query_topk_large_masked(idx, 0, m, K, q_dev, max_dist2, mask_dev, keys_dev, nullptr, nullptr, KNN_QUERY_INIT_KEYS);
    });
}

namespace {

// One shard of a one-shot call, exact kernels only, with the scan hidden under the host-to-device
// copy: the rows go over in chunks on a copy stream and every chunk is scanned (min-folded into the
// same keys) on a compute stream as soon as it has landed.  The reference copies everything first
// (core.cu:885-891) and its own timings are dominated by that copy (README.md:291-292); for
// k = 16, m <= ~1300 the exact scan of a chunk takes less than its PCIe transfer, so the call
// costs the transfer plus one chunk's scan.
int run_shard_streamed(int device, int k, int m, long long rows, long long base, const float *queries_host,
                       const float *refs_host, u64 *keys_host, ShardKeys *keep = nullptr, int nchunks_hint = 8)
{
    DeviceGuard guard(device);
    if (!guard.ok)
        return fail(KNN_EHIP, "cudaCallback: hipSetDevice failed");
    hipDeviceProp_t prop;
    int num_cu = 256;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        num_cu = prop.multiProcessorCount;
    DeviceStreams st;
    HIP_TRY(streams_get(device, &st));
    const size_t row_bytes = (size_t)k * sizeof(float);
    const size_t rbytes = (size_t)rows * row_bytes, qbytes = (size_t)m * row_bytes, kbytes = (size_t)m * sizeof(u64);
    // Chunks of at least 32 MiB, multiples of 1024 rows.  Every pageable copy call costs ~0.25 ms of
    // pipeline fill on top of its bytes (profiles/r02_ingest_timing.txt) and the call ends one chunk's
    // scan after the last byte, so the count that minimises  0.25 ms * c + t_scan / c  is sqrt(t_scan / 0.25 ms)
    // (`nchunks_hint`, from the caller's cost model), kept within 2 .. 16.
    long long want_chunks = nchunks_hint < 2 ? 2 : nchunks_hint > 16 ? 16 : nchunks_hint;
    long long chunk_rows = (rows + want_chunks - 1) / want_chunks;
    const long long lo_rows = (long long)((32u << 20) / row_bytes) + 1;
    chunk_rows = std::max(lo_rows, chunk_rows);
    chunk_rows = (chunk_rows + 1023) / 1024 * 1024;
    const long long nchunks = (rows + chunk_rows - 1) / chunk_rows;

    float *r_dev = nullptr, *q_dev = nullptr;
    u64 *keys_dev = nullptr;
    std::vector<hipEvent_t> events;
    Staging stage(device);
    hipError_t e = stage.get(&r_dev, rbytes);
    if (e == hipSuccess)
        e = stage.get(&q_dev, qbytes);
    if (e == hipSuccess)
        e = (keep ? keep->owner : stage).get(&keys_dev, kbytes);
    if (e == hipSuccess)
        e = hipMemcpyAsync(q_dev, queries_host, qbytes, hipMemcpyHostToDevice, st.compute);
    if (e == hipSuccess)
        e = knn_keys_fill_launch(keys_dev, m, st.compute);
    for (long long c = 0; c < nchunks && e == hipSuccess; ++c) {
        const long long r0 = c * chunk_rows, r1 = std::min(rows, r0 + chunk_rows);
        hipEvent_t ev = nullptr;
        e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess)
            break;
        events.push_back(ev);
        // pageable source: the call returns once the chunk is staged, while the GPU still scans the
        // previous one
        e = hipMemcpyAsync(r_dev + (size_t)r0 * k, refs_host + (size_t)r0 * k, (size_t)(r1 - r0) * row_bytes,
                           hipMemcpyHostToDevice, st.copy);
        if (e == hipSuccess)
            e = hipEventRecord(ev, st.copy);
        if (e == hipSuccess)
            e = hipStreamWaitEvent(st.compute, ev, 0);
        if (e == hipSuccess)
            e = knn_exact_launch(k, m, r1 - r0, base + r0, q_dev, r_dev + (size_t)r0 * k, keys_dev, num_cu, nullptr,
                                 st.compute);
    }
    if (e == hipSuccess && !keep)
        e = hipMemcpyAsync(keys_host, keys_dev, kbytes, hipMemcpyDeviceToHost, st.compute);
    const hipError_t e_sync1 = hipStreamSynchronize(st.copy);
    const hipError_t e_sync2 = hipStreamSynchronize(st.compute);
    if (e == hipSuccess)
        e = e_sync1 != hipSuccess ? e_sync1 : e_sync2;
    for (hipEvent_t ev : events)
        (void)hipEventDestroy(ev);
    if (e != hipSuccess)
        return fail(KNN_EHIP, "cudaCallback: streamed shard", hipGetErrorString(e));
    stage.waited();   // both streams have been synchronised
    if (keep)
        keep->dev = keys_dev;
    return KNN_OK;
}

}  // namespace

namespace {

// Cost model of ONE shard of a one-shot call (host rows in, keys out) on one MI355X: which of the three ways serves it
// and what it is expected to take.  Constants measured on one box: pageable H2D 50-55 GB/s with ~0.25 ms of
// fixed cost per copy call; exact kernels 58e12 lane-ops/s with a compile-time K (or m < 48), 45e12 / 22e12 with a run-time
// k up to 64 / 128 (knn_exact_qregn), 5e12 on the row-per-lane kernels beyond; the MFMA filter ~3.4e-14 s per pair and
// K-step plus its layouts (built under the copy unless option `ingest` = 1); the grid index (k <= 4) four passes over the
// rows to build (~0.1 ms + 0.15 ns per row) and one wave per query.
struct ShardPlan {
    bool streamed = false;   // exact scan chunk by chunk under the copy (run_shard_streamed)
    int want_filter = 0;     // staged: build the MFMA layouts
    bool want_grid = false;  // staged: build the grid index (k <= 4)
    int nchunks = 2;         // streamed: copy calls
    double t_streamed = 0.0, t_staged = 0.0;
    double seconds = 0.0;    // the chosen way
};

// The options the cost model and the call plan read, filled by their callers.
struct ShardOptions {
    long long path = 0, cells = 0, ingest = 0, cells_build = 0, stream = 0, shards = 0, rccl = 0;
};
ShardOptions shard_options()
{
    return {g_opt_path, g_opt_cells, g_opt_ingest, g_opt_cells_build, g_opt_stream, g_opt_shards, g_opt_rccl};
}

ShardPlan plan_shard(int k, int m, long long rows, const ShardOptions &o)
{
    ShardPlan p;
    const double pairs = (double)m * (double)rows;
    const bool fast_k = k == 1 || k == 2 || k == 3 || k == 4 || k == 8 || k == 16;
    const double exact_rate = (fast_k || m < 48) ? 58e12 : k <= 64 ? 45e12 : k <= 128 ? 22e12 : 5e12;
    const double t_exact = (3.0 * k + 3.0) * pairs / exact_rate;
    const int kt = knn_kt_of(k);   // 0: no fp16 layouts for this k (k > 4096)
    const double t_filter = kt == 0 ? 1e30 : 1.0e-3 + 2.5 * 4.0 * k * (double)rows / 4e12 + 3.4e-14 * kt * pairs + 1e-4;
    const double t_filter_under_copy = 6e-4 + 3.4e-14 * kt * pairs + 1e-4;   // host rows: layouts built under the copy
    p.want_filter = o.path == 2 ||
                    (o.path == 0 && m >= 5 && kt != 0 && (o.ingest == 1 ? t_filter : t_filter_under_copy) < t_exact);
    // The pruned scan for a one-shot call (round 5: the cell sort's bucket pass runs under the copy, knn_filter_build_cells_from_host):
    // ~1.0 ms per 2^24 rows stay behind the last byte (cell prefix + placement) where the plain layouts leave 0.07, and a
    // batch of 1024 queries then costs 0.04 ms + 6.5 ps per row instead of 3.4e-14 s per pair — it repays the sort from about
    // 2500 queries on at C3's size (measured: one batch 0.145 ms against 0.58).  Where the library's own policy puts
    // resident indexes on the cells (k <= 16, >= 2^19 / 2^20 rows), and only with the default build options.
    // (same fixed costs as the plain layouts' line above, so that the two differ by what differs)
    const double t_cells_query = 6e-4 + 1.0e-3 * (double)rows / 16777216.0 + ceil(m / 1024.0) * (4e-5 + 6.5e-12 * (double)rows) + 1e-4;
    if (p.want_filter && o.path == 0 && o.cells == 0 && o.ingest == 0 && o.cells_build == 0 && k <= 16 &&
        rows >= knn_cells_size_rule(k) && (double)rows * 96.0 <= 2147483648.0 && t_cells_query < t_filter_under_copy)
        p.want_filter = 2;
    // Third option: the exact scan chunk by chunk under the copy: costs the longer of the two plus one chunk's scan.  The
    // staged alternatives pay the copy in one piece; the filter layouts are then built under the copy's tail
    // (knn_filter_build_from_host), leaving the query itself.
    const double bytes = 4.0 * k * (double)rows;
    const double t_h2d = bytes / 52e9;
    const double kCopyCall = 2.5e-4;
    double nchunks = floor(sqrt(t_exact / kCopyCall) + 0.5);
    nchunks = std::max(2.0, std::min(16.0, std::min(nchunks, floor(bytes / (double)(32u << 20)))));
    p.nchunks = (int)nchunks;
    p.t_streamed = std::max(t_h2d, t_exact) + t_exact / nchunks + kCopyCall * nchunks + 1e-4;
    const double t_filter_query = 6e-4 + 3.4e-14 * kt * pairs + 1e-4;   // layouts under the copy + query
    const double t_query = p.want_filter == 2 ? t_cells_query : p.want_filter ? (o.ingest == 1 ? t_filter : t_filter_query) : t_exact;
    const double t_grid = k <= 4 ? 1.5e-4 + 1.5e-10 * (double)rows + 2e-8 * m : 1e30;
    p.want_grid = k <= 4 && (o.path == 3 || (o.path == 0 && rows >= 65536 && t_grid < t_query));
    p.t_staged = t_h2d + kCopyCall + (p.want_grid ? t_grid : t_query);
    p.streamed = o.path != 2 && !p.want_grid && o.stream != 1 && bytes >= (double)(64u << 20) &&
                 (o.stream == 2 || p.t_streamed < p.t_staged);
    p.seconds = p.streamed ? p.t_streamed : p.t_staged;
    return p;
}

// How many GPUs a one-shot call is split over (reference core.cu:865-872: every GPU, never more than n, ONE when
// n <= min(2^18, m << 10) — which is every case of the TA harness).  Here the reference's small-n rule stands,
// and beyond it the cost model decides: a call fans out over G GPUs when the shards' expected time (each GPU has its own
// PCIe link and copies its own range) plus what fanning out costs — a host thread, an index create / query / destroy and
// a share of the key exchange per GPU — is lowest; of the counts within 10 % of the best the smallest is taken.  The fan-out constants (0.2 ms + 0.02 ms per GPU)
// are estimates: no multi-GPU node was available to measure them.
int shard_policy(int k, int m, long long n, int ndev, const ShardOptions &o)
{
    long long cap = std::min<long long>(ndev, n);                           // core.cu:867-868
    if (cap <= 1 || n <= std::min<long long>(1ll << 18, (long long)m << 10))   // core.cu:871-872
        return 1;
    // candidates: 1, 2, 4, ... and every visible GPU; of those within 10 % of the best, the fewest
    std::vector<int> cand;
    for (int g = 1; g < (int)cap; g *= 2)
        cand.push_back(g);
    cand.push_back((int)cap);
    std::vector<double> t(cand.size(), 0.0);
    double t_min = 1e30;
    for (size_t i = 0; i < cand.size(); ++i) {
        const int g = cand[i];
        t[i] = plan_shard(k, m, (n + g - 1) / g, o).seconds + (g > 1 ? 2e-4 + 2e-5 * g : 0.0);
        t_min = std::min(t_min, t[i]);
    }
    size_t pick = 0;
    while (t[pick] > 1.1 * t_min)
        ++pick;
    const int best = cand[pick];
    return best;
}

}  // namespace

// Test hook (host arithmetic): how ONE shard of a one-shot call would be served — out = {filter layouts: 0 none, 1 plain, 2 cell-sorted
// (the pruned scan), exact scan streamed under the copy, grid index, copy calls of the streamed form}.
extern "C" int knn_debug_plan_shard(int k, int m, long long rows, long long out[4])
{
    if (k < 1 || m < 1 || rows < 1 || !out)
        return fail(KNN_EINVAL, "knn_debug_plan_shard: bad arguments");
    const ShardPlan p = plan_shard(k, m, rows, shard_options());
    out[0] = p.want_filter;
    out[1] = p.streamed ? 1 : 0;
    out[2] = p.want_grid ? 1 : 0;
    out[3] = p.nchunks;
    return KNN_OK;
}

extern "C" int knn_debug_shard_policy(int k, int m, long long n, int ndev)
{
    if (k < 1 || m < 1 || n < 1 || ndev < 1)
        return fail(KNN_EINVAL, "knn_debug_shard_policy: bad arguments");
    return shard_policy(k, m, n, ndev, shard_options());
}

namespace {

// Everything one cudaCallback decides, decided once from the call's sizes, the visible devices and ONE reading of the
// options (a knn_set_option from another thread cannot make the shards and the exchange step disagree).
struct CallShard {
    int device;
    long long lo, hi;   // its rows; hi <= lo: an empty shard (no `way`)
    ShardPlan way;      // which of the three ways serves it: plan_shard (cost model)
};
struct CallPlan {
    int k, m;
    ShardOptions opt;
    long long per = 0;         // rows per shard
    int threads = 1;           // one host thread per GPU (core.cu:873); shards that share a device run back to back
    bool rccl_wanted = false, use_rccl = false;   // the exchange step: RCCL all-reduce on the devices, else a merge on the host
    int refusal = 0;           // option rccl = 1, but 1: the shards are not the visible devices, 2: RCCL cannot be used
    std::string rccl_why;      // why it cannot
    std::vector<CallShard> shard;
};

// rccl_usable (knn_rccl_available: it dlopens librccl) is asked only for a call whose rule wants RCCL.
CallPlan plan_call(int k, int m, long long n, int ndev, const ShardOptions &o, const std::function<int(std::string *)> &rccl_usable)
{
    CallPlan p;
    p.k = k, p.m = m, p.opt = o;
    // core.cu:865-872: how many GPUs take part (never more shards than points; one GPU for the small sets of the TA
    // harness; beyond that by the cost model: shard_policy).  Option `shards` forces a count (test hook).
    const long long shards = std::min(n, o.shards > 0 ? o.shards : (long long)shard_policy(k, m, n, ndev, o));
    // core.cu:875: thread_n = divup(n, num_gpus); the last shard takes what is left.  A shard
    // past the end is empty here (the reference patches it to one overlapping point,
    // core.cu:881-882; an empty shard gives the same minimum).
    p.per = (n + shards - 1) / shards;
    p.threads = (int)std::min<long long>(shards, ndev);
    for (long long g = 0; g < shards; ++g) {
        const long long lo = std::min(g * p.per, n), hi = std::min(lo + p.per, n);
        p.shard.push_back({(int)(g % ndev), lo, hi, hi > lo ? plan_shard(k, m, hi - lo, o) : ShardPlan()});
    }
    // The exchange step.  Several GPUs with one shard each (the reference's configuration, core.cu:873):
    // every shard leaves its m packed keys ON ITS DEVICE and one RCCL all-reduce(uint64, min) merges them
    // (knn_rccl.cpp); device 0's copy comes back to the host.  More shards than devices (the single-GPU
    // test hook), a single device, `rccl` = 2, or no usable librccl: the keys come back per shard and are
    // min-merged on the host — the same unsigned minimum.
    // ONE communicator set per process, for all visible devices (ncclCommInitAll takes seconds on an 8-GPU node): a call
    // that uses fewer GPUs than are visible merges on the host instead of creating a second set.
    p.rccl_wanted = o.rccl != 2 && shards == ndev && (o.rccl == 1 || shards > 1);
    p.use_rccl = p.rccl_wanted && rccl_usable(&p.rccl_why) != 0;
    // (`rccl` = 1 means "always, and die when RCCL cannot serve" — a call that the policy or option `shards`
    // splits over another number of GPUs than are visible has no communicator set, and merging on the host in silence
    // would break that contract)
    p.refusal = o.rccl != 1 ? 0 : shards > 1 && shards != ndev ? 1 : p.rccl_wanted && !p.use_rccl ? 2 : 0;
    return p;
}

// One shard of a call, on the calling thread: its rows of the references against all m queries.
void run_call_shard(const CallPlan &plan, size_t g, const float *queries, const float *refs, bool trace, ShardKeys &out)
{
    using Clock = std::chrono::steady_clock;
    auto ms = [](Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const CallShard &s = plan.shard[g];
    const int k = plan.k, m = plan.m;
    const long long rows = s.hi - s.lo;
    const float *rows_host = refs + (size_t)s.lo * (size_t)k;
    ShardKeys *keep = plan.use_rccl ? &out : nullptr;
    if (!keep)
        out.host.assign((size_t)m, kKeyInit);   // (all that an empty shard leaves)
    int rc = KNN_OK;
    const auto t0 = Clock::now();
    if (rows <= 0 && keep) {   // an empty shard still takes part in the all-reduce: m keys of (+INF, 0)
        DeviceGuard guard(s.device);
        hipError_t e = guard.ok ? keep->owner.get(&keep->dev, (size_t)m * sizeof(u64)) : hipErrorInvalidDevice;
        if (e == hipSuccess)
            e = knn_keys_fill_launch(keep->dev, m, nullptr);
        if (e == hipSuccess)
            e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess)
            rc = fail(KNN_EHIP, "cudaCallback: empty shard keys", hipGetErrorString(e));
    } else if (rows > 0 && s.way.streamed) {
        rc = run_shard_streamed(s.device, k, m, rows, s.lo, queries, rows_host, out.host.data(), keep, s.way.nchunks);
        if (trace)
            fprintf(stderr, "[knn call] shard %zu rows %lld streamed exact scan: %.3f ms (model: streamed %.3f, staged %.3f)\n",
                    g, rows, ms(t0, Clock::now()), s.way.t_streamed * 1e3, s.way.t_staged * 1e3);
    } else if (rows > 0) {
        knn_index *idx = nullptr;
        rc = index_create_impl(&idx, s.device, k, rows, rows_host, 0, s.lo, nullptr, s.way.want_grid ? 0 : s.way.want_filter,
                               s.way.want_grid ? 1 : 0);
        const auto t1 = Clock::now();
        if (rc == KNN_OK)
            rc = staged_query(idx, "query", m, 0, queries, out.host.data(), keep);
        if (rc == KNN_OK && idx->stats[0] == 4)
            ++g_last_cells;
        const auto t2 = Clock::now();
        knn_index_destroy(idx);
        if (trace)
            fprintf(stderr, "[knn call] shard %zu rows %lld filter %d: create (alloc + H2D + layouts) %.3f ms, "
                            "query (stage + scan + D2H) %.3f ms, destroy %.3f ms\n",
                    g, rows, s.way.want_filter, ms(t0, t1), ms(t1, t2), ms(t2, Clock::now()));
    }
    out.rc = rc;
    if (rc != KNN_OK)
        out.err = g_err;
}

// The exchange step on the GPUs: ncclAllReduce(uint64, min) over the shards' keys, one D2H from shard 0's device.
// The reduction writes to scratch buffers, never to the keys: if RCCL fails at run time (communicator
// creation on a node it does not like, a failed collective), the shards' keys are still what the scans left.
bool rccl_merge(const CallPlan &plan, std::vector<ShardKeys> &sk, std::vector<u64> &merged, std::string &err)
{
    const size_t shards = sk.size(), kbytes = (size_t)plan.m * sizeof(u64);
    std::vector<int> devs(shards);
    std::vector<u64 *> keys(shards), scratch(shards, nullptr);   // (scratch: with the shard's keys, in its owner)
    for (size_t g = 0; g < shards; ++g) {
        devs[g] = plan.shard[g].device;
        keys[g] = sk[g].dev;
        DeviceGuard guard(devs[g]);
        const hipError_t e = guard.ok ? sk[g].owner.get(&scratch[g], kbytes) : hipErrorInvalidDevice;
        if (e != hipSuccess) {
            err = std::string("scratch keys for the reduction: ") + hipGetErrorString(e);
            return false;
        }
    }
    // (test hook: a run-time RCCL failure, and — a one-GPU box can only reach this code with `rccl` = 1 — the
    // fallback of the automatic mode with it)
    if (getenv("KNN_MI355X_TEST_RCCL_FAIL")) {
        err = "KNN_MI355X_TEST_RCCL_FAIL is set";
        return false;
    }
    if (knn_rccl_allreduce_min((int)shards, devs.data(), keys.data(), plan.m, nullptr, err, scratch.data()) != 0)
        return false;
    merged.resize((size_t)plan.m);
    DeviceGuard guard0(devs[0]);
    const hipError_t e = hipMemcpy(merged.data(), scratch[0], kbytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        err = std::string("D2H of the reduced keys: ") + hipGetErrorString(e);
        return false;
    }
    for (size_t g = 0; g < shards; ++g) {   // nothing may still be reading the buffers going back to the pool
        DeviceGuard guard(devs[g]);
        if (hipStreamSynchronize(nullptr) == hipSuccess)
            sk[g].owner.waited();
    }
    return true;
}

// The exchange step: the shards' keys -> the call's m merged keys.
int exchange_keys(const CallPlan &plan, std::vector<ShardKeys> &sk, std::vector<u64> &merged)
{
    const size_t m = (size_t)plan.m;
    std::string err;
    if (plan.use_rccl) {
        if (rccl_merge(plan, sk, merged, err)) {
            ++g_rccl_reductions;
            return KNN_OK;
        }
        // option 0 = "RCCL where possible" (and the test hook): the host merge takes over; `rccl` = 1 insists
        if (plan.opt.rccl != 0 && !getenv("KNN_MI355X_TEST_RCCL_FAIL"))
            return fail(KNN_EHIP, "cudaCallback: RCCL key reduction", err.c_str());
        static bool warned = false;
        if (!warned) {
            warned = true;
            fprintf(stderr, "knn_mi355x: RCCL key reduction failed (%s); merging the shards' keys on the host\n", err.c_str());
        }
        (void)hipGetLastError();
        for (size_t g = 0; g < sk.size(); ++g) {   // the (untouched) per-shard keys
            DeviceGuard guard(plan.shard[g].device);
            sk[g].host.resize(m);
            const hipError_t e = hipMemcpy(sk[g].host.data(), sk[g].dev, m * sizeof(u64), hipMemcpyDeviceToHost);
            if (e != hipSuccess)
                return fail(KNN_EHIP, "cudaCallback: RCCL key reduction", (err + "; D2H of shard keys: " + hipGetErrorString(e)).c_str());
        }
    }
    // Host merge: unsigned min of packed keys == lexicographic (distance, global index).
    merged.assign(m, kKeyInit);
    for (const ShardKeys &s : sk)
        for (size_t j = 0; j < m; ++j)
            merged[j] = std::min(merged[j], s.host[j]);
    return KNN_OK;
}

}  // namespace

// Test hook (host arithmetic): the plan of a cudaCallback(k, m, n) under the current options on a node of in[3] devices
// where the RCCL probe would answer in[4] (include/knn_mi355x.h lists `out`).
extern "C" int knn_debug_call_plan(const long long in[5], long long out[16])
{
    if (!in || !out || in[0] < 1 || in[1] < 1 || in[2] < 1 || in[3] < 1 || in[0] > INT_MAX || in[1] > INT_MAX || in[3] > INT_MAX)
        return fail(KNN_EINVAL, "knn_debug_call_plan: bad arguments");
    bool asked = false;
    const CallPlan p = plan_call((int)in[0], (int)in[1], in[2], (int)in[3], shard_options(), [&](std::string *) {
        asked = true;
        return in[4] != 0;
    });
    out[0] = (long long)p.shard.size();
    out[1] = p.per;
    out[2] = p.threads;
    out[3] = p.use_rccl ? 1 : 0;
    out[4] = p.refusal;
    out[5] = out[6] = 0;
    for (size_t g = 0; g < p.shard.size(); ++g) {
        const CallShard &s = p.shard[g];
        if (s.hi <= s.lo) {
            ++out[5];
            continue;
        }
        out[6] = s.hi - s.lo;
        const long long way[4] = {s.way.want_filter, s.way.streamed ? 1 : 0, s.way.want_grid ? 1 : 0, s.way.nchunks};
        for (int i = 0; i < 4; ++i) {   // shard 0's way, and the last non-empty shard's
            if (g == 0)
                out[8 + i] = way[i];
            out[12 + i] = way[i];
        }
    }
    out[7] = asked ? 1 : 0;
    return KNN_OK;
}

// ---------------------------------------------------------------------------------------------
// The drop-in entry point (reference core.h:71, core.cu:1282-1297 -> v8, core.cu:856-958):
// plan the call, run its shards, exchange their keys, unpack the indices.
// ---------------------------------------------------------------------------------------------
extern "C" void cudaCallback(int k, int m, int n, float *searchPoints, float *referencePoints,
                             int **results)
{
    if (k < 1 || m < 1 || n < 1 || !searchPoints || !referencePoints || !results)
        DIE_IF(fail(KNN_EINVAL, "cudaCallback: k, m, n must be >= 1 and pointers non-null"));
    const int ndev = knn_device_count();
    // The reference computes on the CPU here (core.cu:869-870); this library has no CPU path.
    if (ndev < 1)
        DIE_IF(fail(KNN_ENODEV, "cudaCallback: no HIP device visible (this library has no CPU fallback)"));
    const CallPlan plan = plan_call(k, m, n, ndev, shard_options(), knn_rccl_available);
    const size_t shards = plan.shard.size();
    g_last_shards = (long long)shards;
    g_last_cells = 0;
    static const bool trace = getenv("KNN_MI355X_TRACE_CALL") != nullptr;
    if (trace)
        fprintf(stderr, "[knn call] k %d m %d n %d: %d GPU(s) visible -> %zu shard(s)%s\n", k, m, n, ndev, shards,
                plan.opt.shards > 0 ? " (option shards)" : "");
    if (plan.refusal == 1) {
        char why[160];
        snprintf(why, sizeof why, "%zu shards on %d visible GPU(s): the one communicator set of the process spans all visible devices", shards, ndev);
        DIE_IF(fail(KNN_EINVAL, "cudaCallback: option rccl = 1 but the call's shards are not the visible devices", why));
    }
    if (trace && shards > 1 && !plan.use_rccl)
        fprintf(stderr, "[knn call] keys merged on the host: %s\n",
                plan.opt.rccl == 2 ? "option rccl = 2" : shards != (size_t)ndev ? "the shards are not the visible devices" : plan.rccl_why.c_str());
    if (plan.refusal == 2)
        DIE_IF(fail(KNN_EHIP, "cudaCallback: option rccl = 1 but RCCL cannot be used", plan.rccl_why.c_str()));
    std::vector<ShardKeys> keys;
    for (const CallShard &s : plan.shard)
        keys.emplace_back(s.device);
    auto run_shards = [&](size_t first) {
        for (size_t g = first; g < shards; g += (size_t)plan.threads)
            run_call_shard(plan, g, searchPoints, referencePoints, trace, keys[g]);
    };
    std::vector<std::thread> pool;
    for (int t = 0; plan.threads > 1 && t < plan.threads; ++t)
        pool.emplace_back(run_shards, (size_t)t);
    if (pool.empty())
        run_shards(0);   // one thread: this one
    for (auto &th : pool)
        th.join();
    int rc = KNN_OK;
    for (size_t g = 0; g < shards && rc == KNN_OK; ++g)   // the first failed shard's error
        if (keys[g].rc != KNN_OK)
            rc = fail(keys[g].rc, keys[g].err.c_str());
    std::vector<u64> merged;
    if (rc == KNN_OK)
        rc = exchange_keys(plan, keys, merged);
    keys.clear();   // exit() runs no destructor of this frame: the pooled buffers go back before the call dies
    DIE_IF(rc);
    int *out = (int *)malloc(sizeof(int) * (size_t)m);  // caller free()s (main.cu:98,175)
    if (!out)
        die(__FILE__, __LINE__, KNN_ENOMEM, "malloc(results)");
    for (int j = 0; j < m; ++j)
        out[j] = (int)(unsigned)(merged[(size_t)j] & 0xFFFFFFFFull);
    *results = out;
}
