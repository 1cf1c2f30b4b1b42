// cbn_table_plan.h -- the host-side planner of table plans: from the factor
// descriptors' integers, N, the CU count and the diagnostic switches to the
// image layout, the LDS sizes and the query kernel (TableSel).  Plain C++17:
// no HIP call, no device pointer dereferenced (pointers are only copied and
// tested for null), no getenv -- plan_table() is a function of its arguments.
// cbn_plan_create (cbn_infer.hip) allocates, uploads and launches what it
// returns; cbn_table_plan_info reports it without a device.
#ifndef CBN_TABLE_PLAN_H
#define CBN_TABLE_PLAN_H

#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/cbn_amd.h"

#ifndef CBN_SLOTS_FUSED2
#define CBN_SLOTS_FUSED2 1  // fused single launch up to two block rounds (0: one round, beyond -> raw + scale)
#endif

namespace cbn {

constexpr int kWave = 64;
constexpr int kLdsBudget = 160 * 1024;
constexpr int kMaxSlots = 1024;
constexpr int kFastPtrs = 416;  // fast table path: 104 factors x 4 observed parents (3.3 KiB of kernel arguments)

// Device-side factor descriptor (built once per plan, read with wave-uniform
// indices so the compiler keeps it on the scalar path).
struct DevFactor {
    int kind;
    int n_parents;
    int node_card;
    int n_free;
    int parent_card[CBN_MAX_PARENTS];
    int ev_slot[CBN_MAX_PARENTS];
    int cpd_stride[CBN_MAX_PARENTS];
    const float* cpd;
    const int* node_sample_idx;
    const int* parent_sample_idx;
    int table_off;   // float offset of this factor's table ([rows][RS]) in the image
    int rows;        // prod(card of observed parents) (QUERY) or 1
    int n_entries;   // rows * N
    int free_combos; // N^n_free
    int wave_mode;   // build kernel: 1 = one wave per entry (many free combos)
};

struct QSlot {
    int dom_off;  // float offset of the sorted domain in the image
    int card;
    int dense;    // 1: domain is exactly {0, 1, ..., card-1} -> index = value
    int pad;
};

struct BuildItem {
    int factor;
    int unit_begin;
};

// (the table path's own names: cbn_infer.hip opens this namespace, the other
// translation units of the library do not)
namespace table {

constexpr int kMaxP = CBN_MAX_PARENTS;
constexpr int kQueryThreads = 1024;
constexpr int kFastObs = 4;  // fast path: observed parents per factor
// Kernel arguments are copied per launch: plans of <= 32 factors (configs[1],
// [2]) take a 1 KiB table (launch 3.2 us of host time instead of 4.9 us with
// the 3.3 KiB one, profiles/r01_launch_cost.txt).
constexpr int kFastPtrsSmall = 128;
constexpr int kFqInts = 4 + 2 * kMaxP;  // k_query's LDS factor record: img_off, kind, n_obs, pad, obs_slot[], obs_card[]
constexpr int kSR = 256;  // k_query_staged: queries per block round

// Per-factor static record, written into the plan image at plan creation and
// copied to LDS with the tables (one LDS-DMA stream, no per-call build).
struct alignas(16) FastRec {
    int table_off;
    int n_obs;
    int card[kFastObs];     // bit 30: domain is {0..card-1} (index = value)
    int dom_off[kFastObs];
    int slot[kFastObs];
    int pad[2];
};
constexpr int kDenseBit = 1 << 30;
constexpr int kRecFloats = sizeof(FastRec) / 4;

// k_query_cols / k_query_slots: one factor's product-loop record (its comment
// is at the kernels, cbn_infer.hip)
struct alignas(16) ColRec {
    int base;            // float offset of the table (LDS copy when `lds`, else the image)
    int n_obs;           // observed parents (<= kFastObs)
    int par[kFastObs];   // (evidence slot << 24) | row weight in floats (= stride x RS, < 2^24)
    int lds;             // 1: table is in LDS
    int pad;
};

// The query kernel of a table plan.  PairedFast is k_query_fast reading the
// N = 32 bank-half layout; every value but Generic is a "fast path" plan.
enum class TableKernel : int { Generic = 0, Fast, PairedFast, Staged, Cols, Slots };

// The one selection of a table plan: decided by plan_table(), stored in
// cbn_plan, read by every launch and by cbn_plan_flags.
struct TableSel {
    TableKernel kernel = TableKernel::Generic;
    int vpl = 1;              // float4 chunks of one query row per lane (fast path)
    int lanes = 0;            // lanes per query, N / (4 vpl) (fast path)
    bool use_lds = false;     // the table image is copied to LDS
    int ptrs = 0;             // k_query_fast / k_query_staged: pointer-table size (kFastPtrsSmall / kFastPtrs)
    int cols_chunk = 0;       // k_query_cols: slots per lane, 16 or 40
    size_t lds_bytes = 0;     // dynamic LDS of `kernel`
    int blocks_per_cu = 1;
    int max_slots = 0;        // fast path: blocks per max / raw launch at most = words of per-block maxima
    bool fused2 = false;      // a fused launch holds two rounds per block (k_query_slots / k_query_cols)
    bool fast() const { return kernel != TableKernel::Generic; }
};

// cbn_plan_flags' bits of a table plan (all but CBN_PLAN_FUSED, which the
// occupancy query decides): every fast-path kernel also reduces rows itself
inline int table_flags(const TableSel& s) {
    const TableKernel k = s.kernel;
    return (s.fast() ? CBN_PLAN_FAST | CBN_PLAN_ARGMAX | CBN_PLAN_MOMENTS | CBN_PLAN_QUANTILE : 0) |
           (s.use_lds ? CBN_PLAN_LDS : 0) | (s.vpl == 2 ? CBN_PLAN_VPL2 : 0) |
           (k == TableKernel::PairedFast || k == TableKernel::Staged ? CBN_PLAN_PAIRED : 0) |
           (k == TableKernel::Staged ? CBN_PLAN_STAGED : 0) | (k == TableKernel::Cols ? CBN_PLAN_COLS : 0) |
           (k == TableKernel::Slots ? CBN_PLAN_SLOTS : 0);
}

// Diagnostic switches (CBN_* under CBN_DIAG=1), read once by the caller.
struct TableSwitches {
    int fast_vpl = 2;  // CBN_FAST_VPL: float4 chunks per lane at most (8 output values per lane tuned on MI355X: chain20 d32)
    bool no_paired = false, no_prefix = false, no_lds_split = false, no_slots = false, no_staged = false,
         no_cols = false, no_fused = false;
    int slots_bpc = 0;  // CBN_SLOTS_BPC: k_query_slots' blocks per CU forced to 1 or 2 (0: by its LDS)
};

// What plan_table() decides and a plan keeps for its launches: cbn_plan
// (cbn_internal.h) is this plus its device buffers.
struct TableLayout {
    int nf = 0, ns = 0, N = 0, vec = 1, L = 1;
    int RS = 1;                  // table row stride in floats (>= N; padded to spread LDS banks)
    int CH = 1;                  // k_query: queries per block chunk (LDS-sized)
    TableSel sel;
    int n_build = 0, build_units = 0;
    int table_floats = 0, rec_off = 0, image_floats = 0;  // image: [tables | slot domains | FastRec[nf] | QSlot[ns]]
    int zero_off = -1;           // paired layout: float offset of the zero super-row (ones super-row at +64)
    int prefix = 0;              // staged plans: leading 1-row factors folded into factor `prefix` (k_merge_prefix)
    int prefix_offs[9] = {};     // table offsets of factors 0..prefix
    int prefix_rows = 0;         // rows of factor `prefix`'s table
    int lds_tab_floats = 0;      // global-table plans: the small tables packed first, copied to LDS by the kernel
    unsigned long long lds_tab_mask[2] = {0, 0};  // ... and which factors' tables those are (bit f)
    int fast_slot[kFastPtrs];    // evidence slot of observed parent p of factor f at [f*4+p] (-1: none)
};

struct TablePlan : TableLayout {
    int err = CBN_OK;  // else `msg` says why the descriptors were refused
    char msg[200] = {};
    bool global_tables = false;  // unpadded rows read from L2 / HBM
    bool paired_layout = false;  // N = 32 bank-half layout (RS = 64)
    std::vector<DevFactor> fac;
    std::vector<QSlot> slots;             // `dense` is the caller's (it reads the domains)
    std::vector<const float*> slot_dom;   // device pointers, never read here
    std::vector<BuildItem> build;
    std::vector<FastRec> recs;            // fast path (without the slots' dense bit)
    std::vector<ColRec> crec;             // Cols / Slots
    bool fused_candidate = false;         // the occupancy query decides (cbn_plan_create)
};

// Rows of a factor's table: the product of its observed parents' cards
// (clamped, so a sum over the factors cannot overflow).
inline long long observed_rows(const cbn_factor_desc& h) {
    long long rows = 1;
    for (int p = 0; p < h.n_parents && p < kMaxP; ++p)
        if (h.parent_ev_slot[p] >= 0 && h.parent_card[p] > 0) rows = std::min(rows * h.parent_card[p], 1LL << 40);
    return rows;
}

// VPL and lanes per query of the fast path for this N: lanes = N / (4 VPL) a
// power of two <= 64 (VPL 4 exceeds 128 VGPRs at 1024 threads: spills).
// vpl 0: no fast path.
struct FastLanes {
    int vpl = 0, lanes = 0;
};
inline FastLanes fast_lanes(int N, int want_vpl) {
    for (int c : {2, 1}) {
        if (c > want_vpl || (N / 4) % c) continue;
        const int Lc = N / (4 * c);
        if (Lc <= kWave && (kWave % Lc) == 0) return {c, Lc};
    }
    return {};
}

// k_query_fast's side buffers after the image: pointer table, offsets
// [waves][queries per wave][nf4], wave maxima
inline size_t fast_side_bytes(int nf, int lanes) {
    const size_t nf4 = (size_t)((nf + 3) & ~3);
    return (size_t)kFastPtrs * sizeof(void*) + (size_t)(kQueryThreads / kWave) * (kWave / lanes) * nf4 * 4 +
           (kQueryThreads / kWave) * 4 + 64;
}

// dynamic LDS of k_query_fast: the image -- or, global tables, the small
// tables and the records -- then fast_side_bytes
inline size_t fast_lds_bytes(bool use_lds, size_t img_bytes, long long lds_tab_floats, int nf, int lanes) {
    return ((use_lds ? img_bytes : (size_t)lds_tab_floats * 4 + (size_t)nf * kRecFloats * 4) +
            fast_side_bytes(nf, lanes) + 15) & ~size_t(15);
}

// dynamic LDS of k_query_staged over `nfs` factors (unrounded): the image, two
// staging buffers of kSR queries x 4 (nsl + 1) ints, wave maxima
inline size_t staged_lds_bytes(size_t img_bytes, int nfs) {
    const int st_T = (nfs + 2) >> 1, st_S = (st_T + 1) >> 1;  // k_query_staged's nsl
    return img_bytes + (size_t)2 * kSR * (4 * (st_S + 1)) * 4 + (kQueryThreads / kWave) * 4 + 64;
}

// dynamic LDS of k_query_cols: the image -- or the small tables, the records
// and the QSlots -- then slot pointers, sidx[ns][QB] (int16), wave maxima, a
// zero row
inline size_t cols_lds_bytes(bool use_lds, size_t img_bytes, long long lds_tab_floats, int nf, int ns, int N,
                             int lanes) {
    const size_t QB = (size_t)kQueryThreads / lanes;
    return ((use_lds ? img_bytes : (size_t)lds_tab_floats * 4 + ((size_t)nf * kRecFloats + (size_t)ns * 4) * 4) +
            (size_t)((ns + 1) & ~1) * sizeof(void*) + (((size_t)ns * QB + 1) & ~size_t(1)) * 2 +
            (kQueryThreads / kWave) * 4 + 64 + 16 + (size_t)N * 4 + 15) & ~size_t(15);
}

// k_query_slots' sidx row stride in int16 units (its slots_sidx_stride,
// cbn_infer.hip; cbn_plan_create checks the two agree)
inline int slots_sidx_stride_host(int lanes) { return kQueryThreads / lanes + 2 * (lanes >= 16 ? 1 : 16 / lanes); }

// dynamic LDS of k_query_slots (its layout, in order): the small tables,
// QSlot[ns], ColRec[nf], slot pointers, sidx[ns][SQ] (int16, SQ = QB + pad),
// offsets [QB][nf4], wave maxima
inline size_t slots_lds_bytes(long long lds_tab_floats, int ns, int nf, int QB) {
    const size_t nf4 = (size_t)((nf + 3) & ~3);
    const size_t SQ = (size_t)slots_sidx_stride_host(kQueryThreads / QB);
    size_t b = (size_t)lds_tab_floats * 4 + (size_t)ns * sizeof(QSlot) + (size_t)nf * sizeof(ColRec) +
               (size_t)((ns + 1) & ~1) * sizeof(void*) + ((((size_t)ns * SQ + 7) & ~size_t(7)) * 2) +
               (size_t)QB * nf4 * 4 + (kQueryThreads / kWave) * 4 + 64;
    return (b + 15) & ~size_t(15);
}

// The product loops' records of k_query_cols / k_query_slots from the fast
// path's: per observed parent (evidence slot << 24) | row weight in floats.
// false (the kernel declines the plan): a slot's card beyond int16, a parent
// whose card is not its slot's, a weight >= 2^24 or a slot >= 256.
inline bool col_records(const std::vector<FastRec>& recs, const std::vector<QSlot>& slots, int RS, bool all_lds,
                        const unsigned long long (&lds_mask)[2], std::vector<ColRec>& cr) {
    const int nf = (int)recs.size();
    bool ok = true;
    for (const QSlot& s : slots) ok = ok && s.card <= 32767;
    for (int f = 0; f < nf && ok; ++f)
        for (int q = 0; q < recs[f].n_obs; ++q) ok = ok && recs[f].card[q] == slots[recs[f].slot[q]].card;
    cr.resize(nf);
    for (int f = 0; f < nf && ok; ++f) {
        ColRec& c = cr[f];
        memset(&c, 0, sizeof(c));
        c.base = recs[f].table_off;
        c.n_obs = recs[f].n_obs;
        c.lds = all_lds || ((lds_mask[f >> 6] >> (f & 63)) & 1ull) ? 1 : 0;
        long long w = RS;
        for (int q = recs[f].n_obs - 1; q >= 0; --q) {
            ok = ok && w < (1LL << 24) && recs[f].slot[q] < 256;
            c.par[q] = (recs[f].slot[q] << 24) | (int)(w & 0xFFFFFF);
            w *= recs[f].card[q];
        }
    }
    return ok;
}

// Queries one fused launch holds: one block per CU (one barrier slot each),
// one round per wave -- two for the kernels that hold two across the barrier.
inline long long fused_capacity(const TableSel& s, int n_cu) {
    if (!s.fast()) return 0;
    const long long blocks = std::min(n_cu, kMaxSlots);
    return blocks * (kQueryThreads / kWave) * (kWave / s.lanes) * (s.fused2 ? 2 : 1);
}

namespace table_plan_detail {

inline TablePlan& fail(TablePlan& t, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(t.msg, sizeof(t.msg), fmt, ap);
    va_end(ap);
    t.err = code;
    return t;
}

// Global-table plans: the smallest tables go first in the image, as many as
// fit the LDS the fast kernel leaves free (without costing it its second
// block per CU), and k_query_fast copies that prefix into LDS -- an
// ALARM-like plan is 24 tables of <= 2 KB beside two of 128 KB, and
// gathering the small ones from L2 cost as much as the large ones.
// pre_off[f] >= 0: factor f's offset in that prefix.
inline void split_small_tables(const cbn_factor_desc* factors, int nf, int N, int RS, long long talign,
                               const TableSwitches& sw, std::vector<long long>& pre_off, TablePlan& t) {
    const FastLanes fl = fast_lanes(N, sw.fast_vpl);
    if (fl.vpl == 0) return;
    long long side = (long long)fast_side_bytes(nf, fl.lanes);
    long long recb = (long long)nf * kRecFloats * 4;  // the records go to LDS too
    if (fl.lanes > 2 && !sw.no_slots) {
        // k_query_slots (>= 4 lanes per query) takes the plan if it can:
        // budget the small tables beside ITS side buffers -- or beside
        // k_query_fast's side + records where those are larger, since
        // the fast gate runs first and k_query_slots may still
        // decline the plan (a card > 32767, a row weight >= 2^24)
        int ns_est = 0;
        for (int f = 0; f < nf; ++f)
            for (int q = 0; q < factors[f].n_parents && q < kMaxP; ++q)
                ns_est = std::max(ns_est, factors[f].parent_ev_slot[q] + 1);
        side = std::max((long long)slots_lds_bytes(0, ns_est, nf, kQueryThreads / fl.lanes), side + recb);
        recb = 0;
    }
    long long budget = (long long)kLdsBudget - side - recb - 1024;  // bytes
    if (2 * (side + recb) <= (long long)kLdsBudget)
        budget = std::min(budget, (long long)kLdsBudget / 2 - side - recb - 1024);
    std::vector<std::pair<long long, int>> by_size;
    for (int f = 0; f < nf; ++f)
        by_size.push_back({(observed_rows(factors[f]) * RS + talign - 1) & ~(talign - 1), f});
    std::stable_sort(by_size.begin(), by_size.end());
    long long end = 0;  // floats
    for (const auto& [tf, f] : by_size) {
        if ((end + tf) * 4 > budget) break;  // floats vs bytes
        pre_off[f] = end;
        end += tf;
        t.lds_tab_mask[f >> 6] |= 1ull << (f & 63);
    }
    if (end == 0 || end * 4 > (1LL << 20)) {
        std::fill(pre_off.begin(), pre_off.end(), -1);
        end = 0;
        t.lds_tab_mask[0] = t.lds_tab_mask[1] = 0;
    }
    t.lds_tab_floats = (int)end;
}

// The query kernel of a laid-out plan (t.sel), its records and LDS request.
// The kernels are offered the plan in this order: k_query_staged, k_query_cols,
// k_query_slots, else k_query_fast; a plan the fast path declines is Generic.
inline void select_kernel(TablePlan& t, size_t img_bytes, size_t generic_lds, int generic_bpc, int n_cu,
                          const TableSwitches& sw) {
    const int nf = t.nf, ns = t.ns, N = t.N;
    TableSel& s = t.sel;
    s.lds_bytes = generic_lds;
    s.blocks_per_cu = generic_bpc;
    // fast path eligibility: N % 4 == 0, lanes per query a power of two <= 64,
    // <= kFastObs observed parents per factor
    bool fast = t.vec == 4 && nf * kFastObs <= kFastPtrs;
    t.recs.assign(nf, FastRec{});
    for (int f = 0; f < nf && fast; ++f) {
        FastRec& r = t.recs[f];
        r.table_off = t.fac[f].table_off;
        for (int p = 0; p < t.fac[f].n_parents; ++p) {
            const int sl = t.fac[f].ev_slot[p];
            if (sl < 0) continue;
            if (r.n_obs == kFastObs) { fast = false; break; }
            r.card[r.n_obs] = t.fac[f].parent_card[p];
            r.dom_off[r.n_obs] = t.slots[sl].dom_off;
            r.slot[r.n_obs] = sl;
            t.fast_slot[f * kFastObs + r.n_obs] = sl;
            ++r.n_obs;
        }
    }
    const FastLanes fl = fast ? fast_lanes(N, sw.fast_vpl) : FastLanes{};
    if (fl.vpl == 0) return;
    const size_t side = fast_side_bytes(nf, fl.lanes);
    if (s.use_lds && img_bytes + side > (size_t)kLdsBudget) return;  // keep one LDS mode per plan
    // global tables: the LDS-copied small tables + the records + the side buffers must fit
    if (!s.use_lds && (size_t)t.lds_tab_floats * 4 + (size_t)nf * kRecFloats * 4 + side > (size_t)kLdsBudget) return;

    const bool paired = t.paired_layout && fl.vpl == 2 && s.use_lds;
    s.kernel = paired ? TableKernel::PairedFast : TableKernel::Fast;
    s.vpl = fl.vpl;
    s.lanes = fl.lanes;
    s.ptrs = nf * kFastObs <= kFastPtrsSmall ? kFastPtrsSmall : kFastPtrs;
    const size_t fast_bytes = fast_lds_bytes(s.use_lds, img_bytes, t.lds_tab_floats, nf, fl.lanes);
    s.lds_bytes = fast_bytes;
    const size_t st_bytes = staged_lds_bytes(img_bytes, nf - t.prefix);
    if (paired && (nf - t.prefix) * kFastObs <= kFastPtrsSmall && st_bytes <= (size_t)kLdsBudget && !sw.no_staged) {
        s.kernel = TableKernel::Staged;
        s.ptrs = kFastPtrsSmall;
        s.lds_bytes = (st_bytes + 15) & ~size_t(15);
    }
    // column-staged kernel (k_query_cols): non-paired plans of <= 2
    // lanes per query (N <= 16) whose slot indices fit int16 and whose
    // per-slot index buffer fits LDS.  With more lanes per query every
    // lane re-forms every factor's offset: the configs[4] grid (L = 8)
    // ran 459 -> 534 us at 262 144 queries (profiles/r04_cols_ab.json)
    if (s.kernel == TableKernel::Fast && fl.lanes <= 2 && ns <= kFastPtrsSmall && nf <= kWave && !sw.no_cols) {
        const size_t cb = cols_lds_bytes(s.use_lds, img_bytes, t.lds_tab_floats, nf, ns, N, fl.lanes);
        if (col_records(t.recs, t.slots, t.RS, s.use_lds, t.lds_tab_mask, t.crec) && cb <= (size_t)kLdsBudget) {
            s.kernel = TableKernel::Cols;
            s.cols_chunk = (ns + fl.lanes - 1) / fl.lanes <= 16 ? 16 : 40;
            s.lds_bytes = cb;
        }
    }
    // slot-indexed kernel (k_query_slots): global-table plans of >= 4 lanes
    // per query (the configs[4] grid) -- the slots' evidence loaded once per
    // query instead of kFastObs loads per factor
    if (s.kernel == TableKernel::Fast && !s.use_lds && fl.lanes > 2 && ns <= kFastPtrsSmall && nf <= 128 &&
        !sw.no_slots) {
        bool ok = col_records(t.recs, t.slots, t.RS, false, t.lds_tab_mask, t.crec);
        // the offset (table base + row x RS) must fit an int
        for (int f = 0; f < nf; ++f)
            ok = ok && (long long)t.recs[f].table_off + (long long)t.fac[f].rows * t.RS < (1LL << 31);
        const size_t sb = slots_lds_bytes(t.lds_tab_floats, ns, nf, kQueryThreads / fl.lanes);
        if (ok && sb <= (size_t)kLdsBudget) {
            s.kernel = TableKernel::Slots;
            s.lds_bytes = sb;
        }
    }
    // (a staged plan's grid is still sized by k_query_fast's request, as it always was)
    const size_t grid_bytes = s.kernel == TableKernel::Staged ? fast_bytes : s.lds_bytes;
    s.blocks_per_cu = 2 * grid_bytes <= (size_t)kLdsBudget ? 2 : 1;
    if (s.kernel == TableKernel::Slots && sw.slots_bpc) s.blocks_per_cu = sw.slots_bpc == 2 ? 2 : 1;
    s.max_slots = std::min(n_cu * s.blocks_per_cu, kMaxSlots);
    s.fused2 = (s.kernel == TableKernel::Slots || s.kernel == TableKernel::Cols) && CBN_SLOTS_FUSED2;
    t.fused_candidate = !sw.no_fused;
}

}  // namespace table_plan_detail

// The plan of `factors` at N = n_samples on a device of n_cu CUs.
inline TablePlan plan_table(const cbn_factor_desc* factors, int nf, int n_samples, int n_cu, const TableSwitches& sw) {
    using namespace table_plan_detail;
    TablePlan t;
    for (int& sl : t.fast_slot) sl = -1;
    const int N = n_samples;
    t.nf = nf;
    t.N = N;
    t.vec = (N % 4 == 0) ? 4 : 1;
    t.L = N / t.vec;
    if (t.L > kQueryThreads) return fail(t, CBN_E_LIMIT, "N_max %d too large for one block row", N);
    // Table rows: in LDS, +16 B per row so consecutive rows start 4 banks apart;
    // an image that cannot fit LDS is read from L2/HBM, where the pad would make
    // every row straddle one more cache line: unpadded rows, 128-B aligned tables.
    long long total_rows = 0, class_rows[2] = {0, 0};
    for (int f = 0; f < nf; ++f) {
        total_rows += observed_rows(factors[f]);
        class_rows[f & 1] += observed_rows(factors[f]);
    }
    t.global_tables = t.vec == 4 && total_rows * (N + 4) * 4 > (long long)kLdsBudget;
    // Paired layout (N = 32, tables in LDS, 8 columns per lane): factor f's rows
    // sit in bank half (f & 1) of 256-B super-rows -- even factors in banks 0-31,
    // odd factors in banks 32-63, each class packed from super-row 0.  The fast
    // kernel then reads the two factors of a pair (and the two halves of a row)
    // in an order that gives the four queries of every ds_read_b128 lane group
    // four disjoint 16-bank quarters: conflict-free row gathers (the padded
    // layout's random rows collide ~2x, profiles/r02_lds_pmc.txt).
    const bool paired = t.paired_layout =
        t.vec == 4 && N == 32 && !t.global_tables && sw.fast_vpl >= 2 && !sw.no_paired &&
        std::max(class_rows[0], class_rows[1]) * 64 * 4 <= (long long)kLdsBudget * 3 / 4;
    // leading 1-row factors (roots / unobserved-parent factors) fold into the
    // first multi-row factor (k_merge_prefix); the staged kernel skips them
    if (paired && !sw.no_prefix)
        while (t.prefix < nf - 1 && t.prefix < 8 && observed_rows(factors[t.prefix]) == 1) ++t.prefix;
    const int prefix = t.prefix;
    const int RS = t.RS = paired ? 64 : t.vec == 4 && !t.global_tables ? N + 4 : N;
    const long long talign = t.global_tables ? 32 : 4;
    std::vector<long long> pre_off(nf, -1);
    if (t.global_tables && nf <= 128 && !sw.no_lds_split) split_small_tables(factors, nf, N, RS, talign, sw, pre_off, t);

    long long class_start[2] = {0, 0};
    t.fac.resize(nf);
    t.slot_dom.assign(CBN_MAX_EVIDENCE, nullptr);
    std::vector<int> slot_card(CBN_MAX_EVIDENCE, 0);
    int ns = 0;
    long long off = t.lds_tab_floats;  // after the LDS-copied small tables (global-table plans)
    for (int f = 0; f < nf; ++f) {
        const cbn_factor_desc& h = factors[f];
        DevFactor& d = t.fac[f];
        memset(&d, 0, sizeof(d));
        if (h.kind < CBN_FACTOR_SCALAR || h.kind > CBN_FACTOR_QUERY)
            return fail(t, CBN_E_ARG, "factor %d: bad kind %d", f, h.kind);
        if (h.n_parents < 0 || h.n_parents > kMaxP)
            return fail(t, CBN_E_LIMIT, "factor %d: %d parents > %d", f, h.n_parents, kMaxP);
        if ((h.kind == CBN_FACTOR_SCALAR) != (h.n_parents == 0))
            return fail(t, CBN_E_ARG, "factor %d: SCALAR iff root", f);
        if (!h.cpd || !h.node_sample_idx || h.node_card <= 0)
            return fail(t, CBN_E_ARG, "factor %d: missing cpd/node samples", f);
        d.kind = h.kind;
        d.n_parents = h.n_parents;
        d.node_card = h.node_card;
        d.cpd = h.cpd;
        d.node_sample_idx = h.node_sample_idx;
        d.parent_sample_idx = h.parent_sample_idx;
        long long stride = h.node_card, rows = 1, F = 1;
        for (int p = h.n_parents - 1; p >= 0; --p) {
            if (h.parent_card[p] <= 0) return fail(t, CBN_E_ARG, "factor %d: parent %d card", f, p);
            d.parent_card[p] = h.parent_card[p];
            d.ev_slot[p] = h.parent_ev_slot[p];
            d.cpd_stride[p] = (int)stride;
            stride *= h.parent_card[p];
            if (stride >= (1LL << 31)) return fail(t, CBN_E_LIMIT, "factor %d: CPD too large", f);
            const int sl = h.parent_ev_slot[p];
            if (sl >= 0) {
                if (sl >= CBN_MAX_EVIDENCE || !h.parent_domain[p])
                    return fail(t, CBN_E_ARG, "factor %d: bad evidence slot/domain", f);
                if (!t.slot_dom[sl]) {
                    t.slot_dom[sl] = h.parent_domain[p];
                    slot_card[sl] = h.parent_card[p];
                } else if (slot_card[sl] != h.parent_card[p]) {
                    return fail(t, CBN_E_ARG, "evidence slot %d used with different domains", sl);
                }
                ns = std::max(ns, sl + 1);
                rows *= h.parent_card[p];
            } else {
                if (!h.parent_sample_idx) return fail(t, CBN_E_ARG, "factor %d: free parent without samples", f);
                F *= N;
                if (F >= (1LL << 31)) return fail(t, CBN_E_LIMIT, "factor %d: too many free combos", f);
                d.n_free++;
            }
        }
        if ((h.kind == CBN_FACTOR_QUERY) != (rows > 1 || d.n_parents - d.n_free > 0))
            return fail(t, CBN_E_ARG, "factor %d: QUERY iff some parent observed", f);
        if (rows * (long long)RS >= (1LL << 30)) return fail(t, CBN_E_LIMIT, "factor %d: table too large", f);
        d.rows = (int)rows;
        d.free_combos = (int)F;
        d.n_entries = (int)(rows * N);
        const long long F_eff = h.kind == CBN_FACTOR_SCALAR ? N : F;
        d.wave_mode = F_eff >= kWave ? 1 : 0;
        if (paired) {
            // bank half by the index the staged kernel sees (prefix factors: half 0, never read there)
            const int c = f < prefix ? 0 : (f - prefix) & 1;
            d.table_off = (int)(class_start[c] * 64 + c * 32);
            class_start[c] += rows;
            off = std::max(class_start[0], class_start[1]) * 64;
        } else if (pre_off[f] >= 0) {
            if (pre_off[f] + rows * RS > t.lds_tab_floats) return fail(t, CBN_E_ARG, "factor %d: table size changed", f);
            d.table_off = (int)pre_off[f];
        } else {
            d.table_off = (int)off;
            off += (rows * RS + talign - 1) & ~(talign - 1);
        }
    }
    for (int sl = 0; sl < ns; ++sl)
        if (!t.slot_dom[sl]) return fail(t, CBN_E_ARG, "evidence slot %d is not used by any factor", sl);
    t.ns = ns;
    // paired layout: a zero super-row (values outside a domain) and a ones
    // super-row (padding slots) after the tables, both bank halves each
    t.zero_off = paired ? (int)off : -1;
    if (paired) off += 128;
    t.table_floats = (int)off;
    t.slots.assign(ns, QSlot{});
    for (int sl = 0; sl < ns; ++sl) {
        t.slots[sl].dom_off = (int)off;
        t.slots[sl].card = slot_card[sl];
        off += (slot_card[sl] + 3) & ~3LL;
    }
    t.rec_off = (int)off;  // FastRec array (fast path), copied to LDS with the tables
    off += (long long)nf * kRecFloats;
    off += (long long)ns * 4;  // QSlot array right after it (k_query_cols: one LDS-DMA for both)
    if (off >= (1LL << 30)) return fail(t, CBN_E_LIMIT, "plan image too large");
    t.image_floats = (int)off;
    for (int i = 0; i <= prefix && i < 9; ++i) t.prefix_offs[i] = t.fac[i].table_off;
    t.prefix_rows = prefix > 0 ? t.fac[prefix].rows : 0;

    // dynamic LDS of k_query: [image (if use_lds)] [factor records] [slots] [CH x (ns + nf) ints] [wave maxima]
    const size_t fixed = (size_t)nf * kFqInts * 4 + (size_t)ns * sizeof(QSlot) + (kQueryThreads / kWave) * 4 +
                         (size_t)CBN_MAX_EVIDENCE * sizeof(void*) + 64;
    const size_t per_q = (size_t)(ns + nf) * 4;
    const size_t img_bytes = (size_t)off * 4;
    auto chunk_for = [&](size_t avail) -> int {
        if (avail <= fixed) return 0;
        return (int)std::min<size_t>((avail - fixed) / per_q, 1024);
    };
    int ch = t.global_tables ? 0 : chunk_for(kLdsBudget > img_bytes ? kLdsBudget - img_bytes : 0);
    t.sel.use_lds = ch >= 64;  // (a global-table layout stays in L2/HBM even if the unpadded image would fit)
    if (!t.sel.use_lds) ch = chunk_for(kLdsBudget);
    if (ch < 1) return fail(t, CBN_E_LIMIT, "plan needs more LDS than a CU has (nf=%d, ns=%d)", nf, ns);
    t.CH = ch;
    const size_t generic_lds = ((t.sel.use_lds ? img_bytes : 0) + fixed + (size_t)ch * per_q + 15) & ~size_t(15);

    for (int f = 0; f < nf; ++f) {
        const DevFactor& d = t.fac[f];
        t.build.push_back({f, t.build_units});
        t.n_build = f + 1;
        t.build_units += d.wave_mode ? d.n_entries : (d.n_entries + kWave - 1) / kWave;
    }
    select_kernel(t, img_bytes, generic_lds, 2 * generic_lds <= (size_t)kLdsBudget ? 2 : 1, n_cu, sw);
    if (t.sel.kernel != TableKernel::Staged) {
        // the merge is only valid for the staged kernel (the others multiply every
        // factor): a non-staged plan with a paired layout keeps its tables as built
        t.prefix = 0;
        t.prefix_rows = 0;
    }
    return t;
}

}  // namespace table
}  // namespace cbn

#endif  // CBN_TABLE_PLAN_H
