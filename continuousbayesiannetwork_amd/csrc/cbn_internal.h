// cbn_internal.h -- internal layout shared by the translation units of
// libcbn_amd.so (cbn_infer.hip: discrete/table path + C ABI plumbing;
// cbn_param.hip: parametric CPD path).  Not part of the public C ABI
// (include/cbn_amd.h).
#ifndef CBN_INTERNAL_H
#define CBN_INTERNAL_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/cbn_amd.h"
#include "cbn_table_plan.h"  // kWave, kLdsBudget, kMaxSlots, the table plans' records and TableSel

namespace cbn {

// plan sync buffer (unsigned words): line 0 = timeout flag (word 2) and the
// max/raw passes' max staging + arrival counter (words 4-5); from word
// kSlotWordOff, the fused barrier's slots: block b publishes {epoch, max} in
// its own 8-byte slot and every block polls all of them.
constexpr int kSyncLine = 32;
constexpr int kHostStatusWordOff = 8;  // words 8-9 of line 0: device address of the plan's host-mapped status
constexpr int kOneWordOff = 12;  // word 12 of line 0 (table plans): the bits of 1.0f (cbn_plan_run_argmax)
constexpr int kSlotWordOff = kSyncLine;
// then the max/raw passes' per-block maxima (one word per block; the
// consumer -- write pass, k_scale, k_reduce_max, or RCCL -- reduces them: no
// same-address fan-in, ~12 ns per arrival serialised at the memory side)
constexpr int kMaxWordOff = kSlotWordOff + 2 * kMaxSlots;
constexpr int kSyncWords = kMaxWordOff + kMaxSlots;

struct ParamPlan;  // cbn_param.hip
struct DirectPlan;  // cbn_direct.hip

int set_err(int code, const char* fmt, ...);
// getenv(name) when the library was loaded with CBN_DIAG=1, else nullptr
// (diagnostic kernel-selection switches; cbn_infer.hip)
const char* diag_env(const char* name);
int num_cu();

// out[i] /= max(words[0, n_words)) in place on `s`; block 0 also stores that
// max word in *pub when pub is non-null.
int launch_scale(float* out, long long n, const unsigned* words, int n_words, unsigned* pub, hipStream_t s);

// parametric plans (cbn_param.hip)
int param_run(cbn_plan* plan, int64_t n_queries, const float* const* evidence, int32_t n_evidence,
              uint32_t* max_bits, float* out, int32_t flags, hipStream_t s);
void param_destroy(ParamPlan* pp);
int param_max_words(const ParamPlan* pp);

// direct plans (cbn_direct.hip)
int direct_run(cbn_plan* plan, int64_t n_queries, const float* const* evidence, int32_t n_evidence,
               uint32_t* max_bits, float* out, int32_t flags, hipStream_t s);
int direct_build_consts(DirectPlan* dp, hipStream_t s);
void direct_destroy(DirectPlan* dp);
int direct_max_words(const DirectPlan* dp);

}  // namespace cbn

// A plan: the table planner's layout and selection (cbn_table_plan.h; unused
// by parametric and direct plans, which keep nf / ns / N in their own structs)
// and the device buffers made from it.
struct cbn_plan : cbn::table::TableLayout {
    cbn::DevFactor* d_fac = nullptr;
    int* d_crec = nullptr;       // k_query_cols / k_query_slots: per-factor scalar records (ColRec)
    cbn::QSlot* d_slots = nullptr;
    cbn::BuildItem* d_build = nullptr;
    float* d_image = nullptr;    // [tables | observed-column domains | records], 16-B padded pieces
    unsigned* d_sync = nullptr;  // kSyncWords words: status line, fused-barrier slots, per-block maxima (above)
    static constexpr int kRing = 512;
    hipEvent_t ev[kRing][3] = {};  // timing ring (created on first timed call)
    int ev_n = 0;
    unsigned* h_status = nullptr;  // host-mapped: 1 after a fused launch timed out (reported by the next run)
    unsigned fused_epoch = 0;    // tag of the published {epoch, max} granule
    bool fused_ok = false;       // one block per CU fits (LDS/VGPR) -> grid barrier is safe
    cbn::ParamPlan* param = nullptr;  // parametric-CPD plan (cbn_plan_create_param); table fields unused
    cbn::DirectPlan* direct = nullptr;  // direct plan (cbn_plan_create_direct); table fields unused
};

#endif  // CBN_INTERNAL_H
