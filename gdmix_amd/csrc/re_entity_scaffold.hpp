// re_entity_scaffold.hpp — what the per-entity solves that route by LDS footprint share around their kernels: the elastic net and the
// box solve (re_owlqn.hip), TRON (re_tron.hip), and the slot count of the plain solve (re_api.hip).
//
//   device   solver_lds_bytes        the one LDS footprint of a wavefront kernel: the route kernel, the launch and the carve-up use it
//            (The entity preamble, the LDS staging, the global view and the epilogue stay each kernel's own text. As shared inline
//            functions they changed the instructions of every kernel that used them: a function that takes the kernel's BatchDev by
//            reference costs its pointer loads their no-clobber marks, and a shared epilogue reorders TRON's and OWL-QN's stores.)
//   host     launch_lds_route (re_lds_route_kernel: three lists by that footprint, for the solves without the size-class table, and a
//            fourth for a solve with a four-entities-per-wavefront kernel: TRON's rows),
//            block_slots, lists_scratch_bytes, begin_lists_solve, solve_three_lists
#pragma once
#include <math.h>

#include "re_internal.hpp"

namespace gdmix {

// ---------------------------------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------------------------------
// LDS bytes a wavefront kernel needs for an entity when its solver keeps p_vectors coefficient vectors, n_vectors sample vectors and m
// history pairs: the plain kernel's footprint (five and one) and the others. Must match the kernels' carve-ups.
__host__ __device__ inline size_t solver_lds_bytes(int p_vectors, int n_vectors, int p, int n, int nnz, int d, int m, bool has_w) {
  return (wave_lds_bytes(p, n, nnz, d, m, has_w) + (size_t)(p_vectors - 5) * 8 * p + (size_t)(n_vectors - 1) * 8 * n + 15) & ~(size_t)15;
}

// ---------------------------------------------------------------------------------------------------
// routing by LDS footprint, for the solves that do not use the size-class table
// ---------------------------------------------------------------------------------------------------
// words of the batch's count record (gdmix_re_packed::class_count) these solves use: the two counts, then how the wavefront kernel's
// entities split into its two launches. A solve may keep a verdict of its own in the words behind them, read back with the counts.
enum { LDS_COUNT_WAVE = 0, LDS_COUNT_BLOCK = 1, LDS_COUNT_WAVE_LARGE = 2, LDS_MAX_WAVE_LDS = 3, LDS_COUNT_WAVE_SMALL = 4, LDS_COUNT_WORDS = 5,
       LDS_READBACK_WORDS = 8 };
// A solve with a row kernel (four entities per wavefront: M.launch_rows) keeps its words there: how many of the small entities are the
// row kernel's, their largest footprint, and the ticket counter of the others (word 4 counts both kinds, so it cannot hand out the
// places at the front of the small list: ROWS_REST_TICKET ends as word 4 - ROWS_COUNT). Written only under a row limit > 0.
enum { ROWS_COUNT = 5, ROWS_MAX_LDS = 6, ROWS_REST_TICKET = 7 };
static_assert(ROWS_COUNT == LDS_COUNT_WORDS && ROWS_REST_TICKET < LDS_READBACK_WORDS, "the row words ride behind the routing counts");
// The wavefront kernel's workgroup is one wavefront and its LDS is what bounds the wavefronts a CU holds, so its entities are launched
// in two parts: those within WAVE_SMALL_LDS bytes with that much LDS (eight one-wavefront workgroups per CU of 160 KB; a mean C2 entity
// of 16 samples and ~64 coefficients needs 15 KB under OWL-QN, 10 KB of them history, and about 6 KB under TRON), the others with the
// largest footprint among them.
constexpr int WAVE_SMALL_LDS = 20 * 1024;

// re_lds_route_kernel on stream s: the three lists of batch b and their counts (the kernel is in re_owlqn.hip, the first unit that used
// it: a kernel defined in a header would be defined in every unit). row_lds > 0: the small entities within row_lds bytes (<= small_lds)
// are a fourth list, the back end of cls_tmp read from its end (ROWS_COUNT of them); they count in words 0 and 4 like every small entity.
hipError_t launch_lds_route(const gdmix_re_packed* b, int ic, int p_vectors, int n_vectors, int m, int wave_lds_limit, int small_lds, int row_lds,
                            hipStream_t s);

// ---------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------
// scratch slots of a workgroup kernel whose slot is slot_doubles long: enough workgroups to fill the chip a few times over, bounded
// to ~4 GiB of scratch, at least 8, at most one per entity
inline int block_slots(size_t slot_doubles, int64_t E) {
  const size_t bytes = slot_doubles * 8;
  size_t slots = 1024;
  const size_t by_budget = ((size_t)4 << 30) / (bytes ? bytes : 1);
  if (slots > by_budget) slots = by_budget;
  if (slots < 8) slots = 8;
  if ((int64_t)slots > E) slots = (size_t)(E > 0 ? E : 1);
  return (int)slots;
}

// What solve_three_lists takes of a solve, a small object `M` of the entry point's:
//   M.family                                         "re_owlqn" | "re_tron": the kernels' names in messages
//   M.p_vectors, M.n_vectors, M.m                    the footprint (solver_lds_bytes)
//   M.slot_doubles(b, opts)                          doubles of global scratch one slot of its workgroup kernel needs
//   M.launch_wave(list, count, lds_bytes, stream)    its wavefront kernel on list[0, count)
//   M.launch_block(last, count, scratch, slot_doubles, slots, stream)   its workgroup kernel on order[last - count + 1, last], read from the end
//   M.verdict(hc)                                    what it checks in the count record besides the routing (nothing, for most)
//   M.launch_rows(list, count, row_bytes, stream)    OPTIONAL: its four-entities-per-wavefront kernel on list[0, count), row_bytes of LDS a
//                                                    row. A solve without one has no row list (has_launch_rows: the route's row limit is 0).
template <class Method, class = void>
struct has_launch_rows : std::false_type {};
template <class Method>
struct has_launch_rows<Method, std::void_t<decltype(&Method::launch_rows)>> : std::true_type {};

// device scratch such a solve needs beyond the pack workspace: its own slots, or the plain solve's (the entry points forward to it
// for l1 == 0 / no bounds, and FULL variances are its kernels)
template <class Method>
inline size_t lists_scratch_bytes(const gdmix_re_packed* batch, const gdmix_re_opts* opts) {
  if (!batch || !opts || batch->E == 0) return 0;
  const size_t slot_doubles = Method::slot_doubles(batch, opts);
  const size_t own = (size_t)block_slots(slot_doubles, batch->E) * slot_doubles * 8;
  const size_t plain = gdmix_re_solve_scratch_bytes(batch, opts);
  return own > plain ? own : plain;
}

// An entry point behind its argument checks, up to the zeroed count record. *empty: a batch without entities, nothing to do.
inline int begin_lists_solve(gdmix_re_ctx* ctx, const gdmix_re_packed* b, void* stream, const char* who, bool* empty) {
  *empty = b->E == 0;
  if (*empty) return GDMIX_RE_OK;
  if (b->E > 0x7fffffffLL) { set_error("%s: 2^31 entities or more", who); return GDMIX_RE_ERANGE; }
  gdmix_ctx_impl* const ci = &ctx->impl;
  HIP_TRY(hipSetDevice(ci->device));
  for (int c = 0; c < GDMIX_RE_NUM_CLASSES; ++c) ci->ev_used[c] = false;
  HIP_TRY(hipMemsetAsync(b->class_count, 0, sizeof(ClassCounts), static_cast<hipStream_t>(stream)));
  return GDMIX_RE_OK;
}

// what the kernels of such a solve take, whichever list they run
struct ListsArgs {
  BatchDev B;
  OutDev O;
  SolveParams P;
  const double* theta0;
};
inline ListsArgs lists_args(const gdmix_re_packed* b, const gdmix_re_opts* opts, const double* theta0, const gdmix_re_result* out) {
  ListsArgs a{batch_dev(b), OutDev{out->theta, out->theta_thr, opts->variance_mode == GDMIX_RE_VAR_SIMPLE ? out->variance : nullptr, out->fval,
                                   out->gnorm, out->nit, out->nfev, out->status},
              solve_params(*opts), theta0};
  a.P.sum_loss = 0;
  return a;
}

// The solve of a batch, behind begin_lists_solve: route, one read-back (the list lengths, and the verdict of a check queued by the
// caller on the stream before this), the launches, FULL variances. `who` names the entry point in messages.
template <class Method>
inline int solve_three_lists(gdmix_re_ctx* ctx, const gdmix_re_packed* b, const gdmix_re_opts* opts, const Method& M, const gdmix_re_result* out,
                             void* stream, const char* who) {
  gdmix_ctx_impl* const ci = &ctx->impl;
  hipStream_t const s = static_cast<hipStream_t>(stream);

  // the lists and their counts
  const int small_lds = ci->wave_lds_limit < WAVE_SMALL_LDS ? ci->wave_lds_limit : WAVE_SMALL_LDS;
  int row_lds = 0;   // entities within it go four to a wavefront, where the solve has such a kernel
  if constexpr (has_launch_rows<Method>::value) row_lds = ci->tron_row_lds_limit < small_lds ? ci->tron_row_lds_limit : small_lds;
  HIP_TRY(launch_lds_route(b, opts->has_intercept ? 1 : 0, M.p_vectors, M.n_vectors, M.m, ci->wave_lds_limit, small_lds, row_lds, s));
  int32_t* const hc = ci->host_pinned + COUNTS_READBACK_WORDS;
  HIP_TRY(fetch_small(ci, 0, b->class_count, LDS_READBACK_WORDS * sizeof(int32_t), hc, s));
  if (const int rc = M.verdict(hc); rc != GDMIX_RE_OK) return rc;
  const int n_wave = hc[LDS_COUNT_WAVE], n_block = hc[LDS_COUNT_BLOCK], wave_lds = hc[LDS_MAX_WAVE_LDS];
  const int n_small = hc[LDS_COUNT_WAVE_SMALL], n_large = hc[LDS_COUNT_WAVE_LARGE];
  if (n_small < 0 || n_large < 0 || n_block < 0 || n_small + n_large != n_wave || (int64_t)n_wave + n_block != b->E || wave_lds < 0 || wave_lds > 65536) {
    set_error("%s: the routing counted %d + %d of %lld entities (LDS %d)", who, n_wave, n_block, (long long)b->E, wave_lds);
    return GDMIX_RE_EHIP;
  }
  const int n_rows = row_lds > 0 ? hc[ROWS_COUNT] : 0, row_bytes = row_lds > 0 ? hc[ROWS_MAX_LDS] : 0;
  if (n_rows < 0 || n_rows > n_small || row_bytes < 0 || row_bytes > row_lds || (row_bytes & 15)) {
    set_error("%s: the routing counted %d row entities of %d small ones (LDS %d of %d)", who, n_rows, n_small, row_bytes, row_lds);
    return GDMIX_RE_EHIP;
  }
  const int n_rest = n_small - n_rows;   // what the small wavefront launch is left with

  // scratch slots of the workgroup kernel: the context's scratch or the batch's, as many slots as fit (at least one)
  double* scratch = nullptr;
  size_t slot_doubles = 0;
  int slots = 0;
  if (n_block > 0) {
    slot_doubles = M.slot_doubles(b, opts);
    slots = block_slots(slot_doubles, b->E);
    size_t avail = ci->scratch ? ci->scratch_bytes : 0;
    void* base = ci->scratch;
    if (b->scratch_bytes > avail) { avail = b->scratch_bytes; base = b->scratch; }
    if ((size_t)slots * slot_doubles * 8 > avail) slots = (int)(avail / (slot_doubles * 8));
    if (slots < 1) {
      set_error("%d entities need a scratch slot: provide >= %zu bytes via gdmix_re_set_scratch", n_block, slot_doubles * 8);
      return GDMIX_RE_ENOMEM;
    }
    scratch = static_cast<double*>(base);
  }

  // the launches side by side where the context has side streams; every way out joins them back (SideJoin)
  {
    SideJoin side_join{ci, s};
    // the lists that hold entities, the longest-running first: each on a queue of its own while there are side streams
    hipStream_t q[4] = {s, s, s, s};
    const int live = (n_block > 0) + (n_large > 0) + (n_rest > 0) + (n_rows > 0);
    if (live > 1 && ci->n_side > 0) {
      HIP_TRY(hipEventRecord(ci->side_fork, s));
      int k = 0;
      if (n_block > 0) { HIP_TRY(side_join.use(k)); q[0] = ci->side[k]; k = k + 1 < ci->n_side ? k + 1 : k; }
      if (n_large > 0 && n_small > 0) { HIP_TRY(side_join.use(k)); q[1] = ci->side[k]; k = k + 1 < ci->n_side ? k + 1 : k; }
      if (n_rows > 0 && n_rest > 0) { HIP_TRY(side_join.use(k)); q[3] = ci->side[k]; }
    }
    hipError_t rc = M.launch_block(b->E - 1, n_block, scratch, slot_doubles, slots, q[0]);
    if (rc != hipSuccess) { set_error("launch of %s_block_kernel failed: %s", M.family, hipGetErrorString(rc)); return GDMIX_RE_EHIP; }
    rc = M.launch_wave(b->order, n_large, wave_lds, q[1]);
    if (rc == hipSuccess) rc = M.launch_wave(b->cls_tmp, n_rest, small_lds, q[2]);
    if (rc != hipSuccess) { set_error("launch of %s_wave_kernel failed: %s", M.family, hipGetErrorString(rc)); return GDMIX_RE_EHIP; }
    if constexpr (has_launch_rows<Method>::value) {   // the row list is the back end of cls_tmp
      rc = M.launch_rows(b->cls_tmp + (b->E - n_rows), n_rows, row_bytes, q[3]);
      if (rc != hipSuccess) { set_error("launch of %s_rows_kernel failed: %s", M.family, hipGetErrorString(rc)); return GDMIX_RE_EHIP; }
    }
  }
  if (opts->variance_mode == GDMIX_RE_VAR_FULL) {   // of the smooth part at the returned theta, with the same l2 (joins a deferred compaction itself)
    const int rc = gdmix_re_variance_full(ctx, b, opts, out->theta, out->variance, stream);
    if (rc != GDMIX_RE_OK) return rc;
  }
  HIP_TRY(join_unique(ci, s));
  return GDMIX_RE_OK;
}

}  // namespace gdmix
