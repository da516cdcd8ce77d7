// re_owlqn.hip — the random effect's two projected quasi-Newton solves, per entity on the device: the elastic net by OWL-QN
// (include/gdmix_re.h, "elastic net"; ReOwlRule) and the box-constrained fit by projected L-BFGS ("box constraints"; ReBoxRule). The
// two kernel bodies take the rule, and with it the footprint, as a parameter.
//
//   re_box_check_kernel        the caller's bound tables and the batch's feature ids, its verdict in the count record
//   re_lds_route_kernel        an entity goes to the wavefront kernel iff its LDS footprint under the solver is within the context's
//                              wave_lds_limit, else to the workgroup kernel: two lists in the batch's `order`, two counts
//                              (the wavefront kernel's small entities apart, in cls_tmp: they are launched with less LDS); TRON's too
//   (re_entity_scaffold.hpp: the footprint, the count words and the host driver, solve_three_lists, shared with TRON)
//   re_owlqn_wave_kernel       ONE WAVEFRONT PER ENTITY: the entity's block and all solver state live in LDS for the whole solve
//   re_owlqn_block_kernel      one workgroup per entity, state in a global scratch slot per workgroup, X streamed, grid-stride
//   gdmix_re_solve_l1, gdmix_re_solve_l1_scratch_bytes, gdmix_re_solve_box, gdmix_re_solve_box_scratch_bytes
//
// The solve itself is owlqn_solve<LOSS, Rule> of re_owlqn.hpp; the evaluation, the reductions and the SIMPLE variance are those of the plain
// solve (re_solve_core.hpp). No kernel of the plain solve is touched, and the size-class table is not involved.
#include <math.h>

#include "re_entity_scaffold.hpp"
#include "re_owlqn.hpp"

namespace gdmix {

// doubles of global scratch one slot of the workgroup kernel needs: the rule's coefficient vectors | history | alpha rho | residuals
inline size_t owlqn_slot_doubles(int p_vectors, int64_t max_p, int64_t max_n, int m) {
  return (size_t)(p_vectors + 2 * m) * max_p + (size_t)2 * m + max_n + 8;
}

// the bounded solve's words of the count record, behind the routing's: the verdict of re_box_check_kernel, read back with the counts
enum { BOX_BAD_NAN = 5, BOX_BAD_ORDER = 6, BOX_BAD_ID = 7 };
static_assert(BOX_BAD_NAN == LDS_COUNT_WORDS && BOX_BAD_ID < LDS_READBACK_WORDS, "the verdict rides behind the routing counts");

// ---------------------------------------------------------------------------------------------------
// routing, for TRON too (launch_lds_route): an entity goes to the wavefront kernel iff its footprint is within the context's
// wave_lds_limit, else to the workgroup kernel. The wavefront kernel's large entities fill `order` from the front, the workgroup
// kernel's from the back; the wavefront kernel's small entities (WAVE_SMALL_LDS) are a list of their own in `small` (the batch's
// cls_tmp, solver-owned like `order`). Position inside a list is by ticket (per workgroup: LDS counters, then one global atomic per
// list): no entity's result depends on it. row_lds > 0 (TRON): the small entities within row_lds bytes are the row kernel's, a fourth
// list at the back end of `small`; they count in words 0 and 4 as the other small entities do, and in the row words behind them
// (re_entity_scaffold.hpp, ROWS_*), which the kernel leaves alone under row_lds == 0.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void re_lds_route_kernel(const int64_t* __restrict__ ent_row_ptr, const int64_t* __restrict__ ent_nnz_ptr,
                                                           const int64_t* __restrict__ ent_feat_ptr, int64_t E, int ic, bool has_w, int p_vectors,
                                                           int n_vectors, int m, int wave_lds_limit, int small_lds, int row_lds,
                                                           int32_t* __restrict__ order, int32_t* __restrict__ small, int32_t* __restrict__ counts) {
  // lists: 0 wavefront kernel, small; 1 workgroup kernel; 2 wavefront kernel, large; 3 row kernel (small too)
  __shared__ int32_t cnt[4], base[4], lds_max, row_max;
  for (int64_t start = (int64_t)blockIdx.x * blockDim.x; start < E; start += (int64_t)gridDim.x * blockDim.x) {
    if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
    if (threadIdx.x == 4) lds_max = 0;
    if (threadIdx.x == 5) row_max = 0;
    __syncthreads();
    const int64_t e = start + threadIdx.x;
    int which = -1, pos = 0;
    if (e < E) {
      const int n = (int)(ent_row_ptr[e + 1] - ent_row_ptr[e]);
      const int z = (int)(ent_nnz_ptr[e + 1] - ent_nnz_ptr[e]);
      const int d = (int)(ent_feat_ptr[e + 1] - ent_feat_ptr[e]);
      const size_t bytes = solver_lds_bytes(p_vectors, n_vectors, d + ic, n, z, d, m, has_w);
      which = bytes > (size_t)wave_lds_limit ? 1 : (bytes <= (size_t)small_lds ? (bytes <= (size_t)row_lds ? 3 : 0) : 2);
      pos = atomicAdd(&cnt[which], 1);
      if (which == 2) atomicMax(&lds_max, (int32_t)bytes);
      if (which == 3) atomicMax(&row_max, (int32_t)bytes);
    }
    __syncthreads();
    if (row_lds <= 0) {
      if (threadIdx.x == 0) base[0] = cnt[0] ? atomicAdd(&counts[LDS_COUNT_WAVE_SMALL], cnt[0]) : 0;
    } else {   // word 4 counts the row kernel's entities too: the others' places come from a ticket word of their own
      if (threadIdx.x == 0) base[0] = cnt[0] ? atomicAdd(&counts[ROWS_REST_TICKET], cnt[0]) : 0;
      if (threadIdx.x == 5) base[3] = cnt[3] ? atomicAdd(&counts[ROWS_COUNT], cnt[3]) : 0;
      if (threadIdx.x == 6 && cnt[0] + cnt[3] > 0) atomicAdd(&counts[LDS_COUNT_WAVE_SMALL], cnt[0] + cnt[3]);
      if (threadIdx.x == 7 && row_max > 0) atomicMax(&counts[ROWS_MAX_LDS], row_max);
    }
    if (threadIdx.x == 1) base[1] = cnt[1] ? atomicAdd(&counts[LDS_COUNT_BLOCK], cnt[1]) : 0;
    if (threadIdx.x == 2) base[2] = cnt[2] ? atomicAdd(&counts[LDS_COUNT_WAVE_LARGE], cnt[2]) : 0;
    if (threadIdx.x == 3 && cnt[0] + cnt[2] + cnt[3] > 0) atomicAdd(&counts[LDS_COUNT_WAVE], cnt[0] + cnt[2] + cnt[3]);
    if (threadIdx.x == 4 && lds_max > 0) atomicMax(&counts[LDS_MAX_WAVE_LDS], lds_max);
    __syncthreads();
    if (which == 0) small[base[0] + pos] = (int32_t)e;
    else if (which == 3) small[E - 1 - (base[3] + pos)] = (int32_t)e;
    else if (which == 2) order[base[2] + pos] = (int32_t)e;
    else if (which == 1) order[E - 1 - (base[1] + pos)] = (int32_t)e;
    __syncthreads();
  }
}

hipError_t launch_lds_route(const gdmix_re_packed* b, int ic, int p_vectors, int n_vectors, int m, int wave_lds_limit, int small_lds, int row_lds,
                            hipStream_t s) {
  hipLaunchKernelGGL(re_lds_route_kernel, dim3(grid_for(b->E, 256, 2048)), dim3(256), 0, s, b->ent_row_ptr, b->ent_nnz_ptr, b->ent_feat_ptr, b->E, ic,
                     b->weight != nullptr, p_vectors, n_vectors, m, wave_lds_limit, small_lds, row_lds, b->order, b->cls_tmp, b->class_count);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// shared epilogue: theta, thresholded theta, stats (what write_results of re_solve.hip writes for the plain solve)
// ---------------------------------------------------------------------------------------------------
// (a rule may keep a coefficient whatever the threshold: one whose box does not contain 0, so that the written model lies in the box too)
template <class G, class Ent>
__device__ __forceinline__ void owlqn_write_results(G& grp, const OutDev& O, const SolveParams& o, int64_t e, int64_t c0, int p, const Ent& r,
                                                    const QnWork& W, const SolveStats& st) {
  for (int j = grp.tid; j < p; j += grp.NT) {
    const double v = W.x[j];
    if (O.theta) O.theta[c0 + j] = v;
    if (O.theta_thr) O.theta_thr[c0 + j] = (fabs(v) <= o.threshold && !r.keeps(W, j)) ? 0.0 : v;
  }
  if (grp.tid == 0) {
    if (O.fval) O.fval[e] = st.f;
    if (O.gnorm) O.gnorm[e] = st.gnorm;
    if (O.nit) O.nit[e] = st.nit;
    if (O.nfev) O.nfev[e] = st.nfev;
    if (O.status) O.status[e] = st.status;
  }
}

// ---------------------------------------------------------------------------------------------------
// one wavefront per entity, everything LDS-resident: one batch of coalesced staging loads, then no HBM traffic until the results
// ---------------------------------------------------------------------------------------------------
template <int LOSS, class Rule>
__global__ __launch_bounds__(WAVE) void re_owlqn_wave_kernel(BatchDev B, OutDev O, SolveParams o, Rule R, const double* __restrict__ theta0,
                                                             const int32_t* __restrict__ list, int count) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x;
  if ((int)blockIdx.x >= count) return;
  const int64_t e = list[blockIdx.x];
  const int ic = o.has_intercept ? 1 : 0;
  const int64_t r0 = B.ent_row_ptr[e], z0 = B.ent_nnz_ptr[e], f0 = B.ent_feat_ptr[e];
  const int n = (int)(B.ent_row_ptr[e + 1] - r0);
  const int nnz = (int)(B.ent_nnz_ptr[e + 1] - z0);
  const int d = (int)(B.ent_feat_ptr[e + 1] - f0);
  const int p = d + ic;
  const int m = o.m;
  const int64_t c0 = f0 + e * ic;

  // carve-up: doubles first (8-byte aligned), then 4-byte arrays; must match solver_lds_bytes()
  QnWork W;
  double* dp = Rule::carve(W, reinterpret_cast<double*>(smem), (size_t)p);
  W.ws = dp; dp += (size_t)m * p;
  W.wy = dp; dp += (size_t)m * p;
  W.rs = dp; dp += n;
  W.alpha = dp; dp += m;
  W.rho = dp; dp += m;
  float* fp = reinterpret_cast<float*>(dp);
  float* s_csr_val = fp; fp += nnz;
  float* s_csc_val = fp; fp += nnz;
  float* s_y = fp; fp += n;
  float* s_o = fp; fp += n;
  float* s_w = nullptr;
  if (B.weight) { s_w = fp; fp += n; }
  int32_t* ip = reinterpret_cast<int32_t*>(fp);
  int32_t* s_csr_col = ip; ip += nnz;
  int32_t* s_csc_row = ip; ip += nnz;
  int32_t* s_row_ptr = ip; ip += n + 1;
  int32_t* s_col_ptr = ip; ip += d + 1;

  // stage the entity's block: every array is a contiguous slice of the packed batch -> coalesced reads
  for (int k = lane; k < nnz; k += WAVE) {
    s_csr_val[k] = B.csr_val[z0 + k];
    s_csr_col[k] = B.csr_col[z0 + k];
    s_csc_val[k] = B.csc_val[z0 + k];
    s_csc_row[k] = B.csc_row[z0 + k];
  }
  for (int i = lane; i < n; i += WAVE) {
    s_y[i] = B.y[r0 + i];
    s_o[i] = B.offset[r0 + i];
    if (s_w) s_w[i] = B.weight[r0 + i];
  }
  for (int i = lane; i <= n; i += WAVE) s_row_ptr[i] = B.row_ptr[r0 + e + i];
  for (int i = lane; i <= d; i += WAVE) s_col_ptr[i] = B.col_ptr[z0 + e + i];
  for (int j = lane; j < p; j += WAVE) W.xt[j] = R.stage(W, j, ic, f0, theta0 ? theta0[c0 + j] : 0.0);   // lane j mod 64 keeps coefficient j's bounds

  WaveGroup grp{lane};
  grp.sync();
  EntityView P{n, d, p, ic, s_row_ptr, s_csr_col, s_csr_val, s_col_ptr, s_csc_row, s_csc_val, s_y, s_o, s_w};
  SolveStats st;
  owlqn_solve<LOSS>(grp, P, o, R, W, st);
  owlqn_write_results(grp, O, o, e, c0, p, R.entity(n, 0), W, st);
  if (o.variance_mode == GDMIX_RE_VAR_SIMPLE && O.variance) {   // of the smooth part at the returned theta, a coefficient at 0 or at a bound included
    Work V{};
    V.x = W.x; V.rs = W.rs;
    variance_simple<false, LOSS>(grp, P, o, V, O.variance + c0);
  }
}

// ---------------------------------------------------------------------------------------------------
// one workgroup per entity, state in a global scratch slot, X streamed from HBM/L2. No workgroup waits for another.
// The list is read from its end: order[last - idx] (re_lds_route_kernel fills it from the back of `order`).
// ---------------------------------------------------------------------------------------------------
template <int LOSS, class Rule>
__global__ __launch_bounds__(WAVE* BLOCK_NW) void re_owlqn_block_kernel(BatchDev B, OutDev O, SolveParams o, Rule R, const double* __restrict__ theta0,
                                                                         int64_t last, int count, double* scratch, size_t slot_doubles, int64_t max_p) {
  __shared__ double red[2 * BLOCK_NW];
  const int ic = o.has_intercept ? 1 : 0;
  const int m = o.m;
  double* slot = scratch + (size_t)blockIdx.x * slot_doubles;
  for (int idx = blockIdx.x; idx < count; idx += gridDim.x) {
    const int64_t e = B.order[last - idx];
    const int64_t r0 = B.ent_row_ptr[e], z0 = B.ent_nnz_ptr[e], f0 = B.ent_feat_ptr[e];
    const int n = (int)(B.ent_row_ptr[e + 1] - r0);
    const int d = (int)(B.ent_feat_ptr[e + 1] - f0);
    const int p = d + ic;
    const int64_t c0 = f0 + e * ic;
    QnWork W;
    double* dp = Rule::carve(W, slot, (size_t)max_p);
    W.ws = dp; dp += (size_t)m * max_p;
    W.wy = dp; dp += (size_t)m * max_p;
    W.alpha = dp; dp += m;
    W.rho = dp; dp += m;
    W.rs = dp;
    BlockGroup<BLOCK_NW> grp{(int)threadIdx.x, red, 0};
    for (int j = grp.tid; j < p; j += grp.NT) W.xt[j] = R.stage(W, j, ic, f0, theta0 ? theta0[c0 + j] : 0.0);
    grp.sync();
    EntityView P{n, d, p, ic, B.row_ptr + r0 + e, B.csr_col + z0, B.csr_val + z0, B.col_ptr + z0 + e,
                 B.csc_row + z0, B.csc_val + z0, B.y + r0, B.offset + r0, B.weight ? B.weight + r0 : nullptr};
    SolveStats st;
    owlqn_solve<LOSS>(grp, P, o, R, W, st);
    owlqn_write_results(grp, O, o, e, c0, p, R.entity(n, 0), W, st);
    if (o.variance_mode == GDMIX_RE_VAR_SIMPLE && O.variance) {
      Work V{};
      V.x = W.x; V.rs = W.rs;
      variance_simple<false, LOSS>(grp, P, o, V, O.variance + c0);
    }
    grp.sync();   // the slot is reused by the next entity
  }
}

// ---------------------------------------------------------------------------------------------------
// the bounded solve's check of the caller's arrays: the two tables (a NaN bound, lo_j > hi_j) and the batch's feature ids against the
// tables' length. Every writer stores 1; the verdict travels with the routing counts (BOX_BAD_*).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void re_box_check_kernel(const double* __restrict__ lower, const double* __restrict__ upper, int64_t num_features,
                                                           const int32_t* __restrict__ unique_global, const int64_t* __restrict__ ent_feat_ptr, int64_t E,
                                                           int32_t* __restrict__ counts) {
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = first; j < num_features; j += step) {
    const double lo = lower ? lower[j] : -__builtin_inf(), hi = upper ? upper[j] : __builtin_inf();
    if (lo != lo || hi != hi) counts[BOX_BAD_NAN] = 1;
    else if (lo > hi) counts[BOX_BAD_ORDER] = 1;
  }
  const int64_t D = ent_feat_ptr[E];
  for (int64_t k = first; k < D; k += step) {
    const int32_t gid = unique_global[k];
    if (gid < 0 || (int64_t)gid >= num_features) counts[BOX_BAD_ID] = 1;
  }
}

// What a rule's solve checks in the count record besides the routing (nothing, for a rule without arrays of the caller's).
static int owlqn_verdict(const ReOwlRule&, const int32_t*) { return GDMIX_RE_OK; }
static int owlqn_verdict(const ReBoxRule&, const int32_t* hc) {
  if (hc[BOX_BAD_NAN]) { set_error("gdmix_re_solve_box: a bound is NaN"); return GDMIX_RE_EINVAL; }
  if (hc[BOX_BAD_ORDER]) { set_error("gdmix_re_solve_box: a lower bound is above its upper bound"); return GDMIX_RE_EINVAL; }
  if (hc[BOX_BAD_ID]) { set_error("gdmix_re_solve_box: num_features is not above the largest feature id of the batch"); return GDMIX_RE_EINVAL; }
  return GDMIX_RE_OK;
}

// a rule's solve as solve_three_lists takes it
template <class Rule>
struct OwlqnLists {
  ListsArgs a;
  Rule R;
  int64_t max_p;
  int m;
  static constexpr const char* family = "re_owlqn";
  static constexpr int p_vectors = Rule::P_VECTORS, n_vectors = 1;
  static size_t slot_doubles(const gdmix_re_packed* b, const gdmix_re_opts* o) { return owlqn_slot_doubles(Rule::P_VECTORS, b->max_p, b->max_n, o->m); }
  int verdict(const int32_t* hc) const { return owlqn_verdict(R, hc); }
  hipError_t launch_wave(const int32_t* list, int count, int lds_bytes, hipStream_t s) const {
    if (count <= 0) return hipSuccess;
    return with_loss(a.P.loss, [&](auto L) {
      constexpr int LOSS = decltype(L)::value;
      static DynLdsOnce lds_attr;   // one per instantiation of this lambda, i.e. per kernel
      if (hipError_t rc = lds_attr.set(reinterpret_cast<const void*>(re_owlqn_wave_kernel<LOSS, Rule>)); rc != hipSuccess) return rc;
      hipLaunchKernelGGL((re_owlqn_wave_kernel<LOSS, Rule>), dim3(count), dim3(WAVE), (size_t)lds_bytes, s, a.B, a.O, a.P, R, a.theta0, list, count);
      return hipGetLastError();
    });
  }
  hipError_t launch_block(int64_t last, int count, double* scratch, size_t slot_doubles, int slots, hipStream_t s) const {
    if (count <= 0) return hipSuccess;
    const int grid = count < slots ? count : slots;
    return with_loss(a.P.loss, [&](auto L) {
      hipLaunchKernelGGL((re_owlqn_block_kernel<decltype(L)::value, Rule>), dim3(grid), dim3(WAVE * BLOCK_NW), 0, s, a.B, a.O, a.P, R, a.theta0, last, count,
                         scratch, slot_doubles, max_p);
      return hipGetLastError();
    });
  }
};
template <class Rule>
static int owlqn_solve_lists(gdmix_re_ctx* ctx, const gdmix_re_packed* b, const gdmix_re_opts* opts, const Rule& R, const double* theta0,
                             const gdmix_re_result* out, void* stream, const char* who) {
  return solve_three_lists(ctx, b, opts, OwlqnLists<Rule>{lists_args(b, opts, theta0, out), R, b->max_p, opts->m}, out, stream, who);
}

// the options and outputs either solve refuses, in the order gdmix_re_solve_l1 always checked them
static int owlqn_check_args(const gdmix_re_opts* opts, const gdmix_re_result* out, const char* who, const char* sum_loss_hint) {
  if (opts->sum_loss) { set_error("%s: sum_loss is the fixed effect's objective (%s)", who, sum_loss_hint); return GDMIX_RE_EINVAL; }
  if (opts->m < 1 || opts->max_iter < 0 || opts->maxls < 1) { set_error("bad solver options (m, max_iter, maxls)"); return GDMIX_RE_EINVAL; }
  if (!loss_code_ok(opts->loss, who)) return GDMIX_RE_EINVAL;
  if (opts->variance_mode == GDMIX_RE_VAR_FULL && !out->theta) { set_error("variance_mode FULL needs out->theta"); return GDMIX_RE_EINVAL; }
  if (opts->variance_mode != GDMIX_RE_VAR_NONE && !out->variance) { set_error("variance requested but out->variance is NULL"); return GDMIX_RE_EINVAL; }
  return GDMIX_RE_OK;
}

}  // namespace gdmix

using namespace gdmix;

extern "C" {

GDMIX_API size_t gdmix_re_solve_l1_scratch_bytes(const gdmix_re_packed* batch, const gdmix_re_opts* opts) {
  return lists_scratch_bytes<OwlqnLists<ReOwlRule>>(batch, opts);
}

GDMIX_API int gdmix_re_solve_l1(gdmix_re_ctx* ctx, const gdmix_re_packed* b, const gdmix_re_opts* opts, double l1, const double* theta0,
                                const gdmix_re_result* out, void* stream) {
  if (!ctx || !b || !opts || !out) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  if (!(l1 >= 0.0) || isinf(l1)) { set_error("gdmix_re_solve_l1: l1 must be finite and >= 0"); return GDMIX_RE_EINVAL; }
  if (l1 == 0.0) return gdmix_re_solve(ctx, b, opts, theta0, out, stream);   // the plain fit, bit for bit
  if (const int rc = owlqn_check_args(opts, out, "gdmix_re_solve_l1", "gdmix_fe_set_l1 is its elastic net"); rc != GDMIX_RE_OK) return rc;
  bool empty;
  if (const int rc = begin_lists_solve(ctx, b, stream, "gdmix_re_solve_l1", &empty); rc != GDMIX_RE_OK || empty) return rc;
  return owlqn_solve_lists(ctx, b, opts, ReOwlRule{l1}, theta0, out, stream, "gdmix_re_solve_l1");
}

GDMIX_API size_t gdmix_re_solve_box_scratch_bytes(const gdmix_re_packed* batch, const gdmix_re_opts* opts) {
  return lists_scratch_bytes<OwlqnLists<ReBoxRule>>(batch, opts);
}

GDMIX_API int gdmix_re_solve_box(gdmix_re_ctx* ctx, const gdmix_re_packed* b, const gdmix_re_opts* opts, const double* lower, const double* upper,
                                 int64_t num_features, const double* theta0, const gdmix_re_result* out, void* stream) {
  if (!ctx || !b || !opts || !out) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  if (!lower && !upper) return gdmix_re_solve(ctx, b, opts, theta0, out, stream);   // the plain fit, bit for bit
  if (num_features < 0) { set_error("gdmix_re_solve_box: num_features is negative"); return GDMIX_RE_EINVAL; }
  if (const int rc = owlqn_check_args(opts, out, "gdmix_re_solve_box", "gdmix_fe_set_bounds is its box"); rc != GDMIX_RE_OK) return rc;
  bool empty;
  if (const int rc = begin_lists_solve(ctx, b, stream, "gdmix_re_solve_box", &empty); rc != GDMIX_RE_OK || empty) return rc;
  hipStream_t const s = static_cast<hipStream_t>(stream);
  HIP_TRY(join_unique(&ctx->impl, s));   // the check and the solve kernels read unique_global: behind a deferred compaction first
  const int64_t most = num_features > b->Z ? num_features : b->Z;   // (unique_global holds at most Z ids)
  hipLaunchKernelGGL(re_box_check_kernel, dim3(grid_for(most > 0 ? most : 1, 256, 1024)), dim3(256), 0, s, lower, upper, num_features, b->unique_global,
                     b->ent_feat_ptr, b->E, b->class_count);
  HIP_TRY(hipGetLastError());
  return owlqn_solve_lists(ctx, b, opts, ReBoxRule{lower, upper, b->unique_global}, theta0, out, stream, "gdmix_re_solve_box");
}

}  // extern "C"
