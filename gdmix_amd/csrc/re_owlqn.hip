// re_owlqn.hip — the random effect's two projected quasi-Newton solves, per entity on the device: the elastic net by OWL-QN
// (include/gdmix_re.h, "elastic net"; ReOwlRule) and the box-constrained fit by projected L-BFGS ("box constraints"; ReBoxRule). The
// route kernel, the epilogue and the two kernel bodies take the rule, and with it the footprint, as a parameter.
//
//   re_box_check_kernel        the caller's bound tables and the batch's feature ids, its verdict in the count record
//   re_owlqn_route_kernel      an entity goes to the wavefront kernel iff its LDS footprint under the rule is within the context's
//                              wave_lds_limit, else to the workgroup kernel: two lists in the batch's `order`, two counts
//                              (the wavefront kernel's small entities apart, in cls_tmp: they are launched with less LDS)
//   re_owlqn_wave_kernel       ONE WAVEFRONT PER ENTITY: the entity's block and all solver state live in LDS for the whole solve
//   re_owlqn_block_kernel      one workgroup per entity, state in a global scratch slot per workgroup, X streamed, grid-stride
//   gdmix_re_solve_l1, gdmix_re_solve_l1_scratch_bytes, gdmix_re_solve_box, gdmix_re_solve_box_scratch_bytes
//
// The solve itself is owlqn_solve<LOSS, Rule> of re_owlqn.hpp; the evaluation, the reductions and the SIMPLE variance are those of the plain
// solve (re_solve_core.hpp). No kernel of the plain solve is touched, and the size-class table is not involved.
#include <math.h>

#include "re_internal.hpp"
#include "re_owlqn.hpp"

namespace gdmix {

// LDS bytes the wavefront kernel needs for an entity under a rule of p_vectors coefficient vectors: the plain wavefront kernel's (five),
// and the rule's others — OWL-QN's pseudo-gradient; the bounded step's lo and hi (must match the kernel's carve-up). The one footprint:
// the route kernel, the launch and the carve-up use it.
__host__ __device__ inline size_t owlqn_lds_bytes(int p_vectors, int p, int n, int nnz, int d, int m, bool has_w) {
  return (wave_lds_bytes(p, n, nnz, d, m, has_w) + (size_t)(p_vectors - 5) * 8 * p + 15) & ~(size_t)15;
}

// doubles of global scratch one slot of the workgroup kernel needs: the rule's coefficient vectors | history | alpha rho | residuals
inline size_t owlqn_slot_doubles(int p_vectors, int64_t max_p, int64_t max_n, int m) {
  return (size_t)(p_vectors + 2 * m) * max_p + (size_t)2 * m + max_n + 8;
}

static int owlqn_slots_for(int p_vectors, const gdmix_re_packed* b, const gdmix_re_opts* o, size_t* slot_doubles) {
  *slot_doubles = owlqn_slot_doubles(p_vectors, b->max_p, b->max_n, o->m);
  // enough workgroups to fill the chip a few times over, bounded to ~4 GiB of scratch (as the plain solve sizes its slots)
  const size_t bytes = *slot_doubles * 8;
  size_t slots = 1024;
  const size_t by_budget = ((size_t)4 << 30) / (bytes ? bytes : 1);
  if (slots > by_budget) slots = by_budget;
  if (slots < 8) slots = 8;
  if ((int64_t)slots > b->E) slots = (size_t)(b->E > 0 ? b->E : 1);
  return (int)slots;
}

// words of the batch's count record (gdmix_re_packed::class_count) this solve uses: the two counts, then how the wavefront kernel's
// entities split into its two launches
// (the bounded solve: then the verdict of re_box_check_kernel, read back with the counts)
enum { OWL_COUNT_WAVE = 0, OWL_COUNT_BLOCK = 1, OWL_COUNT_WAVE_LARGE = 2, OWL_MAX_WAVE_LDS = 3, OWL_COUNT_WAVE_SMALL = 4,
       BOX_BAD_NAN = 5, BOX_BAD_ORDER = 6, BOX_BAD_ID = 7, OWL_COUNT_WORDS = 8 };
// The wavefront kernel's workgroup is one wavefront and its LDS is what bounds the wavefronts a CU holds, so its entities are launched
// in two parts: those within OWL_SMALL_LDS bytes (eight workgroups per CU of 160 KB: nine tenths of a C2 partition, whose mean entity of
// 16 samples and ~64 coefficients needs 15 KB, 10 KB of them history) with that much LDS, the others with the largest footprint among them.
constexpr int OWL_SMALL_LDS = 20 * 1024;

// ---------------------------------------------------------------------------------------------------
// routing: the wavefront kernel's entities fill `order` from the front, the workgroup kernel's from the back; the wavefront kernel's
// small entities (OWL_SMALL_LDS) are a list of their own in `small` (the batch's cls_tmp, solver-owned like `order`). Position inside
// a list is by ticket (per workgroup: LDS counters, then one global atomic per list): no entity's result depends on it.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void re_owlqn_route_kernel(const int64_t* __restrict__ ent_row_ptr, const int64_t* __restrict__ ent_nnz_ptr,
                                                             const int64_t* __restrict__ ent_feat_ptr, int64_t E, int ic, int m, bool has_w,
                                                             int p_vectors, int wave_lds_limit, int small_lds, int32_t* __restrict__ order, int32_t* __restrict__ small,
                                                             int32_t* __restrict__ counts) {
  __shared__ int32_t cnt[3], base[3], lds_max;   // lists: 0 wavefront kernel, small; 1 workgroup kernel; 2 wavefront kernel, large
  for (int64_t start = (int64_t)blockIdx.x * blockDim.x; start < E; start += (int64_t)gridDim.x * blockDim.x) {
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    if (threadIdx.x == 3) lds_max = 0;
    __syncthreads();
    const int64_t e = start + threadIdx.x;
    int which = -1, pos = 0;
    if (e < E) {
      const int n = (int)(ent_row_ptr[e + 1] - ent_row_ptr[e]);
      const int z = (int)(ent_nnz_ptr[e + 1] - ent_nnz_ptr[e]);
      const int d = (int)(ent_feat_ptr[e + 1] - ent_feat_ptr[e]);
      const size_t bytes = owlqn_lds_bytes(p_vectors, d + ic, n, z, d, m, has_w);
      which = bytes > (size_t)wave_lds_limit ? 1 : (bytes <= (size_t)small_lds ? 0 : 2);
      pos = atomicAdd(&cnt[which], 1);
      if (which == 2) atomicMax(&lds_max, (int32_t)bytes);
    }
    __syncthreads();
    if (threadIdx.x == 0) base[0] = cnt[0] ? atomicAdd(&counts[OWL_COUNT_WAVE_SMALL], cnt[0]) : 0;
    if (threadIdx.x == 1) base[1] = cnt[1] ? atomicAdd(&counts[OWL_COUNT_BLOCK], cnt[1]) : 0;
    if (threadIdx.x == 2) base[2] = cnt[2] ? atomicAdd(&counts[OWL_COUNT_WAVE_LARGE], cnt[2]) : 0;
    if (threadIdx.x == 3 && cnt[0] + cnt[2] > 0) atomicAdd(&counts[OWL_COUNT_WAVE], cnt[0] + cnt[2]);
    if (threadIdx.x == 4 && lds_max > 0) atomicMax(&counts[OWL_MAX_WAVE_LDS], lds_max);
    __syncthreads();
    if (which == 0) small[base[0] + pos] = (int32_t)e;
    else if (which == 2) order[base[2] + pos] = (int32_t)e;
    else if (which == 1) order[E - 1 - (base[1] + pos)] = (int32_t)e;
    __syncthreads();
  }
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

  // carve-up: doubles first (8-byte aligned), then 4-byte arrays; must match owlqn_lds_bytes()
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
// The list is read from its end: order[last - idx] (re_owlqn_route_kernel fills it from the back of `order`).
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

template <class Rule>
static hipError_t launch_owlqn_wave(const BatchDev& B, const OutDev& O, const SolveParams& o, const Rule& R, const double* theta0, const int32_t* list, int count,
                                    int lds_bytes, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  return with_loss(o.loss, [&](auto L) {
    constexpr int LOSS = decltype(L)::value;
    static DynLdsOnce lds_attr;   // one per instantiation of this lambda, i.e. per kernel
    if (hipError_t rc = lds_attr.set(reinterpret_cast<const void*>(re_owlqn_wave_kernel<LOSS, Rule>)); rc != hipSuccess) return rc;
    hipLaunchKernelGGL((re_owlqn_wave_kernel<LOSS, Rule>), dim3(count), dim3(WAVE), (size_t)lds_bytes, s, B, O, o, R, theta0, list, count);
    return hipGetLastError();
  });
}

template <class Rule>
static hipError_t launch_owlqn_block(const BatchDev& B, const OutDev& O, const SolveParams& o, const Rule& R, const double* theta0, int64_t last, int count,
                                     double* scratch, size_t slot_doubles, int slots, int64_t max_p, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  const int grid = count < slots ? count : slots;
  return with_loss(o.loss, [&](auto L) {
    hipLaunchKernelGGL((re_owlqn_block_kernel<decltype(L)::value, Rule>), dim3(grid), dim3(WAVE * BLOCK_NW), 0, s, B, O, o, R, theta0, last, count, scratch,
                       slot_doubles, max_p);
    return hipGetLastError();
  });
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

// The solve of a batch under a rule, behind the argument checks: route, one read-back (the list lengths, and the verdict of a check
// queued by the caller on `s` before this), the launches, FULL variances. `who` names the entry point in messages.
template <class Rule>
static int owlqn_solve_batch(gdmix_re_ctx* ctx, const gdmix_re_packed* b, const gdmix_re_opts* opts, const Rule& R, const double* theta0,
                             const gdmix_re_result* out, void* stream, const char* who) {
  gdmix_ctx_impl* const ci = &ctx->impl;
  hipStream_t const s = static_cast<hipStream_t>(stream);

  // the two lists and their counts
  const int ic = opts->has_intercept ? 1 : 0;
  int32_t* const counts = b->class_count;
  const int small_lds = ci->wave_lds_limit < OWL_SMALL_LDS ? ci->wave_lds_limit : OWL_SMALL_LDS;
  hipLaunchKernelGGL(re_owlqn_route_kernel, dim3(grid_for(b->E, 256, 2048)), dim3(256), 0, s, b->ent_row_ptr, b->ent_nnz_ptr, b->ent_feat_ptr, b->E, ic,
                     opts->m, b->weight != nullptr, Rule::P_VECTORS, ci->wave_lds_limit, small_lds, b->order, b->cls_tmp, counts);
  HIP_TRY(hipGetLastError());
  int32_t* const hc = ci->host_pinned + COUNTS_READBACK_WORDS;
  HIP_TRY(fetch_small(ci, 0, counts, OWL_COUNT_WORDS * sizeof(int32_t), hc, s));
  if (const int rc = owlqn_verdict(R, hc); rc != GDMIX_RE_OK) return rc;
  const int n_wave = hc[OWL_COUNT_WAVE], n_block = hc[OWL_COUNT_BLOCK], wave_lds = hc[OWL_MAX_WAVE_LDS];
  const int n_small = hc[OWL_COUNT_WAVE_SMALL], n_large = hc[OWL_COUNT_WAVE_LARGE];
  if (n_small < 0 || n_large < 0 || n_block < 0 || n_small + n_large != n_wave || (int64_t)n_wave + n_block != b->E || wave_lds < 0 || wave_lds > 65536) {
    set_error("%s: the routing counted %d + %d of %lld entities (LDS %d)", who, n_wave, n_block, (long long)b->E, wave_lds);
    return GDMIX_RE_EHIP;
  }

  SolveParams P = solve_params(*opts);
  P.sum_loss = 0;
  const BatchDev B = batch_dev(b);
  const OutDev O{out->theta, out->theta_thr, opts->variance_mode == GDMIX_RE_VAR_SIMPLE ? out->variance : nullptr, out->fval, out->gnorm, out->nit,
                 out->nfev, out->status};

  // scratch slots of the workgroup kernel: the context's scratch or the batch's, as many slots as fit (at least one)
  double* scratch = nullptr;
  size_t slot_doubles = 0;
  int slots = 0;
  if (n_block > 0) {
    slots = owlqn_slots_for(Rule::P_VECTORS, b, opts, &slot_doubles);
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

  // the two launches side by side where the context has side streams; every way out joins them back (SideJoin)
  {
    SideJoin side_join{ci, s};
    // the lists that hold entities, the longest-running first: each on a queue of its own while there are side streams
    hipStream_t q[3] = {s, s, s};
    const int live = (n_block > 0) + (n_large > 0) + (n_small > 0);
    if (live > 1 && ci->n_side > 0) {
      HIP_TRY(hipEventRecord(ci->side_fork, s));
      int k = 0;
      if (n_block > 0) { HIP_TRY(side_join.use(k)); q[0] = ci->side[k]; k = k + 1 < ci->n_side ? k + 1 : k; }
      if (n_large > 0 && n_small > 0) { HIP_TRY(side_join.use(k)); q[1] = ci->side[k]; }
    }
    hipError_t rc = launch_owlqn_block(B, O, P, R, theta0, b->E - 1, n_block, scratch, slot_doubles, slots, b->max_p, q[0]);
    if (rc != hipSuccess) { set_error("launch of re_owlqn_block_kernel failed: %s", hipGetErrorString(rc)); return GDMIX_RE_EHIP; }
    rc = launch_owlqn_wave(B, O, P, R, theta0, b->order, n_large, wave_lds, q[1]);
    if (rc == hipSuccess) rc = launch_owlqn_wave(B, O, P, R, theta0, b->cls_tmp, n_small, small_lds, q[2]);
    if (rc != hipSuccess) { set_error("launch of re_owlqn_wave_kernel failed: %s", hipGetErrorString(rc)); return GDMIX_RE_EHIP; }
  }
  if (opts->variance_mode == GDMIX_RE_VAR_FULL) {   // of the smooth part at the returned theta, with the same l2 (joins a deferred compaction itself)
    const int rc = gdmix_re_variance_full(ctx, b, opts, out->theta, out->variance, stream);
    if (rc != GDMIX_RE_OK) return rc;
  }
  HIP_TRY(join_unique(ci, s));
  return GDMIX_RE_OK;
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

static size_t owlqn_scratch_bytes(int p_vectors, const gdmix_re_packed* batch, const gdmix_re_opts* opts) {
  if (!batch || !opts || batch->E == 0) return 0;
  size_t slot_doubles;
  const int slots = owlqn_slots_for(p_vectors, batch, opts, &slot_doubles);
  const size_t own = (size_t)slots * slot_doubles * 8;
  const size_t plain = gdmix_re_solve_scratch_bytes(batch, opts);   // l1 == 0 / no bounds forward to the plain solve; FULL variances are its kernels
  return own > plain ? own : plain;
}

}  // namespace gdmix

using namespace gdmix;

extern "C" {

GDMIX_API size_t gdmix_re_solve_l1_scratch_bytes(const gdmix_re_packed* batch, const gdmix_re_opts* opts) {
  return owlqn_scratch_bytes(ReOwlRule::P_VECTORS, batch, opts);
}

GDMIX_API int gdmix_re_solve_l1(gdmix_re_ctx* ctx, const gdmix_re_packed* b, const gdmix_re_opts* opts, double l1, const double* theta0,
                                const gdmix_re_result* out, void* stream) {
  if (!ctx || !b || !opts || !out) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  if (!(l1 >= 0.0) || isinf(l1)) { set_error("gdmix_re_solve_l1: l1 must be finite and >= 0"); return GDMIX_RE_EINVAL; }
  if (l1 == 0.0) return gdmix_re_solve(ctx, b, opts, theta0, out, stream);   // the plain fit, bit for bit
  if (const int rc = owlqn_check_args(opts, out, "gdmix_re_solve_l1", "gdmix_fe_set_l1 is its elastic net"); rc != GDMIX_RE_OK) return rc;
  if (b->E == 0) return GDMIX_RE_OK;
  if (b->E > 0x7fffffffLL) { set_error("gdmix_re_solve_l1: 2^31 entities or more"); return GDMIX_RE_ERANGE; }
  gdmix_ctx_impl* const ci = &ctx->impl;
  hipStream_t const s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(ci->device));
  for (int c = 0; c < GDMIX_RE_NUM_CLASSES; ++c) ci->ev_used[c] = false;
  HIP_TRY(hipMemsetAsync(b->class_count, 0, sizeof(ClassCounts), s));
  return owlqn_solve_batch(ctx, b, opts, ReOwlRule{l1}, theta0, out, stream, "gdmix_re_solve_l1");
}

GDMIX_API size_t gdmix_re_solve_box_scratch_bytes(const gdmix_re_packed* batch, const gdmix_re_opts* opts) {
  return owlqn_scratch_bytes(ReBoxRule::P_VECTORS, batch, opts);
}

GDMIX_API int gdmix_re_solve_box(gdmix_re_ctx* ctx, const gdmix_re_packed* b, const gdmix_re_opts* opts, const double* lower, const double* upper,
                                 int64_t num_features, const double* theta0, const gdmix_re_result* out, void* stream) {
  if (!ctx || !b || !opts || !out) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  if (!lower && !upper) return gdmix_re_solve(ctx, b, opts, theta0, out, stream);   // the plain fit, bit for bit
  if (num_features < 0) { set_error("gdmix_re_solve_box: num_features is negative"); return GDMIX_RE_EINVAL; }
  if (const int rc = owlqn_check_args(opts, out, "gdmix_re_solve_box", "gdmix_fe_set_bounds is its box"); rc != GDMIX_RE_OK) return rc;
  if (b->E == 0) return GDMIX_RE_OK;
  if (b->E > 0x7fffffffLL) { set_error("gdmix_re_solve_box: 2^31 entities or more"); return GDMIX_RE_ERANGE; }
  gdmix_ctx_impl* const ci = &ctx->impl;
  hipStream_t const s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(ci->device));
  for (int c = 0; c < GDMIX_RE_NUM_CLASSES; ++c) ci->ev_used[c] = false;
  HIP_TRY(join_unique(ci, s));   // the check and the solve kernels read unique_global: behind a deferred compaction first
  HIP_TRY(hipMemsetAsync(b->class_count, 0, sizeof(ClassCounts), s));
  const int64_t most = num_features > b->Z ? num_features : b->Z;   // (unique_global holds at most Z ids)
  hipLaunchKernelGGL(re_box_check_kernel, dim3(grid_for(most > 0 ? most : 1, 256, 1024)), dim3(256), 0, s, lower, upper, num_features, b->unique_global,
                     b->ent_feat_ptr, b->E, b->class_count);
  HIP_TRY(hipGetLastError());
  return owlqn_solve_batch(ctx, b, opts, ReBoxRule{lower, upper, b->unique_global}, theta0, out, stream, "gdmix_re_solve_box");
}

}  // extern "C"
