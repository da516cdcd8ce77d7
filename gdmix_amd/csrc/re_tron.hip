// re_tron.hip — the random effect's trust-region Newton solve, per entity on the device (include/gdmix_re.h, "TRON").
//
//   re_tron_route_kernel       an entity goes to the wavefront kernel iff its TRON LDS footprint is within the context's wave_lds_limit,
//                              else to the workgroup kernel: two lists in the batch's `order`, two counts (the wavefront kernel's small
//                              entities apart, in cls_tmp: they are launched with less LDS)
//   re_tron_wave_kernel        ONE WAVEFRONT PER ENTITY: the entity's block and all solver state live in LDS for the whole solve
//   re_tron_block_kernel       one workgroup per entity, state in a global scratch slot per workgroup, X streamed, grid-stride
//   gdmix_re_solve_tron, gdmix_re_solve_tron_scratch_bytes
//
// The solve itself is tron_solve<LOSS> of re_tron.hpp. The shape is the elastic net's (re_owlqn.hip), layer for layer; no kernel of the plain
// solve, the elastic net or the box solve is touched, and the size-class table is not involved.
#include <math.h>

#include "re_internal.hpp"
#include "re_tron.hpp"

namespace gdmix {

// LDS bytes the wavefront kernel needs for an entity: the staged block and the sample vector as wave_lds_bytes counts them, without any
// history (m = 0: five coefficient vectors, one sample vector), plus TRON's other two coefficient vectors and its two D arrays (must match
// the kernel's carve-up). The one footprint: the route kernel, the launch and the carve-up use it.
__host__ __device__ inline size_t tron_lds_bytes(int p, int n, int nnz, int d, bool has_w) {
  return (wave_lds_bytes(p, n, nnz, d, 0, has_w) + (size_t)(TRON_P_VECTORS - 5) * 8 * p + (size_t)(TRON_N_VECTORS - 1) * 8 * n + 15) & ~(size_t)15;
}

// doubles of global scratch one slot of the workgroup kernel needs: the coefficient vectors | the sample vectors | a few words
inline size_t tron_slot_doubles(int64_t max_p, int64_t max_n) { return (size_t)TRON_P_VECTORS * max_p + (size_t)TRON_N_VECTORS * max_n + 8; }

static int tron_slots_for(const gdmix_re_packed* b, size_t* slot_doubles) {
  *slot_doubles = tron_slot_doubles(b->max_p, b->max_n);
  // enough workgroups to fill the chip a few times over, bounded to ~4 GiB of scratch (as the elastic net sizes its slots)
  const size_t bytes = *slot_doubles * 8;
  size_t slots = 1024;
  const size_t by_budget = ((size_t)4 << 30) / (bytes ? bytes : 1);
  if (slots > by_budget) slots = by_budget;
  if (slots < 8) slots = 8;
  if ((int64_t)slots > b->E) slots = (size_t)(b->E > 0 ? b->E : 1);
  return (int)slots;
}

// words of the batch's count record (gdmix_re_packed::class_count) this solve uses: the two counts (where the elastic net has them), then
// how the wavefront kernel's entities split into its two launches
enum { TRON_COUNT_WAVE = 0, TRON_COUNT_BLOCK = 1, TRON_COUNT_WAVE_LARGE = 2, TRON_MAX_WAVE_LDS = 3, TRON_COUNT_WAVE_SMALL = 4, TRON_COUNT_WORDS = 5 };
// The wavefront kernel's workgroup is one wavefront and its LDS is what bounds the wavefronts a CU holds, so its entities are launched in
// two parts: those within TRON_SMALL_LDS bytes with that much LDS (eight one-wavefront workgroups per CU of 160 KB; a mean C2 entity of 16
// samples and ~64 coefficients needs about 6 KB, where OWL-QN's needs 15 KB), the others with the largest footprint among them.
constexpr int TRON_SMALL_LDS = 20 * 1024;

// ---------------------------------------------------------------------------------------------------
// routing, as re_owlqn_route_kernel: the wavefront kernel's large entities fill `order` from the front, the workgroup kernel's from the
// back; the wavefront kernel's small entities are a list of their own in `small` (the batch's cls_tmp). Position inside a list is by
// ticket: no entity's result depends on it.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void re_tron_route_kernel(const int64_t* __restrict__ ent_row_ptr, const int64_t* __restrict__ ent_nnz_ptr,
                                                            const int64_t* __restrict__ ent_feat_ptr, int64_t E, int ic, bool has_w, int wave_lds_limit,
                                                            int small_lds, int32_t* __restrict__ order, int32_t* __restrict__ small,
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
      const size_t bytes = tron_lds_bytes(d + ic, n, z, d, has_w);
      which = bytes > (size_t)wave_lds_limit ? 1 : (bytes <= (size_t)small_lds ? 0 : 2);
      pos = atomicAdd(&cnt[which], 1);
      if (which == 2) atomicMax(&lds_max, (int32_t)bytes);
    }
    __syncthreads();
    if (threadIdx.x == 0) base[0] = cnt[0] ? atomicAdd(&counts[TRON_COUNT_WAVE_SMALL], cnt[0]) : 0;
    if (threadIdx.x == 1) base[1] = cnt[1] ? atomicAdd(&counts[TRON_COUNT_BLOCK], cnt[1]) : 0;
    if (threadIdx.x == 2) base[2] = cnt[2] ? atomicAdd(&counts[TRON_COUNT_WAVE_LARGE], cnt[2]) : 0;
    if (threadIdx.x == 3 && cnt[0] + cnt[2] > 0) atomicAdd(&counts[TRON_COUNT_WAVE], cnt[0] + cnt[2]);
    if (threadIdx.x == 4 && lds_max > 0) atomicMax(&counts[TRON_MAX_WAVE_LDS], lds_max);
    __syncthreads();
    if (which == 0) small[base[0] + pos] = (int32_t)e;
    else if (which == 2) order[base[2] + pos] = (int32_t)e;
    else if (which == 1) order[E - 1 - (base[1] + pos)] = (int32_t)e;
    __syncthreads();
  }
}

// theta, thresholded theta, stats (what write_results of re_solve.hip writes for the plain solve), and the products
template <class G>
__device__ __forceinline__ void tron_write_results(G& grp, const OutDev& O, int32_t* nhv, const SolveParams& o, int64_t e, int64_t c0, int p, const TronWork& W,
                                                   const TronStats& st) {
  for (int j = grp.tid; j < p; j += grp.NT) {
    const double v = W.x[j];
    if (O.theta) O.theta[c0 + j] = v;
    if (O.theta_thr) O.theta_thr[c0 + j] = (fabs(v) <= o.threshold) ? 0.0 : v;
  }
  if (grp.tid == 0) {
    if (O.fval) O.fval[e] = st.f;
    if (O.gnorm) O.gnorm[e] = st.gnorm;
    if (O.nit) O.nit[e] = st.nit;
    if (O.nfev) O.nfev[e] = st.nfev;
    if (O.status) O.status[e] = st.status;
    if (nhv) nhv[e] = st.nhv;
  }
}

// ---------------------------------------------------------------------------------------------------
// one wavefront per entity, everything LDS-resident: one batch of coalesced staging loads, then no HBM traffic until the results
// ---------------------------------------------------------------------------------------------------
template <int LOSS>
__global__ __launch_bounds__(WAVE) void re_tron_wave_kernel(BatchDev B, OutDev O, int32_t* __restrict__ nhv, SolveParams o, const double* __restrict__ theta0,
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
  const int64_t c0 = f0 + e * ic;

  // carve-up: doubles first (8-byte aligned), then 4-byte arrays; must match tron_lds_bytes()
  TronWork W;
  double* dp = reinterpret_cast<double*>(smem);
  W.x = dp; dp += p;
  W.g = dp; dp += p;
  W.xt = dp; dp += p;
  W.gt = dp; dp += p;
  W.s = dp; dp += p;
  W.r = dp; dp += p;
  W.d = dp; dp += p;
  W.rs = dp; dp += n;
  W.dc = dp; dp += n;
  W.dt = dp; dp += n;
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
  for (int j = lane; j < p; j += WAVE) W.xt[j] = theta0 ? theta0[c0 + j] : 0.0;

  TronWave grp{{lane}};
  grp.sync();
  EntityView P{n, d, p, ic, s_row_ptr, s_csr_col, s_csr_val, s_col_ptr, s_csc_row, s_csc_val, s_y, s_o, s_w};
  TronStats st;
  tron_solve<LOSS>(grp, P, o, W, st);
  tron_write_results(grp, O, nhv, o, e, c0, p, W, st);
  if (o.variance_mode == GDMIX_RE_VAR_SIMPLE && O.variance) tron_variance_simple(grp, P, o, W.dc, O.variance + c0);
}

// ---------------------------------------------------------------------------------------------------
// one workgroup per entity, state in a global scratch slot, X streamed from HBM/L2. No workgroup waits for another.
// The list is read from its end: order[last - idx] (re_tron_route_kernel fills it from the back of `order`).
// ---------------------------------------------------------------------------------------------------
template <int LOSS>
__global__ __launch_bounds__(WAVE* BLOCK_NW) void re_tron_block_kernel(BatchDev B, OutDev O, int32_t* __restrict__ nhv, SolveParams o,
                                                                        const double* __restrict__ theta0, int64_t last, int count, double* scratch,
                                                                        size_t slot_doubles, int64_t max_p, int64_t max_n) {
  __shared__ double red[2 * BLOCK_NW];
  __shared__ double red_n[2 * BLOCK_NW * TRON_SUMS];
  const int ic = o.has_intercept ? 1 : 0;
  double* slot = scratch + (size_t)blockIdx.x * slot_doubles;
  for (int idx = blockIdx.x; idx < count; idx += gridDim.x) {
    const int64_t e = B.order[last - idx];
    const int64_t r0 = B.ent_row_ptr[e], z0 = B.ent_nnz_ptr[e], f0 = B.ent_feat_ptr[e];
    const int n = (int)(B.ent_row_ptr[e + 1] - r0);
    const int d = (int)(B.ent_feat_ptr[e + 1] - f0);
    const int p = d + ic;
    const int64_t c0 = f0 + e * ic;
    TronWork W;
    double* dp = slot;
    W.x = dp; dp += max_p;
    W.g = dp; dp += max_p;
    W.xt = dp; dp += max_p;
    W.gt = dp; dp += max_p;
    W.s = dp; dp += max_p;
    W.r = dp; dp += max_p;
    W.d = dp; dp += max_p;
    W.rs = dp; dp += max_n;
    W.dc = dp; dp += max_n;
    W.dt = dp;
    TronBlock grp{{(int)threadIdx.x, red, 0}, red_n, 0};
    for (int j = grp.tid; j < p; j += grp.NT) W.xt[j] = theta0 ? theta0[c0 + j] : 0.0;
    grp.sync();
    EntityView P{n, d, p, ic, B.row_ptr + r0 + e, B.csr_col + z0, B.csr_val + z0, B.col_ptr + z0 + e,
                 B.csc_row + z0, B.csc_val + z0, B.y + r0, B.offset + r0, B.weight ? B.weight + r0 : nullptr};
    TronStats st;
    tron_solve<LOSS>(grp, P, o, W, st);
    tron_write_results(grp, O, nhv, o, e, c0, p, W, st);
    if (o.variance_mode == GDMIX_RE_VAR_SIMPLE && O.variance) tron_variance_simple(grp, P, o, W.dc, O.variance + c0);
    grp.sync();   // the slot is reused by the next entity
  }
}

static hipError_t launch_tron_wave(const BatchDev& B, const OutDev& O, int32_t* nhv, const SolveParams& o, const double* theta0, const int32_t* list, int count,
                                   int lds_bytes, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  return with_loss(o.loss, [&](auto L) {
    constexpr int LOSS = decltype(L)::value;
    static DynLdsOnce lds_attr;   // one per instantiation of this lambda, i.e. per kernel
    if (hipError_t rc = lds_attr.set(reinterpret_cast<const void*>(re_tron_wave_kernel<LOSS>)); rc != hipSuccess) return rc;
    hipLaunchKernelGGL((re_tron_wave_kernel<LOSS>), dim3(count), dim3(WAVE), (size_t)lds_bytes, s, B, O, nhv, o, theta0, list, count);
    return hipGetLastError();
  });
}

static hipError_t launch_tron_block(const BatchDev& B, const OutDev& O, int32_t* nhv, const SolveParams& o, const double* theta0, int64_t last, int count,
                                    double* scratch, size_t slot_doubles, int slots, int64_t max_p, int64_t max_n, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  const int grid = count < slots ? count : slots;
  return with_loss(o.loss, [&](auto L) {
    hipLaunchKernelGGL((re_tron_block_kernel<decltype(L)::value>), dim3(grid), dim3(WAVE * BLOCK_NW), 0, s, B, O, nhv, o, theta0, last, count, scratch,
                       slot_doubles, max_p, max_n);
    return hipGetLastError();
  });
}

// The solve of a batch, behind the argument checks: route, one read-back (the list lengths), the launches, FULL variances.
static int tron_solve_batch(gdmix_re_ctx* ctx, const gdmix_re_packed* b, const gdmix_re_opts* opts, const double* theta0, const gdmix_re_result* out,
                            int32_t* nhv, void* stream) {
  gdmix_ctx_impl* const ci = &ctx->impl;
  hipStream_t const s = static_cast<hipStream_t>(stream);

  const int ic = opts->has_intercept ? 1 : 0;
  int32_t* const counts = b->class_count;
  const int small_lds = ci->wave_lds_limit < TRON_SMALL_LDS ? ci->wave_lds_limit : TRON_SMALL_LDS;
  hipLaunchKernelGGL(re_tron_route_kernel, dim3(grid_for(b->E, 256, 2048)), dim3(256), 0, s, b->ent_row_ptr, b->ent_nnz_ptr, b->ent_feat_ptr, b->E, ic,
                     b->weight != nullptr, ci->wave_lds_limit, small_lds, b->order, b->cls_tmp, counts);
  HIP_TRY(hipGetLastError());
  int32_t* const hc = ci->host_pinned + COUNTS_READBACK_WORDS;
  HIP_TRY(fetch_small(ci, 0, counts, TRON_COUNT_WORDS * sizeof(int32_t), hc, s));
  const int n_wave = hc[TRON_COUNT_WAVE], n_block = hc[TRON_COUNT_BLOCK], wave_lds = hc[TRON_MAX_WAVE_LDS];
  const int n_small = hc[TRON_COUNT_WAVE_SMALL], n_large = hc[TRON_COUNT_WAVE_LARGE];
  if (n_small < 0 || n_large < 0 || n_block < 0 || n_small + n_large != n_wave || (int64_t)n_wave + n_block != b->E || wave_lds < 0 || wave_lds > 65536) {
    set_error("gdmix_re_solve_tron: the routing counted %d + %d of %lld entities (LDS %d)", n_wave, n_block, (long long)b->E, wave_lds);
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
    slots = tron_slots_for(b, &slot_doubles);
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
    hipStream_t q[3] = {s, s, s};
    const int live = (n_block > 0) + (n_large > 0) + (n_small > 0);
    if (live > 1 && ci->n_side > 0) {
      HIP_TRY(hipEventRecord(ci->side_fork, s));
      int k = 0;
      if (n_block > 0) { HIP_TRY(side_join.use(k)); q[0] = ci->side[k]; k = k + 1 < ci->n_side ? k + 1 : k; }
      if (n_large > 0 && n_small > 0) { HIP_TRY(side_join.use(k)); q[1] = ci->side[k]; }
    }
    hipError_t rc = launch_tron_block(B, O, nhv, P, theta0, b->E - 1, n_block, scratch, slot_doubles, slots, b->max_p, b->max_n, q[0]);
    if (rc != hipSuccess) { set_error("launch of re_tron_block_kernel failed: %s", hipGetErrorString(rc)); return GDMIX_RE_EHIP; }
    rc = launch_tron_wave(B, O, nhv, P, theta0, b->order, n_large, wave_lds, q[1]);
    if (rc == hipSuccess) rc = launch_tron_wave(B, O, nhv, P, theta0, b->cls_tmp, n_small, small_lds, q[2]);
    if (rc != hipSuccess) { set_error("launch of re_tron_wave_kernel failed: %s", hipGetErrorString(rc)); return GDMIX_RE_EHIP; }
  }
  if (opts->variance_mode == GDMIX_RE_VAR_FULL) {   // at the returned theta, with the same l2 (joins a deferred compaction itself)
    const int rc = gdmix_re_variance_full(ctx, b, opts, out->theta, out->variance, stream);
    if (rc != GDMIX_RE_OK) return rc;
  }
  HIP_TRY(join_unique(ci, s));
  return GDMIX_RE_OK;
}

}  // namespace gdmix

using namespace gdmix;

extern "C" {

GDMIX_API size_t gdmix_re_solve_tron_scratch_bytes(const gdmix_re_packed* batch, const gdmix_re_opts* opts) {
  if (!batch || !opts || batch->E == 0) return 0;
  size_t slot_doubles;
  const int slots = tron_slots_for(batch, &slot_doubles);
  const size_t own = (size_t)slots * slot_doubles * 8;
  const size_t plain = gdmix_re_solve_scratch_bytes(batch, opts);   // FULL variances are the plain solve's kernels
  return own > plain ? own : plain;
}

GDMIX_API int gdmix_re_solve_tron(gdmix_re_ctx* ctx, const gdmix_re_packed* b, const gdmix_re_opts* opts, const double* theta0,
                                  const gdmix_re_result* out, int32_t* nhv, void* stream) {
  if (!ctx || !b || !opts || !out) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  if (opts->sum_loss) { set_error("gdmix_re_solve_tron: sum_loss is the fixed effect's objective (gdmix_fe_set_optimizer is its TRON)"); return GDMIX_RE_EINVAL; }
  if (opts->max_iter < 0 || opts->maxls < 1) { set_error("bad solver options (max_iter, maxls)"); return GDMIX_RE_EINVAL; }   // (m is ignored)
  if (!loss_code_ok(opts->loss, "gdmix_re_solve_tron")) return GDMIX_RE_EINVAL;
  if (opts->variance_mode == GDMIX_RE_VAR_FULL && !out->theta) { set_error("variance_mode FULL needs out->theta"); return GDMIX_RE_EINVAL; }
  if (opts->variance_mode != GDMIX_RE_VAR_NONE && !out->variance) { set_error("variance requested but out->variance is NULL"); return GDMIX_RE_EINVAL; }
  if (b->E == 0) return GDMIX_RE_OK;
  if (b->E > 0x7fffffffLL) { set_error("gdmix_re_solve_tron: 2^31 entities or more"); return GDMIX_RE_ERANGE; }
  gdmix_ctx_impl* const ci = &ctx->impl;
  hipStream_t const s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(ci->device));
  for (int c = 0; c < GDMIX_RE_NUM_CLASSES; ++c) ci->ev_used[c] = false;
  HIP_TRY(hipMemsetAsync(b->class_count, 0, sizeof(ClassCounts), s));
  return tron_solve_batch(ctx, b, opts, theta0, out, nhv, stream);
}

}  // extern "C"
