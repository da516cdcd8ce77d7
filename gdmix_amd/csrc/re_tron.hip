// re_tron.hip — the random effect's trust-region Newton solve, per entity on the device (include/gdmix_re.h, "TRON").
//
//   (re_owlqn.hip: re_lds_route_kernel, here with the TRON LDS footprint; re_entity_scaffold.hpp: the footprint, the count words and
//    the host driver, solve_three_lists, shared with the elastic net and the box solve)
//   (re_tron_rows.hip: re_tron_rows_kernel, FOUR ENTITIES PER WAVEFRONT, for the entities within the context's TRON row limit; a unit
//    of its own because it is compiled with the packed fp32 instructions switched off, which would change the kernels here: build.UNIT_FLAGS)
//   re_tron_wave_kernel        ONE WAVEFRONT PER ENTITY: the entity's block and all solver state live in LDS for the whole solve
//   re_tron_block_kernel       one workgroup per entity, state in a global scratch slot per workgroup, X streamed, grid-stride
//   gdmix_re_solve_tron, gdmix_re_solve_tron_scratch_bytes
//   Both kernels have a second instantiation per loss, <LOSS, true>: the diagonally preconditioned solve ("TRON_PCG"), nine coefficient
//   vectors instead of seven, taken when the context's preconditioner is on (gdmix_re_set_tron_preconditioner). It has no row kernel.
//
// The solve itself is tron_solve<LOSS> of re_tron.hpp. No kernel of the plain solve, the elastic net or the box solve is touched, and
// the size-class table is not involved.
#include <math.h>

#include "re_entity_scaffold.hpp"
#include "re_tron.hpp"

namespace gdmix {

// re_tron_rows_kernel<a.P.loss> on list[0, count) (re_tron_rows.hip)
hipError_t launch_tron_rows(const ListsArgs& a, int32_t* nhv, const int32_t* list, int count, int row_bytes, hipStream_t s);

// doubles of global scratch one slot of the workgroup kernel needs: the coefficient vectors | the sample vectors | a few words
inline size_t tron_slot_doubles(int p_vectors, int64_t max_p, int64_t max_n) { return (size_t)p_vectors * max_p + (size_t)TRON_N_VECTORS * max_n + 8; }

// what a kernel takes as its options: SolveParams, or under PCG the same with the preconditioner's weight behind it
template <bool PCG>
using TronParams = std::conditional_t<PCG, TronPcgParams, SolveParams>;

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
template <int LOSS, bool PCG>
__global__ __launch_bounds__(WAVE) void re_tron_wave_kernel(BatchDev B, OutDev O, int32_t* __restrict__ nhv, TronParams<PCG> o, const double* __restrict__ theta0,
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

  // carve-up: doubles first (8-byte aligned), then 4-byte arrays; must match solver_lds_bytes() at m = 0 with TRON_P_VECTORS (PCG:
  // TRON_PCG_P_VECTORS) and TRON_N_VECTORS
  TronWork W;
  double* dp = reinterpret_cast<double*>(smem);
  W.x = dp; dp += p;
  W.g = dp; dp += p;
  W.xt = dp; dp += p;
  W.gt = dp; dp += p;
  W.s = dp; dp += p;
  W.r = dp; dp += p;
  W.d = dp; dp += p;
  if constexpr (PCG) { W.m = dp; dp += p; W.im = dp; dp += p; }
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
  tron_solve<LOSS, PCG>(grp, P, o, W, st);
  tron_write_results(grp, O, nhv, o, e, c0, p, W, st);
  if (o.variance_mode == GDMIX_RE_VAR_SIMPLE && O.variance) tron_variance_simple(grp, P, o, W.dc, O.variance + c0);
}

// ---------------------------------------------------------------------------------------------------
// one workgroup per entity, state in a global scratch slot, X streamed from HBM/L2. No workgroup waits for another.
// The list is read from its end: order[last - idx] (re_lds_route_kernel fills it from the back of `order`).
// ---------------------------------------------------------------------------------------------------
template <int LOSS, bool PCG>
__global__ __launch_bounds__(WAVE* BLOCK_NW) void re_tron_block_kernel(BatchDev B, OutDev O, int32_t* __restrict__ nhv, TronParams<PCG> o,
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
    if constexpr (PCG) { W.m = dp; dp += max_p; W.im = dp; dp += max_p; }
    W.rs = dp; dp += max_n;
    W.dc = dp; dp += max_n;
    W.dt = dp;
    TronBlock grp{{(int)threadIdx.x, red, 0}, red_n, 0};
    for (int j = grp.tid; j < p; j += grp.NT) W.xt[j] = theta0 ? theta0[c0 + j] : 0.0;
    grp.sync();
    EntityView P{n, d, p, ic, B.row_ptr + r0 + e, B.csr_col + z0, B.csr_val + z0, B.col_ptr + z0 + e,
                 B.csc_row + z0, B.csc_val + z0, B.y + r0, B.offset + r0, B.weight ? B.weight + r0 : nullptr};
    TronStats st;
    tron_solve<LOSS, PCG>(grp, P, o, W, st);
    tron_write_results(grp, O, nhv, o, e, c0, p, W, st);
    if (o.variance_mode == GDMIX_RE_VAR_SIMPLE && O.variance) tron_variance_simple(grp, P, o, W.dc, O.variance + c0);
    grp.sync();   // the slot is reused by the next entity
  }
}

// the solve as solve_three_lists takes it: the wavefront and the workgroup kernel of either variant
template <bool PCG>
struct TronKernels {
  ListsArgs a;
  int32_t* nhv;
  int64_t max_p, max_n;
  double pcg_a;   // PCG: the preconditioner's weight
  static constexpr const char* family = "re_tron";
  static constexpr int p_vectors = PCG ? TRON_PCG_P_VECTORS : TRON_P_VECTORS, n_vectors = TRON_N_VECTORS, m = 0;   // (no history: gdmix_re_opts.m is ignored)
  static size_t slot_doubles(const gdmix_re_packed* b, const gdmix_re_opts*) { return tron_slot_doubles(p_vectors, b->max_p, b->max_n); }
  static int verdict(const int32_t*) { return GDMIX_RE_OK; }
  TronParams<PCG> params() const {
    if constexpr (PCG) {
      TronPcgParams q;
      static_cast<SolveParams&>(q) = a.P;
      q.a = pcg_a;
      return q;
    } else {
      return a.P;
    }
  }
  hipError_t launch_wave(const int32_t* list, int count, int lds_bytes, hipStream_t s) const {
    if (count <= 0) return hipSuccess;
    return with_loss(a.P.loss, [&](auto L) {
      constexpr int LOSS = decltype(L)::value;
      static DynLdsOnce lds_attr;   // one per instantiation of this lambda, i.e. per kernel
      if (hipError_t rc = lds_attr.set(reinterpret_cast<const void*>(re_tron_wave_kernel<LOSS, PCG>)); rc != hipSuccess) return rc;
      hipLaunchKernelGGL((re_tron_wave_kernel<LOSS, PCG>), dim3(count), dim3(WAVE), (size_t)lds_bytes, s, a.B, a.O, nhv, params(), a.theta0, list, count);
      return hipGetLastError();
    });
  }
  hipError_t launch_block(int64_t last, int count, double* scratch, size_t slot_doubles, int slots, hipStream_t s) const {
    if (count <= 0) return hipSuccess;
    const int grid = count < slots ? count : slots;
    return with_loss(a.P.loss, [&](auto L) {
      hipLaunchKernelGGL((re_tron_block_kernel<decltype(L)::value, PCG>), dim3(grid), dim3(WAVE * BLOCK_NW), 0, s, a.B, a.O, nhv, params(), a.theta0, last,
                         count, scratch, slot_doubles, max_p, max_n);
      return hipGetLastError();
    });
  }
};

// TRON: with the row kernel on list[0, count), four entities a wavefront, row_bytes of LDS each
struct TronLists : TronKernels<false> {
  hipError_t launch_rows(const int32_t* list, int count, int row_bytes, hipStream_t s) const { return launch_tron_rows(a, nhv, list, count, row_bytes, s); }
};
// TRON_PCG: no row kernel, so solve_three_lists routes with a row limit of 0
using TronPcgLists = TronKernels<true>;

}  // namespace gdmix

using namespace gdmix;

extern "C" {

GDMIX_API size_t gdmix_re_solve_tron_scratch_bytes(const gdmix_re_packed* batch, const gdmix_re_opts* opts) {
  // (no context here: the two vectors count while any context of the process has the preconditioner on)
  if (tron_pcg_contexts.load(std::memory_order_relaxed) > 0) return lists_scratch_bytes<TronPcgLists>(batch, opts);
  return lists_scratch_bytes<TronLists>(batch, opts);
}

GDMIX_API int gdmix_re_solve_tron(gdmix_re_ctx* ctx, const gdmix_re_packed* b, const gdmix_re_opts* opts, const double* theta0,
                                  const gdmix_re_result* out, int32_t* nhv, void* stream) {
  if (!ctx || !b || !opts || !out) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  if (opts->sum_loss) { set_error("gdmix_re_solve_tron: sum_loss is the fixed effect's objective (gdmix_fe_set_optimizer is its TRON)"); return GDMIX_RE_EINVAL; }
  if (opts->max_iter < 0 || opts->maxls < 1) { set_error("bad solver options (max_iter, maxls)"); return GDMIX_RE_EINVAL; }   // (m is ignored)
  if (!loss_code_ok(opts->loss, "gdmix_re_solve_tron")) return GDMIX_RE_EINVAL;
  if (opts->variance_mode == GDMIX_RE_VAR_FULL && !out->theta) { set_error("variance_mode FULL needs out->theta"); return GDMIX_RE_EINVAL; }
  if (opts->variance_mode != GDMIX_RE_VAR_NONE && !out->variance) { set_error("variance requested but out->variance is NULL"); return GDMIX_RE_EINVAL; }
  bool empty;
  if (const int rc = begin_lists_solve(ctx, b, stream, "gdmix_re_solve_tron", &empty); rc != GDMIX_RE_OK || empty) return rc;
  const double pcg_a = ctx->impl.tron_pcg_a;
  if (pcg_a > 0.0) return solve_three_lists(ctx, b, opts, TronPcgLists{lists_args(b, opts, theta0, out), nhv, b->max_p, b->max_n, pcg_a}, out, stream, "gdmix_re_solve_tron");
  return solve_three_lists(ctx, b, opts, TronLists{{lists_args(b, opts, theta0, out), nhv, b->max_p, b->max_n, 0.0}}, out, stream, "gdmix_re_solve_tron");
}

}  // extern "C"
