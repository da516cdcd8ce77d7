// re_tron_rows.hip — re_tron_rows_kernel: the random effect's trust-region Newton solve with FOUR ENTITIES PER WAVEFRONT, one per DPP row
// of 16 lanes, for the entities within the context's TRON row limit (include/gdmix_re.h, "TRON"; gdmix_re_set_tron_row_lds_limit). The
// device functions — the reductions, the pass pair, the state machine — are re_tron_rows.hpp's; the routing, the lists and the host driver
// are those of re_entity_scaffold.hpp, and gdmix_re_solve_tron (re_tron.hip) reaches the kernel through launch_tron_rows.
//
// A unit of its own: it is compiled with the packed fp32 instructions switched off (build.UNIT_FLAGS: a guard for a kernel that owes another
// kernel's bits, measured to cost nothing, profiles/re_tron_rows.txt), and that switch changes the instructions of re_tron.hip's existing
// kernels, which stay what they were.
#include <math.h>

#include "re_entity_scaffold.hpp"
#include "re_tron_rows.hpp"

namespace gdmix {

// ---------------------------------------------------------------------------------------------------
// four entities per wavefront: row r (lanes 16 r .. 16 r + 15) solves list[4 blockIdx.x + r] in LDS block r of row_bytes each. The whole
// wavefront stages the four blocks one after another, one batch of coalesced loads and one barrier; then no HBM traffic until the results.
// ---------------------------------------------------------------------------------------------------
template <int LOSS>
__global__ __launch_bounds__(WAVE) void re_tron_rows_kernel(BatchDev B, OutDev O, int32_t* __restrict__ nhv, SolveParams o, const double* __restrict__ theta0,
                                                            const int32_t* __restrict__ list, int count, int row_bytes) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x, row = lane >> 4, rl = lane & (ROW - 1);
  const int ic = o.has_intercept ? 1 : 0;
  const int first = TRON_ROWS * (int)blockIdx.x;
  const bool has_w = B.weight != nullptr;

  // the row's own view: per-lane values, equal inside a row (a row without an entity keeps n = p = 0 and is born finished)
  TronRowView V;
  {
    double* const z = reinterpret_cast<double*>(smem);
    float* const zf = reinterpret_cast<float*>(smem);
    int32_t* const zi = reinterpret_cast<int32_t*>(smem);
    V.P = EntityView{0, 0, 0, ic, zi, zi, zf, zi, zi, zf, zf, zf, zf};
    V.W = TronWork{z, z, z, z, z, z, z, z, z, z};
    V.has_w = has_w;
  }
  int64_t my_e = 0, my_c0 = 0;
  bool valid = false;
  int n_max = 0, p_max = 0;
#pragma unroll
  for (int r = 0; r < TRON_ROWS; ++r) {
    if (first + r >= count) break;
    const int64_t e = list[first + r];
    const int64_t r0 = B.ent_row_ptr[e], z0 = B.ent_nnz_ptr[e], f0 = B.ent_feat_ptr[e];
    const int n = (int)(B.ent_row_ptr[e + 1] - r0);
    const int nnz = (int)(B.ent_nnz_ptr[e + 1] - z0);
    const int d = (int)(B.ent_feat_ptr[e + 1] - f0);
    const int p = d + ic;
    const int64_t c0 = f0 + e * ic;
    n_max = n > n_max ? n : n_max;
    p_max = p > p_max ? p : p_max;

    // the carve-up of re_tron_wave_kernel in block r: must match solver_lds_bytes() at m = 0 with TRON_P_VECTORS and TRON_N_VECTORS
    TronWork W;
    double* dp = reinterpret_cast<double*>(smem + (size_t)r * row_bytes);
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
    float* s_w = s_o;
    if (has_w) { s_w = fp; fp += n; }
    int32_t* ip = reinterpret_cast<int32_t*>(fp);
    int32_t* s_csr_col = ip; ip += nnz;
    int32_t* s_csc_row = ip; ip += nnz;
    int32_t* s_row_ptr = ip; ip += n + 1;
    int32_t* s_col_ptr = ip; ip += d + 1;

    for (int k = lane; k < nnz; k += WAVE) {
      s_csr_val[k] = B.csr_val[z0 + k];
      s_csr_col[k] = B.csr_col[z0 + k];
      s_csc_val[k] = B.csc_val[z0 + k];
      s_csc_row[k] = B.csc_row[z0 + k];
    }
    for (int i = lane; i < n; i += WAVE) {
      s_y[i] = B.y[r0 + i];
      s_o[i] = B.offset[r0 + i];
      if (has_w) s_w[i] = B.weight[r0 + i];
    }
    for (int i = lane; i <= n; i += WAVE) s_row_ptr[i] = B.row_ptr[r0 + e + i];
    for (int i = lane; i <= d; i += WAVE) s_col_ptr[i] = B.col_ptr[z0 + e + i];
    for (int j = lane; j < p; j += WAVE) W.xt[j] = theta0 ? theta0[c0 + j] : 0.0;
    if (row == r) {
      V.P = EntityView{n, d, p, ic, s_row_ptr, s_csr_col, s_csr_val, s_col_ptr, s_csc_row, s_csc_val, s_y, s_o, s_w};
      V.W = W;
      my_e = e;
      my_c0 = c0;
      valid = true;
    }
  }
  const bool n_one = n_max <= ROW, p_one = p_max <= ROW;   // wavefront-uniform: which partials the reductions carry

  TronRowState S{};
  S.phase = valid ? TRON_ROW_FIRST : TRON_ROW_DONE;
  S.status = valid ? -1 : 0;
  while (__any(S.phase != TRON_ROW_DONE)) {
    wave_lds_fence();   // the staged block; the trial point or the CG direction the row pass gathers
    const double nf = tron_rows_pass<LOSS>(V, o, rl, S.phase, n_one, p_one);
    tron_rows_advance(V, o, rl, p_one, nf, S);
  }
  wave_lds_fence();

  if (valid) {
    const int p = V.P.p;
    for (int j = rl; j < p; j += ROW) {
      const double v = V.W.x[j];
      if (O.theta) O.theta[my_c0 + j] = v;
      if (O.theta_thr) O.theta_thr[my_c0 + j] = (fabs(v) <= o.threshold) ? 0.0 : v;
    }
    if (rl == 0) {
      if (O.fval) O.fval[my_e] = S.F;
      if (O.gnorm) O.gnorm[my_e] = S.gmax;
      if (O.nit) O.nit[my_e] = S.nit;
      if (O.nfev) O.nfev[my_e] = S.nfev;
      if (O.status) O.status[my_e] = S.status;
      if (nhv) nhv[my_e] = S.nhv;
    }
  }
  if (o.variance_mode == GDMIX_RE_VAR_SIMPLE && O.variance) tron_rows_variance_simple(V, o, rl, n_one, V.W.dc, O.variance + my_c0);
}

hipError_t launch_tron_rows(const ListsArgs& a, int32_t* nhv, const int32_t* list, int count, int row_bytes, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  return with_loss(a.P.loss, [&](auto L) {
    constexpr int LOSS = decltype(L)::value;
    static DynLdsOnce lds_attr;   // one per instantiation of this lambda, i.e. per kernel
    if (hipError_t rc = lds_attr.set(reinterpret_cast<const void*>(re_tron_rows_kernel<LOSS>)); rc != hipSuccess) return rc;
    hipLaunchKernelGGL((re_tron_rows_kernel<LOSS>), dim3((count + TRON_ROWS - 1) / TRON_ROWS), dim3(WAVE), (size_t)TRON_ROWS * row_bytes, s, a.B, a.O, nhv, a.P,
                       a.theta0, list, count, row_bytes);
    return hipGetLastError();
  });
}

}  // namespace gdmix
