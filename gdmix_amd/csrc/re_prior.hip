// re_prior.hip — incremental training: the change of variables that turns "L2 centred on a prior model, weighted by its precisions"
// into the objective every solve kernel already has (include/gdmix_re.h, "incremental training", states the definition, the
// substitution and its roundings). This unit adds symbols only: no kernel of another unit changes, and no solve kernel knows of priors.
//
//   prior_csr_kernel      one lane per sample row over the whole batch, the entity search of re_score_kernel (re_search.hpp). A row of at
//                         most PRIOR_LONG_ROW non-zeros is walked by its lane (neighbouring lanes own neighbouring rows: a wavefront's
//                         loads cover one contiguous piece of csr_val / csr_col; four non-zeros per load where the row allows it); a
//                         longer row is taken by the whole wavefront, 4 non-zeros per lane and step, its partial sums added by
//                         wave_sum. Each non-zero is read once: x' = (float)((double)x * s) goes to the new csr_val, x * mu into the row's
//                         fp64 sum, which ends as offset' = (float)(mu_0 + sum + offset). mu and s are gathered at (coefficient base +
//                         csr_col): 16 B per non-zero from an array the rows of one entity share (L2). Work per wavefront is bounded by
//                         its 64 rows, whatever the entity sizes are; no atomics.
//   prior_csc_kernel      four consecutive non-zeros of csc_val per lane (one 16-byte load and store when they share a column): the entity
//                         by bisection of ent_nnz_ptr (wavefront-wide first), the column by bisection of the entity's col_ptr (at most
//                         log2(d_e) probes of a list the neighbouring lanes probe too). Dealt by non-zero: a column of 54 k entries or a
//                         head entity of 2^20 non-zeros is as many lanes as its non-zeros need.
//   prior_restore_kernel  one lane per coefficient: theta = mu + s phi, the threshold on theta, variance = s^2 var'.
#include <stdint.h>
#include <math.h>

#include "re_internal.hpp"
#include "re_search.hpp"

namespace gdmix {

constexpr int PRIOR_LONG_ROW = 32;     // rows above this many non-zeros are walked by their whole wavefront

// one non-zero: the transformed value, and its term of the row's shift
__device__ __forceinline__ float prior_one(float x, int32_t col, const double* __restrict__ mu, const double* __restrict__ sc, double& acc) {
  acc = fma((double)x, mu[col], acc);
  return (float)__dmul_rn((double)x, sc[col]);
}

// four non-zeros at a 16-byte boundary, in the row's order
__device__ __forceinline__ void prior_four(const float* __restrict__ val, const int32_t* __restrict__ col, int64_t j, const double* __restrict__ mu,
                                           const double* __restrict__ sc, float* __restrict__ out, double& acc) {
  const float4 v = *reinterpret_cast<const float4*>(val + j);
  const int4 c = *reinterpret_cast<const int4*>(col + j);
  float4 r;
  r.x = prior_one(v.x, c.x, mu, sc, acc);
  r.y = prior_one(v.y, c.y, mu, sc, acc);
  r.z = prior_one(v.z, c.z, mu, sc, acc);
  r.w = prior_one(v.w, c.w, mu, sc, acc);
  *reinterpret_cast<float4*>(out + j) = r;
}

// VEC: csr_val, csr_col and the new csr_val are 16-byte aligned (the host checks), so an index that is a multiple of 4 is a 16-byte address
template <bool VEC>
__global__ __launch_bounds__(256) void prior_csr_kernel(BatchDev B, int64_t E, int64_t N, int ic, const double* __restrict__ mean,
                                                        const double* __restrict__ scale, float* __restrict__ val_out, float* __restrict__ offset_out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t gf = g - lane;
  if (gf >= N) return;            // whole wavefronts only: every lane of a wavefront that stays takes part in the long rows below
  const int64_t e = wave_entity_of(B.ent_row_ptr, E, N, gf, g, lane);
  const bool live = g < N;
  int64_t a = 0, b = 0, cb = 0;   // the row's non-zeros [a, b) of the batch, the entity's first feature coefficient
  double acc = 0.0, off = 0.0;
  if (live) {
    const int64_t r0 = B.ent_row_ptr[e], z0 = B.ent_nnz_ptr[e];
    const int64_t c0 = B.ent_feat_ptr[e] + e * ic;
    const int32_t* rp = B.row_ptr + r0 + e + (g - r0);
    a = z0 + rp[0];
    b = z0 + rp[1];
    cb = c0 + ic;
    off = (double)B.offset[g];
    if (ic) acc = mean[c0];
  }
  const bool long_row = live && (b - a) > PRIOR_LONG_ROW;
  if (live && !long_row) {
    const double* __restrict__ mu = mean + cb;
    const double* __restrict__ sc = scale + cb;
    int64_t j = a;
    while (j < b) {
      if (VEC && (j & 3) == 0 && j + 4 <= b) {
        prior_four(B.csr_val, B.csr_col, j, mu, sc, val_out, acc);
        j += 4;
      } else {
        val_out[j] = prior_one(B.csr_val[j], B.csr_col[j], mu, sc, acc);
        ++j;
      }
    }
  }
  unsigned long long todo = __ballot(long_row);      // uniform: the loop below is taken by all 64 lanes together
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int64_t ra = __shfl(a, src), rb = __shfl(b, src), rc = __shfl(cb, src);
    const double* __restrict__ mu = mean + rc;
    const double* __restrict__ sc = scale + rc;
    double part = 0.0;
    for (int64_t j = (ra & ~(int64_t)3) + 4 * lane; j < rb; j += 4 * WAVE) {
      if (VEC && j >= ra && j + 4 <= rb) {
        prior_four(B.csr_val, B.csr_col, j, mu, sc, val_out, part);
      } else {
        for (int k = 0; k < 4; ++k) {
          const int64_t jj = j + k;
          if (jj >= ra && jj < rb) val_out[jj] = prior_one(B.csr_val[jj], B.csr_col[jj], mu, sc, part);
        }
      }
    }
    const double total = wave_sum(part);
    if (lane == src) acc += total;
  }
  if (live) offset_out[g] = (float)(acc + off);
}

// where non-zero k of the CSC copy lies: its entity (within [e_lo, e_hi]), the end of its column, the scale of its coefficient
struct PriorColumn { int64_t e; int64_t col_end; double s; };
__device__ __forceinline__ PriorColumn prior_locate(const BatchDev& B, int64_t e_lo, int64_t e_hi, int ic, const double* __restrict__ scale, int64_t k) {
  PriorColumn L;
  L.e = entity_of_sample(B.ent_nnz_ptr, e_lo, e_hi, k);
  const int64_t z0 = B.ent_nnz_ptr[L.e], f0 = B.ent_feat_ptr[L.e];
  const int d = (int)(B.ent_feat_ptr[L.e + 1] - f0);
  const int32_t* __restrict__ cp = B.col_ptr + z0 + L.e;      // d + 1 entity-relative offsets, cp[0] = 0
  const int32_t rel = (int32_t)(k - z0);
  int lo = 0, hi = d - 1;                                      // the largest c with cp[c] <= rel
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cp[mid] <= rel) lo = mid; else hi = mid - 1;
  }
  L.col_end = z0 + cp[lo + 1];
  L.s = scale[f0 + L.e * ic + ic + lo];
  return L;
}

template <bool VEC>
__global__ __launch_bounds__(256) void prior_csc_kernel(BatchDev B, int64_t E, int64_t Z, int ic, const double* __restrict__ scale,
                                                        float* __restrict__ val_out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t kf = (t - lane) * 4;       // the wavefront's 256 consecutive non-zeros [kf, kf + 256)
  if (kf >= Z) return;
  const int64_t kl = (kf + 4 * WAVE - 1 < Z) ? kf + 4 * WAVE - 1 : Z - 1;
  const int64_t e_lo = wave_entity_of_sample(B.ent_nnz_ptr, 0, E - 1, kf, lane);
  const int64_t e_hi = wave_entity_of_sample(B.ent_nnz_ptr, e_lo, E - 1, kl, lane);
  const int64_t k0 = t * 4;
  if (k0 >= Z) return;
  PriorColumn L = prior_locate(B, e_lo, e_hi, ic, scale, k0);
  if (VEC && k0 + 4 <= Z && k0 + 4 <= L.col_end) {
    const float4 v = *reinterpret_cast<const float4*>(B.csc_val + k0);
    float4 r;
    r.x = (float)__dmul_rn((double)v.x, L.s);
    r.y = (float)__dmul_rn((double)v.y, L.s);
    r.z = (float)__dmul_rn((double)v.z, L.s);
    r.w = (float)__dmul_rn((double)v.w, L.s);
    *reinterpret_cast<float4*>(val_out + k0) = r;
    return;
  }
  const int64_t k1 = (k0 + 4 < Z) ? k0 + 4 : Z;
  for (int64_t k = k0; k < k1; ++k) {
    if (k >= L.col_end) L = prior_locate(B, L.e, e_hi, ic, scale, k);
    val_out[k] = (float)__dmul_rn((double)B.csc_val[k], L.s);
  }
}

__global__ __launch_bounds__(256) void prior_restore_kernel(int64_t P, const double* __restrict__ mean, const double* __restrict__ scale, double threshold,
                                                            const double* phi, const double* var_phi, double* theta, double* theta_thr, double* variance) {
#pragma clang fp contract(off)      // mu + s phi in two roundings, never one fused multiply-add: the host restatement gets the same bits
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= P) return;
  const double s = scale[j];
  const double v = mean[j] + s * phi[j];
  const double var = (variance && var_phi) ? (s * s) * var_phi[j] : 0.0;
  if (theta) theta[j] = v;
  // threshold_coefficients: |x| <= threshold -> 0.0, intercept included (util/model_utils.py:4-12), on theta
  if (theta_thr) theta_thr[j] = (fabs(v) <= threshold) ? 0.0 : v;
  if (variance && var_phi) variance[j] = var;
}

static inline size_t prior_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
static inline bool prior_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace gdmix

using namespace gdmix;

extern "C" {

GDMIX_API size_t gdmix_re_prior_workspace_bytes(const gdmix_re_packed* packed) {
  if (!packed || packed->Z < 0 || packed->N < 0) return 0;
  return 2 * prior_align((size_t)packed->Z * sizeof(float)) + prior_align((size_t)packed->N * sizeof(float));
}

GDMIX_API int gdmix_re_prior_apply(gdmix_re_ctx* ctx, const gdmix_re_packed* packed, int has_intercept, const double* mean, const double* scale,
                                   void* workspace, size_t workspace_bytes, gdmix_re_packed* out, void* stream) {
  if (!ctx || !packed || !out) { set_error("gdmix_re_prior_apply: NULL argument"); return GDMIX_RE_EINVAL; }
  if (packed->E < 0 || packed->N < 0 || packed->Z < 0 || packed->D < 0) { set_error("gdmix_re_prior_apply: bad batch"); return GDMIX_RE_EINVAL; }
  const size_t need = gdmix_re_prior_workspace_bytes(packed);
  if (need > 0 && (!workspace || workspace_bytes < need)) {
    set_error("gdmix_re_prior_apply: workspace of %zu bytes, %zu needed (gdmix_re_prior_workspace_bytes)", workspace ? workspace_bytes : (size_t)0, need);
    return GDMIX_RE_ENOMEM;
  }
  if (!prior_aligned16(workspace)) { set_error("gdmix_re_prior_apply: the workspace must be 16-byte aligned"); return GDMIX_RE_EINVAL; }
  const int64_t E = packed->E, N = packed->N, Z = packed->Z;
  const int ic = has_intercept ? 1 : 0;
  if (E > 0 && N > 0) {
    if (!packed->ent_row_ptr || !packed->ent_nnz_ptr || !packed->ent_feat_ptr || !packed->row_ptr || !packed->offset ||
        (Z > 0 && (!packed->csr_col || !packed->csr_val || !packed->col_ptr || !packed->csc_val))) {
      set_error("gdmix_re_prior_apply: NULL array in the packed batch");
      return GDMIX_RE_EINVAL;
    }
    if ((packed->D + E * ic > 0) && (!mean || !scale)) { set_error("gdmix_re_prior_apply: NULL mean or scale"); return GDMIX_RE_EINVAL; }
    if ((N + 255) / 256 > 0x7fffffffLL || (Z + 1023) / 1024 > 0x7fffffffLL) { set_error("gdmix_re_prior_apply: too many samples or non-zeros"); return GDMIX_RE_ERANGE; }
  }
  char* w = static_cast<char*>(workspace);
  float* csr_out = reinterpret_cast<float*>(w);
  float* csc_out = reinterpret_cast<float*>(w + prior_align((size_t)Z * sizeof(float)));
  float* off_out = reinterpret_cast<float*>(w + 2 * prior_align((size_t)Z * sizeof(float)));
  gdmix_re_packed result = *packed;
  result.csr_val = csr_out;
  result.csc_val = csc_out;
  result.offset = off_out;
  if (E > 0 && N > 0) {
    HIP_TRY(hipSetDevice(ctx->impl.device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const BatchDev B = batch_dev(packed);
    const unsigned row_blocks = (unsigned)((N + 255) / 256);
    if (prior_aligned16(packed->csr_val) && prior_aligned16(packed->csr_col))
      hipLaunchKernelGGL((prior_csr_kernel<true>), dim3(row_blocks), dim3(256), 0, s, B, E, N, ic, mean, scale, csr_out, off_out);
    else
      hipLaunchKernelGGL((prior_csr_kernel<false>), dim3(row_blocks), dim3(256), 0, s, B, E, N, ic, mean, scale, csr_out, off_out);
    if (Z > 0) {
      const unsigned nz_blocks = (unsigned)((Z + 1023) / 1024);
      if (prior_aligned16(packed->csc_val))
        hipLaunchKernelGGL((prior_csc_kernel<true>), dim3(nz_blocks), dim3(256), 0, s, B, E, Z, ic, scale, csc_out);
      else
        hipLaunchKernelGGL((prior_csc_kernel<false>), dim3(nz_blocks), dim3(256), 0, s, B, E, Z, ic, scale, csc_out);
    }
    HIP_TRY(hipGetLastError());
  }
  *out = result;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_prior_restore(gdmix_re_ctx* ctx, const gdmix_re_packed* packed, int has_intercept, const double* mean, const double* scale,
                                     double threshold, const double* phi, const double* var_phi, double* theta, double* theta_thr,
                                     double* variance, void* stream) {
  if (!ctx || !packed) { set_error("gdmix_re_prior_restore: NULL argument"); return GDMIX_RE_EINVAL; }
  if (packed->E < 0 || packed->D < 0) { set_error("gdmix_re_prior_restore: bad batch"); return GDMIX_RE_EINVAL; }
  const int64_t P = packed->D + (has_intercept ? packed->E : 0);
  if (P == 0) return GDMIX_RE_OK;
  if (!mean || !scale || !phi) { set_error("gdmix_re_prior_restore: NULL mean, scale or phi"); return GDMIX_RE_EINVAL; }
  if (variance && !var_phi) { set_error("gdmix_re_prior_restore: variance asked for without var_phi"); return GDMIX_RE_EINVAL; }
  if ((P + 255) / 256 > 0x7fffffffLL) { set_error("gdmix_re_prior_restore: too many coefficients"); return GDMIX_RE_ERANGE; }
  HIP_TRY(hipSetDevice(ctx->impl.device));
  hipLaunchKernelGGL(prior_restore_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), P, mean, scale, threshold, phi,
                     var_phi, theta, theta_thr, variance);
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

}  // extern "C"
