// re_search.hpp — which entity owns item g of a batch, by bisection of an offsets array (ent_row_ptr for samples, ent_feat_ptr for
// coefficient slots). One thread per item over the whole batch, whatever the entity sizes are: the wavefront's first and last item by
// a 64-way search of the whole wavefront, each lane then within that range, which is a handful of entities or a single one.
// Used by re_score_kernel (re_solve.hip) and by the join and score kernels of the sweep (re_sweep.hip).
#pragma once
#include "re_device.hpp"

namespace gdmix {

// largest e in [lo, hi] with ptr[e] <= g (ptr[lo] <= g)
__device__ __forceinline__ int64_t entity_of_sample(const int64_t* __restrict__ ptr, int64_t lo, int64_t hi, int64_t g) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (ptr[mid] <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The same by a whole wavefront (uniform arguments, all lanes active): 64 probes per step instead of one, so a
// million entities take four dependent loads instead of twenty.
__device__ __forceinline__ int64_t wave_entity_of_sample(const int64_t* __restrict__ ptr, int64_t lo, int64_t hi, int64_t g, int lane) {
  while (lo < hi) {
    const int64_t step = (hi - lo + WAVE - 1) / WAVE;
    const int64_t probe = lo + (int64_t)(lane + 1) * step;
    const bool le = ptr[probe < hi ? probe : hi] <= g;     // non-decreasing in the lane index
    const int c = __popcll(__ballot(le));
    const int64_t below = lo + (int64_t)c * step;           // last probe that is <= g (lo itself when c == 0)
    const int64_t above = lo + (int64_t)(c + 1) * step;     // first probe that is > g
    const int64_t nhi = (c < WAVE && above <= hi) ? above - 1 : hi;
    lo = below < hi ? below : hi;
    hi = (c == WAVE) ? lo : nhi;
  }
  return lo;
}

// the entity of item g of a wavefront's 64 consecutive items [gf, gf + 64) under the offsets `ptr` ([E + 1], items in all: M)
__device__ __forceinline__ int64_t wave_entity_of(const int64_t* __restrict__ ptr, int64_t E, int64_t M, int64_t gf, int64_t g, int lane) {
  const int64_t gl = (gf + WAVE - 1 < M) ? gf + WAVE - 1 : M - 1;
  const int64_t e_lo = wave_entity_of_sample(ptr, 0, E - 1, gf, lane);
  const int64_t w_hi = (e_lo + WAVE < E) ? e_lo + WAVE : E - 1;   // 64 items span at most 64 non-empty entities
  const int64_t e_hi = wave_entity_of_sample(ptr, e_lo, (ptr[w_hi] > gl) ? w_hi : E - 1, gl, lane);
  return entity_of_sample(ptr, e_lo, e_hi, g < M ? g : gl);
}

}  // namespace gdmix
