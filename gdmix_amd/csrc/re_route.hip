// re_route.hip — which class an entity of a batch goes to, and which stream a class runs on.
//
//   make_class_table      the routing rules of one solve (context settings + options) as the kernels read them
//   re_classify_kernel    a class per entity, the classes' counts and the tall classes' candidates    \
//   class_base_kernel     the batch's tall thresholds, then bases and cursors                          > route(): ClassCounts
//   re_order_kernel       `order`: the entities class by class                                         /
//   plan_launches         class -> (range of `order`, stream): host arithmetic only, no HIP call
#include <stdlib.h>

#include "re_internal.hpp"
#include "re_solve_team.hpp"

namespace gdmix {

int make_class_table(const gdmix_ctx_impl* ci, const gdmix_re_opts* opts, ClassTable* out) {
  ClassTable& tab = *out;
  for (int c = 0; c < GDMIX_RE_NUM_CLASSES; ++c) {
    const ClassDesc& d = kClasses[c];
    tab.kind[c] = d.kind;
    tab.ncap[c] = d.ncap;
    tab.zcap[c] = d.zcap;
    int lds = d.lds;
    const int gl = d.lanes;
    if (lds > 0 && gl > 0)   // LDS of a whole workgroup: the entities of a wavefront, or the wavefronts of an entity
      lds = (gl >= WAVE ? 1 : WAVE / gl) * quad_layout(gl * d.epl, d.ncap, d.zcap, gl > WAVE ? gl / WAVE : 1).bytes;
    bool on = lds > 0 && (lds <= ci->wave_lds_limit || (gl > WAVE && ci->wave_lds_limit >= 65536 && lds <= 160 * 1024));
    if (gl > 0 && !(ci->kernel_mask & 4)) on = false;
    if (d.kind == KIND_WLDS && !(ci->kernel_mask & 2)) on = false;
    tab.lds_bytes[c] = on ? lds : 0;
  }
  // the compact-form team kernels keep TEAM_MCAP history pairs
  tab.giant_nnz = opts->m <= TEAM_MCAP ? ci->giant_nnz : 0;
  tab.team_nnz = opts->m <= TEAM_MCAP ? ci->team_nnz : 0;
  tab.tall_min_n = ci->tall_min_n;
  tab.tall_split_n = ci->tall_split_n;
  tab.tall_adapt_limit = ci->tall_split_set ? 0 : ci->tall_adapt_limit;   // an explicit split is kept, whatever its value
  {   // > 0: adaptive from team_n on; < 0: everything from -team_n on (tests); never below TALL_TEAM_MIN_N samples
    const int tn = ci->tall_team_n;
    tab.tall_team_n = tn > 0 ? tn : -tn;
    if (tab.tall_team_n > 0 && tab.tall_team_n < TALL_TEAM_MIN_N) tab.tall_team_n = TALL_TEAM_MIN_N;
    tab.tall_team_limit = tn > 0 ? ci->tall_team_limit : 0;
  }
  // the mid class adapts with the split: a caller who pinned the split (gdmix_re_set_tall_split_n) pinned the routing — no per-batch class
  tab.tall_mid_n = (ci->tall_mid_n < 0 && ci->tall_split_set) ? 0 : ci->tall_mid_n;
  // the narrow kernel: four rows of its layout per workgroup, within the same LDS limit as the classes
  tab.narrow = (ci->narrow && tab.lds_bytes[NARROW_HOST_CLASS] > 0 &&
                (WAVE / NARROW_LANES) * quad_layout(NARROW_LANES * NARROW_EPL, NARROW_NCAP, NARROW_ZCAP).bytes <= ci->wave_lds_limit) ? 1 : 0;
  if (opts->sum_loss) {
    // the fixed-effect objective lives in the team kernels only: every entity goes device-wide, one after another
    if (opts->m > TEAM_MCAP) { set_error("sum_loss needs m <= %d", TEAM_MCAP); return GDMIX_RE_EINVAL; }
    if (opts->variance_mode != GDMIX_RE_VAR_NONE) { set_error("variance is not available with sum_loss"); return GDMIX_RE_EINVAL; }
    tab.giant_nnz = 1;
  }
  // a loss without sum_loss is the random effect's: the normal class table, every launcher picks its <LOSS> kernels by P.loss (with_loss)
  return GDMIX_RE_OK;
}

// ---------------------------------------------------------------------------------------------------
// classification
// ---------------------------------------------------------------------------------------------------
__global__ void re_classify_kernel(const int64_t* __restrict__ ent_row_ptr, const int64_t* __restrict__ ent_nnz_ptr,
                                   const int64_t* __restrict__ ent_feat_ptr, int64_t E, int ic, int m, bool has_w,
                                   ClassTable tab, int32_t* __restrict__ cls_out, ClassCounts* __restrict__ counts) {
  __shared__ int32_t local[GDMIX_RE_NUM_CLASSES];
  __shared__ int32_t tall_ge[TALL_ADAPT_STEPS], team_ge[TALL_TEAM_STEPS], mid_ge[TALL_MID_STEPS];
  if (threadIdx.x < GDMIX_RE_NUM_CLASSES) local[threadIdx.x] = 0;
  if (threadIdx.x < TALL_ADAPT_STEPS) tall_ge[threadIdx.x] = 0;
  if (threadIdx.x < TALL_TEAM_STEPS) team_ge[threadIdx.x] = 0;
  if (threadIdx.x < TALL_MID_STEPS) mid_ge[threadIdx.x] = 0;
  __syncthreads();
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(ent_row_ptr[e + 1] - ent_row_ptr[e]);
    const int z = (int)(ent_nnz_ptr[e + 1] - ent_nnz_ptr[e]);
    const int d = (int)(ent_feat_ptr[e + 1] - ent_feat_ptr[e]);
    const int p = d + ic;
    int c = BLOCK_CLASS;
    // cheapest first: the group kernel with the fewest lanes and coefficient slots that holds the entity, smallest LDS bucket;
    // then the LDS-resident wavefront kernel (any m); the one-workgroup team kernel takes what is left
    const size_t wlds_bytes = wave_lds_bytes(p, n, z, d, m, has_w);
    for (int k = 0; k < BLOCK_CLASS; ++k) {
      if (tab.lds_bytes[k] <= 0) continue;
      const int kind = tab.kind[k];
      if (group_lanes(kind) > 0) {
        const int cap = group_lanes(kind) * group_epl(kind);
        if (m <= M_REG && p <= cap && n <= tab.ncap[k] && z <= tab.zcap[k]) { c = k; break; }
      } else if (kind == KIND_WLDS) {
        if (wlds_bytes <= (size_t)tab.lds_bytes[k]) { c = k; break; }
      }
    }
    if (tab.tall_min_n > 0 && m <= M_REG && p <= TALL_MAX_P && n >= tab.tall_min_n && !(tab.giant_nnz > 0 && z >= tab.giant_nnz)) c = (n >= tab.tall_split_n) ? TALL_CLASS
        : (tall_resident_bytes(1, tall_sets(1, p), d, n, z, has_w) <= (size_t)TALL_LEAN_ARENA ? TALL_L_CLASS : TALL_S_CLASS);
    else if (tab.giant_nnz > 0 && z >= tab.giant_nnz) c = GIANT_CLASS;
    else if (c == BLOCK_CLASS || (tab.team_nnz > 0 && z >= tab.team_nnz)) {
      // too large for a wavefront group: a team of CUs, sized by the non-zeros (streaming bandwidth)
      if (tab.team_nnz > 0 && z >= tab.team_nnz)
        c = (z >= 128 * tab.team_nnz) ? TEAM8_CLASS : ((z >= 8 * tab.team_nnz) ? TEAM32_CLASS : TEAM128_CLASS);
    }
    cls_out[e] = (c == NARROW_HOST_CLASS && tab.narrow && narrow_fits(p, n, z)) ? (c | NARROW_FLAG) : c;
    atomicAdd(&local[c], 1);
    if (c == TALL_S_CLASS && tab.tall_adapt_limit > 0 && n >= tall_adapt_n(0)) {
#pragma unroll
      for (int k = 0; k < TALL_ADAPT_STEPS; ++k)
        if (n >= tall_adapt_n(k)) atomicAdd(&tall_ge[k], 1);
    }
    if (c == TALL_S_CLASS && tab.tall_mid_n < 0 && n >= tall_mid_step(0)) {      // candidates of the mid class (class_base_kernel decides)
#pragma unroll
      for (int k = 0; k < TALL_MID_STEPS; ++k)
        if (n >= tall_mid_step(k)) atomicAdd(&mid_ge[k], 1);
    }
    if (c == TALL_S_CLASS && tab.tall_mid_n > 0 && n >= tab.tall_mid_n) atomicAdd(&mid_ge[0], 1);      // a fixed threshold: slot 0 counts them
    if (c == TALL_CLASS && tab.tall_team_n > 0 && n >= tab.tall_team_n) {   // candidates of the team class (class_base_kernel decides)
#pragma unroll
      for (int k = 0; k < TALL_TEAM_STEPS; ++k)
        if ((int64_t)n >= ((int64_t)tab.tall_team_n << k)) atomicAdd(&team_ge[k], 1);
    }
    if (c >= TEAM128_CLASS && c <= TEAM8_CLASS) {
      // work of the team tiers (non-zeros: total and largest entity), for the choice of the team size; rare entities
      atomicAdd(&counts->team_nnz_total[c], (unsigned long long)z);
      atomicMax(&counts->largest_nnz(c), z);
    }
  }
  __syncthreads();
  if (threadIdx.x < GDMIX_RE_NUM_CLASSES && local[threadIdx.x]) atomicAdd(&counts->count[threadIdx.x], local[threadIdx.x]);
  if (threadIdx.x < TALL_ADAPT_STEPS && tall_ge[threadIdx.x]) atomicAdd(&counts->tall.tall_ge[threadIdx.x], tall_ge[threadIdx.x]);
  if (threadIdx.x < TALL_TEAM_STEPS && team_ge[threadIdx.x]) atomicAdd(&counts->tall.team_ge[threadIdx.x], team_ge[threadIdx.x]);
  if (threadIdx.x < TALL_MID_STEPS && mid_ge[threadIdx.x]) atomicAdd(&counts->tall.mid_ge[threadIdx.x], mid_ge[threadIdx.x]);
}

// The batch's tall thresholds (they move entities between the tall classes: the counts follow here, the entities in
// re_order_kernel), then count -> exclusive bases, cursors = 0.
__global__ void class_base_kernel(ClassCounts* cc, int tall_adapt_limit, int tall_adapt_small, int tall_team_n, int tall_team_limit, int tall_mid_n) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    // The split between the one-wavefront and the eight-wavefront tall kernels (4 096 samples by default: right for a batch with
    // thousands of tall entities, where a CU is better spent on eight entities than on one) is lowered for a batch whose
    // eight-wavefront class stays small anyway — a share of a strongly scaled job: 17 k users, 5 - 11 of them above 4 096 samples, and
    // the step lasts as long as ONE wavefront needs for a 4 000-sample entity (tools/share_timeline.py). The lowest of 512 / 1 024 /
    // 2 048 that keeps the class within `tall_adapt_limit` workgroups (one per CU) wins; re_order_kernel moves the entities.
    int32_t* const count = cc->count;
    TallRouting& t = cc->tall;
    // The team class (four workgroups per entity) takes the tallest entities of the batch: those above the lowest of
    // tall_team_n x {1, 2, 4} samples that keeps it within one round of teams — a batch with more than that above the highest
    // threshold has no team class (throughput binds it, not one entity's chain). No limit: everything from tall_team_n on.
    int team_from = 0;
    if (tall_team_n > 0) {
      if (tall_team_limit <= 0) { if (t.team_ge[0] > 0) team_from = tall_team_n; }
      else
        for (int k = 0; k < TALL_TEAM_STEPS && team_from == 0; ++k)
          if (t.team_ge[k] > 0 && t.team_ge[k] <= tall_team_limit) team_from = tall_team_n << k;
      if (team_from > 0) {
        const int moved = t.team_ge[team_from == tall_team_n ? 0 : (team_from == 2 * tall_team_n ? 1 : 2)];
        count[TALL_T_CLASS] += moved;
        count[TALL_CLASS] -= moved;
      }
    }
    t.team_from = team_from;
    // ... and only for a batch whose one-wavefront class is small itself (at most `tall_adapt_small` entities: two rounds of its launch):
    // a whole population is bound by throughput, where the one-wavefront kernel is the better use of a CU (MovieLens-20M per user on one
    // GPU, 14 k such entities: 8.9 ms with the split at 4 096, 9.4 ms when 224 more entities took a CU each)
    int split = 0;
    if (tall_adapt_limit > 0 && count[TALL_S_CLASS] <= tall_adapt_small) {
      for (int k = 0; k < TALL_ADAPT_STEPS && split == 0; ++k)
        if (t.tall_ge[k] > 0 && count[TALL_CLASS] + t.tall_ge[k] <= tall_adapt_limit) {
          split = tall_adapt_n(k);
          count[TALL_CLASS] += t.tall_ge[k];
          count[TALL_S_CLASS] -= t.tall_ge[k];
        }
    }
    t.split = split;
    // The mid class (four wavefronts per entity, two workgroups per CU) takes the largest one-wavefront entities BELOW the split: the
    // lowest threshold of tall_mid_step() that keeps it within one round of its launch (-tall_mid_n workgroups), in a small batch only
    // (same test as the split: a whole population is bound by throughput). tall_mid_n > 0: everything from that many samples on.
    int mid_from = 0;
    // entities of at least `split` samples have left the one-wavefront class (counted with the same rule: tall_ge[k] of the chosen split)
    const int gone = split > 0 ? t.tall_ge[split == tall_adapt_n(0) ? 0 : (split == tall_adapt_n(1) ? 1 : 2)] : 0;
    if (tall_mid_n > 0) {
      const int cnt = (split > 0 && split <= tall_mid_n) ? 0 : t.mid_ge[0] - gone;
      if (cnt > 0) { mid_from = tall_mid_n; count[TALL_M_CLASS] += cnt; count[TALL_S_CLASS] -= cnt; }
    } else if (tall_mid_n < 0 && count[TALL_S_CLASS] <= tall_adapt_small) {
      for (int k = 0; k < TALL_MID_STEPS && mid_from == 0; ++k) {
        if (split > 0 && tall_mid_step(k) >= split) break;
        const int cnt = t.mid_ge[k] - gone;
        if (cnt > 0 && cnt <= -tall_mid_n) { mid_from = tall_mid_step(k); count[TALL_M_CLASS] += cnt; count[TALL_S_CLASS] -= cnt; }
      }
    }
    t.mid_from = mid_from;
    int run = 0;
#pragma unroll   // (all 40, as the compiler did of its own accord while the rows were offsets from one pointer: one thread, loads up front)
    for (int c = 0; c < GDMIX_RE_NUM_CLASSES; ++c) { cc->base[c] = run; run += count[c]; cc->cursor[c] = 0; }
  }
}

// order[base[c] + k] = e. Position inside a class is by ticket: the launch order inside a class
// does not influence any entity's result (every entity is solved independently and deterministically),
// only which workgroup picks it up. Tickets are taken per workgroup (LDS histogram, then one global
// atomic per class per workgroup): per-entity global atomics on 8 addresses serialise in L2.
// The narrow entities of class NARROW_HOST_CLASS (marked by re_classify_kernel; the mark is taken off cls here) fill the class's segment
// from the front, the others from the back, each with tickets of its own: the front part is the narrow kernel's launch (narrow_count).
// split > 0 (class_base_kernel lowered the split of the tall classes for this batch): one-wavefront tall entities of at least
// `split` samples move to the eight-wavefront class here, in cls as well (the per-class times are attributed through it).
__global__ __launch_bounds__(256) void re_order_kernel(int32_t* __restrict__ cls, int64_t E, ClassCounts* __restrict__ cc,
                                                       int32_t* __restrict__ order, const int64_t* __restrict__ ent_row_ptr) {
  __shared__ int32_t cnt[GDMIX_RE_NUM_CLASSES], base[GDMIX_RE_NUM_CLASSES];
  __shared__ int32_t nar_cnt, nar_base;
  const int split = cc->tall.split;
  const int team_from = cc->tall.team_from;   // > 0: eight-wavefront tall entities of at least this many samples get a team
  const int mid_from = cc->tall.mid_from;     // > 0: one-wavefront tall entities of at least this many samples (below the split) go to the mid class
  const int64_t chunk = (int64_t)blockDim.x * 8;
  for (int64_t start = (int64_t)blockIdx.x * chunk; start < E; start += (int64_t)gridDim.x * chunk) {
    if (threadIdx.x < GDMIX_RE_NUM_CLASSES) cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) nar_cnt = 0;
    __syncthreads();
    int c[8], pos[8];
    unsigned nar = 0;   // bit k: entity k of this thread is narrow
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t e = start + (int64_t)k * blockDim.x + threadIdx.x;
      c[k] = (e < E) ? cls[e] : -1;
      if (c[k] >= NARROW_FLAG) { c[k] -= NARROW_FLAG; cls[e] = c[k]; nar |= 1u << k; }
      if (split > 0 && c[k] == TALL_S_CLASS && ent_row_ptr[e + 1] - ent_row_ptr[e] >= split) { c[k] = TALL_CLASS; cls[e] = TALL_CLASS; }
      else if (team_from > 0 && c[k] == TALL_CLASS && ent_row_ptr[e + 1] - ent_row_ptr[e] >= team_from) { c[k] = TALL_T_CLASS; cls[e] = TALL_T_CLASS; }
      else if (mid_from > 0 && c[k] == TALL_S_CLASS && ent_row_ptr[e + 1] - ent_row_ptr[e] >= mid_from) { c[k] = TALL_M_CLASS; cls[e] = TALL_M_CLASS; }
      pos[k] = (c[k] >= 0) ? atomicAdd((nar >> k) & 1u ? &nar_cnt : &cnt[c[k]], 1) : 0;
    }
    __syncthreads();
    if (threadIdx.x < GDMIX_RE_NUM_CLASSES)
      base[threadIdx.x] = cnt[threadIdx.x] ? atomicAdd(&cc->cursor[threadIdx.x], cnt[threadIdx.x]) : 0;
    if (threadIdx.x == GDMIX_RE_NUM_CLASSES) nar_base = nar_cnt ? atomicAdd(&cc->narrow_count, nar_cnt) : 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t e = start + (int64_t)k * blockDim.x + threadIdx.x;
      if (c[k] < 0) continue;
      const int seg = cc->base[c[k]];
      if ((nar >> k) & 1u) order[seg + nar_base + pos[k]] = (int32_t)e;                                                   // from the front
      else if (c[k] == NARROW_HOST_CLASS) order[seg + cc->count[c[k]] - 1 - (base[c[k]] + pos[k])] = (int32_t)e;           // from the back
      else order[seg + base[c[k]] + pos[k]] = (int32_t)e;
    }
    __syncthreads();
  }
}

static hipError_t launch_classify(const gdmix_re_packed* b, int ic, int m, const ClassTable& tab, ClassCounts* counts, hipStream_t s) {
  int grid = (int)((b->E + 255) / 256);
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(re_classify_kernel, dim3(grid), dim3(256), 0, s, b->ent_row_ptr, b->ent_nnz_ptr,
                     b->ent_feat_ptr, b->E, ic, m, b->weight != nullptr, tab, b->cls_tmp, counts);
  return hipGetLastError();
}

static hipError_t launch_order(const gdmix_re_packed* b, ClassCounts* counts, hipStream_t s) {
  int grid = (int)((b->E + 2047) / 2048);
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(re_order_kernel, dim3(grid), dim3(256), 0, s, b->cls_tmp, b->E, counts, b->order, b->ent_row_ptr);
  return hipGetLastError();
}

int route(gdmix_ctx_impl* ci, const gdmix_re_packed* b, const ClassTable& tab, const gdmix_re_opts* opts, hipStream_t s,
          const ClassCounts** host) {
  ClassCounts* const cc = reinterpret_cast<ClassCounts*>(b->class_count);
  HIP_TRY(hipMemsetAsync(cc, 0, sizeof(ClassCounts), s));
  HIP_TRY(launch_classify(b, opts->has_intercept ? 1 : 0, opts->m, tab, cc, s));
  hipLaunchKernelGGL(class_base_kernel, dim3(1), dim3(1), 0, s, cc, tab.tall_adapt_limit, 16 * ci->num_cus, tab.tall_team_n, tab.tall_team_limit, tab.tall_mid_n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(launch_order(b, cc, s));
  ClassCounts* const hc = reinterpret_cast<ClassCounts*>(ci->host_pinned + COUNTS_READBACK_WORDS);
  HIP_TRY(fetch_small(ci, 0, cc, sizeof(ClassCounts), hc, s));
  *host = hc;
  return GDMIX_RE_OK;
}

// A class whose launch cannot fill the device: fewer wavefronts than three quarters of what the CUs hold at two per SIMD (the eight-wavefront
// tall workgroups: fewer entities than one and a half times the CUs). Such a class runs on one of the context's side streams, next to
// the large ones and to the other small ones.
static bool class_is_small(const ClassDesc& d, int count, int num_cus) {
  const long waves = ((long)count * d.occ_lanes + WAVE - 1) / WAVE;
  return waves < (long)num_cus * 6;
}

// Launch plan of the classes below the block class. The tall classes go first: their kernels are the longest chains of a small batch
// (one workgroup, or one wavefront, per entity, for as long as that entity's solve lasts) and each is preceded by three small launches
// (fill, sort, tail) that must not queue behind the group kernels' workgroups. Stream of a class:
//   large class                      -> dealt over the caller's stream and the side streams in launch order (gdmix_re_set_spread);
//   small tall class (<8>, <1>, lean) -> a side stream of its own (side 1, 2, 0: the device has four hardware queues by default,
//                                        a fourth side stream would share one — measured: both tall classes of a MovieLens share on
//                                        one queue, 1.1 + 2.1 ms one after the other);
//   other small classes              -> the caller's stream when no large class uses it, else side 0 (behind the lean tall class,
//                                        the shortest of the three). The mid tall class is one of them: ahead of the group classes.
// Only the streams that get work are woken (SideJoin::use): a C2 partition touches the caller's stream and side 0.
// Disjoint entities and outputs; the tall variants have a tail slot each: a schedule changes the time, never a bit of the result.
//
// Large classes are dealt over the caller's stream and the side streams, in launch order (round 4): side by side their tails overlap
// — a class launch ends with the workgroups whose entities need the most iterations while the rest of the device idles — and
// wavefronts of different classes share a SIMD. C2: 9.35 -> 8.93 ms of solve, step 10.70 -> 10.30 ms; MovieLens-20M per-movie 6.04 -> 5.70 ms
// (tools/r04_spread.sh: 2 / 3 / 4 queues 10.44 / 10.31 / 10.30 ms; most-entities-first changes nothing). spread == 0: one after
// another on the caller's stream, as before (A/B, and the per-kernel durations of a profile: overlapped kernels stretch each other).
//
// A lean tall class of a few thousand entities (fewer than lean_rounds rounds of its launch) is not worth a launch of its own (a
// launch lasts at least one entity's solve and ends in a thin tail): it then runs with the class behind it — its entities sit right
// in front of that class's in `order`, and the general one-wavefront kernel takes any of them. An entity's result does not depend
// on which of the two ran it: same accumulator sets, same order of the adds (the variants differ in where loads are issued and in
// occupancy only).
LaunchPlan plan_launches(const ClassCounts& counts, int num_cus, int n_side, int spread, int lean_rounds) {
  LaunchPlan plan;
  plan.n = 0;
  const int lean = counts.count[TALL_L_CLASS];
  plan.lean_merged = (lean > 0 && lean < lean_rounds * num_cus * TALL_LEAN_WGS) ? lean : 0;
  // the ranges of `order`, the merged lean class with the one-wavefront class behind it
  int begin[GDMIX_RE_NUM_CLASSES], count[GDMIX_RE_NUM_CLASSES], n_launch_classes = 0;
  for (int c = 0; c < GDMIX_RE_NUM_CLASSES; ++c) { begin[c] = counts.base[c]; count[c] = counts.count[c]; }
  if (plan.lean_merged) { count[TALL_L_CLASS] = 0; begin[TALL_S_CLASS] -= plan.lean_merged; count[TALL_S_CLASS] += plan.lean_merged; }
  // (as counted since the merge came in: a merged lean class is left out, and does not make an empty one-wavefront class count)
  for (int c = 0; c < GDMIX_RE_NUM_CLASSES; ++c) n_launch_classes += (counts.count[c] > 0 && !(c == TALL_L_CLASS && plan.lean_merged)) ? 1 : 0;
  // side streams are used at all (the caller forks them) when a class is small, or large classes are spread
  plan.fork = false;
  if (n_side > 0 && n_launch_classes > 1) {
    for (int c = 0; c < BLOCK_CLASS && !plan.fork; ++c) plan.fork = count[c] > 0 && class_is_small(kClasses[c], count[c], num_cus);
    if (spread > 1) plan.fork = true;
  }
  bool small[GDMIX_RE_NUM_CLASSES], any_large = false;
  for (int k = 0; k < TALL_VARIANTS + BLOCK_CLASS; ++k) {   // the tall classes by rank, then the others as they come
    const int c = k < TALL_VARIANTS ? tall_class_of_rank(k) : k - TALL_VARIANTS;
    if (k >= TALL_VARIANTS && kClasses[c].tall_rank >= 0) continue;
    if (count[c] <= 0) continue;
    small[plan.n] = plan.fork && class_is_small(kClasses[c], count[c], num_cus);
    any_large = any_large || !small[plan.n];
    plan.launch[plan.n++] = Launch{c, begin[c], count[c], -1, c == NARROW_HOST_CLASS ? counts.narrow_count : 0};
  }
  int spread_rr = 0;
  for (int k = 0; k < plan.n; ++k) {
    Launch& L = plan.launch[k];
    if (small[k]) {
      const int side = kClasses[L.c].small_side;
      L.stream = side >= 0 ? side % n_side : (any_large ? 0 : -1);
    } else if (plan.fork && spread > 1) {   // large classes side by side
      const int nq = spread < n_side + 1 ? spread : n_side + 1;
      L.stream = spread_rr++ % nq - 1;
    }
  }
  return plan;
}

}  // namespace gdmix
