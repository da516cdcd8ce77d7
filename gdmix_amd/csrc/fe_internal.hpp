// fe_internal.hpp — what the two units of the fixed-effect trainer share: fe_solve.hip (the passes, the step, every gdmix_fe_*
// entry point) and fe_copy.hip (the passes' copies of the non-zeros, built when a problem is created).
#pragma once
#include "re_internal.hpp"

#include <optional>
#include <vector>

namespace gdmix {

#ifndef GDMIX_FE_B
#define GDMIX_FE_B 2048
#endif
#ifndef GDMIX_FE_UNROLL
#define GDMIX_FE_UNROLL 8
#endif
#ifndef GDMIX_FE_PACK
#define GDMIX_FE_PACK 1      // 0: always the three-array form (tests of that path)
#endif
constexpr int FE_B = GDMIX_FE_B;        // accumulators (rows / columns) per block: 16 KiB of LDS per wavefront
constexpr int FE_U = GDMIX_FE_UNROLL;   // entries per lane in flight
constexpr int FE_THREADS = 256;
constexpr int FE_XCDS = 8;           // accelerator dies of an MI355X, each with its own L2; workgroup i runs on die i % 8
constexpr int FE_WAVES = FE_THREADS / WAVE;
constexpr int FE_DOT_BLOCKS = 512;
constexpr int FE_FIN_BLOCKS = 64;   // workgroups (= lanes of the final wavefront) that add up the per-unit partial sums
static_assert(FE_U % 2 == 0 && FE_B <= 65536 && FE_B % FE_THREADS == 0, "16-bit accumulator index");

// one pass's copy of the non-zeros
constexpr int FE_LOC_BITS = 11;
static_assert((1 << FE_LOC_BITS) == GDMIX_FE_B || !GDMIX_FE_PACK, "the packed word holds the accumulator index in its low bits");
struct FeCopy {
  const uint2* ent;        // packed [z]: x = (key - kbase[unit]) << FE_LOC_BITS | loc, y = bits of the value; else NULL and:
  const int32_t* key;      // [z] element of the gathered vector: local column (row pass) / row (column pass)
  const float* val;        // [z]
  const uint16_t* loc;     // [z] accumulator within the block
  const int32_t* kbase;    // [nunit] key of the unit's first entry (the smallest: a unit's keys ascend)
  const int32_t* ustart;   // [nunit+1] unit -> first entry; units tile the copy
  const int32_t* ublock;   // [nunit]
  const int32_t* ufirst;   // [nblock+1] block -> first unit
  const int32_t* order;    // [nlaunch] workgroup -> unit or -1: units that gather the same stretch of the vector on one XCD (fe_xcd_order)
  double* part;            // [nunit][FE_B] partial sums of the blocks that have several units (column pass: of all)
  int nunit, nblock, nlaunch;
  // the 6-byte form (round 5; fe_cpack_kernel): a unit's entries in trips of 512, per trip 2 KB of values + 1 KB of 16-bit words
  // {5-bit key delta to the entry before, 11-bit accumulator}, keys rebuilt by a wavefront scan
  const unsigned char* cdata;
  const int64_t* cbase;    // [nunit] byte offset of the unit in cdata; -1: the unit is read in the 8-byte / three-array form (or NULL)
  const int32_t* ctrip;    // [nunit] trips
  int64_t stream_bytes;    // (host bookkeeping) bytes of entries one pass reads: 6-byte-form units incl. fillers and padding + 8 / 10 B per entry of the others
};

// Frequent features (real feature frequencies are Zipf-like: one feature can hold a tenth of the non-zeros): in the column pass
// their adds pile up on one LDS address (of the 64 lanes of an instruction, those that hold an entry of the same column
// serialise), 0.34 ms instead of 0.25 on the Zipf shard of tools/fe_bench.py. A dense pass per frequent column straight off the
// column-major arrays was tried and lost (0.52 ms): every such column then gathers the residuals on its own, 64 columns =
// 64 sweeps over them instead of one. So the scatter form stays and the frequent columns (at least FE_HOT_MIN entries, the
// FE_HOT_MAX most frequent of them) get FE_HOT_REP accumulators each: in the column pass's copy an entry of frequent column h in
// row r goes to the virtual column vbase + h * FE_HOT_REP + r % FE_HOT_REP. The virtual columns form one more block at the end
// (entries by ascending row like every block: one sweep over the residuals for all of them), neighbouring rows land on different
// accumulators, and fe_hot_finish_block (the first workgroups of fe_finish_kernel) adds a column's FE_HOT_REP sums in replica order. No atomics across workgroups, fixed shape.
constexpr int FE_HOT_MAX = 64;
constexpr int FE_HOT_REP = 32;
constexpr long FE_HOT_MIN = 1 << 16;
static_assert(FE_HOT_MAX * FE_HOT_REP <= FE_B && FE_B % FE_HOT_REP == 0, "the virtual columns are one block");
struct FeHot {
  int n, vbase;              // vbase: first virtual column (a multiple of FE_B, >= d)
  const int32_t* col;        // [n] local column of frequent column h
};

struct FeSync { unsigned arrive, gen, aborted; };      // fe_tail_kernel's hand-off. aborted: sticky, set by a waiter whose watchdog fired (never cleared: the problem is dead)
struct CompactState;
struct CompactPlan;
struct CompactMats;
struct FeDev {
  int n, d, ic, P, m;
  int64_t z, D;
  FeCopy rc, cc;            // row pass, column pass
  FeHot hot;                // frequent columns: left out of cc
  const int32_t* multi;     // [nmulti] row blocks cut into several units
  int nmulti, nred;         // nred = rc.nunit + nmulti * (workgroups of fe_rows_fix_kernel per block) entries of loss_part / rsum_part
  const float *y, *o, *w;   // w may be NULL
  const int32_t* umap;      // [d] local -> global feature id
  double* xl;               // [d] x of the features present in this shard
  double* rs;               // [n] per-sample residual
  double* fg;               // [P + 1] global data gradient (intercept last), then the data value
  double *loss_part, *rsum_part, *loss_lo_part;   // [nred] each: value (hi), residual sum, value (lo)
  double* acc_part;         // [FE_DOT_BLOCKS][COMPACT_KD]
  double* fin_part;         // [FE_FIN_BLOCKS][3]: value hi, residual sum, value lo
  unsigned* fin_count;      // workgroups of fe_finish_kernel that have delivered their range sums
  int32_t* inv;             // [P] global coefficient -> local column of this shard, -1: absent (intercept: -1)
  struct FeSync* sync;      // ticket + generation stamp of fe_tail_kernel
  CompactState* state;
  CompactPlan* plan;
  CompactMats* mats;
  Work W;                   // global coefficient space, P each; ws / wy m*P
  const double *mu, *sc;    // [P] prior mean and scale (include/gdmix_fe.h, "incremental training"), NULL without one; read by the PRIOR variants only
};

// ---- the trust-region Newton step (include/gdmix_fe.h, "(ABI 24) TRON"; csrc/fe_tron.hip) ------------------------------------------------
// A buffer of the problem's own, allocated when TRON is first selected (or gdmix_fe_hessian_vec first called): this record, then the
// vectors below. What a pass pair computes is decided on the device: the HV variant of the row kernels reads `mode` at entry.
enum {
  FE_TM_EVAL = 0,        // evaluation at the trial point (xl, intercept xt[D]); the emit writes the curvature of that point into c[1 - cur]
  FE_TM_PRODUCT = 1,     // X~' D X~ d: gathers vl, intercept d[D], D = c[cur], the accepted point's
  FE_TM_CURVATURE = 2,   // gdmix_fe_hessian_vec, first row pass: as FE_TM_EVAL at F.W.x[D] / xl, whatever the status
  FE_TM_VECTOR = 3       // gdmix_fe_hessian_vec, second row pass: as FE_TM_PRODUCT with intercept `vb` and D = c[1 - cur], whatever the status
};
struct FeTronState {
  int mode, cur;                 // what the next pass pair computes; which of c[2] belongs to the accepted point
  int ncg, nrej, moved;          // products of this outer iteration; consecutive rejected trials; a step has been accepted
  int action;                    // what the update does (fe_tron.hip: TA_*)
  int saved_mode, pad;           // gdmix_fe_hessian_vec puts `mode` back
  long long nhv;                 // products so far (gdmix_fe_products)
  double delta, gnorm, gg, rr;   // radius; |g|_2, g'g at the accepted point; r'r of the CG residual
  double coef, beta;             // the update: s += coef d, r -= coef Hd; d = r + beta d
  double vb;                     // intercept entry of gdmix_fe_hessian_vec's v
};
struct FeTron {                  // the buffer's parts, P (or d, n) doubles each
  FeTronState* st;
  double *s, *r, *d, *h, *xt, *g;   // CG iterate, residual, direction; what the last pass pair left (H d, or the gradient at the trial); trial point; accepted gradient
  double* vl;                    // [d] the direction in the shard's local order (what the product's row pass gathers)
  double* c[2];                  // [n] curvature weights w rho (1 - rho) | 2 w | w exp(z)
};
constexpr size_t FE_TRON_HEAD = 256;      // bytes kept for the record
__host__ __device__ inline size_t fe_tron_pad(size_t k) { return (k + 31) & ~(size_t)31; }      // doubles: every part 256-byte aligned
__host__ __device__ inline size_t fe_tron_bytes(int P, int d, int n) {
  return FE_TRON_HEAD + (6 * fe_tron_pad((size_t)P) + fe_tron_pad((size_t)d + 1) + 2 * fe_tron_pad((size_t)n + 1)) * 8;
}
// The buffer's address travels in W.part — a field of Work that only the team kernels use, NULL in a fixed-effect problem until the problem
// first needs the buffer — so that FeDev keeps its size and layout, and with them every existing kernel its argument offsets and its code.
__host__ __device__ inline FeTronState* fe_tron_state(const FeDev& F) { return reinterpret_cast<FeTronState*>(F.W.part); }
__host__ __device__ inline FeTron fe_tron_of(const FeDev& F) {
  FeTron T;
  T.st = fe_tron_state(F);
  double* v = reinterpret_cast<double*>(reinterpret_cast<char*>(T.st) + FE_TRON_HEAD);
  const size_t p = fe_tron_pad((size_t)F.P);
  T.s = v; T.r = v + p; T.d = v + 2 * p; T.h = v + 3 * p; T.xt = v + 4 * p; T.g = v + 5 * p;
  T.vl = v + 6 * p;
  T.c[0] = T.vl + fe_tron_pad((size_t)F.d + 1);
  T.c[1] = T.c[0] + fe_tron_pad((size_t)F.n + 1);
  return T;
}
static_assert(sizeof(FeTronState) <= FE_TRON_HEAD, "the record fits its slot");

// Sort key of an entry on its way into a copy: the block, refined by the window of 2^FE_SPAN_BITS gathered elements the entry's key
// lies in. The entries of a block already come by ascending key, so the windows do not change the sorted order; they only add cut
// points, so that no unit's keys span more than the packed word can hold (a block with few entries is one unit over the whole vector
// otherwise, and one such unit would send the whole copy to the three-array form: the Zipf shard of tools/fe_bench.py, 0.34 ms
// instead of 0.26).
constexpr int FE_SPAN_BITS = 32 - FE_LOC_BITS;

#ifndef GDMIX_FE_COMPRESS_DEFAULT
#define GDMIX_FE_COMPRESS_DEFAULT 2     // the column pass: 0.268 -> 0.235 ms; the row pass gets slower in this form (0.246 -> 0.257): measured, docs/rounds/r05.md
#endif
constexpr int FE_COMPRESS_DEFAULT = GDMIX_FE_COMPRESS_DEFAULT;
constexpr int FE_CTRIP = WAVE * 8;            // entries per trip of the 6-byte form
constexpr int FE_CTRIP_BYTES = FE_CTRIP * 6;  // [2][64] x 16 B of values, then [64] x 16 B of index words
constexpr int FE_CDELTA_MAX = 31;
static_assert(FE_LOC_BITS == 11, "index word = delta << 11 | accumulator");

// The test hooks (include/gdmix_fe.h). gdmix_fe_create reads the environment once into this record and passes it down; nothing
// else of the fixed effect looks at the environment, so a problem keeps what it was created under. Empty = not set.
struct FeHooks {
  std::optional<long> chunk;         // GDMIX_FE_CHUNK >= 64: entries per unit (small shards through the several-units-per-block code)
  std::optional<int> window_bits;    // 1 <= GDMIX_FE_WINDOW_BITS < FE_SPAN_BITS: several windows on a small shard (narrower is always valid)
  std::optional<bool> pack;          // GDMIX_FE_PACK: false = the three-array form on a small shard (it only ever narrows)
  std::optional<long> hot_min;       // GDMIX_FE_HOT_MIN: entries from which a column is frequent (<= 0: no frequent columns)
  std::optional<int> compress;       // GDMIX_FE_COMPRESS & 3: bit 0 the row pass, bit 1 the column pass may use the 6-byte form
  std::optional<bool> fused_tail;    // GDMIX_FE_FUSED_TAIL: the step as one launch, or as three, whatever the device looks like
};

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
// one allocation carved into 256-byte-aligned parts: take() -> the part's byte offset, off: the bytes so far
struct Arena {
  size_t off = 0;
  size_t take(size_t bytes) { const size_t r = off; off = up256(off + bytes); return r; }
};

// ---- fe_copy.hip ----
// One pass's copy from segment-major source arrays: ptr [nseg + 1], idx / val [z]; len = extent of idx (the outputs of the pass).
struct FeSource {
  const int32_t* ptr; int nseg; const int32_t* idx; const float* val; int64_t z; int len;
  bool cut_sparse;      // blocks with few entries per line of the gathered vector get shorter units (fe_block_chunk)
  bool compress;        // units may take the 6-byte form
};
// Device memory of the result in *tables (unit tables and entries) and *cdata (the 6-byte form; empty if no unit takes it);
// ufirst_host (may be NULL): the block -> unit table on the host as well. Synchronises the stream.
int fe_build_copy(hipStream_t s, int num_cus, const FeHooks& hooks, const FeSource& src, FeCopy* out, DevBuf* tables, DevBuf* cdata,
                  std::vector<int32_t>* ufirst_host);
// The column pass's copy of a packed shard with d columns, n rows and z non-zeros, its frequent columns (*hot, their list in
// *hot_mem) under their virtual numbers.
int fe_build_column_copy(hipStream_t s, int num_cus, const FeHooks& hooks, const gdmix_re_packed* b, int n, int d, int64_t z, FeCopy* out,
                         FeHot* hot, DevBuf* tables, DevBuf* cdata, DevBuf* hot_mem);

// ---- fe_qn.hip: the two projected quasi-Newton steps ----
// One OWL-QN step (products, decision, update: three launches) on the reduced [gradient, value] buffer of a problem with l1 > 0;
// the status lands in *status_dev as the L-BFGS-B step's does.
void fe_owlqn_enqueue_step(const FeDev& F, const SolveParams& o, double l1, int32_t* status_dev, hipStream_t s);

// ---- fe_tron.hip ----
// One TRON step (products, decision, update: three launches) on the reduced buffer of a problem whose optimiser is TRON: the buffer
// holds [gradient, value] after an evaluation and [X~' D X~ d, 0] after a product; the step knows which from the record.
void fe_tron_enqueue_step(const FeDev& F, const SolveParams& o, int32_t* status_dev, hipStream_t s);
// The buffer as a restart leaves it: record cleared (an evaluation at the start point comes first), trial point = theta0 (NULL: zeros).
void fe_tron_enqueue_reset(const FeDev& F, const double* theta0, hipStream_t s);
// gdmix_fe_hessian_vec: `mode` set to FE_TM_CURVATURE (the old one kept), then to FE_TM_VECTOR with vl filled from v; then put back.
void fe_tron_enqueue_hv_begin(const FeDev& F, hipStream_t s);
void fe_tron_enqueue_hv_vector(const FeDev& F, const double* v, hipStream_t s);
void fe_tron_enqueue_hv_end(const FeDev& F, hipStream_t s);

// ---- fe_qn.hip, the bounded step ----
// One projected L-BFGS step (products, decision, update: three launches) on the reduced [gradient, value] buffer of a problem with bounds
// (include/gdmix_fe.h, "(ABI 26) box constraints"); lower / upper: [P] device doubles of the problem's own, the intercept's infinite.
void fe_box_enqueue_step(const FeDev& F, const SolveParams& o, const double* lower, const double* upper, int32_t* status_dev, hipStream_t s);
// gdmix_fe_set_bounds' check of the caller's arrays: bad_dev[0] a NaN, [1] lower > upper, [2] a finite bound on the intercept (the caller clears them).
void fe_box_enqueue_check(const double* lower, const double* upper, int P, int ic, int32_t* bad_dev, hipStream_t s);
// Behind fe_init_kernel: the start point clamped into the box (W.x, W.t, xl).
void fe_box_enqueue_start(const FeDev& F, const double* lower, const double* upper, hipStream_t s);

}  // namespace gdmix
