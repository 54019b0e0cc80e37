// C ABI of the MI355X FlashAttention library (declared in include/flash_attn_mi355x.h):
// kernel dispatch for the device-pointer entry points and the host-pointer launchers that stand in
// for the reference's launch_flash_attn_fw / launch_flash_attn_bw (src/flash_attn_fw.cu:300-359,
// src/flash_attn_bw.cu:275-365, src/flash_attn2_fw.cu:310-372, src/flash_attn2_bw.cu:277-369).
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <atomic>

#include "../../include/flash_attn_mi355x.h"
#include "fa_kernels.h"

namespace {

thread_local char g_err[512] = "";

int set_err(int code, const char* what, hipError_t e = hipSuccess) {
  if (e != hipSuccess)
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  else
    snprintf(g_err, sizeof(g_err), "%s", what);
  return code;
}

#define FA_HIP_TRY(expr)                                             \
  do {                                                               \
    hipError_t e_ = (expr);                                          \
    if (e_ != hipSuccess) return set_err(FA_ERR_HIP, #expr, e_);     \
  } while (0)

// fwd_kernel workgroups per CU up to which the fp32 split-key forward takes the launch (measured, profiles/r04_fwd_splitk_f32.txt: 64 / 128
// workgroups 0.076 -> 0.027 / 0.044 ms, 256 level, 512 slower; causal: 256 workgroups 0.160 -> 0.111, 512 slower)
constexpr double FWD_SPLITK_MAX_WGS_PER_CU = 0.5, FWD_SPLITK_MAX_WGS_PER_CU_CAUSAL = 1.0;

inline bool d_supported(int d) { return d == 32 || d == 64 || d == 128; }
inline int d_padded(int d) { return d <= 32 ? 32 : (d <= 64 ? 64 : 128); }

// Per-call kernel selection (fa_mi355x_fwd_ex / fa_mi355x_bwd_ex; every other entry point runs the defaults): [0] dK/dV geometry
// (6 = the 8-wave slot builds wherever the 64-keys-per-wave build would run, 7 = that build wherever it is valid: select_dkdv),
// [1] forward kernel, [2] dQ kernel, [3] reserved, [4] preprocess / fp32 one-pass backward, [5] 1 = one head per workgroup in the
// tiled slot builds, [6] reserved, [7] causal block order.  Only values whose kernels give correct results are accepted (parse_opts).
// [8] where tau*log2(e) is applied (see select_call): 0 = by the call's scale guard when it has one, else fp32 scaling; 1 = the caller
// vouches for the operand range (inputs of the north star's U(-1, 1) magnitude): the kernels that fold it into a bf16 operand run
// without a guard; 2 = fp32 scaling whatever the guard says; 3 = (fa_mi355x_plan only) plan a guarded call.  [9] 1 = bf16 output.
constexpr int NTUN = 10;
struct Tun { int v[NTUN]; };
inline Tun default_tun() { return Tun{{0, 0, 0, 0, 0, 0, 0, 0, 0, 0}}; }
int parse_opts(const int* opts, int nopts, Tun& t) {
  t = default_tun();
  if (nopts < 0 || nopts > NTUN || (nopts > 0 && !opts)) return set_err(FA_ERR_BAD_ARG, "bad options array");
  for (int i = 0; i < nopts; ++i) t.v[i] = opts[i];
  // (the values that lost their A/B were retired with their kernels: DESIGN.md section 3, "Retired experiments")
  static const int allowed[NTUN][7] = {{0, 3, 4, 5, 6, 7, -1}, {0, 2, 3, 4, -1}, {0, 2, 3, -1}, {0, -1}, {0, 1, 4, 5, -1}, {0, 1, -1}, {0, -1}, {0, 1, 2, -1},
                                       {0, 1, 2, 3, -1}, {0, 1, -1}};
  for (int i = 0; i < NTUN; ++i) {
    bool ok = false;
    for (int j = 0; allowed[i][j] >= 0; ++j) ok |= allowed[i][j] == t.v[i];
    if (!ok) return set_err(FA_ERR_BAD_ARG, "option value not supported (retired diagnostic values included)");
  }
  return FA_OK;
}

constexpr int WS_VECS = 3;   // row-constant vectors of the backward workspace: -L/tau, -delta, -L*log2(e)

// One device call.  An entry point fills in its arguments, validate() checks them and completes the call (batch, tun, lay), and
// fwd_dispatch / bwd_dispatch run it; the host-pointer launchers fill in the completed fields themselves.
struct Call {
  // forward: q, k, v -> out, l, m; backward: q, k, v, out, dout, l, m (read only) -> dq, dk, dv, with the workspace ws
  const void *q = nullptr, *k = nullptr, *v = nullptr, *dout = nullptr;
  float *out = nullptr, *l = nullptr, *m = nullptr, *dq = nullptr, *dk = nullptr, *dv = nullptr, *ws = nullptr;
  bool bwd = false;
  int B = 0, H = 1;            // B batch elements of H heads (by_heads); otherwise B is the number of (batch*head) matrices
  bool by_heads = false;       // the B, H, layout form of the *_layout / _scaled / _masked / _dropout / _guarded entry points
  int layout = FA_LAYOUT_BHND;
  int N = 0, d = 0;
  bool padded = false;         // fa_mi355x_*_padded: rows of dp elements; otherwise dp = d
  int dp = 0;
  int causal = 0, variant = 0, dtype = 0;
  int stages = 0;              // backward stage mask
  const int* opts = nullptr;
  int nopts = 0;
  const float* kmask = nullptr;   // additive key mask, one row per mask_heads (batch*head) matrices
  int mask_heads = 1;
  float drop_rate = 0.f, drop_scale = 1.f;
  unsigned drop_seed = 0;
  float scale = 0.f;           // softmax scale, 0 = sqrt(1/d)
  bool scale_required = false;   // fa_mi355x_*_scaled: 0 is not accepted
  const float* guard = nullptr;
  int produce = 0;             // forward: fill the guard instead of reading it
  // grouped-query heads (fa_mi355x_*_gqa): k, v (and the caller's dk, dv) have Hkv heads, query head h reads kv head h / (H / Hkv).
  // validate() then points dk, dv at the workspace's two q-shaped scratch tensors and keeps the caller's pointers in gdk, gdv.
  bool gqa = false;
  int Hkv = 0;
  float *gdk = nullptr, *gdv = nullptr;
  hipStream_t st = nullptr;
  // completed by validate() (tau by fwd_dispatch / bwd_dispatch)
  int batch = 0;               // (batch*head) matrices
  Tun tun = default_tun();
  fa::Layout lay{};
  float tau = 0.f;
  // the workspace's row-constant vectors
  float* nlc() const { return ws; }                           // -L / tau        (raw score units)
  float* delta() const { return ws + (long)batch * N; }       // -rowsum(dO * O)
  float* nl2() const { return ws + 2 * (long)batch * N; }     // -L * log2(e)    (the slot dK/dV kernel: its K fragments carry tau*log2(e))
};

int device_cus_raw();
// Compute units the launch-size rules assume: the current device's, or 256 (an MI355X) when there is none -- fa_mi355x_plan without a
// GPU must name the kernels a real launch would select.  Never 0.
int device_cus() {
  const int n = device_cus_raw();
  return n > 0 ? n : 256;
}
int device_cus_raw() {   // compute units of the current device (cached per device; any thread); 0 without one
  static std::mutex mu;
  static int cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  std::lock_guard<std::mutex> lock(mu);
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    cus[dev] = n;
  }
  return cus[dev];
}

// Causal slot builds: heads per XCD dispatched together, longest block first (fa::map_block_ranked): a chunk of two rounds of the chip
int rank_chunk(int wgs_per_cu, int nb) {
  return std::max(1, device_cus() * wgs_per_cu / (4 * nb));
}

// Causal slot builds of the forward / dQ kernels: one block per workgroup in ranked order (measured 1-20 % faster than paired blocks
// up to 4 rounds of the chip, 1-2 % slower from 16 rounds on: B = 32 at the metric shape, configs[3]) or blocks p and nqb-1-p paired
// in one workgroup.  Option 7: 0 = by launch size, 1 = paired, 2 = ranked.
bool causal_ranked(const Tun& tun, int blocks, int wgs_per_cu) {
  if (tun.v[7]) return tun.v[7] == 2;
  return blocks < 8 * device_cus() * wgs_per_cu;
}

// The tiled slot builds of dK/dV and dQ: block kb (qb) of several consecutive heads per workgroup (no set-up, no wait for the K / V
// fragments or the first stage, no store drain between them) while the grid of nb blocks per head still covers every CU; option
// 5 = 1: one head per workgroup
// (grouped-query heads: one head per workgroup.  The tiled builds keep K and V where q lives: their hand-over from head to head has no
// SGPRs left for a second base and stride, fa_bwd_dq.h)
int head_tiles(const Call& c, int nb) {
  int tiles = 1;
  if (c.N % 256 == 0 && c.tun.v[5] == 0 && c.lay.G == 1) {
    const int cus = device_cus();
    for (int t = 2; t <= 16; ++t)
      if (c.batch % t == 0 && (c.batch / t) % 8 == 0 && (long)(c.batch / t) * nb >= cus) tiles = t;
  }
  return tiles;
}

// only bf16 rows of 64 / 128 elements ever reach a kernel that folds the scale into an operand: everything else gets an all-zero
// guard ("within the budget"; those calls run fp32-scaling kernels whatever it says)
inline bool guard_rows_fold(int dtype, int row_elems) { return dtype == FA_DTYPE_BF16 && (row_elems == 64 || row_elems == 128); }
int launch_scale_guard(const void* q, const void* k, long rows, long krows, int row_elems, int dtype, void* guard, hipStream_t st) {
  if (!guard_rows_fold(dtype, row_elems)) {
    FA_HIP_TRY(hipMemsetAsync(guard, 0, (size_t)2 * fa::GUARD_SLOTS * sizeof(float), st));
    return FA_OK;
  }
  const dim3 grid(fa::GUARD_SLOTS, 2);
  if (row_elems == 64)
    hipLaunchKernelGGL((fa::scale_guard_kernel<64>), grid, dim3(256), 0, st, (const fa::bf16_t*)q, (const fa::bf16_t*)k, rows, krows, (float*)guard);
  else
    hipLaunchKernelGGL((fa::scale_guard_kernel<128>), grid, dim3(256), 0, st, (const fa::bf16_t*)q, (const fa::bf16_t*)k, rows, krows, (float*)guard);
  FA_HIP_TRY(hipGetLastError());
  return FA_OK;
}

// ---- kernel selection: a value ---------------------------------------------------------------------------------------------------
// What a call runs is computed ONCE, by pure code, as a Selection: an ordered list of steps.  select_call() builds it from the validated
// Call (no HIP call but the cached device_cus(), no thread-local or global mutable state), execute() walks it and launches, and
// fa_mi355x_plan() walks the same value and reads the names: what bench.py labels and what the library launches cannot drift apart.
// Every build this file instantiates, and the few steps that are no kernel of ours, with the name fa_mi355x_plan lists them under
// (nullptr: not listed).  The four phased forward / dQ builds keep the order drop, mask, care, main (select_phased).
#define FA_KERNS(X)                                                                                                                  \
  X(FWD_SPLITK, "fwd_splitk_f32_kernel")                                                                                             \
  X(FWD_SLOT_CAUSAL, "fwd_slot_kernel") X(FWD_SLOT_WHOLE, "fwd_slot_kernel") X(FWD_SLOT_MASKED, "fwd_slot_kernel")                   \
  X(FWD_DROP, "fwd_kernel") X(FWD_MASK, "fwd_kernel") X(FWD_CARE, "fwd_kernel") X(FWD_MAIN, "fwd_kernel")                            \
  X(BWD_PREP, "bwd_prep_kernel")                                                                                                     \
  X(DQ_DROP, "bwd_dq_kernel") X(DQ_MASK, "bwd_dq_kernel") X(DQ_CARE, "bwd_dq_kernel") X(DQ_MAIN, "bwd_dq_kernel")                    \
  X(DQ_WAVE8, "bwd_dq_kernel")                                                                                                       \
  X(DQ_SLOT_CAUSAL, "bwd_dq_slot_kernel") X(DQ_SLOT_TILED, "bwd_dq_slot_kernel") X(DQ_SLOT_WHOLE, "bwd_dq_slot_kernel")              \
  X(DQ_SLOT_MASKED, "bwd_dq_slot_kernel")                                                                                            \
  X(DKDV_SLOT, "bwd_dkdv_slot_kernel") X(DKDV_SLOT_CAUSAL, "bwd_dkdv_slot_kernel")                                                   \
  X(DKDV_SLOT64_TILED, "bwd_dkdv_slot_kernel")   /* fa::bwd_dkdv_slot64_kernel: the family's 4-wave, 64-keys-per-wave build */         \
  X(DKDV_CARE_DROP, "bwd_dkdv_kernel") X(DKDV_CARE, "bwd_dkdv_kernel") X(DKDV_DROP_F32, "bwd_dkdv_kernel")                           \
  X(DKDV_CARE_MAIN, "bwd_dkdv_kernel") X(DKDV_PAIRED, "bwd_dkdv_kernel") X(DKDV_PAIRED_M3, "bwd_dkdv_kernel")                        \
  X(DKDV_PLAIN, "bwd_dkdv_kernel") X(DKDV_F32_64, "bwd_dkdv_kernel")                                                                 \
  X(ONEPASS, "bwd_onepass_f32_kernel")                                                                                               \
  X(GROUP_SUM, "group_sum_kernel")      /* grouped-query heads: the group's per-head dK, dV summed into the caller's Hkv heads */    \
  X(GUARD_PASS, "scale_guard_kernel")   /* the separate pass over q and k ... */                                                     \
  X(GUARD_PASS_ZERO, nullptr)           /* ... of rows no kernel folds: launch_scale_guard only zeroes the guard */                  \
  X(GUARD_ZERO, "memset")               /* the guard memset in front of a forward that fills it */                                   \
  X(ZERO_GRADS, nullptr)                /* the one-pass backward's memsets of dq (and dk, dv when the sweep is cut) */
#define X(id, name) id,
enum Kern : int { FA_KERNS(X) };
#undef X
#define X(id, name) name,
constexpr const char* KERN_NAME[] = {FA_KERNS(X)};
#undef X
#define X(id, name) #id,
constexpr const char* BUILD_NAME[] = {FA_KERNS(X)};   // fa_mi355x_plan_builds: one name per build, where KERN_NAME has one per family
#undef X

struct Step {
  Kern kern;
  unsigned grid, block;
  int nb;    // query / key blocks per head, as the kernel is told
  int arg;   // the build's mode argument: only_qb (phased forward / dQ), thin_mode (phased dK/dV), the block order of a causal slot
             // build, `causal` of the other slot builds, the split of ONEPASS / ZERO_GRADS
  int rank_chunk = 0, tiles = 0, twin_blocks = 0, guard_want = 0;   // the fa::Layout fields that belong to this launch alone
  bool prep = false;    // a dQ launch that also preprocesses its rows (fa::DqPrep)
  bool check = true;    // hipGetLastError() behind this launch (false: behind its follow-up launch)
};
struct Selection {
  Step steps[8] = {};   // (the most: memsets, preprocess, two launches each of dQ and dK/dV, the group sum)
  int n = 0;
  bool folds = false;            // a kernel carries tau*log2(e) in a bf16 operand (the MFMA-slot forward without masked periods) ...
  bool produces_guard = false;   // ... and can fill the call's scale guard inside its own launch (its non-causal builds: guard_produce)
  bool fuses_prep = false;       // the dQ launch preprocesses its own rows: no preprocess kernel, stage order dQ -> dK/dV
  int onepass = 0;               // parts of the fp32 one-pass backward's query sweep, 0 = two kernels
  Step& add(Kern kern, int grid, int block, int nb = 0, int arg = 0) {
    return steps[n++] = Step{kern, (unsigned)grid, (unsigned)block, nb, arg};
  }
  void append(const Selection& o, int guard_want = 0) {
    for (int i = 0; i < o.n; ++i) (steps[n++] = o.steps[i]).guard_want = guard_want;
    folds |= o.folds;
    produces_guard |= o.produces_guard;
    fuses_prep |= o.fuses_prep;
    onepass |= o.onepass;
  }
};

// The phased forward (base = FWD_DROP) and dQ (DQ_DROP) kernels, 128-query blocks.  bf16 rows with fewer than 64 admissible keys need
// the split-operand build (CARE): whole launches under a key mask, dropout or N < 64; behind a causal launch, query block 0 alone is
// redone by it (one small workgroup per batch*head).  care_main: ONE launch of the split-operand build instead (forward, d = 64:
// measured 1 % faster than the main build + the block-0 follow-up launch (7.8 us); the dQ kernel is the other way round (+7 %)).
// only_qb >= 0: that query block alone, split operands (the follow-up of a masked slot build).  prep: see select_dq.
void select_phased(Selection& s, const Call& c, bool bf, Kern base, int only_qb, int care_main, int ranked, bool prep) {
  const int batch = c.batch, N = c.N, causal = c.causal, nqb = (N + 127) / 128;
  const bool fwd = base == FWD_DROP;
  // causal: query blocks p and nqb-1-p share a workgroup, or (ranked) one block per workgroup, longest first across a chunk of heads
  const int chunk = (ranked && causal && only_qb < 0) ? rank_chunk(2, nqb) : 0;
  // the fp32-scaling twin of a guarded non-causal call: four query blocks per workgroup while the launch still covers the chip twice
  // (its workgroups almost always return at their guard check: 4.7 -> about 1.5 us at the metric shape)
  int twin = 1;
  if (fwd && c.lay.guard && c.lay.guard_want == 1 && !causal && only_qb < 0)
    for (int t = 4; t > 1; t >>= 1)
      if (nqb % t == 0 && (long)batch * (nqb / t) >= 2L * device_cus()) { twin = t; break; }
  const int nblk = only_qb >= 0 ? 1 : ((causal && !chunk) ? (nqb + 1) / 2 : nqb / twin);
  const int build = c.lay.drop_thr ? 0      // dropout on P (and the key mask, staged as zeros when absent)
                    : c.lay.kmask  ? 1      // additive key mask: staged per tile, enters S^T as the accumulator input
                    : (bf && (N < 64 || only_qb >= 0 || (causal && care_main))) ? 2 : 3;
  Step& m = s.add(Kern(base + build), batch * nblk, 256, nqb, only_qb);
  m.rank_chunk = chunk;
  m.twin_blocks = fwd ? twin : 0;
  if (build != 3) return;
  m.prep = prep;
  if (bf && causal) {   // rows 0..63 see fewer than 64 keys: query block 0 again, split operands (not ranked)
    m.check = false;
    s.add(Kern(base + 2), batch, 256, nqb, 0).twin_blocks = m.twin_blocks;
  }
}

template <typename T, int D>
Selection select_fwd(const Call& c) {
  constexpr bool BF = sizeof(T) == 2;
  const int batch = c.batch, N = c.N, causal = c.causal;
  const Tun& tun = c.tun;
  const bool plain = !c.lay.kmask && !c.lay.drop_thr;
  Selection s;
  if (!BF && D == 64) {
    // fp32, d = 64, launches that leave most of the chip idle under fwd_kernel's geometry (a wave = 32 queries x all keys, 128-query
    // workgroups, two per CU): the split-key forward (fa_fwd_splitk_f32.h: a workgroup = one 32-query block, its four waves a quarter
    // of the keys each).  Option 1: 4 = always, 2 = never.
    const long wgs = (long)batch * ((N + 127) / 128), cus = device_cus();
    if (plain && !c.lay.out_bf16 && N >= 128 && (tun.v[1] == 4 ||
         (tun.v[1] == 0 && wgs <= (causal ? FWD_SPLITK_MAX_WGS_PER_CU_CAUSAL : FWD_SPLITK_MAX_WGS_PER_CU) * cus))) {
      const int nqb = (N + 31) / 32;
      s.add(FWD_SPLITK, batch * nqb, 256, nqb);
      return s;
    }
  }
  if (BF && (D == 64 || D == 128)) {
    // FA-2 side output, bf16, d = 64 / 128, non-causal: slot-interleaved three-deep pipeline.  Under the causal mask the slot build
    // WITH masked period variants is 3.6 % slower than the phased kernel (128-query workgroups, per-wave tile skipping), which keeps
    // the causal launches the build below does not take; tuning key 1: 2 = always phased, 3 = always slot.
    // (N < 64: every row has few keys and takes the phased kernel's split-operand path)
    // Causal, d = 64, N a multiple of 256: the causal slot build (unmasked sweep + the diagonal block per wave, query blocks p and
    // nqb-1-p paired): 0.155 vs 0.192 ms for the phased kernel at the metric shape; it needs about one 8-wave workgroup per CU to pay.
    const int nqb = (N + 255) / 256;
    const bool cslot = causal && N % 256 == 0 && (tun.v[1] == 3 || (tun.v[1] == 0 && batch * nqb >= 256));
    if (c.variant == FA_VARIANT_FA2 && tun.v[1] != 2 && (!causal || tun.v[1] == 3 || cslot) && plain && N >= 64) {
      if (cslot) {   // (d = 64: four waves per SIMD, two workgroups per CU; d = 128: two waves per SIMD, one workgroup)
        const bool ranked = causal_ranked(tun, batch * nqb, D == 64 ? 2 : 1);
        s.add(FWD_SLOT_CAUSAL, ranked ? batch * nqb : batch * ((nqb + 1) / 2), 512, nqb, ranked ? 2 : 1).rank_chunk =
            rank_chunk(D == 64 ? 2 : 1, nqb);
        s.folds = true;
        return s;
      }
      if (!causal && N % (8192 / D) == 0) {   // no sub-tile needs a mask.  d = 64 default: 64-key stages (64 KiB of rings), two
        // workgroups per CU = four waves per SIMD at 122 VGPRs: 0.268 vs 0.282 ms for the 128-key-stage build at two waves per SIMD
        s.add(FWD_SLOT_WHOLE, batch * nqb, 512, nqb, causal);
        s.folds = s.produces_guard = true;
        return s;
      }
      if (D == 64) {   // ragged N / forced causal: the variant with masked periods (d = 128 takes the phased kernel)
        s.add(FWD_SLOT_MASKED, batch * nqb, 512, nqb, causal);
        // under the causal mask rows 0..63 see fewer than 64 keys: the slot kernel has no split-operand path, so the phased
        // kernel redoes query block 0 (one small workgroup per batch*head) behind it
        if (causal) select_phased(s, c, BF, FWD_DROP, 0, 0, 0, false);
        return s;
      }
    }
  }
  select_phased(s, c, BF, FWD_DROP, -1, D == 64 ? 1 : 0, tun.v[7] == 2 || (tun.v[7] == 0 && BF && D == 32), false);   // (d = 32: ranked measured 10 % faster)
  return s;
}

// The phased dK/dV kernel in the geometry of <T, D>: 8 waves x 32 keys (bf16) or 4 (fp32) per workgroup; mode3 (bf16, d = 64): the
// slot-interleaved build.  bf16 launches whose rows may see fewer than 64 admissible keys everywhere (key mask, dropout, N < 64) run
// the split-operand build (CARE) in a 4-wave geometry that has the registers for it.  A causal launch runs the requested geometry with
// the sub-slices of queries 0..63 SKIPPED (thin_mode 1) and then one CARE workgroup per batch*head that handles exactly those and
// adds its dK, dV (thin_mode 2): the main kernel keeps its registers and its speed.
// (fp32, d = 64 comes here for dropout calls alone: its plain launches have a build of their own, see execute.)
template <typename T, int D>
void select_dkdv_phased(Selection& s, const Call& c, bool mode3 = false, int care_main = 0, int rank_causal = 1) {
  constexpr bool BF = sizeof(T) == 2;
  constexpr int NW = BF ? 8 : 4;
  const int batch = c.batch, N = c.N, causal = c.causal;
  const int nkb = (N + NW * 32 - 1) / (NW * 32), nkb4 = (N + 127) / 128;
  const bool rank = causal && rank_causal;
  if (c.lay.drop_thr) {   // dropout: the plain per-sub-slice path regenerates the mask from (bh, query, key)
    // (these whole-launch builds take one key block per workgroup: under the causal mask longest first across a chunk of heads)
    if (BF) s.add(DKDV_CARE_DROP, batch * nkb4, 256, nkb4).rank_chunk = rank ? rank_chunk(2, nkb4) : 0;
    else s.add(DKDV_DROP_F32, batch * nkb, NW * 64, nkb).rank_chunk = rank ? rank_chunk(2, nkb) : 0;
    return;
  }
  if (BF && (c.lay.kmask || N < 64)) {
    s.add(DKDV_CARE, batch * nkb4, 256, nkb4).rank_chunk = rank ? rank_chunk(2, nkb4) : 0;
    return;
  }
  if (mode3 && causal && care_main) {   // d = 64 default: the split-operand path inside the main (paired) kernel: 2 % faster than main + corner launch
    s.add(DKDV_CARE_MAIN, batch * ((nkb + 1) / 2), NW * 64, nkb);
    return;
  }
  const int thin = (BF && causal) ? 1 : 0;
  // causal: key blocks p and nkb-1-p share a workgroup (uniform work, no tail: -13 % at the metric shape).  Not for the 8-wave
  // d = 128 geometry, whose register allocation has no room for the pass loop (it would spill).
  // (mode3 always runs its paired build: hipcc's allocation of the unpaired instance spills, the paired one does not)
  Step* m;
  if ((causal || mode3) && !(BF && D == 128)) {
    m = &s.add(mode3 ? DKDV_PAIRED_M3 : DKDV_PAIRED, batch * ((nkb + 1) / 2), NW * 64, nkb, thin);
  } else {
    // unpaired causal launch (the 8-wave d = 128 geometry): longest block first across a chunk of heads instead of head by head:
    // 2.05 vs 2.21 ms at configs[3]'s shape, 0.157 vs 0.207 at B = 8, N = 2048 (option 7 = 1: head by head)
    m = &s.add(DKDV_PLAIN, batch * nkb, NW * 64, nkb, thin);
    m->rank_chunk = rank ? rank_chunk(NW == 8 ? 1 : 2, nkb) : 0;
  }
  if (thin) {
    m->check = false;
    s.add(DKDV_CARE, batch, 256, nkb4, 2).rank_chunk = m->rank_chunk;
  }
}

// fp32, d = 64, N >= 256, no key mask / dropout, dQ and dK/dV asked for together: the one-pass backward
// (fa_bwd_onepass_f32.h: five products instead of the two-kernel path's seven, dQ by fp32 atomics) when its launch fills the chip:
// one 8-wave workgroup per CU and 256-key block, so batch * ceil(N / 256) workgroups run in ceil(that / CUs) rounds; below one
// workgroup per CU the query sweep of every key block is cut into 2, 4 or 8 parts (one workgroup each; dK and dV are then added with
// atomics as well).  It takes the call when the rounds are at least 80 % full (measured, profiles/r04_onepass_f32_launch_sizes.txt: B = 1,
// H = 8, N = 1024 -- the reference's own test shape -- 0.085 vs 0.240 ms in 8 parts; 128 unsplit workgroups would be 0.64 vs 0.49).
// Returns the number of parts, 0 = two kernels.  Option 4: 4 = two kernels always (dq bitwise repeatable from run to run), 5 = one
// pass whatever the launch size.
template <typename T, int D>
int onepass_f32(const Call& c) {   // 0: two kernels; else the split
  const int N = c.N;
  const Tun& tun = c.tun;
  const int both = FA_BWD_STAGE_DKDV | FA_BWD_STAGE_DQ;
  if (!(sizeof(T) == 4 && D == 64 && (c.stages & both) == both && (tun.v[4] == 0 || tun.v[4] == 5) && !c.lay.kmask &&
        !c.lay.drop_thr && N >= 256))
    return 0;
  // FA_MI355X_DETERMINISTIC=1: never by default (the reference ABI has no options argument: a caller who needs a bitwise repeatable dq there)
  static const bool deterministic = [] { const char* e = getenv("FA_MI355X_DETERMINISTIC"); return e && e[0] == '1'; }();
  if (deterministic && tun.v[4] != 5) return 0;
  // Launches below one workgroup per CU: the query sweep of every key block is cut into 2, 4 or 8 parts (one workgroup each, dK / dV
  // summed by atomics as well) while a part keeps at least 4 stages of 32 queries
  const long cus = device_cus(), wgs1 = (long)c.batch * ((N + 255) / 256), nqi = (N + 31) / 32;
  // (causal: key block 0 sweeps N / 256 times the stages of the last one, so one round is bound by its longest workgroup -- 0.65 ms
  // against 0.36 of balanced work at B = 4, H = 8, N = 2048: first look for a cut that gives the longest-first dispatch two rounds)
  // (from four key blocks per head on: at N = 256 / 512 the cut costs more than the imbalance, 0.146 vs 0.087 and 0.181 vs 0.164 ms)
  for (int pass = (c.causal && N >= 1024) ? 0 : 1; pass < 2; ++pass)
    for (int split = 1; split <= 8; split *= 2) {
      if (split > 1 && nqi / split < 4) break;
      const long wgs = wgs1 * split, rounds = (wgs + cus - 1) / cus;
      if (pass == 0 && rounds < 2) continue;
      if (5 * wgs >= 4 * rounds * cus) return split;   // the launch's rounds are at least 80 % full
    }
  return tun.v[4] == 5 ? 1 : 0;
}

// bf16, d = 64: does the dQ stage take the phased kernel instead of the slot build (key mask, dropout and N < 64 aside)?  The phased
// kernel is 1 % faster than the slot build WITH masked periods under the causal mask (option 2 = 3 forces the slot kernel).  Causal
// launches with N a multiple of 256 take the causal slot build (unmasked sweep + diagonal block per wave, paired query blocks): 0.199
// vs 0.223 ms at the metric shape
bool dq64_phased(const Call& c) {
  return c.tun.v[2] == 2 || (c.causal && c.tun.v[2] != 3 && !(c.N % 256 == 0 && c.batch * (c.N / 256) >= 128));
}

// The dQ stage of a backward call: kernel selection by dtype / head dim / launch shape / options.
// prep: the call asks for the preprocess AND dQ (and option 4 = 0: 1 keeps the separate preprocess kernel, A/B).  The launch then
// preprocesses its own rows whenever the stage lands on a plain main build: not under a key mask or dropout, not bf16 with N < 64
// (split-operand builds), not the bf16 d = 64 slot build with masked periods (no registers).  What was chosen is what is reported:
// fuses_prep, and dQ is then launched BEFORE dK/dV, which reads the workspace the dQ launch wrote.
template <typename T, int D>
Selection select_dq(const Call& c, bool prep) {
  constexpr bool BF = sizeof(T) == 2;
  const int batch = c.batch, N = c.N, causal = c.causal;
  Selection s;
  const bool few_keys = c.lay.kmask || c.lay.drop_thr || N < 64;   // (key mask and dropout live in the phased kernel)
  if (BF && D == 128 && !causal && !few_keys) {   // non-causal default: 8 waves x 32 queries, one workgroup per CU (each staged K / V
    // tile feeds twice the waves); otherwise 4 waves x 32 queries, two workgroups per CU
    const int nqb = (N + 255) / 256;
    s.add(DQ_WAVE8, batch * nqb, 512, nqb, -1).prep = prep;
  } else if (BF && D == 64 && !few_keys && !dq64_phased(c)) {   // d = 64: slot-interleaved three-deep pipeline (default).  Its mask-free
    // builds carry both scalings and pick one per launch (Layout::scale_sel): no twin launch.
    const int nqb = (N + 255) / 256;
    Step* m;
    if (causal && N % 256 == 0) {   // causal build: unmasked sweep + the diagonal block per wave; one block per workgroup,
      // longest first across all heads (paired: blocks p and nqb-1-p in one workgroup)
      const bool paired = !causal_ranked(c.tun, batch * nqb, 1);
      m = &s.add(DQ_SLOT_CAUSAL, paired ? batch * ((nqb + 1) / 2) : batch * nqb, 512, nqb, paired ? 1 : 2);
    } else if (!causal && N % 128 == 0) {   // no sub-tile needs a mask: the build without masked period variants
      // (query block qb of several consecutive heads per workgroup: head_tiles, the rule of the tiled dK/dV launch)
      const int tiles = head_tiles(c, nqb);
      m = tiles > 1 ? &s.add(DQ_SLOT_TILED, (batch / tiles) * nqb, 512, nqb, causal) : &s.add(DQ_SLOT_WHOLE, batch * nqb, 512, nqb, causal);
      m->tiles = tiles > 1 ? tiles : 0;
    } else {
      m = &s.add(DQ_SLOT_MASKED, batch * nqb, 512, nqb, causal);
      prep = false;
    }
    m->prep = prep;
    m->rank_chunk = rank_chunk(1, nqb);
    // the masked slot build forced onto a causal launch: rows 0..63 (few keys) are redone by the phased kernel's split-operand
    // path (query block 0); the causal slot build (N a multiple of 256) splits them itself
    if (m->kern == DQ_SLOT_MASKED && causal) select_phased(s, c, BF, DQ_DROP, 0, 0, 0, false);
  } else {
    // every launch the branches above do not take runs the phased kernel with 32-key tiles (bf16 d = 32: they run 3 waves/SIMD,
    // measured 2 % faster), causal query blocks ranked by default at bf16 d = 32 (option 7)
    select_phased(s, c, BF, DQ_DROP, -1, 0, c.tun.v[7] == 2 || (c.tun.v[7] == 0 && BF && D == 32), prep);
  }
  s.fuses_prep = s.steps[0].prep;   // (only a stage's first launch ever takes it)
  return s;
}

// The dK/dV stage of a backward call: kernel selection by dtype / head dim / launch shape / options.
template <typename T, int D>
Selection select_dkdv(const Call& c) {
  constexpr bool BF = sizeof(T) == 2;
  const int batch = c.batch, N = c.N, causal = c.causal;
  const Tun& tun = c.tun;
  Selection s;
  if (BF && D == 64) {
    // The continuous slot pipeline (no drain at stage boundaries, three-slot LDS-DMA ring) carries both scalings and picks one per
    // launch (Layout::scale_sel): no twin launch.  Option 0 = 4: the compiler-interleaved phased kernel below.
    const bool plain = !c.lay.drop_thr && !c.lay.kmask;
    if (!causal && (tun.v[0] == 0 || tun.v[0] == 6 || tun.v[0] == 7) && plain && N >= 64) {
      // d = 64, non-causal default: the continuous slot pipeline; rows thinned by a key mask or N < 64 go to the kernel below, whose
      // per-sub-slice path splits P and dS.  Key block kb of several consecutive heads per workgroup: head_tiles
      const int nkb = (N + 255) / 256, tiles = head_tiles(c, nkb);
      // The 64-keys-per-wave build (fa_bwd_dkdv64.h: four waves, one per SIMD, half the LDS reads per MFMA, bitwise the same dK, dV)
      // takes every launch the tiled 8-wave build would take: those give every CU a workgroup, and with one 256-thread workgroup
      // per CU nothing else fills a CU that has none.  It replaced the 8-wave several-heads build (1.8 % of the step at the metric
      // shape, bitwise the same).  Option 0 = 6 runs the 8-wave one-head build there instead (for A/B runs and tests in one process);
      // 7 runs the 64-key build wherever it is valid (N a multiple of 256, ungrouped heads), in head groups of 4 where head_tiles
      // forms none, the last one partial.
      const bool can64 = N % 256 == 0 && c.lay.G == 1;
      if (can64 && (tun.v[0] == 7 || (tun.v[0] == 0 && tiles > 1))) {
        const int t64 = tiles > 1 ? tiles : (c.tun.v[5] ? 1 : 4);
        s.add(DKDV_SLOT64_TILED, ((batch + t64 - 1) / t64) * nkb, 256, nkb).tiles = t64;
      } else s.add(DKDV_SLOT, batch * nkb, 512, nkb);
      return s;
    }
    if (causal && plain && N % 256 == 0 && (tun.v[0] == 5 || (tun.v[0] == 0 && batch * (N / 256) >= 128))) {   // (tuning key 0 = 5 forces it)
      // d = 64, causal, N a multiple of 256: the causal build of the continuous pipeline (sweep of the stages below the
      // diagonal block, the block per wave, workgroups longest first); tuning key 0 = 3: the phased kernel below
      // (key blocks p and nkb-1-p of several consecutive heads per workgroup, a causal tiled build, gave bitwise the same results
      // 4-8 % slower: profiles/r04_causal_tiled_dkdv.txt)
      const int nkb = N / 256;
      s.add(DKDV_SLOT_CAUSAL, batch * nkb, 512, nkb).rank_chunk = rank_chunk(1, nkb);
      return s;
    }
    // d = 64, causal (or tuning 3): slot-interleaved fast path for unmasked stages, per-sub-slice path on the diagonal
    // (a build with the masked paths compiled out, for non-causal launches, measured the same: 0.4983 vs 0.4992 ms)
    if (tun.v[0] != 4) {
      select_dkdv_phased<T, D>(s, c, true, 1);
      return s;
    }
  }
  if (BF && D <= 64) {
    // measured at B=8,H=8,N=4096,d=64 (ms, one device, profiles/README.md): 8 waves x 32 keys, 128-query stages,
    // software-pipelined sub-slices 0.505; not pipelined 0.514; 64-query stages 0.519; 256-query 0.525;
    // 4 waves x 32 keys (two workgroups per CU) 0.521; 4 waves x 64 keys (one wave per SIMD) 0.559
    select_dkdv_phased<T, D>(s, c);   // compiler-interleaved software pipeline (the d = 32 default; d = 64: option 0 = 4)
  } else if (BF) {
    // d = 128 default (dropout / key mask / N < 64: the 4-wave split-operand build, which has the registers for it): 8 waves x 32 keys,
    // one 256-key workgroup per CU (half the Q / dO staging per MFMA): 3.64 vs 3.92 ms
    select_dkdv_phased<T, D>(s, c, false, 0, tun.v[7] != 1);
  } else if (D == 64 && !c.lay.drop_thr) {
    // fp32, d = 64 (configs[1], [2]): the allocation lands on 256 VGPRs + 2 AGPRs = one wave per SIMD; asking for two
    // (launch bound) keeps it under 256
    const int nkb = (N + 127) / 128;
    // causal: longest block first across a chunk of heads instead of head by head: 0.57 vs 0.80 ms at the reference's timing-harness
    // shape (B = 8, H = 8, N = 2048, fp32), bitwise the same (option 7 = 1: head by head)
    s.add(DKDV_F32_64, batch * nkb, 256, nkb).rank_chunk = (causal && tun.v[7] != 1) ? rank_chunk(2, nkb) : 0;
  } else {
    select_dkdv_phased<T, D>(s, c);
  }
  return s;
}

template <typename T, int D>
Selection select_bwd(const Call& c) {
  const long rows = (long)c.batch * c.N;
  constexpr int RPB = 256 / (D / 8);
  const int need = FA_BWD_STAGE_PREP | FA_BWD_STAGE_DQ;
  Selection s, dq;
  s.onepass = onepass_f32<T, D>(c);
  // grouped-query heads: the one-pass kernel's cut sweep ADDS dK, dV into zeroed outputs with atomics; a grouped call that would take it
  // runs exactly what option 4 = 4 selects instead (two kernels, separate preprocess), whose per-head stores the ordered group sum adds
  const bool two_kernels = s.onepass && c.lay.G > 1;
  if (two_kernels) s.onepass = 0;
  if ((c.stages & FA_BWD_STAGE_DQ) && !s.onepass)
    dq = select_dq<T, D>(c, (c.stages & need) == need && c.tun.v[4] == 0 && !two_kernels);
  s.fuses_prep = dq.fuses_prep;
  if ((c.stages & FA_BWD_STAGE_PREP) && !s.fuses_prep) s.add(BWD_PREP, (int)((rows + RPB - 1) / RPB), 256);
  if (s.fuses_prep) s.append(dq);   // dQ first: it preprocesses its own rows and leaves -L/tau, -delta in the workspace for the dK/dV kernel
  if (s.onepass) {
    // the workgroups ADD into dq (the reference's caller zeroes q_grad for its atomicAdd as well: minitorch/cuda_kernel_ops.py:609-611);
    // the parts of a key block's sweep ADD their dK, dV
    s.add(ZERO_GRADS, 0, 0, 0, s.onepass);
    const int nkb = (c.N + 255) / 256;
    s.add(ONEPASS, c.batch * nkb * s.onepass, 512, nkb, s.onepass).rank_chunk =
        c.causal ? rank_chunk(1, nkb) : 0;   // key block 0 (the longest sweep) of a chunk of heads first
    return s;
  }
  if (c.stages & FA_BWD_STAGE_DKDV) {
    s.append(select_dkdv<T, D>(c));
    // grouped-query heads: the launches above stored dK, dV per QUERY head into the workspace's scratch; one ordered sum per group
    // (fa_aux.h: group_sum_kernel) writes the caller's Hkv heads, one thread per 16-byte chunk of them
    if (c.lay.G > 1) s.add(GROUP_SUM, (int)((rows / c.lay.G * (D / 4) + 255) / 256), 256);
  }
  if (!s.fuses_prep) s.append(dq);
  return s;
}

// The one executor: walks a selection and launches.  Which builds exist for <T, D> is decided here, by the if constexpr around each
// typed launch (fp32 d = 64 has no plain phased dK/dV build: its dropout calls alone come to that geometry).
template <typename T, int D>
int execute(const Call& c, const Selection& sel) {
  constexpr bool BF = sizeof(T) == 2;
  constexpr int BN = BF ? 64 : 32, NW = BF ? 8 : 4, QS = BF ? (D == 128 ? 64 : 128) : 32;   // forward key tile; phased dK/dV geometry
  const int batch = c.batch, N = c.N, causal = c.causal;
  const long rows = (long)batch * N;
#define FA_GO(kern, ...) hipLaunchKernelGGL(kern, dim3(s.grid), dim3(s.block), 0, c.st, __VA_ARGS__)
#define FA_QKV (const T*)c.q, (const T*)c.k, (const T*)c.v
#define FA_FWD(FEAT, CARE) \
  FA_GO((fa::fwd_kernel<T, D, BN, 1, FEAT, CARE>), FA_QKV, c.out, c.l, c.m, N, s.nb, batch, lay, causal, c.variant, c.tau, s.arg)
#define FA_FWD_SLOT(...) FA_GO((fa::fwd_slot_kernel<__VA_ARGS__>), FA_QKV, c.out, c.l, N, s.nb, batch, lay, s.arg, c.tau)
#define FA_DQ(FEAT, NWQ, ...)                                                                                                    \
  FA_GO((fa::bwd_dq_kernel<T, D, 32, FEAT, NWQ, ##__VA_ARGS__>), FA_QKV, (const T*)c.dout, c.nlc(), c.delta(), c.dq, N, s.nb, batch, lay, \
        causal, c.tau, s.arg, pa)
#define FA_DQ_SLOT(...)                                                                                                            \
  FA_GO((fa::bwd_dq_slot_kernel<T, D, ##__VA_ARGS__>), FA_QKV, (const T*)c.dout, c.nlc(), c.delta(), c.dq, N, s.nb, batch, lay, s.arg, \
        c.tau, pa)
#define FA_DKDV_SLOT(...)                                                                                                         \
  FA_GO((fa::bwd_dkdv_slot_kernel<T, 64, ##__VA_ARGS__>), FA_QKV, (const T*)c.dout, c.nl2(), c.delta(), c.dk, c.dv, N, s.nb, batch, lay, \
        c.tau)
#define FA_DKDV(...)                                                                                                               \
  FA_GO((fa::bwd_dkdv_kernel<T, D, 32, __VA_ARGS__>), FA_QKV, (const T*)c.dout, c.nlc(), c.delta(), c.dk, c.dv, N, s.nb, batch, lay, \
        causal, c.tau, s.arg)
#define FA_ONEPASS(C, R)                                                                                                         \
  FA_GO((fa::bwd_onepass_f32_kernel<D, C, R>), FA_QKV, (const T*)c.dout, c.nlc(), c.delta(), c.dq, c.dk, c.dv, N, s.nb, batch, lay, \
        c.tau, s.arg)
  for (int i = 0; i < sel.n; ++i) {
    const Step& s = sel.steps[i];
    fa::Layout lay = c.lay;
    lay.rank_chunk = s.rank_chunk;
    lay.tiles = s.tiles;
    lay.twin_blocks = s.twin_blocks;
    lay.guard_want = s.guard_want;
    const fa::DqPrep pa = s.prep ? fa::DqPrep{c.out, c.l, c.m, c.nlc(), c.delta(), c.nl2(), c.variant, 1.0f / c.tau} : fa::DqPrep{};
    switch (s.kern) {
      case FWD_SPLITK:
        if constexpr (!BF && D == 64)
          FA_GO((fa::fwd_splitk_f32_kernel<D>), FA_QKV, c.out, c.l, c.m, N, s.nb, batch, lay, causal, c.variant, c.tau);
        break;
      case FWD_SLOT_CAUSAL:
        if constexpr (BF && D >= 64) FA_FWD_SLOT(T, D, false, 64, (D == 64 ? 4 : 2), true);
        break;
      case FWD_SLOT_WHOLE:
        if constexpr (BF && D == 64) FA_FWD_SLOT(T, 64, false, 64, 4);
        else if constexpr (BF && D == 128) FA_FWD_SLOT(T, D, false);
        break;
      case FWD_SLOT_MASKED:
        if constexpr (BF && D == 64) FA_FWD_SLOT(T, D, true);
        break;
      case FWD_DROP: FA_FWD(2, BF); break;
      case FWD_MASK: FA_FWD(1, BF); break;
      case FWD_CARE: FA_FWD(0, BF); break;
      case FWD_MAIN: FA_FWD(0, false); break;
      case BWD_PREP:
        FA_GO((fa::bwd_prep_kernel<T, D>), c.out, (const T*)c.dout, c.l, c.m, c.nlc(), c.delta(), c.nl2(), rows, N, lay, c.variant,
              1.0f / c.tau);
        break;
      case DQ_DROP: FA_DQ(2, 4, BF); break;
      case DQ_MASK: FA_DQ(1, 4, BF); break;
      case DQ_CARE: FA_DQ(0, 4, BF); break;
      case DQ_MAIN: FA_DQ(0, 4, false); break;
      case DQ_WAVE8:
        if constexpr (BF && D == 128) FA_DQ(0, 8);
        break;
      case DQ_SLOT_CAUSAL:
        if constexpr (BF && D == 64) FA_DQ_SLOT(false, true);
        break;
      case DQ_SLOT_TILED:
        if constexpr (BF && D == 64) FA_DQ_SLOT(false, false, true);
        break;
      case DQ_SLOT_WHOLE:
        if constexpr (BF && D == 64) FA_DQ_SLOT(false);
        break;
      case DQ_SLOT_MASKED:
        if constexpr (BF && D == 64) FA_DQ_SLOT();
        break;
      case DKDV_SLOT64_TILED:
        if constexpr (BF && D == 64)
          FA_GO((fa::bwd_dkdv_slot64_kernel<T, 64>), FA_QKV, (const T*)c.dout, c.nl2(), c.delta(), c.dk, c.dv, N, s.nb, batch, lay, c.tau);
        break;
      case DKDV_SLOT:
        if constexpr (BF && D == 64) FA_DKDV_SLOT();
        break;
      case DKDV_SLOT_CAUSAL:
        if constexpr (BF && D == 64) FA_DKDV_SLOT(true);
        break;
      case DKDV_CARE_DROP:
        if constexpr (BF) FA_DKDV(4, 64, 1, true, 1, BF);
        break;
      case DKDV_CARE:
        if constexpr (BF) FA_DKDV(4, 64, 1, false, 1, BF);
        break;
      case DKDV_DROP_F32:
        if constexpr (!BF) FA_DKDV(NW, QS, 1, true);
        break;
      case DKDV_CARE_MAIN:
        if constexpr (BF && D == 64) FA_DKDV(NW, QS, 3, false, 1, true, true);
        break;
      case DKDV_PAIRED:
        if constexpr (!(BF && D == 128) && !(!BF && D == 64)) FA_DKDV(NW, QS, 0, false, 1, false, true);
        break;
      case DKDV_PAIRED_M3:
        if constexpr (BF && D == 64) FA_DKDV(NW, QS, 3, false, 1, false, true);
        break;
      case DKDV_PLAIN:
        if constexpr (!(!BF && D == 64)) FA_DKDV(NW, QS, 0);
        break;
      case DKDV_F32_64:
        if constexpr (!BF && D == 64)
          FA_GO((fa::bwd_dkdv_kernel<T, D, 32, 4, 32, 0, false, 2>), FA_QKV, (const T*)c.dout, c.nlc(), c.delta(), c.dk, c.dv, N, s.nb,
                batch, lay, causal, c.tau);
        break;
      case ONEPASS:
        if constexpr (!BF && D == 64) {
          if (N % 256 == 0) {
            if (causal) FA_ONEPASS(true, false); else FA_ONEPASS(false, false);
          } else {
            if (causal) FA_ONEPASS(true, true); else FA_ONEPASS(false, true);
          }
        }
        break;
      case GROUP_SUM:   // inner: 16-byte chunks between the heads of a group ([B][N][H][d]: d / 4; [B][H][N][d]: N * d / 4)
        FA_GO(fa::group_sum_kernel, c.dk, c.dv, c.gdk, c.gdv, rows / lay.G * (D / 4),
              c.layout == FA_LAYOUT_BNHD ? (long)(D / 4) : (long)N * (D / 4), lay.G);
        break;
      case GUARD_PASS:
      case GUARD_PASS_ZERO:
        if (const int rc = launch_scale_guard(c.q, c.k, rows, rows / lay.G, c.dp, c.dtype, const_cast<float*>(c.guard), c.st)) return rc;
        continue;
      case GUARD_ZERO:
        FA_HIP_TRY(hipMemsetAsync(const_cast<float*>(c.guard), 0, (size_t)2 * fa::GUARD_SLOTS * sizeof(float), c.st));
        continue;
      case ZERO_GRADS:   // [B][N][H][d] or [BH][N][d]: the tensor is one contiguous range either way
        FA_HIP_TRY(hipMemsetAsync(c.dq, 0, (size_t)rows * D * sizeof(float), c.st));
        if (s.arg > 1) {
          FA_HIP_TRY(hipMemsetAsync(c.dk, 0, (size_t)rows * D * sizeof(float), c.st));
          FA_HIP_TRY(hipMemsetAsync(c.dv, 0, (size_t)rows * D * sizeof(float), c.st));
        }
        continue;
    }
    if (s.check) FA_HIP_TRY(hipGetLastError());
  }
#undef FA_GO
#undef FA_QKV
#undef FA_FWD
#undef FA_FWD_SLOT
#undef FA_DQ
#undef FA_DQ_SLOT
#undef FA_DKDV_SLOT
#undef FA_DKDV
#undef FA_ONEPASS
  return FA_OK;
}

// tau uses the caller's d even when the rows are zero-padded to dp columns (zero columns of Q/K add
// nothing to the scores; zero columns of V produce zero output columns that are dropped).
// (K and V of an ungrouped call live where q does: group size 1, the same strides)
fa::Layout ungrouped(fa::Layout l) {
  l.G = 1;
  l.kvH = l.H;
  l.ldk = l.ld;
  return l;
}
fa::Layout bhnd(int N, int dp) { return ungrouped(fa::Layout{1, dp, (long)N * dp, 0, nullptr, 1, 0u, 1.0f, 0u, 0}); }
fa::Layout bnhd(int H, int N, int dp) { return ungrouped(fa::Layout{H, H * dp, (long)N * H * dp, (long)dp, nullptr, 1, 0u, 1.0f, 0u, 0}); }
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- where tau*log2(e) is applied (round 4) -------------------------------------------------------------------------------------
// The MFMA-slot kernels fold c = tau*log2(e) into one bf16 operand (one more 2^-9 relative rounding of q or k, worth 8-10 % of the
// step); everything else scales each score in fp32, as the reference does (src/flash_attn2_fw.cu:152-167).  The fold is invisible at
// the north star's U(-1, 1) inputs and grows with the square of the input magnitude (x2: 1.4e-3 on O against 0.7e-3; x6: 3.6e-2
// against 3.6e-3, profiles/r03_prescale_accuracy.txt), so it needs evidence about the operands:
//   * a call WITH a scale guard (fa_mi355x_scale_guard: one pass over q and k on the device, no host synchronisation) launches the
//     selected kernels AND their fp32-scaling twins; every workgroup evaluates the guard on entry and the launch on the wrong side of
//     the budget returns at once (fa_common.h: guard_skip).  Estimate: 2^-9 / sqrt(3) * c * max_rows |q| * max_rows |k| against
//     GUARD_BUDGET (log2 units): U(-1, 1) gives 5.7e-3 at d = 64 and 7e-3 at d = 128, inputs 1.3x larger go to fp32 scaling.
//   * a call WITHOUT one scales in fp32 (the phased forward; the backward's slot kernels carry both scalings in one launch and
//     take their fp32 copy of the sweep: no twin launches in the backward at all), unless
//     option 8 = 1 (the caller vouches for the range), the selection folds nothing anyway (fp32, d = 32, key mask, dropout, ragged N:
//     Selection::folds), or c is 1 (softmax_scale = ln 2: the operand multiply is exact).
constexpr float GUARD_BUDGET = 1e-2f;
inline Call exact(Call call) {   // the forward that scales every score in fp32 (the phased kernel), whatever else the caller selected
  call.tun.v[1] = 2;
  return call;
}
template <typename T, int D>
Selection select_one(const Call& c) { return c.bwd ? select_bwd<T, D>(c) : select_fwd<T, D>(c); }

// Everything one call runs, in order; completes call.lay (scale_sel, guard, guard_coef; guard_want belongs to the steps).
// produce (forward calls only, option 8 = 0): the call FILLS `guard` instead of reading it, so that the backward of the same (q, k)
// can take it: a forward that folds produces it inside its own launch (fa_common.h: guard_produce: no separate pass over q and k;
// the launch runs with the folded scale and its fp32-scaling twin, behind it, redoes the call if the finished guard says so);
// a forward whose selection folds nothing runs the separate pass, because the backward of the same call may fold.
// planning: fa_mi355x_plan is asking (option 8 = 3 then plans a guarded call; a real call has its guard or none).
template <typename T, int D>
Selection select_call(Call& call, bool planning) {
  const float c = call.tau * fa::LOG2E;
  const int mode = call.tun.v[8], produce = call.produce;
  const float* guard = call.guard;
  fa::Layout& lay = call.lay;
  lay.scale_sel = 0;
  const Selection sel = select_one<T, D>(call);
  if (mode == 1 || fabsf(c - 1.0f) < 1e-6f) return sel;
  if (mode == 3 && planning) guard = reinterpret_cast<const float*>(16);   // both launches of a guarded call
  // the backward's MFMA-slot kernels hold both scalings in one launch: fp32 scaling without a guard, the guard's choice with one
  lay.scale_sel = (mode == 2 || !guard) ? 1 : 2;
  if (lay.scale_sel == 2) {
    lay.guard = guard;
    lay.guard_coef = c * (0.001953125f * 0.57735027f) / GUARD_BUDGET;
  }
  // ... any forward that cannot fill the guard itself by the separate pass over q and k
  const Kern pass = guard_rows_fold(call.dtype, call.dp) ? GUARD_PASS : GUARD_PASS_ZERO;
  Selection out;
  if (!sel.folds) {
    if (produce && guard && mode == 0) out.add(pass, 0, 0);
    out.append(sel, lay.scale_sel == 2 ? 3 : 0);   // (guard_want 3: no launch of this run is skipped)
    return out;
  }
  if (mode == 2 || !guard) return select_one<T, D>(exact(call));
  if (produce && sel.produces_guard) out.add(GUARD_ZERO, 0, 0);   // the folding forward fills the zeroed buffer
  else if (produce) out.add(pass, 0, 0);                         // (a folding forward that cannot: the causal slot build)
  out.append(sel, (produce && sel.produces_guard) ? 2 : 0);
  lay.guard_want = 1;   // (the twin's launch shape depends on it: select_phased)
  out.append(select_one<T, D>(exact(call)), 1);
  return out;
}

#define FA_DISPATCH(FN, ...)                                                              \
  do {                                                                                    \
    if (c.dtype == FA_DTYPE_BF16) {                                                       \
      if (c.dp == 32) return FN<fa::bf16_t, 32>(__VA_ARGS__);                             \
      if (c.dp == 64) return FN<fa::bf16_t, 64>(__VA_ARGS__);                             \
      return FN<fa::bf16_t, 128>(__VA_ARGS__);                                            \
    } else {                                                                              \
      if (c.dp == 32) return FN<float, 32>(__VA_ARGS__);                                  \
      if (c.dp == 64) return FN<float, 64>(__VA_ARGS__);                                  \
      return FN<float, 128>(__VA_ARGS__);                                                 \
    }                                                                                     \
  } while (0)
Selection select_any(Call& c, bool planning) {
  c.tau = c.scale > 0.f ? c.scale : sqrtf(1.0f / (float)c.d);   // (scale: fa_mi355x_*_scaled / _guarded; the reference has sqrt(1/d) only)
  if (!c.bwd) c.lay.out_bf16 = c.tun.v[9] == 1 ? 1 : 0;
  FA_DISPATCH(select_call, c, planning);
}
int execute_any(const Call& c, const Selection& sel) { FA_DISPATCH(execute, c, sel); }
#undef FA_DISPATCH

int dispatch(Call c, bool bwd) {
  c.bwd = bwd;
  const Selection sel = select_any(c, false);
  return execute_any(c, sel);
}
int fwd_dispatch(const Call& c) { return dispatch(c, false); }
int bwd_dispatch(const Call& c) { return dispatch(c, true); }

// The checks of every device entry point, in one order: the first that fails decides the return code and fa_mi355x_last_error().
// The rules that differ between entry points are the call's fields (bwd, by_heads, padded, scale_required; arguments an entry point
// does not take keep defaults that pass).  Completes the call: batch, dp, tun, lay.
int validate(Call& c) {
  g_err[0] = 0;
  if (int rc = parse_opts(c.opts, c.nopts, c.tun)) return rc;
  if (c.bwd && (c.stages <= 0 || c.stages > FA_BWD_STAGE_ALL)) return set_err(FA_ERR_BAD_ARG, "bad stages mask");
  if (c.by_heads && (c.B <= 0 || c.H <= 0)) return set_err(FA_ERR_BAD_ARG, "B and H must be positive");
  if (c.gqa && (c.Hkv <= 0 || c.H % c.Hkv != 0)) return set_err(FA_ERR_BAD_ARG, "Hkv must be positive and divide H");
  c.batch = c.B * c.H;
  if (c.batch <= 0 || c.N <= 0 || c.d <= 0) return set_err(FA_ERR_BAD_ARG, "batch, N and d must be positive");
  if (c.variant != FA_VARIANT_FA1 && c.variant != FA_VARIANT_FA2) return set_err(FA_ERR_BAD_ARG, "unknown variant");
  if (c.dtype != FA_DTYPE_F32 && c.dtype != FA_DTYPE_BF16) return set_err(FA_ERR_BAD_ARG, "unknown dtype");
  if ((long)c.N * 128 * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "N too large: one (batch*head) matrix must stay under 2 GiB");
  if (!c.q || !c.k || !c.v || !c.out || !c.l || (c.variant == FA_VARIANT_FA1 && !c.m) ||
      (c.bwd && (!c.dout || !c.dq || !c.dk || !c.dv || !c.ws)))
    return set_err(FA_ERR_BAD_ARG, "null pointer argument");
  if (c.produce && !c.guard) return set_err(FA_ERR_BAD_ARG, "produce_guard needs a guard buffer");
  if (!c.padded) c.dp = c.d;
  if (c.padded && (!d_supported(c.dp) || c.d > c.dp))
    return set_err(FA_ERR_UNSUPPORTED_D, "padded row length dp must be 32, 64 or 128 and >= d");
  if (!d_supported(c.dp)) return set_err(FA_ERR_UNSUPPORTED_D, "device path supports d in {32, 64, 128}");
  if (c.by_heads && c.layout != FA_LAYOUT_BHND && c.layout != FA_LAYOUT_BNHD) return set_err(FA_ERR_BAD_ARG, "unknown layout");
  if (c.scale_required && (!(c.scale > 0.f) || !std::isfinite(c.scale)))
    return set_err(FA_ERR_BAD_ARG, "softmax_scale must be positive and finite");
  if (c.scale != 0.f && (!(c.scale > 0.f) || !std::isfinite(c.scale)))
    return set_err(FA_ERR_BAD_ARG, "softmax_scale must be positive and finite (0: sqrt(1/d))");
  if (c.by_heads && (long)c.N * c.H * c.d * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "one batch element must stay under 2 GiB");
  if (!(c.drop_rate >= 0.0f && c.drop_rate < 1.0f)) return set_err(FA_ERR_BAD_ARG, "dropout rate must be in [0, 1)");
  c.lay = c.layout == FA_LAYOUT_BNHD ? bnhd(c.H, c.N, c.dp) : bhnd(c.N, c.dp);
  c.lay.kmask = c.kmask;
  c.lay.mask_heads = c.mask_heads;
  c.lay.drop_thr = (uint32_t)((double)c.drop_rate * 16777216.0);   // floor(rate * 2^24); 0 disables dropout
  c.lay.drop_scale = c.drop_scale;
  c.lay.drop_seed = c.drop_seed;
  if (c.gqa && c.Hkv < c.H) {   // (Hkv == H is by definition the ungrouped call: no scratch, no group sum)
    // K / V with their own row stride (fa::Layout; their matrices are no larger than q's: the size bounds above cover them)
    c.lay.G = c.H / c.Hkv;
    const bool rows_by_head = c.layout == FA_LAYOUT_BNHD;
    c.lay.kvH = rows_by_head ? c.Hkv : 1;
    c.lay.ldk = rows_by_head ? c.Hkv * c.dp : c.dp;
    if (c.bwd) {   // the dK/dV kernels store per query head into the scratch behind the row constants (fa_mi355x_bwd_workspace_bytes_gqa)
      // (the group sum reads it in 16-byte pieces)
      if ((uintptr_t)c.ws % 256 != 0) return set_err(FA_ERR_BAD_ARG, "the workspace of a grouped backward must be 256-byte aligned");
      const size_t elems = (size_t)c.batch * c.N * c.dp;
      float* scratch = reinterpret_cast<float*>(reinterpret_cast<char*>(c.ws) + align256((size_t)WS_VECS * c.batch * c.N * sizeof(float)));
      c.gdk = c.dk;
      c.gdv = c.dv;
      c.dk = scratch;
      c.dv = scratch + elems;
    }
  }
  return FA_OK;
}

int validate_and_dispatch(Call c) {
  if (int rc = validate(c)) return rc;
  return c.bwd ? bwd_dispatch(c) : fwd_dispatch(c);
}

Call fwd_call(const void* q, const void* k, const void* v, float* out, float* l, float* m, int B, int N, int d, int causal,
              int variant, int dtype, void* stream) {
  Call c;
  c.q = q; c.k = k; c.v = v; c.out = out; c.l = l; c.m = m;
  c.B = B; c.N = N; c.d = d; c.causal = causal ? 1 : 0; c.variant = variant; c.dtype = dtype; c.st = (hipStream_t)stream;
  return c;
}
Call bwd_call(const void* q, const void* k, const void* v, const float* out, const void* dout, float* dq, float* dk, float* dv,
              const float* l, const float* m, void* ws, int B, int N, int d, int causal, int variant, int dtype, int stages,
              void* stream) {
  Call c = fwd_call(q, k, v, const_cast<float*>(out), const_cast<float*>(l), const_cast<float*>(m), B, N, d, causal, variant, dtype,
                    stream);
  c.bwd = true;
  c.dout = dout; c.dq = dq; c.dk = dk; c.dv = dv; c.ws = (float*)ws; c.stages = stages;
  return c;
}
Call heads(Call c, int H, int layout) {   // the B, H, layout form (fwd_call / bwd_call took B)
  c.by_heads = true;
  c.H = H;
  c.layout = layout;
  return c;
}


// ---- host-pointer path ------------------------------------------------------------------------
// A grow-only device arena replaces the reference's per-call cudaMalloc/cudaFree of 6 (fw) or 10 (bw)
// buffers (src/flash_attn_fw.cu:315-322,352-357).
std::mutex g_pool_mu;
void* g_pool = nullptr;
size_t g_pool_bytes = 0;
int g_pool_dev = -1;   // the arena belongs to the device that was current when it was allocated

hipError_t pool_reserve(size_t bytes) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (g_pool && dev == g_pool_dev && bytes <= g_pool_bytes) return hipSuccess;
  if (g_pool) {   // grow, or the caller moved to another device: the old arena is released on ITS device
    int cur = dev;
    if (g_pool_dev != dev) hipSetDevice(g_pool_dev);
    e = hipFree(g_pool);
    if (g_pool_dev != cur) hipSetDevice(cur);
    g_pool = nullptr;
    g_pool_bytes = 0;
    if (e != hipSuccess) return e;
  }
  e = hipMalloc(&g_pool, bytes);
  if (e == hipSuccess) {
    g_pool_bytes = bytes;
    g_pool_dev = dev;
  }
  return e;
}

[[noreturn]] void die(const char* what, hipError_t e) {
  // src/flash_attn_fw.cu:343-349: message on stderr, exit(EXIT_FAILURE)
  fprintf(stderr, "Flash Attention Error: %s%s%s\n", what, e != hipSuccess ? ": " : "",
          e != hipSuccess ? hipGetErrorString(e) : "");
  exit(EXIT_FAILURE);
}
#define FA_HOST_TRY(expr)                        \
  do {                                           \
    hipError_t e_ = (expr);                      \
    if (e_ != hipSuccess) die(#expr, e_);        \
  } while (0)

// host [rows][d] -> device [rows][dp] (zero padded columns)
void h2d_rows(float* dst, const float* src, size_t rows, int d, int dp, hipStream_t st) {
  if (d == dp) {
    FA_HOST_TRY(hipMemcpyAsync(dst, src, rows * d * sizeof(float), hipMemcpyHostToDevice, st));
  } else {
    FA_HOST_TRY(hipMemsetAsync(dst, 0, rows * dp * sizeof(float), st));
    FA_HOST_TRY(hipMemcpy2DAsync(dst, dp * sizeof(float), src, d * sizeof(float), d * sizeof(float), rows,
                                 hipMemcpyHostToDevice, st));
  }
}
void d2h_rows(float* dst, const float* src, size_t rows, int d, int dp, hipStream_t st) {
  if (d == dp) {
    FA_HOST_TRY(hipMemcpyAsync(dst, src, rows * d * sizeof(float), hipMemcpyDeviceToHost, st));
  } else {
    FA_HOST_TRY(hipMemcpy2DAsync(dst, d * sizeof(float), src, dp * sizeof(float), d * sizeof(float), rows,
                                 hipMemcpyDeviceToHost, st));
  }
}


// ---- host-pointer path as a pipeline --------------------------------------------------------
// The reference uploads everything, runs one kernel, downloads everything (src/flash_attn_fw.cu:314-357).  Here the call is
// cut into chunks of (batch*head) rows: H2D of chunk c+1, the kernels of chunk c and D2H of chunk c-1 run on three streams
// (both DMA directions and the compute overlap), and the caller's arrays are pinned in place for the duration of the call
// (hipHostRegister: no staging copy by the CPU; a range that cannot be pinned is copied pageable, same results).
// The caller's arrays, pinned in place for the duration of one host-pointer call.  Round 3: the arrays of a call are registered as
// PAGE-ALIGNED, MERGED ranges.  Registering each array on its own (round 2) broke intermittently: NumPy arrays of 1-32 MiB come from the
// malloc heap once glibc has raised its mmap threshold, so two arrays of one call (l and m, say) can share a boundary page; registering
// overlapping pages twice made a later hipHostUnregister fail ("pointer does not correspond to a registered memory region", which then
// surfaced as the NEXT call's last error) and, worse, left the runtime with a stale pinned range that a later pageable copy into the
// recycled pages tripped over (an abort from a runtime thread: seen twice in sixteen runs of the GPU suite).  Unregistering clears the
// sticky error; every host call starts by clearing whatever an earlier HIP user left behind.
// Process-wide counters of the host launchers' pinning (fa_mi355x_host_pin_stats): merged ranges registered, and ranges that could not
// be (copied pageable instead: same results, slower).  A regression to "nothing is ever pinned" shows here, not only as time.
std::atomic<unsigned long long> g_pin_ok{0}, g_pin_fallback{0};
struct PinSet {
  struct Range { uintptr_t b, e; };
  std::vector<Range> want, held;
  // Opt-in since the end of round 4 (FA_MI355X_HOST_PIN=1).  Default: the caller's arrays are copied as pageable memory, as the reference
  // does (src/flash_attn_fw.cu:314-357): HIP's own pageable path measured the SAME time inside the C call at configs[1] / configs[2]
  // (1.44 / 2.94 and 3.09 / 6.4 ms fw / bw) and is faster through the Python operator surface at the metric shape (13.0 vs 36.9 ms
  // forward: registering freshly allocated result arrays faults their pages in); in-place pinning wins only the metric-shape backward
  // (10.9 vs 15.6 ms).  And one more abort from an HSA runtime thread (main thread in a later, unrelated pageable torch copy) was seen in
  // about fifteen runs of the GPU suite after round 3's merged-range fix: registrations of recycled heap pages by this library and the
  // runtime's own pin cache for pageable copies can still overlap.  Not registering anything removes this library's side of that.
  static bool enabled() {
    static const bool on = [] { const char* e = getenv("FA_MI355X_HOST_PIN"); return e && e[0] == '1'; }();
    return on;
  }
  // EVERY host array of the call is added, whatever its size: an array that shares a page with a pinned neighbour must lie inside the
  // pinned range as a whole (a copy that starts inside a registered range and runs past its end is an invalid argument to HIP)
  void add(const void* ptr, size_t bytes) {
    if (!enabled() || !ptr || !bytes) return;
    static const uintptr_t page = [] { const long p = sysconf(_SC_PAGESIZE); return (uintptr_t)(p > 0 ? p : 4096); }();
    const uintptr_t a = (uintptr_t)ptr;
    want.push_back(Range{a & ~(page - 1), (a + bytes + page - 1) & ~(page - 1)});
  }
  void lock() {
    std::sort(want.begin(), want.end(), [](const Range& x, const Range& y) { return x.b < y.b; });
    std::vector<Range> merged;
    for (const Range& r : want) {
      if (!merged.empty() && r.b <= merged.back().e) merged.back().e = std::max(merged.back().e, r.e);
      else merged.push_back(r);
    }
    for (const Range& r : merged) {
      if (r.e - r.b < (4u << 20)) continue;   // (small and on pages of its own: the pageable path costs less than a registration)
      if (hipHostRegister((void*)r.b, r.e - r.b, hipHostRegisterDefault) == hipSuccess) {
        held.push_back(r);
        g_pin_ok.fetch_add(1, std::memory_order_relaxed);
      } else {
        (void)hipGetLastError();   // (already registered by the caller, or not lockable: copied pageable)
        g_pin_fallback.fetch_add(1, std::memory_order_relaxed);
      }
    }
  }
  ~PinSet() {
    for (const Range& r : held)
      if (hipHostUnregister((void*)r.b) != hipSuccess) (void)hipGetLastError();
  }
  PinSet() = default;
  PinSet(const PinSet&) = delete;
  PinSet& operator=(const PinSet&) = delete;
};
struct HostPipe {
  hipStream_t up = nullptr, down = nullptr;
  std::vector<hipEvent_t> ev;
  int dev = -1;   // streams and events belong to the device that was current when they were created (like the arena)
  hipEvent_t event(size_t i) {
    while (ev.size() <= i) {
      hipEvent_t e;
      FA_HOST_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      ev.push_back(e);
    }
    return ev[i];
  }
  void release() {   // on the device they were created on
    if (dev < 0) return;
    int cur = 0;
    FA_HOST_TRY(hipGetDevice(&cur));
    if (cur != dev) FA_HOST_TRY(hipSetDevice(dev));
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    ev.clear();
    if (up) (void)hipStreamDestroy(up);
    if (down) (void)hipStreamDestroy(down);
    up = down = nullptr;
    if (cur != dev) FA_HOST_TRY(hipSetDevice(cur));
    dev = -1;
  }
  void init() {
    int cur = 0;
    FA_HOST_TRY(hipGetDevice(&cur));
    if (dev >= 0 && dev != cur) release();   // the caller moved to another device since the last host-pointer call
    if (!up) FA_HOST_TRY(hipStreamCreateWithFlags(&up, hipStreamNonBlocking));
    if (!down) FA_HOST_TRY(hipStreamCreateWithFlags(&down, hipStreamNonBlocking));
    dev = cur;
  }
};
HostPipe g_pipe;   // guarded by g_pool_mu, like the arena
// FA_MI355X_HOST_TIMING=1: one stderr line per host-pointer call with the time spent pinning, in the pipeline, and unpinning
struct HostTimer {
  const char* what;
  bool on;
  std::chrono::steady_clock::time_point t0, t1, t2;
  explicit HostTimer(const char* w) : what(w), on(getenv("FA_MI355X_HOST_TIMING") != nullptr) { t0 = t1 = t2 = std::chrono::steady_clock::now(); }
  void pinned() { t1 = std::chrono::steady_clock::now(); }
  void piped() { t2 = std::chrono::steady_clock::now(); }
  ~HostTimer() {
    if (!on) return;
    const auto t3 = std::chrono::steady_clock::now();
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    fprintf(stderr, "[fa_mi355x host %s] pin %.2f ms, pipeline %.2f ms, unpin %.2f ms\n", what, ms(t0, t1), ms(t1, t2), ms(t2, t3));
  }
};
// The call of one chunk of a host-pointer launcher (fp32 rows of dp elements in the arena, default options; the launcher has checked
// its arguments itself): the pointers are filled in per chunk
Call host_call(int batch, int N, int d, int dp, bool causal, int variant, hipStream_t st) {
  Call c;
  c.batch = batch; c.N = N; c.d = d; c.dp = dp; c.causal = causal ? 1 : 0; c.variant = variant; c.dtype = FA_DTYPE_F32; c.st = st;
  c.lay = bhnd(N, dp);
  return c;
}
inline int host_chunks(int batch, size_t bytes_per_bh) {
  // ~32 MiB of input per chunk and tensor, at most 8 chunks: enough to hide the tails, few enough to keep the launches cheap
  const size_t want = (bytes_per_bh * (size_t)batch + (32u << 20) - 1) / (32u << 20);
  return (int)std::max<size_t>(1, std::min<size_t>({want, (size_t)8, (size_t)batch}));
}


// the selectors only pass the call's pointers on to the steps, which are not executed here: any non-null values do
Call plan_call(int B, int N, int d, int causal, int variant, int dtype, int stages, const int* opts, int nopts) {
  float* one = reinterpret_cast<float*>(256);   // (aligned as validate() asks of a grouped backward's workspace)
  Call c = bwd_call(one, one, one, one, one, one, one, one, one, one, one, B, N, d, causal, variant, dtype, stages, nullptr);
  c.bwd = stages != 0;   // stages = 0: the forward
  c.opts = opts;
  c.nopts = nopts;
  return c;
}
int plan(Call c, char* out, size_t n, bool builds = false) {
  if (int rc = validate(c)) return rc;
  if (!out || n == 0) return set_err(FA_ERR_BAD_ARG, "null output buffer");
  const Selection sel = select_any(c, true);   // built exactly as a real call builds it
  std::string joined;
  for (int i = 0; i < sel.n; ++i)
    if (const char* name = KERN_NAME[sel.steps[i].kern])
      joined += (joined.empty() ? "" : ";") + std::string(builds ? BUILD_NAME[sel.steps[i].kern] : name);
  if (joined.size() + 1 > n) return set_err(FA_ERR_BAD_ARG, "plan buffer too small");
  memcpy(out, joined.c_str(), joined.size() + 1);
  return FA_OK;
}
Call grouped(Call c, int H, int Hkv, int layout) {   // the B, H, Hkv, layout form of fa_mi355x_*_gqa
  c = heads(c, H, layout);
  c.gqa = true;
  c.Hkv = Hkv;
  return c;
}

}  // namespace

extern "C" {

const char* fa_mi355x_last_error(void) { return g_err; }
const char* fa_mi355x_version(void) { return "flash_attn_mi355x 0.2 gfx950"; }

int fa_mi355x_measure_mfma_peak(double min_ms, double* tflops, double* clock_ghz, void* stream) {
  g_err[0] = 0;
  if (!tflops || !clock_ghz || !(min_ms > 0)) return set_err(FA_ERR_BAD_ARG, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  hipDeviceProp_t prop;
  int dev = 0;
  FA_HIP_TRY(hipGetDevice(&dev));
  FA_HIP_TRY(hipGetDeviceProperties(&prop, dev));
  const int blocks = prop.multiProcessorCount, iters = 4000;
  struct Res {   // released on every exit
    float* sink = nullptr;
    unsigned long long* stamps = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Res() {
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
      if (sink) (void)hipFree(sink);
      if (stamps) (void)hipFree(stamps);
    }
  } r;
  FA_HIP_TRY(hipMalloc(&r.sink, (size_t)blocks * 512 * sizeof(float)));
  FA_HIP_TRY(hipMalloc(&r.stamps, (size_t)blocks * 16 * sizeof(unsigned long long)));
  FA_HIP_TRY(hipEventCreate(&r.e0));
  FA_HIP_TRY(hipEventCreate(&r.e1));
  // back-to-back launches until min_ms have passed (the clock settles under load); the last batch is the one reported
  double ms_per = 0.0, spent = 0.0;
  int reps = 4;
  for (int round = 0; round < 6 && spent < min_ms; ++round) {
    FA_HIP_TRY(hipEventRecord(r.e0, st));
    for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(fa::mfma_peak_kernel, dim3(blocks), dim3(512), 0, st, r.sink, r.stamps, iters);
    FA_HIP_TRY(hipEventRecord(r.e1, st));
    FA_HIP_TRY(hipEventSynchronize(r.e1));
    float ms = 0.f;
    FA_HIP_TRY(hipEventElapsedTime(&ms, r.e0, r.e1));
    ms_per = ms / reps;
    spent += ms;
    reps *= 2;
  }
  std::vector<unsigned long long> h((size_t)blocks * 16);
  FA_HIP_TRY(hipMemcpy(h.data(), r.stamps, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  double cyc = 0, ticks = 0;
  for (size_t i = 0; i + 1 < h.size(); i += 2) { cyc += (double)h[i]; ticks += (double)h[i + 1]; }
  *clock_ghz = ticks > 0 ? cyc / ticks * 0.1 : 0.0;
  *tflops = (double)blocks * 8.0 * iters * 8.0 * (2.0 * 32 * 32 * 16) / (ms_per * 1e-3) / 1e12;
  return FA_OK;
}


int fa_mi355x_plan(int batch, int N, int d, int causal, int variant, int dtype, int stages, const int* opts, int nopts, char* out,
                   size_t n) {
  return plan(plan_call(batch, N, d, causal, variant, dtype, stages, opts, nopts), out, n);
}

int fa_mi355x_plan_builds(int batch, int N, int d, int causal, int variant, int dtype, int stages, const int* opts, int nopts,
                          char* out, size_t n) {
  return plan(plan_call(batch, N, d, causal, variant, dtype, stages, opts, nopts), out, n, true);
}

int fa_mi355x_plan_gqa(int B, int H, int Hkv, int N, int d, int causal, int variant, int dtype, int stages, const int* opts,
                       int nopts, char* out, size_t n) {
  return plan(grouped(plan_call(B, N, d, causal, variant, dtype, stages, opts, nopts), H, Hkv, FA_LAYOUT_BHND), out, n);
}

int fa_mi355x_fwd(const void* q, const void* k, const void* v, float* out, float* l, float* m, int batch, int N,
                  int d, int causal, int variant, int dtype, void* stream) {
  return validate_and_dispatch(fwd_call(q, k, v, out, l, m, batch, N, d, causal, variant, dtype, stream));
}

int fa_mi355x_fwd_ex(const void* q, const void* k, const void* v, float* out, float* l, float* m, int batch, int N, int d,
                     int causal, int variant, int dtype, const int* opts, int nopts, void* stream) {
  Call c = fwd_call(q, k, v, out, l, m, batch, N, d, causal, variant, dtype, stream);
  c.opts = opts;
  c.nopts = nopts;
  return validate_and_dispatch(c);
}

int fa_mi355x_bwd_ex(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad,
                     float* k_grad, float* v_grad, const float* l, const float* m, void* workspace, int batch, int N, int d,
                     int causal, int variant, int dtype, int stages, const int* opts, int nopts, void* stream) {
  Call c = bwd_call(q, k, v, out, out_grad, q_grad, k_grad, v_grad, l, m, workspace, batch, N, d, causal, variant, dtype, stages, stream);
  c.opts = opts;
  c.nopts = nopts;
  return validate_and_dispatch(c);
}

int fa_mi355x_fwd_scaled(const void* q, const void* k, const void* v, float* out, float* l, float* m, int B, int H, int N, int d,
                         int layout, float softmax_scale, int causal, int variant, int dtype, void* stream) {
  Call c = heads(fwd_call(q, k, v, out, l, m, B, N, d, causal, variant, dtype, stream), H, layout);
  c.scale = softmax_scale;
  c.scale_required = true;
  return validate_and_dispatch(c);
}

int fa_mi355x_bwd_scaled(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad,
                         float* k_grad, float* v_grad, const float* l, const float* m, void* workspace, int B, int H, int N, int d,
                         int layout, float softmax_scale, int causal, int variant, int dtype, void* stream) {
  Call c = heads(bwd_call(q, k, v, out, out_grad, q_grad, k_grad, v_grad, l, m, workspace, B, N, d, causal, variant, dtype,
                          FA_BWD_STAGE_ALL, stream), H, layout);
  c.scale = softmax_scale;
  c.scale_required = true;
  return validate_and_dispatch(c);
}

int fa_mi355x_fwd_padded(const void* q, const void* k, const void* v, float* out, float* l, float* m, int batch, int N, int d,
                         int dp, int causal, int variant, int dtype, void* stream) {
  Call c = fwd_call(q, k, v, out, l, m, batch, N, d, causal, variant, dtype, stream);
  c.padded = true;
  c.dp = dp;
  return validate_and_dispatch(c);
}

int fa_mi355x_bwd_padded(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad,
                         float* k_grad, float* v_grad, const float* l, const float* m, void* workspace, int batch, int N, int d,
                         int dp, int causal, int variant, int dtype, void* stream) {
  Call c = bwd_call(q, k, v, out, out_grad, q_grad, k_grad, v_grad, l, m, workspace, batch, N, d, causal, variant, dtype,
                    FA_BWD_STAGE_ALL, stream);
  c.padded = true;
  c.dp = dp;
  return validate_and_dispatch(c);
}

int fa_mi355x_fwd_layout(const void* q, const void* k, const void* v, float* out, float* l, float* m, int B, int H,
                         int N, int d, int layout, int causal, int variant, int dtype, void* stream) {
  return validate_and_dispatch(heads(fwd_call(q, k, v, out, l, m, B, N, d, causal, variant, dtype, stream), H, layout));
}

int fa_mi355x_bwd_layout(const void* q, const void* k, const void* v, const float* out, const void* out_grad,
                         float* q_grad, float* k_grad, float* v_grad, const float* l, const float* m, void* workspace,
                         int B, int H, int N, int d, int layout, int causal, int variant, int dtype, void* stream) {
  return validate_and_dispatch(heads(bwd_call(q, k, v, out, out_grad, q_grad, k_grad, v_grad, l, m, workspace, B, N, d, causal,
                                              variant, dtype, FA_BWD_STAGE_ALL, stream), H, layout));
}

int fa_mi355x_fwd_masked(const void* q, const void* k, const void* v, float* out, float* l, float* m,
                         const float* key_mask, int B, int H, int N, int d, int layout, int causal, int variant,
                         int dtype, void* stream) {
  Call c = heads(fwd_call(q, k, v, out, l, m, B, N, d, causal, variant, dtype, stream), H, layout);
  c.kmask = key_mask;   // NULL: same as fa_mi355x_fwd_layout
  c.mask_heads = H;
  return validate_and_dispatch(c);
}

int fa_mi355x_bwd_masked(const void* q, const void* k, const void* v, const float* out, const void* out_grad,
                         float* q_grad, float* k_grad, float* v_grad, const float* l, const float* m,
                         const float* key_mask, void* workspace, int B, int H, int N, int d, int layout, int causal,
                         int variant, int dtype, void* stream) {
  Call c = heads(bwd_call(q, k, v, out, out_grad, q_grad, k_grad, v_grad, l, m, workspace, B, N, d, causal, variant, dtype,
                          FA_BWD_STAGE_ALL, stream), H, layout);
  c.kmask = key_mask;
  c.mask_heads = H;
  return validate_and_dispatch(c);
}

int fa_mi355x_fwd_dropout(const void* q, const void* k, const void* v, float* out, float* l, float* m,
                          const float* key_mask, float rate, float scale, unsigned seed, int B, int H, int N, int d,
                          int layout, int causal, int variant, int dtype, void* stream) {
  Call c = heads(fwd_call(q, k, v, out, l, m, B, N, d, causal, variant, dtype, stream), H, layout);
  c.kmask = key_mask;
  c.mask_heads = H;
  c.drop_rate = rate;
  c.drop_scale = scale;
  c.drop_seed = seed;
  return validate_and_dispatch(c);
}

int fa_mi355x_bwd_dropout(const void* q, const void* k, const void* v, const float* out, const void* out_grad,
                          float* q_grad, float* k_grad, float* v_grad, const float* l, const float* m,
                          const float* key_mask, float rate, float scale, unsigned seed, void* workspace, int B, int H,
                          int N, int d, int layout, int causal, int variant, int dtype, void* stream) {
  Call c = heads(bwd_call(q, k, v, out, out_grad, q_grad, k_grad, v_grad, l, m, workspace, B, N, d, causal, variant, dtype,
                          FA_BWD_STAGE_ALL, stream), H, layout);
  c.kmask = key_mask;
  c.mask_heads = H;
  c.drop_rate = rate;
  c.drop_scale = scale;
  c.drop_seed = seed;
  return validate_and_dispatch(c);
}

void fa_mi355x_host_pin_stats(unsigned long long* pinned_ranges, unsigned long long* pageable_ranges) {
  if (pinned_ranges) *pinned_ranges = g_pin_ok.load(std::memory_order_relaxed);
  if (pageable_ranges) *pageable_ranges = g_pin_fallback.load(std::memory_order_relaxed);
}

size_t fa_mi355x_guard_bytes(void) { return (size_t)2 * fa::GUARD_SLOTS * sizeof(float); }

int fa_mi355x_scale_guard(const void* q, const void* k, long rows, int row_elems, int dtype, void* guard, void* stream) {
  g_err[0] = 0;
  if (!q || !k || !guard || rows <= 0) return set_err(FA_ERR_BAD_ARG, "bad argument");
  if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_BF16) return set_err(FA_ERR_BAD_ARG, "unknown dtype");
  return launch_scale_guard(q, k, rows, rows, row_elems, dtype, guard, (hipStream_t)stream);
}

int fa_mi355x_scale_guard_gqa(const void* q, const void* k, long q_rows, long k_rows, int row_elems, int dtype, void* guard,
                              void* stream) {
  g_err[0] = 0;
  if (!q || !k || !guard || q_rows <= 0 || k_rows <= 0) return set_err(FA_ERR_BAD_ARG, "bad argument");
  if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_BF16) return set_err(FA_ERR_BAD_ARG, "unknown dtype");
  return launch_scale_guard(q, k, q_rows, k_rows, row_elems, dtype, guard, (hipStream_t)stream);
}

int fa_mi355x_fwd_guarded(const void* q, const void* k, const void* v, float* out, float* l, float* m, int B, int H, int N, int d,
                          int layout, float softmax_scale, int causal, int variant, int dtype, const int* opts, int nopts,
                          void* guard, int produce_guard, void* stream) {
  Call c = heads(fwd_call(q, k, v, out, l, m, B, N, d, causal, variant, dtype, stream), H, layout);
  c.scale = softmax_scale;
  c.opts = opts;
  c.nopts = nopts;
  c.guard = (const float*)guard;
  c.produce = produce_guard ? 1 : 0;
  return validate_and_dispatch(c);
}

int fa_mi355x_bwd_guarded(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad,
                          float* k_grad, float* v_grad, const float* l, const float* m, void* workspace, int B, int H, int N, int d,
                          int layout, float softmax_scale, int causal, int variant, int dtype, int stages, const int* opts,
                          int nopts, const void* guard, void* stream) {
  Call c = heads(bwd_call(q, k, v, out, out_grad, q_grad, k_grad, v_grad, l, m, workspace, B, N, d, causal, variant, dtype, stages,
                          stream), H, layout);
  c.scale = softmax_scale;
  c.opts = opts;
  c.nopts = nopts;
  c.guard = (const float*)guard;
  return validate_and_dispatch(c);
}

int fa_mi355x_fwd_gqa(const void* q, const void* k, const void* v, float* out, float* l, float* m, int B, int H, int Hkv, int N, int d,
                      int layout, float softmax_scale, int causal, int variant, int dtype, const int* opts, int nopts, void* guard,
                      int produce_guard, void* stream) {
  Call c = grouped(fwd_call(q, k, v, out, l, m, B, N, d, causal, variant, dtype, stream), H, Hkv, layout);
  c.scale = softmax_scale;
  c.opts = opts;
  c.nopts = nopts;
  c.guard = (const float*)guard;
  c.produce = produce_guard ? 1 : 0;
  return validate_and_dispatch(c);
}

int fa_mi355x_bwd_gqa(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad,
                      float* k_grad, float* v_grad, const float* l, const float* m, void* workspace, int B, int H, int Hkv, int N,
                      int d, int layout, float softmax_scale, int causal, int variant, int dtype, int stages, const int* opts,
                      int nopts, const void* guard, void* stream) {
  Call c = grouped(bwd_call(q, k, v, out, out_grad, q_grad, k_grad, v_grad, l, m, workspace, B, N, d, causal, variant, dtype, stages,
                            stream), H, Hkv, layout);
  c.scale = softmax_scale;
  c.opts = opts;
  c.nopts = nopts;
  c.guard = (const float*)guard;
  return validate_and_dispatch(c);
}

size_t fa_mi355x_bwd_workspace_bytes_gqa(int B, int H, int Hkv, int N, int d) {
  if (B <= 0 || H <= 0 || Hkv <= 0 || H % Hkv != 0 || N <= 0 || d <= 0) return 0;
  const size_t vecs = fa_mi355x_bwd_workspace_bytes(B * H, N, d);
  if (Hkv == H) return vecs;
  return align256(vecs) + (size_t)2 * B * H * N * d * sizeof(float);   // + the per-query-head dK and dV of the group sum
}

size_t fa_mi355x_bwd_workspace_bytes(int batch, int N, int /*d*/) {
  if (batch <= 0 || N <= 0) return 0;
  return (size_t)WS_VECS * batch * N * sizeof(float);
}

size_t fa_mi355x_bwd_workspace_bytes_ex(int batch, int N, int d, const int* /*opts*/, int /*nopts*/) {
  return fa_mi355x_bwd_workspace_bytes(batch, N, d);
}

int fa_mi355x_bwd_status(const void* workspace, int batch, int N, int /*d*/, int* status) {
  g_err[0] = 0;
  if (!workspace || !status || batch <= 0 || N <= 0) return set_err(FA_ERR_BAD_ARG, "bad argument");
  *status = 0;
  return FA_OK;
}

int fa_mi355x_bwd(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad,
                  float* k_grad, float* v_grad, const float* l, const float* m, void* workspace, int batch, int N,
                  int d, int causal, int variant, int dtype, void* stream) {
  return fa_mi355x_bwd_stages(q, k, v, out, out_grad, q_grad, k_grad, v_grad, l, m, workspace, batch, N, d, causal,
                              variant, dtype, FA_BWD_STAGE_ALL, stream);
}


int fa_mi355x_bwd_stages(const void* q, const void* k, const void* v, const float* out, const void* out_grad,
                         float* q_grad, float* k_grad, float* v_grad, const float* l, const float* m, void* workspace,
                         int batch, int N, int d, int causal, int variant, int dtype, int stages, void* stream) {
  return validate_and_dispatch(bwd_call(q, k, v, out, out_grad, q_grad, k_grad, v_grad, l, m, workspace, batch, N, d, causal,
                                        variant, dtype, stages, stream));
}


void fa_mi355x_launch_fw_host(int variant, float* q, float* k, float* v, float* out, float* l, float* m, int batch,
                              int N, int d, bool causal_mask, void* stream) {
  if (!q || !k || !v || !out || !l || !m) die("null pointer argument", hipSuccess);
  if (batch <= 0 || N <= 0 || d <= 0) die("batch, N and d must be positive", hipSuccess);
  // The reference kernels assert d <= 128 (FA-1, src/flash_attn_fw.cu:43) / d <= 126 (FA-2, src/flash_attn2_fw.cu:43).
  if (d > 128) die("head dimension d > 128 is not supported", hipSuccess);
  hipStream_t st = (hipStream_t)stream;
  const int dp = d_padded(d);
  const size_t rows = (size_t)batch * N;
  const size_t tb = align256(rows * dp * sizeof(float)), rb = align256(rows * sizeof(float));
  std::lock_guard<std::mutex> lock(g_pool_mu);
  FA_HOST_TRY(pool_reserve(4 * tb + 2 * rb));
  g_pipe.init();
  char* p = (char*)g_pool;
  float* dq_ = (float*)p;
  float* dk_ = (float*)(p + tb);
  float* dv_ = (float*)(p + 2 * tb);
  float* do_ = (float*)(p + 3 * tb);
  float* dl_ = (float*)(p + 4 * tb);
  float* dm_ = (float*)(p + 4 * tb + rb);
  const size_t tbytes = rows * d * sizeof(float), rbytes = rows * sizeof(float);
  HostTimer tm("fw");
  (void)hipGetLastError();   // (a sticky error of an earlier HIP user is not this call's)
  PinSet pins;
  pins.add(q, tbytes); pins.add(k, tbytes); pins.add(v, tbytes); pins.add(out, tbytes); pins.add(l, rbytes); pins.add(m, rbytes);
  pins.lock();
  tm.pinned();
  const int nch = host_chunks(batch, (size_t)N * d * sizeof(float));
  const int cb = (batch + nch - 1) / nch;
  FA_HOST_TRY(hipStreamSynchronize(st));   // the arena may still be in use by work the caller queued on this stream
  for (int c = 0, b0 = 0; b0 < batch; ++c, b0 += cb) {
    const int nb = std::min(cb, batch - b0);
    const size_t r0 = (size_t)b0 * N, nr = (size_t)nb * N;
    h2d_rows(dq_ + r0 * dp, q + r0 * d, nr, d, dp, g_pipe.up);
    h2d_rows(dk_ + r0 * dp, k + r0 * d, nr, d, dp, g_pipe.up);
    h2d_rows(dv_ + r0 * dp, v + r0 * d, nr, d, dp, g_pipe.up);
    FA_HOST_TRY(hipEventRecord(g_pipe.event(2 * c), g_pipe.up));
    FA_HOST_TRY(hipStreamWaitEvent(st, g_pipe.event(2 * c), 0));
    Call call = host_call(nb, N, d, dp, causal_mask, variant, st);
    call.q = dq_ + r0 * dp; call.k = dk_ + r0 * dp; call.v = dv_ + r0 * dp; call.out = do_ + r0 * dp; call.l = dl_ + r0; call.m = dm_ + r0;
    if (fwd_dispatch(call)) die(g_err, hipSuccess);
    FA_HOST_TRY(hipEventRecord(g_pipe.event(2 * c + 1), st));
    FA_HOST_TRY(hipStreamWaitEvent(g_pipe.down, g_pipe.event(2 * c + 1), 0));
    d2h_rows(out + r0 * d, do_ + r0 * dp, nr, d, dp, g_pipe.down);
    FA_HOST_TRY(hipMemcpyAsync(l + r0, dl_ + r0, nr * sizeof(float), hipMemcpyDeviceToHost, g_pipe.down));
    // FA-2 never writes m (src/flash_attn2_fw.cu:279-294): the caller's m comes back unchanged.
    if (variant == FA_VARIANT_FA1)
      FA_HOST_TRY(hipMemcpyAsync(m + r0, dm_ + r0, nr * sizeof(float), hipMemcpyDeviceToHost, g_pipe.down));
  }
  FA_HOST_TRY(hipStreamSynchronize(g_pipe.down));
  FA_HOST_TRY(hipStreamSynchronize(st));
  FA_HOST_TRY(hipGetLastError());
  tm.piped();
}

void fa_mi355x_launch_bw_host(int variant, float* q, float* k, float* v, float* out, float* out_grad, float* q_grad,
                              float* k_grad, float* v_grad, float* l, float* m, int batch, int N, int d,
                              bool causal_mask, void* stream) {
  if (!q || !k || !v || !out || !out_grad || !q_grad || !k_grad || !v_grad || !l || !m)
    die("null pointer argument", hipSuccess);
  if (batch <= 0 || N <= 0 || d <= 0) die("batch, N and d must be positive", hipSuccess);
  if (d > 128) die("head dimension d > 128 is not supported", hipSuccess);
  hipStream_t st = (hipStream_t)stream;
  const int dp = d_padded(d);
  const size_t rows = (size_t)batch * N;
  const size_t tb = align256(rows * dp * sizeof(float)), rb = align256(rows * sizeof(float));
  std::lock_guard<std::mutex> lock(g_pool_mu);
  FA_HOST_TRY(pool_reserve(8 * tb + (2 + WS_VECS) * rb + 256));
  g_pipe.init();
  char* p = (char*)g_pool;
  float* bq = (float*)p;
  float* bk = (float*)(p + tb);
  float* bv = (float*)(p + 2 * tb);
  float* bo = (float*)(p + 3 * tb);
  float* bdo = (float*)(p + 4 * tb);
  float* bdq = (float*)(p + 5 * tb);
  float* bdk = (float*)(p + 6 * tb);
  float* bdv = (float*)(p + 7 * tb);
  float* bl = (float*)(p + 8 * tb);
  float* bm = (float*)(p + 8 * tb + rb);
  float* ws = (float*)(p + 8 * tb + 2 * rb);   // WS_VECS * rows floats: the row constants of every chunk at its own rows
  const size_t tbytes = rows * d * sizeof(float), rbytes = rows * sizeof(float);
  HostTimer tm("bw");
  (void)hipGetLastError();
  PinSet pins;
  for (const float* t : {(const float*)q, (const float*)k, (const float*)v, (const float*)out, (const float*)out_grad,
                         (const float*)q_grad, (const float*)k_grad, (const float*)v_grad})
    pins.add(t, tbytes);
  pins.add(l, rbytes); pins.add(m, rbytes);
  pins.lock();
  tm.pinned();
  const int nch = host_chunks(batch, (size_t)N * d * sizeof(float));
  const int cb = (batch + nch - 1) / nch;
  FA_HOST_TRY(hipStreamSynchronize(st));
  for (int c = 0, b0 = 0; b0 < batch; ++c, b0 += cb) {
    const int nb = std::min(cb, batch - b0);
    const size_t r0 = (size_t)b0 * N, nr = (size_t)nb * N;
    h2d_rows(bq + r0 * dp, q + r0 * d, nr, d, dp, g_pipe.up);
    h2d_rows(bk + r0 * dp, k + r0 * d, nr, d, dp, g_pipe.up);
    h2d_rows(bv + r0 * dp, v + r0 * d, nr, d, dp, g_pipe.up);
    h2d_rows(bo + r0 * dp, out + r0 * d, nr, d, dp, g_pipe.up);
    h2d_rows(bdo + r0 * dp, out_grad + r0 * d, nr, d, dp, g_pipe.up);
    FA_HOST_TRY(hipMemcpyAsync(bl + r0, l + r0, nr * sizeof(float), hipMemcpyHostToDevice, g_pipe.up));
    FA_HOST_TRY(hipMemcpyAsync(bm + r0, m + r0, nr * sizeof(float), hipMemcpyHostToDevice, g_pipe.up));
    FA_HOST_TRY(hipEventRecord(g_pipe.event(2 * c), g_pipe.up));
    FA_HOST_TRY(hipStreamWaitEvent(st, g_pipe.event(2 * c), 0));
    // the chunk's row-constant vectors sit at ws + WS_VECS * r0 (the kernels take ws, ws + rows, ws + 2 * rows of THEIR launch)
    Call call = host_call(nb, N, d, dp, causal_mask, variant, st);
    call.q = bq + r0 * dp; call.k = bk + r0 * dp; call.v = bv + r0 * dp; call.out = bo + r0 * dp; call.dout = bdo + r0 * dp;
    call.dq = bdq + r0 * dp; call.dk = bdk + r0 * dp; call.dv = bdv + r0 * dp; call.l = bl + r0; call.m = bm + r0; call.ws = ws + WS_VECS * r0;
    call.stages = FA_BWD_STAGE_ALL;
    if (bwd_dispatch(call)) die(g_err, hipSuccess);
    FA_HOST_TRY(hipEventRecord(g_pipe.event(2 * c + 1), st));
    FA_HOST_TRY(hipStreamWaitEvent(g_pipe.down, g_pipe.event(2 * c + 1), 0));
    d2h_rows(q_grad + r0 * d, bdq + r0 * dp, nr, d, dp, g_pipe.down);
    d2h_rows(k_grad + r0 * d, bdk + r0 * dp, nr, d, dp, g_pipe.down);
    d2h_rows(v_grad + r0 * d, bdv + r0 * dp, nr, d, dp, g_pipe.down);
  }
  FA_HOST_TRY(hipStreamSynchronize(g_pipe.down));
  FA_HOST_TRY(hipStreamSynchronize(st));
  FA_HOST_TRY(hipGetLastError());
  tm.piped();
}

int fa_mi355x_probe(const void* tile, const void* b, float* row_out, float* tr_out, float* mma_out, float* swap_out,
                    int d, int dtype, void* stream) {
  g_err[0] = 0;
  if (!tile || !b || !row_out || !tr_out || !mma_out || !swap_out) return set_err(FA_ERR_BAD_ARG, "null pointer");
  if (!d_supported(d)) return set_err(FA_ERR_UNSUPPORTED_D, "probe supports d in {32, 64, 128}");
  hipStream_t st = (hipStream_t)stream;
#define FA_PROBE(T, DD)                                                                                      \
  hipLaunchKernelGGL((fa::probe_kernel<T, DD>), dim3(1), dim3(256), 0, st, (const T*)tile, (const T*)b, row_out, \
                     tr_out, mma_out, swap_out)
  if (dtype == FA_DTYPE_BF16) {
    if (d == 32) FA_PROBE(fa::bf16_t, 32); else if (d == 64) FA_PROBE(fa::bf16_t, 64); else FA_PROBE(fa::bf16_t, 128);
  } else if (dtype == FA_DTYPE_F32) {
    if (d == 32) FA_PROBE(float, 32); else if (d == 64) FA_PROBE(float, 64); else FA_PROBE(float, 128);
  } else {
    return set_err(FA_ERR_BAD_ARG, "unknown dtype");
  }
#undef FA_PROBE
  FA_HIP_TRY(hipGetLastError());
  return FA_OK;
}

}  // extern "C"
