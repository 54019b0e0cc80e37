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

bool plan_mode();   // a fa_mi355x_plan() call is recording on this thread (see FA_LAUNCH)

int set_err(int code, const char* what, hipError_t e = hipSuccess) {
  if (e != hipSuccess)
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  else
    snprintf(g_err, sizeof(g_err), "%s", what);
  return code;
}

#define FA_HIP_TRY(expr)                                             \
  do {                                                               \
    if (!plan_mode()) {   /* fa_mi355x_plan: no HIP call at all */   \
      hipError_t e_ = (expr);                                        \
      if (e_ != hipSuccess) return set_err(FA_ERR_HIP, #expr, e_);   \
    }                                                                \
  } while (0)

// Every kernel launch of the dispatch code below goes through FA_LAUNCH.  fa_mi355x_plan() runs the SAME dispatch functions with a
// recorder installed: the launch is then skipped and the kernel's name appended to the plan, so what bench.py labels and what the
// library launches cannot drift apart (one source of truth for the kernel selection).
thread_local std::vector<std::string>* t_plan = nullptr;
// A second dry-run mode, for run_scaled below: the dispatch code runs with every launch and HIP call skipped and nothing recorded but
// t_fold: did the selection reach a kernel that carries tau*log2(e) in a bf16 operand (FA_LAUNCH_FOLD sites)?
thread_local bool t_probe = false, t_fold = false, t_fold_produces = false;   // (..._produces: the folding launch can fill the guard itself)
bool plan_mode() { return t_plan != nullptr || t_probe; }
void plan_add(const char* expr) {   // "(fa::fwd_slot_kernel<T, 64, false>)" -> "fwd_slot_kernel"
  const char* b = expr;
  while (*b == '(' || *b == ' ') ++b;
  if (strncmp(b, "fa::", 4) == 0) b += 4;
  const char* e = b;
  while (*e && *e != '<' && *e != ')' && *e != ' ') ++e;
  t_plan->emplace_back(b, e);
}
#define FA_LAUNCH(kern, grid, block, shmem, st, ...)                        \
  do {                                                                      \
    if (t_probe) break;                                                     \
    if (t_plan) plan_add(#kern);                                            \
    else hipLaunchKernelGGL(kern, grid, block, shmem, st, __VA_ARGS__);     \
  } while (0)
// ... of a kernel whose lane-stationary bf16 operand carries tau*log2(e) (the MFMA-slot builds without masked periods)
#define FA_LAUNCH_FOLD(kern, grid, block, shmem, st, ...)                   \
  do {                                                                      \
    t_fold = true;                                                          \
    FA_LAUNCH(kern, grid, block, shmem, st, __VA_ARGS__);                   \
  } while (0)
// ... and can fill the call's scale guard inside its own launch (the non-causal builds of the slot forward: guard_produce)
#define FA_LAUNCH_FOLD_P(kern, grid, block, shmem, st, ...)                 \
  do {                                                                      \
    t_fold_produces = true;                                                 \
    FA_LAUNCH_FOLD(kern, grid, block, shmem, st, __VA_ARGS__);              \
  } while (0)

// fwd_kernel workgroups per CU up to which the fp32 split-key forward takes the launch (measured, profiles/r04_fwd_splitk_f32.txt: 64 / 128
// workgroups 0.076 -> 0.027 / 0.044 ms, 256 level, 512 slower; causal: 256 workgroups 0.160 -> 0.111, 512 slower)
constexpr double FWD_SPLITK_MAX_WGS_PER_CU = 0.5, FWD_SPLITK_MAX_WGS_PER_CU_CAUSAL = 1.0;

inline bool d_supported(int d) { return d == 32 || d == 64 || d == 128; }
inline int d_padded(int d) { return d <= 32 ? 32 : (d <= 64 ? 64 : 128); }

// Per-call kernel selection (fa_mi355x_fwd_ex / fa_mi355x_bwd_ex; every other entry point runs the defaults): [0] dK/dV geometry,
// [1] forward kernel, [2] dQ kernel, [3] reserved, [4] preprocess / fp32 one-pass backward, [5] 1 = one head per workgroup in the
// tiled slot builds, [6] reserved, [7] causal block order.  Only values whose kernels give correct results are accepted (parse_opts).
// [8] where tau*log2(e) is applied (see run_scaled): 0 = by the call's scale guard when it has one, else fp32 scaling; 1 = the caller
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
  static const int allowed[NTUN][7] = {{0, 3, 4, 5, -1}, {0, 2, 3, 4, -1}, {0, 2, 3, -1}, {0, -1}, {0, 1, 4, 5, -1}, {0, 1, -1}, {0, -1}, {0, 1, 2, -1},
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
int head_tiles(const Call& c, int nb) {
  int tiles = 1;
  if (c.N % 256 == 0 && c.tun.v[5] == 0) {
    const int cus = device_cus();
    for (int t = 2; t <= 16; ++t)
      if (c.batch % t == 0 && (c.batch / t) % 8 == 0 && (long)(c.batch / t) * nb >= cus) tiles = t;
  }
  return tiles;
}

// Phased forward.  bf16 rows with fewer than 64 admissible keys need the split-operand build (CARE): whole launches under a key
// mask, dropout or N < 64; behind a causal launch, query block 0 alone is redone by it (one small workgroup per batch*head).
template <typename T, int D, int BN>
int fwd_launch_cfg(const Call& c, int only_qb = -1, int care_main = 0, int ranked = 0) {
  constexpr bool BF = sizeof(T) == 2;
  const int batch = c.batch, N = c.N, causal = c.causal;
  const int nqb = (N + 127) / 128;
  fa::Layout lay = c.lay;
  // causal: query blocks p and nqb-1-p share a workgroup, or (ranked) one block per workgroup, longest first across a chunk of heads
  lay.rank_chunk = (ranked && causal && only_qb < 0) ? rank_chunk(2, nqb) : 0;
  // the fp32-scaling twin of a guarded non-causal call: four query blocks per workgroup while the launch still covers the chip twice
  // (its workgroups almost always return at their guard check: 4.7 -> about 1.5 us at the metric shape)
  lay.twin_blocks = 1;
  if (lay.guard && lay.guard_want == 1 && !causal && only_qb < 0)
    for (int t = 4; t > 1; t >>= 1)
      if (nqb % t == 0 && (long)batch * (nqb / t) >= 2L * device_cus()) { lay.twin_blocks = t; break; }
  const int nblk = only_qb >= 0 ? 1 : ((causal && !lay.rank_chunk) ? (nqb + 1) / 2 : nqb / lay.twin_blocks);
  fa::Layout lay1 = lay;   // (the follow-up launch of one block per head below is not ranked)
  lay1.rank_chunk = 0;
#define FA_FWD_LAUNCH(FEAT, CARE, BLOCKS, ONLY)                                                                          \
  FA_LAUNCH((fa::fwd_kernel<T, D, BN, 1, FEAT, CARE>), dim3(batch * (BLOCKS)), dim3(256), 0, c.st, (const T*)c.q,    \
            (const T*)c.k, (const T*)c.v, c.out, c.l, c.m, N, nqb, batch, lay, causal, c.variant, c.tau, ONLY)
  if (lay.drop_thr) {   // dropout on P (and the key mask, staged as zeros when absent)
    FA_FWD_LAUNCH(2, BF, nblk, only_qb);
  } else if (lay.kmask) {   // additive key mask: staged per tile, enters S^T as the accumulator input
    FA_FWD_LAUNCH(1, BF, nblk, only_qb);
  } else if (BF && (N < 64 || only_qb >= 0 || (causal && care_main))) {   // care_main (d = 64): ONE launch of the split-operand build,
    // measured 1 % faster than the main build + the block-0 follow-up launch (7.8 us); the dQ kernel is the other way round (+7 %)
    FA_FWD_LAUNCH(0, BF, nblk, only_qb);
  } else {
    FA_FWD_LAUNCH(0, false, nblk, only_qb);
    if (BF && causal) {   // rows 0..63 see fewer than 64 keys: query block 0 again, split operands
      FA_LAUNCH((fa::fwd_kernel<T, D, BN, 1, 0, BF>), dim3(batch), dim3(256), 0, c.st, (const T*)c.q, (const T*)c.k, (const T*)c.v,
                c.out, c.l, c.m, N, nqb, batch, lay1, causal, c.variant, c.tau, 0);
    }
  }
#undef FA_FWD_LAUNCH
  FA_HIP_TRY(hipGetLastError());
  return FA_OK;
}

template <typename T, int D>
int fwd_launch(const Call& c) {
  const int batch = c.batch, N = c.N, causal = c.causal;
  const Tun& tun = c.tun;
  if constexpr (sizeof(T) == 4 && D == 64) {
    // fp32, d = 64, launches that leave most of the chip idle under fwd_kernel's geometry (a wave = 32 queries x all keys, 128-query
    // workgroups, two per CU): the split-key forward (fa_fwd_splitk_f32.h: a workgroup = one 32-query block, its four waves a quarter
    // of the keys each).  Option 1: 4 = always, 2 = never.
    const long wgs = (long)batch * ((N + 127) / 128), cus = device_cus();
    if (!c.lay.kmask && !c.lay.drop_thr && !c.lay.out_bf16 && N >= 128 && (tun.v[1] == 4 ||
         (tun.v[1] == 0 && wgs <= (causal ? FWD_SPLITK_MAX_WGS_PER_CU_CAUSAL : FWD_SPLITK_MAX_WGS_PER_CU) * cus))) {
      const int nqb = (N + 31) / 32;
      FA_LAUNCH((fa::fwd_splitk_f32_kernel<D>), dim3((unsigned)(batch * nqb)), dim3(256), 0, c.st, (const float*)c.q, (const float*)c.k,
                (const float*)c.v, c.out, c.l, c.m, N, nqb, batch, c.lay, causal, c.variant, c.tau);
      FA_HIP_TRY(hipGetLastError());
      return FA_OK;
    }
  }
  if constexpr (sizeof(T) == 2 && (D == 64 || D == 128)) {
    // FA-2 side output, bf16, d = 64 / 128, non-causal: slot-interleaved three-deep pipeline.  Under the causal mask the slot build
    // WITH masked period variants is 3.6 % slower than the phased kernel (128-query workgroups, per-wave tile skipping), which keeps
    // the causal launches the build below does not take; tuning key 1: 2 = always phased, 3 = always slot.
    // (N < 64: every row has few keys and takes the phased kernel's split-operand path)
    // Causal, d = 64, N a multiple of 256: the causal slot build (unmasked sweep + the diagonal block per wave, query blocks p and
    // nqb-1-p paired): 0.155 vs 0.192 ms for the phased kernel at the metric shape; it needs about one 8-wave workgroup per CU to pay.
    const int nqb = (N + 255) / 256;
    const bool cslot = causal && N % 256 == 0 && (tun.v[1] == 3 || (tun.v[1] == 0 && batch * nqb >= 256));
    if (c.variant == FA_VARIANT_FA2 && tun.v[1] != 2 && (!causal || tun.v[1] == 3 || cslot) && !c.lay.kmask && !c.lay.drop_thr &&
        N >= 64) {
      const bool whole = !causal && N % (8192 / D) == 0;   // no sub-tile needs a mask
      if (cslot) {   // (d = 64: four waves per SIMD, two workgroups per CU; d = 128: two waves per SIMD, one workgroup)
        const bool ranked = causal_ranked(tun, batch * nqb, D == 64 ? 2 : 1);
        fa::Layout lay = c.lay;
        lay.rank_chunk = rank_chunk(D == 64 ? 2 : 1, nqb);
        FA_LAUNCH_FOLD((fa::fwd_slot_kernel<T, D, false, 64, (D == 64 ? 4 : 2), true>),
                       dim3(ranked ? batch * nqb : batch * ((nqb + 1) / 2)), dim3(512), 0, c.st, (const T*)c.q, (const T*)c.k,
                       (const T*)c.v, c.out, c.l, N, nqb, batch, lay, ranked ? 2 : 1, c.tau);
        FA_HIP_TRY(hipGetLastError());
        return FA_OK;
      }
      if (whole && D == 64) {   // d = 64 default: 64-key stages (64 KiB of rings), two workgroups per CU = four waves per SIMD at
        // 122 VGPRs: 0.268 vs 0.282 ms for the 128-key-stage build at two waves per SIMD
        FA_LAUNCH_FOLD_P((fa::fwd_slot_kernel<T, 64, false, 64, 4>), dim3(batch * nqb), dim3(512), 0, c.st, (const T*)c.q,
                         (const T*)c.k, (const T*)c.v, c.out, c.l, N, nqb, batch, c.lay, causal, c.tau);
        FA_HIP_TRY(hipGetLastError());
        return FA_OK;
      }
      if constexpr (D == 128) {
        if (whole) {
          FA_LAUNCH_FOLD_P((fa::fwd_slot_kernel<T, D, false>), dim3(batch * nqb), dim3(512), 0, c.st, (const T*)c.q,
                           (const T*)c.k, (const T*)c.v, c.out, c.l, N, nqb, batch, c.lay, causal, c.tau);
          FA_HIP_TRY(hipGetLastError());
          return FA_OK;
        }
      }
      if constexpr (D == 64) {   // ragged N / forced causal: the variant with masked periods (d = 128 takes the phased kernel)
        FA_LAUNCH((fa::fwd_slot_kernel<T, D, true>), dim3(batch * nqb), dim3(512), 0, c.st, (const T*)c.q,
                  (const T*)c.k, (const T*)c.v, c.out, c.l, N, nqb, batch, c.lay, causal, c.tau);
        FA_HIP_TRY(hipGetLastError());
        // under the causal mask rows 0..63 see fewer than 64 keys: the slot kernel has no split-operand path, so the phased
        // kernel redoes query block 0 (one small workgroup per batch*head) behind it
        if (causal) return fwd_launch_cfg<T, D, 64>(c, 0);
        return FA_OK;
      }
    }
  }
  return fwd_launch_cfg<T, D, (sizeof(T) == 2 ? 64 : 32)>(c, -1, D == 64 ? 1 : 0,
                                                          tun.v[7] == 2 || (tun.v[7] == 0 && sizeof(T) == 2 && D == 32));   // (d = 32: ranked measured 10 % faster)
}

// bf16 launches whose rows may see fewer than 64 admissible keys everywhere (key mask, dropout, N < 64) run the split-operand
// build (CARE) in a 4-wave geometry that has the registers for it.  A causal launch runs the requested geometry with the
// sub-slices of queries 0..63 SKIPPED (thin_mode 1) and then one CARE workgroup per batch*head that handles exactly those and
// adds its dK, dV (thin_mode 2): the main kernel keeps its registers and its speed.
// DROP_ONLY: the instantiation serves dropout calls alone (fp32 d = 64: the plain launches have a build of their own), so the plain
// kernels of this geometry are not compiled into the library.
template <typename T, int D, int KPW, int NW, int QS, int MODE = 0, bool DROP_ONLY = false>
int dkdv_launch(const Call& c, int care_main = 0, int rank_causal = 1) {
  constexpr bool BF = sizeof(T) == 2;
  const int batch = c.batch, N = c.N, causal = c.causal;
  const int nkb = (N + NW * KPW - 1) / (NW * KPW);
  const int nkb4 = (N + 127) / 128;
  fa::Layout lay = c.lay;
#define FA_CARE_LAUNCH(HD, GRID, THIN)                                                                                        \
  FA_LAUNCH((fa::bwd_dkdv_kernel<T, D, 32, 4, 64, 1, HD, 1, BF>), dim3(GRID), dim3(256), 0, c.st, (const T*)c.q, (const T*)c.k, \
            (const T*)c.v, (const T*)c.dout, c.nlc(), c.delta(), c.dk, c.dv, N, nkb4, batch, lay, causal, c.tau, THIN)
  if (lay.drop_thr) {   // dropout: the plain per-sub-slice path regenerates the mask from (bh, query, key)
    // (these whole-launch builds take one key block per workgroup: under the causal mask longest first across a chunk of heads)
    if constexpr (BF) {
      if (causal && rank_causal) lay.rank_chunk = rank_chunk(2, nkb4);
      FA_CARE_LAUNCH(true, batch * nkb4, 0);
    } else {
      if (causal && rank_causal) lay.rank_chunk = rank_chunk(2, nkb);
      FA_LAUNCH((fa::bwd_dkdv_kernel<T, D, KPW, NW, QS, 1, true>), dim3(batch * nkb), dim3(NW * 64), 0, c.st,
                (const T*)c.q, (const T*)c.k, (const T*)c.v, (const T*)c.dout, c.nlc(), c.delta(), c.dk, c.dv, N, nkb, batch, lay,
                causal, c.tau, 0);
    }
    FA_HIP_TRY(hipGetLastError());
    return FA_OK;
  }
  if constexpr (BF) {
    if (lay.kmask || N < 64) {
      if (causal && rank_causal) lay.rank_chunk = rank_chunk(2, nkb4);
      FA_CARE_LAUNCH(false, batch * nkb4, 0);
      FA_HIP_TRY(hipGetLastError());
      return FA_OK;
    }
  }
  if constexpr (BF && MODE == 3) {
    if (causal && care_main) {   // d = 64 default: the split-operand path inside the main (paired) kernel: 2 % faster than main + corner launch
      FA_LAUNCH((fa::bwd_dkdv_kernel<T, D, KPW, NW, QS, MODE, false, 1, true, true>), dim3(batch * ((nkb + 1) / 2)),
                dim3(NW * 64), 0, c.st, (const T*)c.q, (const T*)c.k, (const T*)c.v, (const T*)c.dout, c.nlc(), c.delta(), c.dk, c.dv,
                N, nkb, batch, lay, causal, c.tau, 0);
      FA_HIP_TRY(hipGetLastError());
      return FA_OK;
    }
  }
  if constexpr (DROP_ONLY) {
    return set_err(FA_ERR_BAD_ARG, "internal: dropout-only dK/dV launch without dropout");
  } else {
  const int thin = (BF && causal) ? 1 : 0;
  // causal: key blocks p and nkb-1-p share a workgroup (uniform work, no tail: -13 % at the metric shape).  Not for the 8-wave
  // d = 128 geometry, whose register allocation has no room for the pass loop (it would spill).
  constexpr bool CAN_PAIR = !(BF && D == 128 && NW == 8);
  // (MODE 3 always runs its paired build: hipcc's allocation of the unpaired MODE 3 instance spills, the paired one does not)
  if ((causal || MODE == 3) && CAN_PAIR) {
    if constexpr (CAN_PAIR)
      FA_LAUNCH((fa::bwd_dkdv_kernel<T, D, KPW, NW, QS, MODE, false, 1, false, true>), dim3(batch * ((nkb + 1) / 2)),
                dim3(NW * 64), 0, c.st, (const T*)c.q, (const T*)c.k, (const T*)c.v, (const T*)c.dout, c.nlc(), c.delta(), c.dk, c.dv,
                N, nkb, batch, lay, causal, c.tau, thin);
  } else {
    // unpaired causal launch (the 8-wave d = 128 geometry): longest block first across a chunk of heads instead of head by head:
    // 2.05 vs 2.21 ms at configs[3]'s shape, 0.157 vs 0.207 at B = 8, N = 2048 (option 7 = 1: head by head)
    if (causal && rank_causal) lay.rank_chunk = rank_chunk(NW == 8 ? 1 : 2, nkb);
    if constexpr (MODE != 3 || !CAN_PAIR)
      FA_LAUNCH((fa::bwd_dkdv_kernel<T, D, KPW, NW, QS, MODE>), dim3(batch * nkb), dim3(NW * 64), 0, c.st, (const T*)c.q,
                (const T*)c.k, (const T*)c.v, (const T*)c.dout, c.nlc(), c.delta(), c.dk, c.dv, N, nkb, batch, lay, causal, c.tau, thin);
  }
  if constexpr (BF) {
    if (thin) FA_CARE_LAUNCH(false, batch, 2);
  }
  FA_HIP_TRY(hipGetLastError());
  return FA_OK;
  }   // !DROP_ONLY
#undef FA_CARE_LAUNCH
}

template <typename T, int D, int BN>
int dq_launch(const Call& c, int only_qb = -1, int care_main = 0, const fa::DqPrep* prep = nullptr, int ranked = 0) {
  // prep != nullptr (only when dq_fuses_prep said so: the plain main build runs): the launch also preprocesses its rows
  constexpr bool BF = sizeof(T) == 2;   // CARE policy as fwd_launch_cfg's
  const int batch = c.batch, N = c.N, causal = c.causal;
  const int nqb = (N + 127) / 128;
  fa::Layout lay = c.lay;
  // causal: query blocks p and nqb-1-p share a workgroup, or (ranked) one block per workgroup, longest first across a chunk of heads
  lay.rank_chunk = (ranked && causal && only_qb < 0) ? rank_chunk(2, nqb) : 0;
  const int nblk = only_qb >= 0 ? 1 : ((causal && !lay.rank_chunk) ? (nqb + 1) / 2 : nqb);
  fa::Layout lay1 = lay;   // (the follow-up launch of one block per head below is not ranked)
  lay1.rank_chunk = 0;
#define FA_DQ_LAUNCH(FEAT, CARE, BLOCKS, ONLY)                                                                              \
  FA_LAUNCH((fa::bwd_dq_kernel<T, D, BN, FEAT, 4, CARE>), dim3(batch * (BLOCKS)), dim3(256), 0, c.st, (const T*)c.q,   \
            (const T*)c.k, (const T*)c.v, (const T*)c.dout, c.nlc(), c.delta(), c.dq, N, nqb, batch, lay, causal, c.tau, ONLY,   \
            fa::DqPrep{})
  if (lay.drop_thr) {
    FA_DQ_LAUNCH(2, BF, nblk, only_qb);
  } else if (lay.kmask) {
    FA_DQ_LAUNCH(1, BF, nblk, only_qb);
  } else if (BF && (N < 64 || only_qb >= 0 || (causal && care_main))) {
    FA_DQ_LAUNCH(0, BF, nblk, only_qb);
  } else {
    FA_LAUNCH((fa::bwd_dq_kernel<T, D, BN, 0, 4, false>), dim3(batch * nblk), dim3(256), 0, c.st, (const T*)c.q, (const T*)c.k,
              (const T*)c.v, (const T*)c.dout, c.nlc(), c.delta(), c.dq, N, nqb, batch, lay, causal, c.tau, only_qb,
              prep ? *prep : fa::DqPrep{});
    if (BF && causal)   // rows 0..63 again with split operands
      FA_LAUNCH((fa::bwd_dq_kernel<T, D, BN, 0, 4, BF>), dim3(batch), dim3(256), 0, c.st, (const T*)c.q, (const T*)c.k, (const T*)c.v,
                (const T*)c.dout, c.nlc(), c.delta(), c.dq, N, nqb, batch, lay1, causal, c.tau, 0, fa::DqPrep{});
  }
#undef FA_DQ_LAUNCH
  FA_HIP_TRY(hipGetLastError());
  return FA_OK;
}

// The MFMA-slot dQ kernel.  Its mask-free builds carry both scalings and pick one per launch (Layout::scale_sel): no twin launch.
template <typename T, int D>
int dq_slot_launch(const Call& c, const fa::DqPrep* prep) {
  // prep != nullptr: the launch also does the preprocess for its rows and writes the workspace (see dq_fuses_prep)
  const int batch = c.batch, N = c.N, causal = c.causal;
  const fa::DqPrep pa = prep ? *prep : fa::DqPrep{};
  const int nqb = (N + 255) / 256;
  fa::Layout lay = c.lay;
  lay.rank_chunk = rank_chunk(1, nqb);
  const bool paired = !causal_ranked(c.tun, batch * nqb, 1);
  if (causal && N % 256 == 0) {   // causal build: unmasked sweep + the diagonal block per wave; one block per workgroup,
    // longest first across all heads (paired: blocks p and nqb-1-p in one workgroup)
    const dim3 grid(paired ? batch * ((nqb + 1) / 2) : batch * nqb);
    FA_LAUNCH((fa::bwd_dq_slot_kernel<T, D, false, true>), grid, dim3(512), 0, c.st, (const T*)c.q, (const T*)c.k,
              (const T*)c.v, (const T*)c.dout, c.nlc(), c.delta(), c.dq, N, nqb, batch, lay, paired ? 1 : 2, c.tau, pa);
  } else if (!causal && N % 128 == 0) {   // no sub-tile needs a mask: the build without masked period variants
    // (query block qb of several consecutive heads per workgroup: head_tiles, the rule of the tiled dK/dV launch)
    if (const int tiles = head_tiles(c, nqb); tiles > 1) {
      lay.tiles = tiles;
      FA_LAUNCH((fa::bwd_dq_slot_kernel<T, D, false, false, true>), dim3((batch / tiles) * nqb), dim3(512), 0, c.st, (const T*)c.q,
                (const T*)c.k, (const T*)c.v, (const T*)c.dout, c.nlc(), c.delta(), c.dq, N, nqb, batch, lay, causal, c.tau, pa);
    } else {
      FA_LAUNCH((fa::bwd_dq_slot_kernel<T, D, false>), dim3(batch * nqb), dim3(512), 0, c.st, (const T*)c.q, (const T*)c.k,
                (const T*)c.v, (const T*)c.dout, c.nlc(), c.delta(), c.dq, N, nqb, batch, lay, causal, c.tau, pa);
    }
  } else {
    FA_LAUNCH((fa::bwd_dq_slot_kernel<T, D>), dim3(batch * nqb), dim3(512), 0, c.st, (const T*)c.q, (const T*)c.k,
              (const T*)c.v, (const T*)c.dout, c.nlc(), c.delta(), c.dq, N, nqb, batch, lay, causal, c.tau, fa::DqPrep{});
  }
  FA_HIP_TRY(hipGetLastError());
  return FA_OK;
}

// Does a backward call that asks for the preprocess AND dQ fold the preprocess into its dQ launch (dQ is then launched BEFORE dK/dV,
// which reads the workspace the dQ launch wrote)?  Yes whenever dq_stage sends the call to a plain main build: not under a key mask
// or dropout, not bf16 with N < 64 (split-operand builds), not the bf16 d = 64 slot build with masked periods (no registers); option
// 4 = 1 keeps the separate preprocess kernel (A/B).
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

template <typename T, int D>
bool dq_fuses_prep(const Call& c) {
  constexpr bool BF = sizeof(T) == 2;
  if (onepass_f32<T, D>(c)) return false;
  const int need = FA_BWD_STAGE_PREP | FA_BWD_STAGE_DQ;
  if ((c.stages & need) != need || c.tun.v[4] != 0 || c.lay.kmask || c.lay.drop_thr || (BF && c.N < 64)) return false;
  if constexpr (BF && D == 64) {
    if (!dq64_phased(c)) return c.causal ? c.N % 256 == 0 : c.N % 128 == 0;   // the slot kernel: its unmasked / causal builds only
  }
  return true;
}

// The dQ stage of a backward call: kernel selection by dtype / head dim / launch shape / options.  prep != nullptr: the launch also does
// the preprocess for its rows (dq_fuses_prep decided that a plain main build runs).
template <typename T, int D>
int dq_stage(const Call& c, const fa::DqPrep* prep) {
  // every launch the branches below do not take runs the phased kernel with 32-key tiles (bf16 d = 32: they run 3 waves/SIMD,
  // measured 2 % faster), causal query blocks ranked by default at bf16 d = 32 (option 7)
  const int ranked = c.tun.v[7] == 2 || (c.tun.v[7] == 0 && sizeof(T) == 2 && D == 32);
  const bool few_keys = c.lay.kmask || c.lay.drop_thr || c.N < 64;   // (key mask and dropout live in the phased kernel)
  if constexpr (sizeof(T) == 2 && D == 128) {
    if (!c.causal && !few_keys) {   // non-causal default: 8 waves x 32 queries, one workgroup per CU (each staged K / V tile feeds
      // twice the waves); otherwise 4 waves x 32 queries, two workgroups per CU
      const int nqb = (c.N + 255) / 256;
      FA_LAUNCH((fa::bwd_dq_kernel<T, D, 32, 0, 8>), dim3(c.batch * nqb), dim3(512), 0, c.st, (const T*)c.q, (const T*)c.k,
                (const T*)c.v, (const T*)c.dout, c.nlc(), c.delta(), c.dq, c.N, nqb, c.batch, c.lay, c.causal, c.tau, -1,
                prep ? *prep : fa::DqPrep{});
      FA_HIP_TRY(hipGetLastError());
      return FA_OK;
    }
  } else if constexpr (sizeof(T) == 2 && D == 64) {   // d = 64: slot-interleaved three-deep pipeline (default)
    if (!few_keys && !dq64_phased(c)) {
      const int rc = dq_slot_launch<T, D>(c, prep);
      // the masked slot build forced onto a causal launch: rows 0..63 (few keys) are redone by the phased kernel's split-operand
      // path (query block 0); the causal slot build (N a multiple of 256) splits them itself
      if (!rc && c.causal && c.N % 256 != 0) return dq_launch<T, D, 32>(c, 0);
      return rc;
    }
  }
  return dq_launch<T, D, 32>(c, -1, 0, prep, ranked);
}

// The dK/dV stage of a backward call: kernel selection by dtype / head dim / launch shape / options.
template <typename T, int D>
int dkdv_stage(const Call& c) {
  const int batch = c.batch, N = c.N, causal = c.causal;
  const Tun& tun = c.tun;
  if constexpr (sizeof(T) == 2 && D == 64) {
    // The continuous slot pipeline (no drain at stage boundaries, three-slot LDS-DMA ring) carries both scalings and picks one per
    // launch (Layout::scale_sel): no twin launch.  Option 0 = 4: the compiler-interleaved phased kernel below.
    fa::Layout lay = c.lay;
    if (!causal && tun.v[0] == 0 && !lay.drop_thr && !lay.kmask && N >= 64) {
      // d = 64, non-causal default: the continuous slot pipeline; rows thinned by a key mask or N < 64 go to the kernel below, whose
      // per-sub-slice path splits P and dS.  Key block kb of several consecutive heads per workgroup: head_tiles
      const int nkb = (N + 255) / 256;
      if (const int tiles = head_tiles(c, nkb); tiles > 1) {
        lay.tiles = tiles;
        FA_LAUNCH((fa::bwd_dkdv_slot_kernel<T, 64, false, true>), dim3((batch / tiles) * nkb), dim3(512), 0, c.st,
                  (const T*)c.q, (const T*)c.k, (const T*)c.v, (const T*)c.dout, c.nl2(), c.delta(), c.dk, c.dv, N, nkb, batch, lay, c.tau);
      } else {
        FA_LAUNCH((fa::bwd_dkdv_slot_kernel<T, 64>), dim3(batch * nkb), dim3(512), 0, c.st, (const T*)c.q,
                  (const T*)c.k, (const T*)c.v, (const T*)c.dout, c.nl2(), c.delta(), c.dk, c.dv, N, nkb, batch, lay, c.tau);
      }
      FA_HIP_TRY(hipGetLastError());
      return FA_OK;
    }
    if (causal && !lay.drop_thr && !lay.kmask && N % 256 == 0 &&
        (tun.v[0] == 5 || (tun.v[0] == 0 && batch * (N / 256) >= 128))) {   // (tuning key 0 = 5 forces it)
      // d = 64, causal, N a multiple of 256: the causal build of the continuous pipeline (sweep of the stages below the
      // diagonal block, the block per wave, workgroups longest first); tuning key 0 = 3: the phased kernel below
      // (key blocks p and nkb-1-p of several consecutive heads per workgroup, a causal tiled build, gave bitwise the same results
      // 4-8 % slower: profiles/r04_causal_tiled_dkdv.txt)
      const int nkb = N / 256;
      lay.rank_chunk = rank_chunk(1, nkb);
      FA_LAUNCH((fa::bwd_dkdv_slot_kernel<T, 64, true>), dim3(batch * nkb), dim3(512), 0, c.st, (const T*)c.q,
                (const T*)c.k, (const T*)c.v, (const T*)c.dout, c.nl2(), c.delta(), c.dk, c.dv, N, nkb, batch, lay, c.tau);
      FA_HIP_TRY(hipGetLastError());
      return FA_OK;
    }
    // d = 64, causal (or tuning 3): slot-interleaved fast path for unmasked stages, per-sub-slice path on the diagonal
    // (a build with the masked paths compiled out, for non-causal launches, measured the same: 0.4983 vs 0.4992 ms)
    if (tun.v[0] != 4) return dkdv_launch<T, D, 32, 8, 128, 3>(c, 1);
  }
  if constexpr (sizeof(T) == 2 && D <= 64) {
    // measured at B=8,H=8,N=4096,d=64 (ms, one device, profiles/README.md): 8 waves x 32 keys, 128-query stages,
    // software-pipelined sub-slices 0.505; not pipelined 0.514; 64-query stages 0.519; 256-query 0.525;
    // 4 waves x 32 keys (two workgroups per CU) 0.521; 4 waves x 64 keys (one wave per SIMD) 0.559
    return dkdv_launch<T, D, 32, 8, 128, 0>(c);   // compiler-interleaved software pipeline (the d = 32 default; d = 64: option 0 = 4)
  } else if constexpr (sizeof(T) == 2) {
    // d = 128 default (dropout / key mask / N < 64: dkdv_launch runs the 4-wave split-operand build, which has the registers for it): 8 waves x 32 keys, one 256-key workgroup per CU (half the Q / dO staging per MFMA): 3.64 vs 3.92 ms
    return dkdv_launch<T, D, 32, 8, 64>(c, 0, tun.v[7] != 1);
  } else if constexpr (D == 64) {
    // fp32, d = 64 (configs[1], [2]): the allocation lands on 256 VGPRs + 2 AGPRs = one wave per SIMD; asking for two
    // (launch bound) keeps it under 256
    if (c.lay.drop_thr) return dkdv_launch<T, D, 32, 4, 32, 0, true>(c);
    const int nkb = (N + 127) / 128;
    fa::Layout lay = c.lay;
    // causal: longest block first across a chunk of heads instead of head by head: 0.57 vs 0.80 ms at the reference's timing-harness
    // shape (B = 8, H = 8, N = 2048, fp32), bitwise the same (option 7 = 1: head by head)
    if (causal && tun.v[7] != 1) lay.rank_chunk = rank_chunk(2, nkb);
    FA_LAUNCH((fa::bwd_dkdv_kernel<T, D, 32, 4, 32, 0, false, 2>), dim3(batch * nkb), dim3(256), 0, c.st,
              (const T*)c.q, (const T*)c.k, (const T*)c.v, (const T*)c.dout, c.nlc(), c.delta(), c.dk, c.dv, N, nkb, batch, lay,
              causal, c.tau);
    FA_HIP_TRY(hipGetLastError());
    return FA_OK;
  } else {
    return dkdv_launch<T, D, 32, 4, 32>(c);
  }
}

template <typename T, int D>
int bwd_launch(const Call& c) {
  const long rows = (long)c.batch * c.N;
  constexpr int RPB = 256 / (D / 8);
  const bool fuse_prep = dq_fuses_prep<T, D>(c);
  if ((c.stages & FA_BWD_STAGE_PREP) && !fuse_prep) {
    FA_LAUNCH((fa::bwd_prep_kernel<T, D>), dim3((unsigned)((rows + RPB - 1) / RPB)), dim3(256), 0, c.st, c.out,
              (const T*)c.dout, c.l, c.m, c.nlc(), c.delta(), c.nl2(), rows, c.N, c.lay, c.variant, 1.0f / c.tau);
    FA_HIP_TRY(hipGetLastError());
  }
  if (fuse_prep) {   // dQ first: it preprocesses its own rows and leaves -L/tau, -delta in the workspace for the dK/dV kernel
    const fa::DqPrep pa{c.out, c.l, c.m, c.nlc(), c.delta(), c.nl2(), c.variant, 1.0f / c.tau};
    if (const int rc = dq_stage<T, D>(c, &pa)) return rc;
  }
  if constexpr (sizeof(T) == 4 && D == 64) {
    if (const int nsplit = onepass_f32<T, D>(c)) {
      // the workgroups ADD into dq (the reference's caller zeroes q_grad for its atomicAdd as well: minitorch/cuda_kernel_ops.py:609-611);
      // [B][N][H][d] or [BH][N][d]: the tensor is one contiguous range either way
      if (!t_probe && !t_plan) {
        FA_HIP_TRY(hipMemsetAsync(c.dq, 0, (size_t)rows * D * sizeof(float), c.st));
        if (nsplit > 1) {   // the parts of a key block's sweep ADD their dK, dV
          FA_HIP_TRY(hipMemsetAsync(c.dk, 0, (size_t)rows * D * sizeof(float), c.st));
          FA_HIP_TRY(hipMemsetAsync(c.dv, 0, (size_t)rows * D * sizeof(float), c.st));
        }
      }
      const int nkb = (c.N + 255) / 256;
      fa::Layout lay = c.lay;
      if (c.causal) lay.rank_chunk = rank_chunk(1, nkb);   // key block 0 (the longest sweep) of a chunk of heads first
#define FA_ONEPASS(C, R)                                                                                                             \
  FA_LAUNCH((fa::bwd_onepass_f32_kernel<D, C, R>), dim3((unsigned)(c.batch * nkb * nsplit)), dim3(512), 0, c.st, (const float*)c.q,   \
            (const float*)c.k, (const float*)c.v, (const float*)c.dout, c.nlc(), c.delta(), c.dq, c.dk, c.dv, c.N, nkb, c.batch, lay,   \
            c.tau, nsplit)
      if (c.N % 256 == 0) {
        if (c.causal) FA_ONEPASS(true, false); else FA_ONEPASS(false, false);
      } else {
        if (c.causal) FA_ONEPASS(true, true); else FA_ONEPASS(false, true);
      }
#undef FA_ONEPASS
      FA_HIP_TRY(hipGetLastError());
      return FA_OK;
    }
  }
  if (c.stages & FA_BWD_STAGE_DKDV)
    if (const int rc = dkdv_stage<T, D>(c)) return rc;
  if ((c.stages & FA_BWD_STAGE_DQ) && !fuse_prep)
    if (const int rc = dq_stage<T, D>(c, nullptr)) return rc;
  return FA_OK;
}

#define FA_DISPATCH(FN)                                                                   \
  do {                                                                                    \
    if (c.dtype == FA_DTYPE_BF16) {                                                       \
      if (c.dp == 32) return FN<fa::bf16_t, 32>(c);                                       \
      if (c.dp == 64) return FN<fa::bf16_t, 64>(c);                                       \
      return FN<fa::bf16_t, 128>(c);                                                      \
    } else {                                                                              \
      if (c.dp == 32) return FN<float, 32>(c);                                            \
      if (c.dp == 64) return FN<float, 64>(c);                                            \
      return FN<float, 128>(c);                                                           \
    }                                                                                     \
  } while (0)
int fwd_dispatch_one(const Call& c) { FA_DISPATCH(fwd_launch); }
int bwd_dispatch_one(const Call& c) { FA_DISPATCH(bwd_launch); }
#undef FA_DISPATCH

// tau uses the caller's d even when the rows are zero-padded to dp columns (zero columns of Q/K add
// nothing to the scores; zero columns of V produce zero output columns that are dropped).
fa::Layout bhnd(int N, int dp) { return fa::Layout{1, dp, (long)N * dp, 0, nullptr, 1, 0u, 1.0f, 0u, 0}; }
fa::Layout bnhd(int H, int N, int dp) { return fa::Layout{H, H * dp, (long)N * H * dp, (long)dp, nullptr, 1, 0u, 1.0f, 0u, 0}; }

int launch_scale_guard(const void* q, const void* k, long rows, int row_elems, int dtype, void* guard, hipStream_t st) {
  // only bf16 rows of 64 / 128 elements ever reach a kernel that folds the scale into an operand: everything else gets an all-zero
  // guard ("within the budget"; those calls run fp32-scaling kernels whatever it says)
  if (dtype != FA_DTYPE_BF16 || (row_elems != 64 && row_elems != 128)) {
    FA_HIP_TRY(hipMemsetAsync(guard, 0, (size_t)2 * fa::GUARD_SLOTS * sizeof(float), st));
    return FA_OK;
  }
  if (plan_mode()) {
    if (t_plan) t_plan->emplace_back("scale_guard_kernel");
    return FA_OK;
  }
  const dim3 grid(fa::GUARD_SLOTS, 2);
  if (row_elems == 64)
    hipLaunchKernelGGL((fa::scale_guard_kernel<64>), grid, dim3(256), 0, st, (const fa::bf16_t*)q, (const fa::bf16_t*)k, rows, (float*)guard);
  else
    hipLaunchKernelGGL((fa::scale_guard_kernel<128>), grid, dim3(256), 0, st, (const fa::bf16_t*)q, (const fa::bf16_t*)k, rows, (float*)guard);
  FA_HIP_TRY(hipGetLastError());
  return FA_OK;
}

// produce: a folding forward fills the call's guard inside its own launch, into the zeroed buffer ...
int zero_guard(const Call& c) {
  if (t_plan) { t_plan->emplace_back("memset"); return FA_OK; }
  FA_HIP_TRY(hipMemsetAsync(const_cast<float*>(c.guard), 0, (size_t)2 * fa::GUARD_SLOTS * sizeof(float), c.st));
  return FA_OK;
}
// ... any other forward by the separate pass over q and k
int guard_pass(const Call& c) {
  return launch_scale_guard(c.q, c.k, (long)c.batch * c.N, c.dp, c.dtype, const_cast<float*>(c.guard), c.st);
}

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
//     probed with a dry run of the dispatch code), or c is 1 (softmax_scale = ln 2: the operand multiply is exact).
constexpr float GUARD_BUDGET = 1e-2f;
inline Call exact(Call call) {   // the forward that scales every score in fp32 (the phased kernel), whatever else the caller selected
  call.tun.v[1] = 2;
  return call;
}
// produce (forward calls only, option 8 = 0): the call FILLS `guard` instead of reading it, so that the backward of the same (q, k)
// can take it: a forward that folds produces it inside its own launch (fa_common.h: guard_produce: no separate pass over q and k;
// the launch runs with the folded scale and its fp32-scaling twin, behind it, redoes the call if the finished guard says so);
// a forward whose selection folds nothing runs the separate pass (guard_pass), because the backward of the same call may fold.
int run_scaled(Call call, int (*run)(const Call&)) {
  const float c = call.tau * fa::LOG2E;
  const int mode = call.tun.v[8], produce = call.produce;
  const float* guard = call.guard;
  fa::Layout& lay = call.lay;
  lay.scale_sel = 0;
  if (mode == 1 || fabsf(c - 1.0f) < 1e-6f) return run(call);
  if (mode == 3 && t_plan) guard = reinterpret_cast<const float*>(16);   // fa_mi355x_plan: both launches of a guarded call
  // the backward's MFMA-slot kernels hold both scalings in one launch: fp32 scaling without a guard, the guard's choice with one
  lay.scale_sel = (mode == 2 || !guard) ? 1 : 2;
  if (lay.scale_sel == 2) {
    lay.guard = guard;
    lay.guard_coef = c * (0.001953125f * 0.57735027f) / GUARD_BUDGET;
    lay.guard_want = 3;   // (no launch of this run is skipped)
  }
  if (!plan_mode() || t_plan) {   // does the selection fold at all?  (dry run: no launch, no HIP call, nothing recorded)
    std::vector<std::string>* keep = t_plan;
    t_plan = nullptr;
    t_probe = true;
    t_fold = t_fold_produces = false;
    const int rc = run(call);
    t_probe = false;
    t_plan = keep;
    if (rc) return rc;
    if (!t_fold) {
      if (produce && guard && mode == 0)
        if (const int rc2 = guard_pass(call)) return rc2;
      return run(call);
    }
  }
  if (mode == 2 || !guard) return run(exact(call));
  lay.guard = guard;
  lay.guard_coef = c * (0.001953125f * 0.57735027f) / GUARD_BUDGET;
  if (produce && t_fold_produces) {
    if (const int rc = zero_guard(call)) return rc;
    lay.guard_want = 2;
  } else {
    if (produce)   // (a folding forward that cannot fill the guard itself: the causal slot build)
      if (const int rc = guard_pass(call)) return rc;
    lay.guard_want = 0;
  }
  if (const int rc = run(call)) return rc;
  lay.guard_want = 1;
  return run(exact(call));
}

int fwd_dispatch(Call c) {
  c.tau = c.scale > 0.f ? c.scale : sqrtf(1.0f / (float)c.d);   // (scale: fa_mi355x_*_scaled / _guarded; the reference has sqrt(1/d) only)
  c.lay.out_bf16 = c.tun.v[9] == 1 ? 1 : 0;
  return run_scaled(c, fwd_dispatch_one);
}

int bwd_dispatch(Call c) {
  c.tau = c.scale > 0.f ? c.scale : sqrtf(1.0f / (float)c.d);
  return run_scaled(c, bwd_dispatch_one);
}

// The checks of every device entry point, in one order: the first that fails decides the return code and fa_mi355x_last_error().
// The rules that differ between entry points are the call's fields (bwd, by_heads, padded, scale_required; arguments an entry point
// does not take keep defaults that pass).  Completes the call: batch, dp, tun, lay.
int validate(Call& c) {
  g_err[0] = 0;
  if (int rc = parse_opts(c.opts, c.nopts, c.tun)) return rc;
  if (c.bwd && (c.stages <= 0 || c.stages > FA_BWD_STAGE_ALL)) return set_err(FA_ERR_BAD_ARG, "bad stages mask");
  if (c.by_heads && (c.B <= 0 || c.H <= 0)) return set_err(FA_ERR_BAD_ARG, "B and H must be positive");
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

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

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
  // the dispatch functions only pass their pointers on to the (skipped) launches: any non-null values do
  float* one = reinterpret_cast<float*>(16);
  Call c = bwd_call(one, one, one, one, one, one, one, one, one, one, one, batch, N, d, causal, variant, dtype, stages, nullptr);
  c.bwd = stages != 0;   // stages = 0: the forward
  c.opts = opts;
  c.nopts = nopts;
  if (int rc = validate(c)) return rc;
  if (!out || n == 0) return set_err(FA_ERR_BAD_ARG, "null output buffer");
  std::vector<std::string> names;
  t_plan = &names;
  const int rc = c.bwd ? bwd_dispatch(c) : fwd_dispatch(c);
  t_plan = nullptr;
  if (rc) return rc;
  std::string joined;
  for (size_t i = 0; i < names.size(); ++i) joined += (i ? ";" : "") + names[i];
  if (joined.size() + 1 > n) return set_err(FA_ERR_BAD_ARG, "plan buffer too small");
  memcpy(out, joined.c_str(), joined.size() + 1);
  return FA_OK;
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
  return launch_scale_guard(q, k, rows, row_elems, dtype, guard, (hipStream_t)stream);
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
