// Which kernels does a KV-cache call launch?  A host program that needs no GPU and no Python:
//   c++ -std=c++17 -O1 -I include tools/kv_launch_record.cpp -o kv_launch_record -rdynamic -ldl
//   ./kv_launch_record <path to libflash_attn_mi355x_decode.so>
// It dlopens the library and walks a fixed grid of calls with dummy non-null pointers.  The few HIP runtime functions the library calls
// between its checks and its return (what `<<<>>>` expands to, the launch and the last-error query) are defined HERE and exported
// (-rdynamic), and the executable comes first in the dynamic linker's search order, so the library's calls bind to them: every launch
// is recorded as (kernel symbol via dladdr, grid.x, block.x, dynamic LDS) and nothing runs.  One line per call:
//   <label> | <return code> <splits> <workspace bytes> <kernel>:<grid.x>:<block.x>:<lds> ...
// (the two size queries are those of the call's form; 0 0 for an append).  tests/test_kv_select_cpu.py compares the lines with
// tests/golden/kv_launch_grid.json, which was recorded from the library before its selection became a table.
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "flash_attn_mi355x_decode.h"

struct dim3 {
  unsigned x, y, z;
};

namespace {
std::string g_launches;
struct {
  dim3 grid, block;
  size_t lds;
  void* stream;
} g_config;
}  // namespace

extern "C" {
int __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, void* stream) {
  g_config = {grid, block, lds, stream};
  return 0;
}
int __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, void** stream) {
  *grid = g_config.grid, *block = g_config.block, *lds = g_config.lds, *stream = g_config.stream;
  return 0;
}
int hipLaunchKernel(const void* kernel, dim3 grid, dim3 block, void**, size_t lds, void*) {
  Dl_info info;
  const char* name = dladdr(kernel, &info) && info.dli_sname ? info.dli_sname : "?";
  g_launches += " " + std::string(name) + ":" + std::to_string(grid.x) + ":" + std::to_string(block.x) + ":" + std::to_string(lds);
  return 0;
}
int hipGetLastError(void) { return 0; }
const char* hipGetErrorString(int) { return "no error"; }
}

namespace {
void* g_lib;
int g_calls;

void* need(const char* name) {
  void* p = dlsym(g_lib, name);
  if (!p) {
    fprintf(stderr, "kv_launch_record: %s\n", dlerror());
    exit(2);
  }
  return p;
}
#define SYM(name) reinterpret_cast<decltype(&name)>(need(#name))

void line(const std::string& label, int rc, int splits, size_t ws) {
  printf("%s | %d %d %zu%s\n", label.c_str(), rc, splits, ws, g_launches.c_str());
  g_launches.clear();
  ++g_calls;
}

alignas(256) char g_mem[256];   // every pointer argument: non-null, never read
void* const P = g_mem;
float* const PF = reinterpret_cast<float*>(g_mem);
const int* const PI = reinterpret_cast<const int*>(g_mem);

const char* const FAMILY[3] = {"decode", "extend", "ragged"};
const int DS[3] = {32, 64, 128}, DTYPES[2] = {FA_DTYPE_BF16, FA_DTYPE_F32}, NQS[3] = {1, 3, 161}, NCAP = 520, PAGE = 128, MAX_PAGES = 5;
const int BATCHES[2][2] = {{64, 16}, {2, 2}};   // (B, Hkv): one split, several
enum Feature { NONE, SINK, SOFTCAP, LSINK, FP8 };
const char* const FEATURE[5] = {"none", "sink4", "softcap30", "lsink", "fp8"};
enum Form { ATTEND, FUSED };

struct Shape {
  int family, dtype, d, paged, window, G, B, Hkv, n;
  int H() const { return Hkv * G; }
  const int* table() const { return paged ? PI : nullptr; }
  int pages() const { return B * MAX_PAGES; }
  int ncap() const { return paged ? MAX_PAGES * PAGE : NCAP; }   // (what the size queries take)
  std::string label() const {
    return std::string(FAMILY[family]) + (dtype == FA_DTYPE_BF16 ? " bf16" : " fp32") + " d" + std::to_string(d) + (paged ? " paged" : " slab") + " w" +
           std::to_string(window) + " G" + std::to_string(G) + " B" + std::to_string(B) + " Hkv" + std::to_string(Hkv) + " n" + std::to_string(n);
  }
};

// ---- the general form: _window, _sink, _softcap, _lsink, _fp8 ----
void general(const Shape& s, Feature x, Form form, int causal = 1) {
  const void* kn = form == FUSED ? P : nullptr;
  const int sink = x == SINK ? 4 : 0, H = s.H();
  const float scale = 0.f;
  int rc;
#define GENERAL_HEAD P, kn, kn, P, P, PF, PF
#define GENERAL_TAIL s.table(), P, s.B, H, s.Hkv, s.n, NCAP, s.pages(), PAGE, MAX_PAGES, s.d, s.d, FA_LAYOUT_BNHD, scale, causal
  if (x == FP8) {
    static const decltype(&fa_mi355x_fwd_decode_fp8) f[2] = {SYM(fa_mi355x_fwd_decode_fp8), SYM(fa_mi355x_fwd_extend_fp8)};
    rc = f[s.family](P, kn, kn, P, P, PF, PF, PF, PF, PI, GENERAL_TAIL, s.dtype, nullptr);
  } else if (s.family == 2) {
    static const auto win = SYM(fa_mi355x_fwd_ragged_window);
    static const auto snk = SYM(fa_mi355x_fwd_ragged_sink);
    static const auto cap = SYM(fa_mi355x_fwd_ragged_softcap);
    static const auto lsk = SYM(fa_mi355x_fwd_ragged_lsink);
    rc = x == NONE      ? win(GENERAL_HEAD, PI, PI, GENERAL_TAIL, s.window, s.dtype, nullptr)
         : x == SINK    ? snk(GENERAL_HEAD, PI, PI, GENERAL_TAIL, s.window, sink, s.dtype, nullptr)
         : x == SOFTCAP ? cap(GENERAL_HEAD, PI, PI, GENERAL_TAIL, s.window, 30.f, s.dtype, nullptr)
                        : lsk(GENERAL_HEAD, PI, PI, GENERAL_TAIL, s.window, PF, s.dtype, nullptr);
  } else {
    static const decltype(&fa_mi355x_fwd_decode_window) win[2] = {SYM(fa_mi355x_fwd_decode_window), SYM(fa_mi355x_fwd_extend_window)};
    static const decltype(&fa_mi355x_fwd_decode_sink) snk[2] = {SYM(fa_mi355x_fwd_decode_sink), SYM(fa_mi355x_fwd_extend_sink)};
    static const decltype(&fa_mi355x_fwd_decode_softcap) cap[2] = {SYM(fa_mi355x_fwd_decode_softcap), SYM(fa_mi355x_fwd_extend_softcap)};
    static const decltype(&fa_mi355x_fwd_decode_lsink) lsk[2] = {SYM(fa_mi355x_fwd_decode_lsink), SYM(fa_mi355x_fwd_extend_lsink)};
    rc = x == NONE      ? win[s.family](GENERAL_HEAD, PI, GENERAL_TAIL, s.window, s.dtype, nullptr)
         : x == SINK    ? snk[s.family](GENERAL_HEAD, PI, GENERAL_TAIL, s.window, sink, s.dtype, nullptr)
         : x == SOFTCAP ? cap[s.family](GENERAL_HEAD, PI, GENERAL_TAIL, s.window, 30.f, s.dtype, nullptr)
                        : lsk[s.family](GENERAL_HEAD, PI, GENERAL_TAIL, s.window, PF, s.dtype, nullptr);
  }
  static const decltype(&fa_mi355x_decode_sink_splits) splits[3] = {SYM(fa_mi355x_decode_sink_splits), SYM(fa_mi355x_extend_sink_splits),
                                                                    SYM(fa_mi355x_ragged_sink_splits)};
  static const decltype(&fa_mi355x_decode_sink_workspace_bytes) bytes[3] = {
      SYM(fa_mi355x_decode_sink_workspace_bytes), SYM(fa_mi355x_extend_sink_workspace_bytes), SYM(fa_mi355x_ragged_sink_workspace_bytes)};
  line(s.label() + " " + FEATURE[x] + (form == FUSED ? " fused" : " attend") + (causal ? "" : " causal0"), rc,
       splits[s.family](s.B, H, s.Hkv, s.n, s.ncap(), s.d, s.dtype, s.window, sink),
       bytes[s.family](s.B, H, s.Hkv, s.n, s.ncap(), s.d, s.window, sink));
}

// ---- the legacy fixed forms: attend-only and fused, slab and _paged ----
void legacy(const Shape& s, Form form) {
  const int H = s.H();
  int rc;
#define LEGACY_TAIL FA_LAYOUT_BNHD, 0.f, 1, s.dtype, nullptr
  if (s.family == 2) {
    static const auto a = SYM(fa_mi355x_fwd_ragged);
    static const auto ap = SYM(fa_mi355x_fwd_ragged_paged);
    static const auto f = SYM(fa_mi355x_fwd_ragged_append);
    static const auto fp = SYM(fa_mi355x_fwd_ragged_append_paged);
    rc = form == ATTEND ? (s.paged ? ap(P, P, P, PF, PF, PI, PI, PI, P, s.B, H, s.Hkv, s.n, s.pages(), PAGE, MAX_PAGES, s.d, LEGACY_TAIL)
                                   : a(P, P, P, PF, PF, PI, PI, P, s.B, H, s.Hkv, s.n, NCAP, s.d, LEGACY_TAIL))
                        : (s.paged ? fp(P, P, P, P, P, PF, PF, PI, PI, PI, P, s.B, H, s.Hkv, s.n, s.pages(), PAGE, MAX_PAGES, s.d, s.d, LEGACY_TAIL)
                                   : f(P, P, P, P, P, PF, PF, PI, PI, P, s.B, H, s.Hkv, s.n, NCAP, s.d, s.d, LEGACY_TAIL));
  } else {
    static const decltype(&fa_mi355x_fwd_extend) a[2] = {SYM(fa_mi355x_fwd_decode_gqa), SYM(fa_mi355x_fwd_extend)};
    static const decltype(&fa_mi355x_fwd_extend_paged) ap[2] = {SYM(fa_mi355x_fwd_decode_paged), SYM(fa_mi355x_fwd_extend_paged)};
    static const decltype(&fa_mi355x_fwd_extend_append) f[2] = {SYM(fa_mi355x_fwd_decode_append), SYM(fa_mi355x_fwd_extend_append)};
    static const decltype(&fa_mi355x_fwd_extend_append_paged) fp[2] = {SYM(fa_mi355x_fwd_decode_append_paged),
                                                                       SYM(fa_mi355x_fwd_extend_append_paged)};
    const int i = s.family;
    rc = form == ATTEND ? (s.paged ? ap[i](P, P, P, PF, PF, PI, PI, P, s.B, H, s.Hkv, s.n, s.pages(), PAGE, MAX_PAGES, s.d, LEGACY_TAIL)
                                   : a[i](P, P, P, PF, PF, PI, P, s.B, H, s.Hkv, s.n, NCAP, s.d, LEGACY_TAIL))
                        : (s.paged ? fp[i](P, P, P, P, P, PF, PF, PI, PI, P, s.B, H, s.Hkv, s.n, s.pages(), PAGE, MAX_PAGES, s.d, s.d, LEGACY_TAIL)
                                   : f[i](P, P, P, P, P, PF, PF, PI, P, s.B, H, s.Hkv, s.n, NCAP, s.d, s.d, LEGACY_TAIL));
  }
  static const decltype(&fa_mi355x_extend_splits) splits[3] = {SYM(fa_mi355x_decode_splits_gqa), SYM(fa_mi355x_extend_splits),
                                                               SYM(fa_mi355x_ragged_splits)};
  static const decltype(&fa_mi355x_extend_workspace_bytes) bytes[3] = {
      SYM(fa_mi355x_decode_workspace_bytes_gqa), SYM(fa_mi355x_extend_workspace_bytes), SYM(fa_mi355x_ragged_workspace_bytes)};
  line(s.label() + " legacy" + (form == FUSED ? " fused" : " attend"), rc, splits[s.family](s.B, H, s.Hkv, s.n, s.ncap(), s.d, s.dtype),
       bytes[s.family](s.B, H, s.Hkv, s.n, s.ncap(), s.d));
}

// ---- the appends: the legacy forms, fa_mi355x_append_fp8 and fa_mi355x_append_d256; k_new on 16 bytes or 2 bytes past them, d_new = d
// or d - 1, so that both lane widths appear ----
enum AppendKind { LEGACY_APPEND, FP8_APPEND, D256_APPEND };
void append(const Shape& s, AppendKind kind, int offset, int d_new) {
  const void* kn = g_mem + offset;
  int rc;
#define APPEND_TAIL d_new, s.d, FA_LAYOUT_BNHD, s.dtype, nullptr
  if (kind == FP8_APPEND) {
    static const auto f = SYM(fa_mi355x_append_fp8);
    rc = f(kn, P, P, P, PF, PF, PI, s.table(), s.B, s.Hkv, s.n, NCAP, s.pages(), PAGE, MAX_PAGES, APPEND_TAIL);
  } else if (kind == D256_APPEND) {
    static const auto f = SYM(fa_mi355x_append_d256);
    rc = f(kn, P, P, P, PI, s.table(), s.B, s.Hkv, s.n, NCAP, s.pages(), PAGE, MAX_PAGES, APPEND_TAIL);
  } else if (s.family == 2) {
    static const auto f = SYM(fa_mi355x_ragged_append);
    static const auto fp = SYM(fa_mi355x_ragged_append_paged);
    rc = s.paged ? fp(kn, P, P, P, PI, PI, PI, s.B, s.Hkv, s.n, s.pages(), PAGE, MAX_PAGES, APPEND_TAIL)
                 : f(kn, P, P, P, PI, PI, s.B, s.Hkv, s.n, NCAP, APPEND_TAIL);
  } else {
    static const decltype(&fa_mi355x_extend_append) f[2] = {SYM(fa_mi355x_decode_append), SYM(fa_mi355x_extend_append)};
    static const decltype(&fa_mi355x_extend_append_paged) fp[2] = {SYM(fa_mi355x_decode_append_paged), SYM(fa_mi355x_extend_append_paged)};
    rc = s.paged ? fp[s.family](kn, P, P, P, PI, PI, s.B, s.Hkv, s.n, s.pages(), PAGE, MAX_PAGES, APPEND_TAIL)
                 : f[s.family](kn, P, P, P, PI, s.B, s.Hkv, s.n, NCAP, APPEND_TAIL);
  }
  line(s.label() + (kind == FP8_APPEND ? " fp8" : kind == D256_APPEND ? " d256" : " legacy") + " append k_new+" + std::to_string(offset) + " d_new" +
           std::to_string(d_new), rc, 0, 0);
}

// ---- head dim 256: the _softcap prototypes on the kernels of their own ----
void d256(const Shape& s, float softcap, Form form) {
  const void* kn = form == FUSED ? P : nullptr;
  static const decltype(&fa_mi355x_fwd_decode_d256) f[2] = {SYM(fa_mi355x_fwd_decode_d256), SYM(fa_mi355x_fwd_extend_d256)};
  static const decltype(&fa_mi355x_decode_d256_splits) splits[2] = {SYM(fa_mi355x_decode_d256_splits), SYM(fa_mi355x_extend_d256_splits)};
  static const decltype(&fa_mi355x_decode_d256_workspace_bytes) bytes[2] = {SYM(fa_mi355x_decode_d256_workspace_bytes),
                                                                            SYM(fa_mi355x_extend_d256_workspace_bytes)};
  const float scale = 0.f;
  const int causal = 1, H = s.H();
  const int rc = f[s.family](GENERAL_HEAD, PI, GENERAL_TAIL, s.window, softcap, s.dtype, nullptr);
  line(s.label() + " d256 " + (softcap > 0.f ? "softcap30" : "none") + (form == FUSED ? " fused" : " attend"), rc,
       splits[s.family](s.B, H, s.Hkv, s.n, s.ncap(), s.d, s.dtype, s.window), bytes[s.family](s.B, H, s.Hkv, s.n, s.ncap(), s.d, s.window));
}

// ---- the roped appends: bf16 slab NeoX pairs and fp8 paged interleaved pairs; ragged paged NeoX and ragged slab interleaved ----
void rope() {
  static const auto f = SYM(fa_mi355x_rope_append);
  static const auto fr = SYM(fa_mi355x_rope_append_ragged);
  const int B = 2, H = 8, Hkv = 2, d = 64, rot = 32, max_pos = 1024, bf16 = FA_DTYPE_BF16, L = FA_LAYOUT_BNHD;
  line("rope_append slab bf16 il0", f(P, P, P, P, P, P, nullptr, nullptr, PF, PF, PI, nullptr, B, H, Hkv, 40, NCAP, 0, 0, 0, d, d, rot, max_pos, L, 0, 0, bf16, nullptr), 0, 0);
  line("rope_append paged fp8 il1", f(P, P, P, P, P, P, PF, PF, PF, PF, PI, PI, B, H, Hkv, 40, NCAP, B * MAX_PAGES, PAGE, MAX_PAGES, d, d, rot, max_pos, L, 1, 1, bf16, nullptr), 0, 0);
  line("rope_append_ragged paged bf16 il0", fr(P, P, P, P, P, P, PF, PF, PI, PI, PI, B, H, Hkv, 200, NCAP, B * MAX_PAGES, PAGE, MAX_PAGES, d, d, rot, max_pos, L, 0, bf16, nullptr), 0, 0);
  line("rope_append_ragged slab bf16 il1", fr(P, P, P, P, P, P, PF, PF, PI, PI, nullptr, B, H, Hkv, 200, NCAP, 0, 0, 0, d, d, rot, max_pos, L, 1, bf16, nullptr), 0, 0);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <libflash_attn_mi355x_decode.so>\n", argv[0]);
    return 2;
  }
  g_lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!g_lib) {
    fprintf(stderr, "kv_launch_record: %s\n", dlerror());
    return 2;
  }
  for (int family = 0; family < 3; ++family)
    for (int d : DS)
      for (int dtype : DTYPES)
        for (int paged = 0; paged < 2; ++paged)
          for (int G : {1, 4})
            for (const int* b : BATCHES)
              for (int n : NQS) {
                if (family == 0 && n > 3) continue;   // (decode stops at 3)
                for (int window : {0, 200}) {
                  const Shape s = {family, dtype, d, paged, window, G, b[0], b[1], n};
                  for (Form form : {ATTEND, FUSED}) {
                    for (Feature x : {NONE, SINK, SOFTCAP, LSINK}) general(s, x, form);
                    if (window == 0 && family != 2) general(s, FP8, form);   // (the fp8 entry points take no window; fp32: refused)
                    if (window == 0) legacy(s, form);
                  }
                }
                if (G != 1) continue;   // (an append has no query heads)
                const Shape s = {family, dtype, d, paged, 0, 1, b[0], b[1], n};
                for (int offset : {0, 2})
                  for (int d_new : {d, d - 1}) {
                    append(s, LEGACY_APPEND, offset, d_new);
                    if (family == 1) append(s, FP8_APPEND, offset, d_new);   // (the extend family's checks: any Nq)
                  }
              }
  for (int family = 0; family < 2; ++family)
    for (int paged = 0; paged < 2; ++paged)
      for (int G : {1, 4})
        for (const int* b : BATCHES)
          for (int n : NQS) {
            if (family == 0 && n > 3) continue;
            for (int window : {0, 200})
              for (float softcap : {0.f, 30.f})
                for (Form form : {ATTEND, FUSED}) d256({family, FA_DTYPE_BF16, 256, paged, window, G, b[0], b[1], n}, softcap, form);
            if (G != 1 || family != 1) continue;
            for (int offset : {0, 2})
              for (int d_new : {256, 255}) append({1, FA_DTYPE_BF16, 256, paged, 0, 1, b[0], b[1], n}, D256_APPEND, offset, d_new);
          }
  rope();
  // ---- refused combinations (fp32 with fp8 is in the grid above) ----
  const Shape ok = {0, FA_DTYPE_BF16, 64, 0, 200, 4, 2, 2, 3};
  Shape s = ok;
  s.d = 256;   // d = 256 on an old entry point
  general(s, NONE, ATTEND);
  legacy(s, ATTEND);
  append(s, LEGACY_APPEND, 0, 256);
  d256(ok, 0.f, ATTEND);   // d = 64 on a _d256 one
  append(ok, D256_APPEND, 0, 64);
  s = ok, s.d = 256, s.dtype = FA_DTYPE_F32;   // the d = 256 kernels are bf16 alone
  d256(s, 0.f, ATTEND);
  general(ok, NONE, ATTEND, 0);   // a window without the causal mask
  general(ok, SOFTCAP, ATTEND, 0);
  fprintf(stderr, "kv_launch_record: %d calls\n", g_calls);
  return 0;
}
