// C ABI of libflash_attn_mi355x_mla_prefill.so (include/flash_attn_mi355x_mla_prefill.h): causal packed attention at the MLA head
// shape before absorption (192 score columns = k_nope | k_pe, 128 value columns), forward, bf16, under the two cu_seqlens of the
// causal two-array library.  This library's checks and the launch of fa_mla_prefill.h's kernel behind fa_bidir.h's schedule kernel;
// the error buffer, the launch macro and the block-map sizing are fa_side_host.h's.
#include "../../include/flash_attn_mi355x_mla_prefill.h"
#include "fa_mla_prefill.h"
#include "fa_side_host.h"

namespace {

constexpr long GIB2 = 1L << 31;
constexpr int OVERHANG = fa::BIDIR_QBLOCK;   // rows past a buffer's end that a last tile's offsets may name (they read as zero)

struct Call {
  const void *q, *k_nope, *k_pe, *v;
  float *out, *lse;
  const int *cu_q, *cu_k;
  char* ws;
  int nseq, Tq, Tk, H, k_ld, k_hs, v_ld, v_hs;
  float scale;
  hipStream_t st;
};

inline bool sizes_ok(int nseq, int Tq, int Tk, int H) { return nseq >= 1 && Tq > 0 && Tk > 0 && H > 0; }
inline size_t prefill_map_bytes(int Tq, int nseq) { return map_bytes(Tq, nseq, fa::BIDIR_ENTRY_BYTES, fa::BIDIR_QBLOCK); }

// one strided operand (k_nope or v): H heads of 128 columns in a row
int check_strided(const Call& c, const char* name, int ld, int hs) {
  char msg[160];
  const char* what = nullptr;
  if (ld % 8 != 0 || hs % 8 != 0) what = "row stride and head stride must be multiples of 8 elements";
  else if (hs < fa::MLAP_DN) what = "head stride below the head's 128 columns";
  else if ((long)ld < (long)(c.H - 1) * hs + fa::MLAP_DN) what = "row stride below what H heads need ((H - 1) * head stride + 128)";
  else if (((long)c.Tk + OVERHANG) * ld * 2 >= GIB2) what = "byte offsets must stay under 2 GiB ((Tk + 128) * row stride * 2)";
  if (!what) return FA_OK;
  snprintf(msg, sizeof(msg), "%s: %s", name, what);
  return set_err(FA_ERR_BAD_ARG, msg);
}

// Every check, in the order of fa_prefix.hip's, before any HIP call.
int validate(const Call& c) {
  g_err[0] = 0;
  if (!sizes_ok(c.nseq, c.Tq, c.Tk, c.H)) return set_err(FA_ERR_BAD_ARG, "nseq, Tq, Tk and H must be positive");
  if (!c.q || !c.k_nope || !c.k_pe || !c.v || !c.out || !c.lse || !c.cu_q || !c.cu_k || !c.ws) return set_err(FA_ERR_BAD_ARG, "null pointer argument");
  if (!(c.scale == 0.f || (c.scale > 0.f && std::isfinite(c.scale))))
    return set_err(FA_ERR_BAD_ARG, "softmax_scale must be positive and finite (0: 192^-1/2)");
  if (int rc = check_strided(c, "k_nope", c.k_ld, c.k_hs)) return rc;
  if (int rc = check_strided(c, "v", c.v_ld, c.v_hs)) return rc;
  if (((long)c.Tq + OVERHANG) * c.H * fa::MLAP_DQ * 2 >= GIB2) return set_err(FA_ERR_BAD_ARG, "q: byte offsets must stay under 2 GiB ((Tq + 128) * H * 192 * 2)");
  if ((long)c.Tq * c.H * fa::MLAP_DV * 4 >= GIB2) return set_err(FA_ERR_BAD_ARG, "out: byte offsets must stay under 2 GiB (Tq * H * 128 * 4)");
  if ((long)c.H * map_cap(c.Tq, c.nseq, fa::BIDIR_QBLOCK) >= GIB2) return set_err(FA_ERR_BAD_ARG, "too many workgroups for one launch");
  for (const void* p : {c.q, c.k_nope, c.k_pe, c.v, (const void*)c.out})
    if ((uintptr_t)p % 16 != 0) return set_err(FA_ERR_BAD_ARG, "q, k_nope, k_pe, v and out must be 16-byte aligned");
  if ((uintptr_t)c.ws % 256 != 0) return set_err(FA_ERR_BAD_ARG, "the workspace must be 256-byte aligned");
  return FA_OK;
}

// The workspace: the query-block map.
int run(const Call& c) {
  int4* map_q = reinterpret_cast<int4*>(c.ws);
  const int cap_q = (int)map_cap(c.Tq, c.nseq, fa::BIDIR_QBLOCK);
  fa::BidirFill fill{};
  fill.H = c.H;
  fill.ldq = c.H * fa::MLAP_DV;   // out's width, not q's
  fill.qmat = c.out;
  fill.rowc = c.lse;
  FA_SIDE_LAUNCH("bidir_schedule_kernel", fa::bidir_schedule_kernel, 1 + fa::BIDIR_FILL_BLOCKS, 256, c.cu_q, c.cu_k, c.nseq, c.Tq, c.Tk,
                 map_q, cap_q, (int4*)nullptr, 0, 0, fill);
  const float tau = c.scale > 0.f ? c.scale : sqrtf(1.0f / (float)fa::MLAP_DQ);
  using bf = fa::bf16_t;
  FA_SIDE_LAUNCH("mla_prefill_fwd_kernel", fa::mla_prefill_fwd_kernel, c.H * cap_q, 256, (const bf*)c.q, (const bf*)c.k_nope,
                 (const bf*)c.k_pe, (const bf*)c.v, c.out, c.lse, (const int4*)map_q, c.Tq, cap_q, c.H, c.k_ld, c.k_hs, c.v_ld, c.v_hs, tau);
  return FA_OK;
}

}  // namespace

extern "C" {

const char* fa_mi355x_mla_prefill_last_error(void) { return g_err; }

size_t fa_mi355x_fwd_mla_prefill_workspace_bytes(int nseq, int Tq, int Tk, int H) {
  return sizes_ok(nseq, Tq, Tk, H) ? prefill_map_bytes(Tq, nseq) : 0;
}

int fa_mi355x_fwd_mla_prefill(const void* q, const void* k_nope, const void* k_pe, const void* v, float* out, float* lse,
                              const int* cu_seqlens_q, const int* cu_seqlens_k, void* workspace, int nseq, int Tq, int Tk, int H, int k_ld,
                              int k_hstride, int v_ld, int v_hstride, float softmax_scale, void* stream) {
  const Call c{q, k_nope, k_pe, v, out, lse, cu_seqlens_q, cu_seqlens_k, (char*)workspace, nseq, Tq, Tk, H, k_ld, k_hstride, v_ld, v_hstride,
               softmax_scale, (hipStream_t)stream};
  if (int rc = validate(c)) return rc;
  return run(c);
}

}  // extern "C"
