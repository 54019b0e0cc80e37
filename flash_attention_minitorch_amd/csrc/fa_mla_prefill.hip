// C ABI of libflash_attn_mi355x_mla_prefill.so (include/flash_attn_mi355x_mla_prefill.h): causal packed attention at the MLA head
// shape before absorption (192 score columns = k_nope | k_pe, 128 value columns), forward and backward, bf16, under the two
// cu_seqlens of the causal two-array library.  This library's checks and the launches of fa_mla_prefill.h's and
// fa_mla_prefill_bwd.h's kernels behind fa_bidir.h's schedule kernel; the error buffer, the launch macro, the block-map sizing and
// the row-constant kernel (bwd_prep_kernel of fa_bwd_dkdv.h, run over all Tq rows as one sequence) are fa_side_host.h's.
#include "../../include/flash_attn_mi355x_mla_prefill.h"
#include "fa_mla_prefill_bwd.h"
#include "fa_side_host.h"

namespace {

constexpr long GIB2 = 1L << 31;
constexpr int OVERHANG = fa::BIDIR_QBLOCK;   // rows past a buffer's end that a last tile's offsets may name (they read as zero)
static_assert(fa::MLAP_BWD_BK == fa::BIDIR_QBLOCK, "prefill_map_bytes sizes the key-block map too");

struct Call {
  const void *q, *k_nope, *k_pe, *v;
  float *out, *lse;
  const int *cu_q, *cu_k;
  char* ws;
  int nseq, Tq, Tk, H, k_ld, k_hs, v_ld, v_hs;
  float scale;
  hipStream_t st;
  // the backward's
  bool bwd;
  const void* dout;
  float *dq, *dk_nope, *dk_pe, *dv;
  int dk_ld, dk_hs, dv_ld, dv_hs;
};

inline bool sizes_ok(int nseq, int Tq, int Tk, int H) { return nseq >= 1 && Tq > 0 && Tk > 0 && H > 0; }
inline size_t prefill_map_bytes(int T, int nseq) { return map_bytes(T, nseq, fa::BIDIR_ENTRY_BYTES, fa::BIDIR_QBLOCK); }
inline int head_groups(int H) { return (H + fa::mla_prefill_heads_per_group(H) - 1) / fa::mla_prefill_heads_per_group(H); }
inline size_t rowc_bytes(int Tq, int H) { return align256((size_t)WS_VECS * H * Tq * sizeof(float)); }

// one strided operand: H heads of 128 columns in a row; esz 2: k_nope or v (bf16), esz 4: dk_nope or dv (fp32); strides in elements
int check_strided(const Call& c, const char* name, int ld, int hs, int esz) {
  char msg[160];
  const char* what = nullptr;
  if (ld % (16 / esz) != 0 || hs % (16 / esz) != 0)
    what = esz == 2 ? "row stride and head stride must be multiples of 8 elements" : "row stride and head stride must be multiples of 4 elements";
  else if (hs < fa::MLAP_DN) what = "head stride below the head's 128 columns";
  else if ((long)ld < (long)(c.H - 1) * hs + fa::MLAP_DN) what = "row stride below what H heads need ((H - 1) * head stride + 128)";
  else if (esz == 2 && ((long)c.Tk + OVERHANG) * ld * 2 >= GIB2) what = "byte offsets must stay under 2 GiB ((Tk + 128) * row stride * 2)";
  else if (esz == 4 && (long)c.Tk * ld * 4 >= GIB2) what = "byte offsets must stay under 2 GiB (Tk * row stride * 4)";
  if (!what) return FA_OK;
  snprintf(msg, sizeof(msg), "%s: %s", name, what);
  return set_err(FA_ERR_BAD_ARG, msg);
}

// Every check, in the order of fa_prefix.hip's, before any HIP call.
int validate(const Call& c) {
  g_err[0] = 0;
  if (!sizes_ok(c.nseq, c.Tq, c.Tk, c.H)) return set_err(FA_ERR_BAD_ARG, "nseq, Tq, Tk and H must be positive");
  if (!c.q || !c.k_nope || !c.k_pe || !c.v || !c.out || !c.lse || !c.cu_q || !c.cu_k || !c.ws ||
      (c.bwd && (!c.dout || !c.dq || !c.dk_nope || !c.dk_pe || !c.dv)))
    return set_err(FA_ERR_BAD_ARG, "null pointer argument");
  if (!(c.scale == 0.f || (c.scale > 0.f && std::isfinite(c.scale))))
    return set_err(FA_ERR_BAD_ARG, "softmax_scale must be positive and finite (0: 192^-1/2)");
  if (int rc = check_strided(c, "k_nope", c.k_ld, c.k_hs, 2)) return rc;
  if (int rc = check_strided(c, "v", c.v_ld, c.v_hs, 2)) return rc;
  if (c.bwd) {
    if (int rc = check_strided(c, "dk_nope", c.dk_ld, c.dk_hs, 4)) return rc;
    if (int rc = check_strided(c, "dv", c.dv_ld, c.dv_hs, 4)) return rc;
  }
  if (((long)c.Tq + OVERHANG) * c.H * fa::MLAP_DQ * 2 >= GIB2) return set_err(FA_ERR_BAD_ARG, "q: byte offsets must stay under 2 GiB ((Tq + 128) * H * 192 * 2)");
  if ((long)c.Tq * c.H * fa::MLAP_DV * 4 >= GIB2) return set_err(FA_ERR_BAD_ARG, "out: byte offsets must stay under 2 GiB (Tq * H * 128 * 4)");
  if (c.bwd && (long)c.Tq * c.H * fa::MLAP_DQ * 4 >= GIB2) return set_err(FA_ERR_BAD_ARG, "dq: byte offsets must stay under 2 GiB (Tq * H * 192 * 4)");
  if ((long)c.H * map_cap(c.Tq, c.nseq, fa::BIDIR_QBLOCK) >= GIB2 ||
      (c.bwd && (long)head_groups(c.H) * map_cap(c.Tk, c.nseq, fa::MLAP_BWD_BK) >= GIB2))
    return set_err(FA_ERR_BAD_ARG, "too many workgroups for one launch");
  for (const void* p : {c.q, c.k_nope, c.k_pe, c.v, (const void*)c.out})
    if ((uintptr_t)p % 16 != 0) return set_err(FA_ERR_BAD_ARG, "q, k_nope, k_pe, v and out must be 16-byte aligned");
  if (c.bwd)
    for (const void* p : {c.dout, (const void*)c.dq, (const void*)c.dk_nope, (const void*)c.dk_pe, (const void*)c.dv})
      if ((uintptr_t)p % 16 != 0) return set_err(FA_ERR_BAD_ARG, "dout, dq, dk_nope, dk_pe and dv must be 16-byte aligned");
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

// The backward's workspace: the query-block map, the key-block map, the row constants (the three vectors of H * Tq floats that
// bwd_prep_kernel writes; the kernels read two) and, with more than one head group, the dK_pe partials [groups][Tk][64].
int run_bwd(const Call& c) {
  using bf = fa::bf16_t;
  const int H = c.H, Tq = c.Tq, Tk = c.Tk, hpg = fa::mla_prefill_heads_per_group(H), groups = head_groups(H);
  const size_t mbq = prefill_map_bytes(Tq, c.nseq), mbk = prefill_map_bytes(Tk, c.nseq);
  int4 *map_q = reinterpret_cast<int4*>(c.ws), *map_k = reinterpret_cast<int4*>(c.ws + mbq);
  const long rows = (long)H * Tq;
  float *nlc = reinterpret_cast<float*>(c.ws + mbq + mbk), *ndelta = nlc + rows, *nl2 = nlc + 2 * rows;
  float* part = groups > 1 ? reinterpret_cast<float*>(c.ws + mbq + mbk + rowc_bytes(Tq, H)) : c.dk_pe;
  const int cap_q = (int)map_cap(Tq, c.nseq, fa::BIDIR_QBLOCK), cap_k = (int)map_cap(Tk, c.nseq, fa::MLAP_BWD_BK);
  // both maps, and zeros in the unowned rows of dq and dk_pe (whole rows of one stride: the schedule kernel's fill) ...
  fa::BidirFill fill{};
  fill.H = H;
  fill.ldq = H * fa::MLAP_DQ;
  fill.ldk = fa::MLAP_DR;
  fill.qmat = c.dq;
  fill.kmat[0] = c.dk_pe;
  FA_SIDE_LAUNCH("bidir_schedule_kernel", fa::bidir_schedule_kernel, 1 + fa::BIDIR_FILL_BLOCKS, 256, c.cu_q, c.cu_k, c.nseq, Tq, Tk, map_q,
                 cap_q, map_k, fa::MLAP_BWD_BK, cap_k, fill);
  // ... and of dk_nope and dv, heads under strides of their own
  FA_SIDE_LAUNCH("mla_prefill_bwd_fill_kernel", fa::mla_prefill_bwd_fill_kernel, fa::BIDIR_FILL_BLOCKS, 256, c.cu_k, c.nseq, Tk, H,
                 c.dk_nope, c.dk_ld, c.dk_hs, c.dv, c.dv_ld, c.dv_hs);
  const float tau = c.scale > 0.f ? c.scale : sqrtf(1.0f / (float)fa::MLAP_DQ);
  const fa::Layout lay = side_layout(true, Tq, H, H, fa::MLAP_DV);   // out and dO: [1][Tq][H][128]
  constexpr int RPB = 256 / (fa::MLAP_DV / 8);
  FA_SIDE_LAUNCH("bwd_prep_kernel", (fa::bwd_prep_kernel<bf, fa::MLAP_DV>), (int)((rows + RPB - 1) / RPB), 256, (const float*)c.out,
                 (const bf*)c.dout, (const float*)c.lse, (const float*)nullptr, nlc, ndelta, nl2, rows, Tq, lay, fa::AUX_FA2, 1.0f / tau);
  FA_SIDE_LAUNCH("mla_prefill_dkdv_kernel", fa::mla_prefill_dkdv_kernel, groups * cap_k, 64 * fa::MLAP_BWD_NW, (const bf*)c.q,
                 (const bf*)c.k_nope, (const bf*)c.k_pe, (const bf*)c.v, (const bf*)c.dout, (const float*)nlc, (const float*)ndelta,
                 c.dk_nope, part, c.dv, (const int4*)map_k, Tq, Tk, cap_k, groups, H, hpg, c.k_ld, c.k_hs, c.v_ld, c.v_hs, c.dk_ld, c.dk_hs,
                 c.dv_ld, c.dv_hs, tau);
  if (groups > 1)
    FA_SIDE_LAUNCH("mla_prefill_dkpe_sum_kernel", fa::mla_prefill_dkpe_sum_kernel, (int)(((long)Tk * (fa::MLAP_DR / 4) + 255) / 256), 256,
                   (const float*)part, c.dk_pe, c.cu_k, c.nseq, Tk, groups);
  FA_SIDE_LAUNCH("mla_prefill_dq_kernel", fa::mla_prefill_dq_kernel, H * cap_q, 256, (const bf*)c.q, (const bf*)c.k_nope,
                 (const bf*)c.k_pe, (const bf*)c.v, (const bf*)c.dout, (const float*)nlc, (const float*)ndelta, c.dq, (const int4*)map_q, Tq,
                 cap_q, H, c.k_ld, c.k_hs, c.v_ld, c.v_hs, tau);
  return FA_OK;
}

}  // namespace

extern "C" {

const char* fa_mi355x_mla_prefill_last_error(void) { return g_err; }

size_t fa_mi355x_fwd_mla_prefill_workspace_bytes(int nseq, int Tq, int Tk, int H) {
  return sizes_ok(nseq, Tq, Tk, H) ? prefill_map_bytes(Tq, nseq) : 0;
}

size_t fa_mi355x_bwd_mla_prefill_workspace_bytes(int nseq, int Tq, int Tk, int H) {
  if (!sizes_ok(nseq, Tq, Tk, H)) return 0;
  const int groups = head_groups(H);
  return prefill_map_bytes(Tq, nseq) + prefill_map_bytes(Tk, nseq) + rowc_bytes(Tq, H) +
         (groups > 1 ? (size_t)groups * Tk * fa::MLAP_DR * sizeof(float) : 0);
}

int fa_mi355x_fwd_mla_prefill(const void* q, const void* k_nope, const void* k_pe, const void* v, float* out, float* lse,
                              const int* cu_seqlens_q, const int* cu_seqlens_k, void* workspace, int nseq, int Tq, int Tk, int H, int k_ld,
                              int k_hstride, int v_ld, int v_hstride, float softmax_scale, void* stream) {
  const Call c{q, k_nope, k_pe, v, out, lse, cu_seqlens_q, cu_seqlens_k, (char*)workspace, nseq, Tq, Tk, H, k_ld, k_hstride, v_ld, v_hstride,
               softmax_scale, (hipStream_t)stream};
  if (int rc = validate(c)) return rc;
  return run(c);
}

int fa_mi355x_bwd_mla_prefill(const void* q, const void* k_nope, const void* k_pe, const void* v, const float* out, const void* dout,
                              const float* lse, float* dq, float* dk_nope, float* dk_pe, float* dv, const int* cu_seqlens_q,
                              const int* cu_seqlens_k, void* workspace, int nseq, int Tq, int Tk, int H, int k_ld, int k_hstride, int v_ld,
                              int v_hstride, int dk_ld, int dk_hstride, int dv_ld, int dv_hstride, float softmax_scale, void* stream) {
  const Call c{q, k_nope, k_pe, v, const_cast<float*>(out), const_cast<float*>(lse), cu_seqlens_q, cu_seqlens_k, (char*)workspace, nseq, Tq,
               Tk, H, k_ld, k_hstride, v_ld, v_hstride, softmax_scale, (hipStream_t)stream, true, dout, dq, dk_nope, dk_pe, dv, dk_ld,
               dk_hstride, dv_ld, dv_hstride};
  if (int rc = validate(c)) return rc;
  return run_bwd(c);
}

}  // extern "C"
