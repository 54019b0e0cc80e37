// Sliding-window and attention-sink forward / backward kernels for MI355X (gfx950): the kernels of libflash_attn_mi355x_window.so
// (include/flash_attn_mi355x_window.h), written against fa_atoms.h.  Kernels of their own beside fwd_kernel, bwd_dq_kernel and
// bwd_dkdv_kernel (fa_fwd.h, fa_bwd_dq.h, fa_bwd_dkdv.h), whose phased structure they share: the query (forward, dQ) or the key
// (dK/dV) on the lane, the other operand staged through LDS in double-buffered tiles, tau*log2(e) applied to every score in fp32.
//
// The mask is the decode family's (flash_attn_mi355x_decode_window.h, _sink.h) with the query of row i at position i:
//     row i admits key j   iff   j <= i   and   (j > i - W   or   j < S)                       1 <= W <= N, 0 <= S <= N
// Every row admits its own position, so no row is empty.  What the mask saves is never loaded: a query block walks only the key
// tiles that hold a key some row of it admits, a key block only the query slices that hold a query admitting one of its keys; a
// 32 x 32 sub-tile is masked per element only where it straddles an edge (the diagonal, a window edge, S), by a wave-uniform test,
// as fa_decode_extend_body.h does.  Under a window every block does about the same work: no paired or ranked block orders.
//
// bf16: rows that can admit fewer than 64 keys (W + S < 64: every row; otherwise positions 0..63) take P and dS into the second
// product as two bf16 fragments (Atom::pack_lo), the project's rule for thin rows; the dK/dV kernel does the same for the waves that
// hold a sink key (see there).  No atomics, a fixed summation order.
#pragma once
#include "fa_common.h"

// The packed variable-length library (fa_varlen.h) builds the three kernels of this file under names of its own, with the block
// taken from a device-side map instead of blockIdx alone: it defines the hooks below and includes this file as text, the way the
// sink builds of fa_decode.h share their bodies.  Left undefined, the hooks spell the window library's kernels, token for token.
//   FA_WIN_KERNEL(stem)       the kernel's name
//   FA_WIN_GEOM_PARAMS        the parameters that say where the blocks are;  FA_WIN_MASK_PARAMS: the window and the sink
//   FA_WIN_LOCATE(blk, nb)    sets bh and blk (query blocks);  FA_WIN_LOCATE_KEYS: the same for the key blocks of dK/dV
//   FA_WIN_ROW0               the first row of the block's matrix within the buffers (a sequence's offset), as size_t
//   FA_WIN_ROWCONST0          where the row constants (lse, nlc, ndelta) of the block's matrix begin
#ifndef FA_WIN_KERNEL
#define FA_WIN_KERNEL(stem) win_##stem##_kernel
#define FA_WIN_GEOM_PARAMS int N, int nblk, int BH
#define FA_WIN_MASK_PARAMS int W, int S
#define FA_WIN_LOCATE(blk, nb) map_block(blockIdx.x, BH, nb, bh, blk);
#define FA_WIN_LOCATE_KEYS(blk, nb)                                       \
  if (S > 0) map_block_ranked(blockIdx.x, BH, nb, max(BH >> 3, 1), bh, blk); \
  else map_block(blockIdx.x, BH, nb, bh, blk);
#define FA_WIN_ROW0 (size_t)0
#define FA_WIN_ROWCONST0 (size_t)bh * N
#endif

namespace fa {

constexpr float WIN_DEFER_SUM = 64.0f;   // as fa_fwd.h's MAX_DEFER_SUM: bound on a lane's partial row sum while the reference stands

// (wave-uniform) does the 32 x 32 sub-tile of queries q0 .. q0 + 31 and keys k0 .. k0 + 31 hold an admitted pair / a pair that is not
FA_DEV bool win_any(int q0, int k0, int W, int S) { return k0 <= q0 + 31 && (k0 + 31 > q0 - W || k0 < S); }
FA_DEV bool win_straddles(int q0, int k0, int W, int S) { return k0 + 31 > q0 || (k0 <= q0 + 31 - W && k0 + 31 >= S); }
FA_DEV bool win_admits(int query, int key, int W, int S) { return key <= query && (key > query - W || key < S); }

// The key tiles (BN keys each) of the query block q_lo .. q_hi, in ascending order: the ns tiles that hold a sink key and lie wholly
// below the window's range, then the tiles from the first row's window edge (rounded down to a tile) up to the last row's position.
struct WinWalk {
  int ns, lo_t, nt;
  template <int BN> FA_DEV void init(int q_lo, int q_hi, int W, int S) {
    lo_t = max(q_lo - W + 1, 0) / BN;
    ns = min((S + BN - 1) / BN, lo_t);
    nt = ns + q_hi / BN - lo_t + 1;
  }
  FA_DEV int tile(int t) const { return t < ns ? t : t - ns + lo_t; }
};

// The three kernels are text (fa_window_body.h), built once as they always were and, where the includer asks for them, once more
// under logit soft-capping (include/flash_attn_mi355x_window_softcap.h): every score becomes z = softcap * tanh(tau * s / softcap)
// between the QK products and the masks (cap_rcp, cap_z of fa_common.h: the decode family's arithmetic).  The cap builds carry names
// of their own and one more argument, the cap; every difference sits under `if constexpr (CAP)`, so the other builds are the code
// they were.  Only fa_window.hip defines FA_WIN_SOFTCAP_KERNEL: the packed library gains no kernel.
//   FA_WIN_SOFTCAP_KERNEL(stem)   the name of the kernel's cap build; undefined: no cap builds
#define FA_WIN_CAP 0
#define FA_WIN_NAME(stem) FA_WIN_KERNEL(stem)
#define FA_WIN_CAP_PARAM
#define FA_WIN_CAP_VALUE 0.f
#define FA_WIN_LSINK 0
#define FA_WIN_LSINK_PARAM
#define FA_WIN_LSINK_LOGIT 0.f
#include "fa_window_body.h"
#undef FA_WIN_CAP
#undef FA_WIN_NAME
#undef FA_WIN_CAP_PARAM
#undef FA_WIN_CAP_VALUE
#ifdef FA_WIN_SOFTCAP_KERNEL
#define FA_WIN_CAP 1
#define FA_WIN_NAME(stem) FA_WIN_SOFTCAP_KERNEL(stem)
#define FA_WIN_CAP_PARAM , float softcap
#define FA_WIN_CAP_VALUE softcap
#include "fa_window_body.h"
#undef FA_WIN_CAP
#undef FA_WIN_NAME
#undef FA_WIN_CAP_PARAM
#undef FA_WIN_CAP_VALUE
#endif
#undef FA_WIN_LSINK
#undef FA_WIN_LSINK_PARAM
#undef FA_WIN_LSINK_LOGIT
// Once more, where the includer asks for it, with learned sink logits in the FORWARD's epilogue (include/flash_attn_mi355x_lsink.h):
// the head's logit a = sink_logits[bh % sink_heads] joins the row's softmax as a column without a value vector where the row's
// 1 / l is formed (lsink_finish of fa_common.h, the KV-cache calls' arithmetic): out = O wa / denom, lse = ln(e^a + sum_j e^z_j).
// Every difference sits under `if constexpr (LSINK)`, so the other builds are the code they were.  The backward needs no build: P =
// exp2(s c - lse log2 e) and delta = rowsum(dO o out) are what the dQ and dK/dV kernels form from the lse and out they are given, and
// with this forward's lse and out those are the sink softmax's (the dq and dkdv templates of this inclusion are never instantiated).
// Only fa_lsink.hip defines FA_WIN_LSINK_KERNEL: neither the window library nor the packed one gains a kernel.
//   FA_WIN_LSINK_KERNEL(stem)   the name of the kernel's lsink build; undefined: no lsink builds
#ifdef FA_WIN_LSINK_KERNEL
#define FA_WIN_CAP 0
#define FA_WIN_NAME(stem) FA_WIN_LSINK_KERNEL(stem)
#define FA_WIN_CAP_PARAM
#define FA_WIN_CAP_VALUE 0.f
#define FA_WIN_LSINK 1
#define FA_WIN_LSINK_PARAM , const float* __restrict__ sink_logits, int sink_heads
#define FA_WIN_LSINK_LOGIT sink_logits[bh % sink_heads]
#include "fa_window_body.h"
#undef FA_WIN_CAP
#undef FA_WIN_NAME
#undef FA_WIN_CAP_PARAM
#undef FA_WIN_CAP_VALUE
#undef FA_WIN_LSINK
#undef FA_WIN_LSINK_PARAM
#undef FA_WIN_LSINK_LOGIT
#endif

}  // namespace fa
