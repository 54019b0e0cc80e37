/*
 * flash_attn_mi355x_window_softcap.h -- the logit soft-capping entry points of libflash_attn_mi355x_window.so: the differentiable
 * forward and backward of flash_attn_mi355x_window.h in which every score passes through softcap * tanh(score / softcap).  It
 * includes that header, whose status codes, dtypes, layouts, workspace query and fa_mi355x_window_last_error these calls share.
 *
 * The KV-cache calls generate under a cap (flash_attn_mi355x_decode_softcap.h: Gemma-2's attn_logit_softcapping, Grok-1); these two
 * calls train under the same function.  With tau = softmax_scale, or 1/sqrt(d) when that is 0, and the admitted keys j of row i as
 * the window header defines them (j <= i and (j > i - W or j < S)):
 *
 *   z_ij = softcap * tanh(tau * (q_i . k_j) / softcap)
 *   P    = softmax of z over the admitted keys,    out = P . V,    lse = ln sum_j exp(z_ij)
 *   dZ   = P o (dP - delta),    dS = dZ o (1 - tanh^2(tau * s / softcap)) * tau,    dQ = dS . K,  dK = dS^T . Q,  dV = P^T . dO
 *
 * The cap acts on every score BEFORE the mask: a key that is not admitted stays out, whatever the cap (a mask applied first would
 * come out of the cap as -softcap, an admitted key).  |z| <= softcap, so |lse| <= softcap + ln(admitted keys).
 *
 *   softcap = 0      the _window call exactly: the same launches and bits.
 *   softcap < 0, NaN or infinite   FA_ERR_BAD_ARG with a message, before any HIP call, with the other argument checks.
 *   window           W >= 1 as there; W > N is clamped to N, so a capped causal call without a window passes window = N.
 *   sink             S >= 0 as there.  Sinks are allowed beside a cap HERE: the mask is orthogonal to the cap in these kernels.  The
 *                    KV-cache calls still refuse that pair (flash_attn_mi355x_decode_softcap.h), so a model that is to generate
 *                    through them trains without sinks.
 *   workspace        fa_mi355x_bwd_window_workspace_bytes, unchanged: it does not depend on the cap.
 *   Not built: a cap without the causal mask, and a cap in the packed (cu_seqlens) libraries.
 *
 * Both prototypes are the _window ones with `float softcap` behind `int window`, as the decode headers place it, and every argument
 * check of those applies.  Asynchronous on `stream`, no allocation, no host synchronisation, no atomics: a call repeats bit for bit.
 *
 * How it runs (win_fwd_softcap_kernel, win_dq_softcap_kernel, win_dkdv_softcap_kernel: the cap builds of the three kernels' text).
 * With k2 = 2 log2(e) tau / softcap, computed once per workgroup, a raw score s becomes
 *     t = exp2(s * k2),    r = 1 / (t + 1),    z = softcap - 2 softcap r
 * right after the QK products: one v_exp_f32 and one v_rcp_f32 per score (gfx950 has no tanh instruction), the decode family's
 * arithmetic.  From there on the scores are the logits: the softmax constant is log2(e) and the backward's row constant is -lse.
 * The backward recomputes r in both of its kernels and takes 1 - tanh^2 = 4 r (1 - r) from it: no further transcendental, 0 at
 * both saturations and finite for every finite score.  The walk over the tiles, the mask and the split-operand rules are the
 * uncapped builds', which are the machine code they were.
 */
#ifndef FLASH_ATTN_MI355X_WINDOW_SOFTCAP_H
#define FLASH_ATTN_MI355X_WINDOW_SOFTCAP_H

#include "flash_attn_mi355x_window.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out = softmax over the admitted keys of the capped scores . v, and the natural-log logsumexp lse of the capped scores. */
int fa_mi355x_fwd_window_softcap(const void* q, const void* k, const void* v, float* out, float* lse, int B, int H, int Hkv, int N,
                                 int d, int layout, float softmax_scale, int window, float softcap, int sink, int dtype, void* stream);

/* q_grad, k_grad, v_grad from out_grad, the capped forward's out and lse, under the same window, cap and sink.  workspace and
 * launches as fa_mi355x_bwd_window (the row constants are -lse and -rowsum(out_grad * out)). */
int fa_mi355x_bwd_window_softcap(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad,
                                 float* k_grad, float* v_grad, const float* lse, void* workspace, int B, int H, int Hkv, int N, int d,
                                 int layout, float softmax_scale, int window, float softcap, int sink, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_WINDOW_SOFTCAP_H */
