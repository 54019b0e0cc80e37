"""attention_stack(window=, sink=, rope=) on the GPU: against a dense masked torch stack, against the prefill of a
KVCache(window=, sink=, rope=) with the same weights (what trains is what generates), and its weight gradients.  Tolerances: the
model tolerance tests/test_gpu_window.py uses for _dense_window_stack (tests/test_gpu_extend.py: _model_tol)."""
import numpy as np
import pytest

from gpu_util import maxabs, to_np
from test_gpu_decode import _tdt, _torch
from test_gpu_decode_append import _stack
from test_gpu_extend import _model_tol

pytestmark = pytest.mark.gpu

E, H, HKV, L, B, N, W, S = 256, 4, 2, 2, 2, 300, 70, 4


def _dense_stack(x, layers, n_head, W, S, rope):
    """tests/test_gpu_window.py's _dense_window_stack with sink tokens and the rotation: projections, rotation and residual as
    modules_transformer makes them, the scores of all N x N pairs in torch fp32 under the mask."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    Bx, Nx, Ex = x.shape
    i = torch.arange(Nx, device=x.device)
    ok = (i[None, :] <= i[:, None]) & ((i[None, :] > i[:, None] - W) | (i[None, :] < S))
    for wq, wk, wv, wo in layers:
        q, k, v = mt._project(x, wq, wk, wv, n_head)
        if rope is not None:
            q, k = rope.apply(q), rope.apply(k)
        G = n_head // k.shape[2]
        qf, kf, vf = (t.float().permute(0, 2, 1, 3) for t in (q, k.repeat_interleave(G, 2), v.repeat_interleave(G, 2)))
        s = (qf @ kf.transpose(2, 3)) * q.shape[3] ** -0.5
        p = torch.softmax(s.masked_fill(~ok, float("-inf")), dim=-1)
        o = (p @ vf).permute(0, 2, 1, 3)
        x = x + (o.reshape(Bx * Nx, Ex).to(x.dtype) @ wo).view(Bx, Nx, Ex)
    return x


def _rope(mt):
    return mt.Rotary.table(512, E // H, device="cuda")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "permuted"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_windowed_stack_matches_the_dense_masked_stack_and_the_prefill_of_a_windowed_cache(dtype, fused):
    from flash_attention_minitorch_amd import modules_transformer as mt
    x, layers = _stack(np.random.default_rng(W + S), dtype, B, E, H, HKV, L, N)
    rope = _rope(mt)
    want = to_np(_dense_stack(x, layers, H, W, S, rope))
    tol = _model_tol(dtype, want)
    got = to_np(mt.attention_stack(x, layers, H, fused_layout=fused, rope=rope, window=W, sink=S))
    assert maxabs(got, want) < tol, (maxabs(got, want), tol)
    cache = mt.KVCache(L, B, 384, H, E // H, _tdt(dtype), "cuda", n_kv_head=HKV, window=W, sink=S, rope=rope)
    gen = to_np(mt.attention_stack_prefill(x, layers, H, cache))
    assert maxabs(got, gen) < tol, (maxabs(got, gen), tol)
    if dtype == "f32":   # and a real window is not the causal stack
        assert maxabs(got, to_np(mt.attention_stack(x, layers, H, rope=rope))) > 100 * tol


def test_weight_gradients_match_the_dense_masked_stack_in_fp32():
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    x, layers = _stack(np.random.default_rng(3), "f32", B, E, H, HKV, L, N)
    rope = _rope(mt)
    dy = torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, (B, N, E)).astype(np.float32)).to("cuda")

    def grads(fn):
        ws = [tuple(w.clone().requires_grad_() for w in layer) for layer in layers]
        xg = x.clone().requires_grad_()
        fn(xg, ws).backward(dy)
        return [xg.grad] + [w.grad for layer in ws for w in layer]
    got = grads(lambda xg, ws: mt.attention_stack(xg, ws, H, rope=rope, window=W, sink=S))
    want = grads(lambda xg, ws: _dense_stack(xg, ws, H, W, S, rope))
    for g, w in zip(got, want):
        tol = _model_tol("f32", to_np(w))
        assert maxabs(to_np(g), to_np(w)) < tol, (maxabs(to_np(g), to_np(w)), tol, tuple(w.shape))
