"""Helpers shared by the GPU parity tests (imported only under -m gpu)."""
import os
import numpy as np

import oracle


def rand_u(rng, shape):
    # U(-1, 1) like the reference harness, test_utils.py:104-105
    return ((rng.random(shape, dtype=np.float32) - np.float32(0.5)) * np.float32(2)).astype(np.float32)


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


def to_np(t):
    return t.detach().float().cpu().numpy()


def oracle_heads(q, k, v, do, causal, heads):
    """fp64 dense oracle on a subset of the flattened (BH, N, d) heads.  Returns dict of stacked arrays."""
    out = {n: [] for n in ("o", "L", "m", "l", "dq", "dk", "dv")}
    for hh in heads:
        o, L, m, l = oracle.dense_attention_fw(q[hh], k[hh], v[hh], causal)
        out["o"].append(o); out["L"].append(L); out["m"].append(m); out["l"].append(l)
        if do is not None:
            dq, dk, dv = oracle.dense_attention_bw(q[hh], k[hh], v[hh], do[hh], causal)
            out["dq"].append(dq); out["dk"].append(dk); out["dv"].append(dv)
    return {n: np.stack(a) for n, a in out.items() if a}


LEFT_PAD = 70   # keys [0, 70) dropped: the whole first bf16 key tile (64), the first two fp32 tiles (32) and part of the next one


def left_padding_row(N, pad=LEFT_PAD):
    """Key-mask row of a left-padded sequence: -inf on keys [0, pad), 0 behind them."""
    row = np.zeros(N, dtype=np.float32)
    row[:pad] = -np.inf
    return row


def hole_and_finite_row(N, rng):
    """Key-mask row with key 0 kept, an interior -inf hole (keys [128, 256): one whole 128-key block, where N >= 320; keys [32, 96)
    below that) and a random 20 % of the other keys (never key 0) alternating between the two finite values callers pass for
    "minus infinity": -1e4 and the lowest float32."""
    row = np.zeros(N, dtype=np.float32)
    lo, hi = (128, 256) if N >= 320 else (32, 96)
    row[lo:hi] = -np.inf
    pick = rng.uniform(size=N) < 0.2
    pick[0] = False
    pick[lo:hi] = False
    idx = np.nonzero(pick)[0]
    row[idx[0::2]] = np.float32(-1e4)
    row[idx[1::2]] = np.finfo(np.float32).min
    return row


def padding_and_hole_mask(N, seed=0):
    """(2, N) key mask: batch 0 left-padded (left_padding_row), batch 1 hole_and_finite_row."""
    return np.stack([left_padding_row(N), hole_and_finite_row(N, np.random.default_rng(9000 + N + seed))])


def finite_drops_as_inf(mask):
    """The mask with its finite "minus infinity" entries (anything <= -1e4) replaced by -inf."""
    return np.where(mask <= np.float32(-1e4), np.float32(-np.inf), mask).astype(np.float32)


def masked_row_max(q, k, mask, causal):
    """fp64 row maximum of tau * q.k + mask under the causal rule (FA-1's m) for (B, H, N, d) arrays and a (B, N) mask."""
    q, k = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64)
    N, d = q.shape[-2], q.shape[-1]
    s = np.matmul(q, np.swapaxes(k, -1, -2)) / np.sqrt(d)
    if causal:
        s = np.where(np.tril(np.ones((N, N), dtype=bool)), s, -np.inf)
    return (s + np.asarray(mask, dtype=np.float64)[:, None, None, :]).max(axis=-1)


def core_fwd(layout, q, k, v, key_mask=None, dropout=None, causal=False, variant=2):
    """fa_mi355x_fwd_masked / _dropout through the C ABI, as device_ops._fwd calls them, in either layout (device_ops exposes these
    calls for (B, H, N, d) tensors only).  dropout: (rate, scale, seed).  Returns (out, l, m), l and m as (B, H, N)."""
    import torch
    from flash_attention_minitorch_amd import _lib, device_ops
    if layout == _lib.FA_LAYOUT_BNHD:
        B, N, H, d = q.shape
    else:
        B, H, N, d = q.shape
    out = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    l = torch.empty((B, H, N), dtype=torch.float32, device=q.device)
    m = torch.empty((B, H, N), dtype=torch.float32, device=q.device) if variant == _lib.FA_VARIANT_FA1 else None
    p = device_ops._ptr
    ptrs = (p(q), p(k), p(v), p(out), p(l), p(m), p(key_mask))
    tail = (B, H, N, d, layout, int(causal), variant, device_ops._dtype_code(q), device_ops._stream_ptr())
    if dropout is not None:
        rate, scale, seed = dropout
        _lib.check(_lib.core().fa_mi355x_fwd_dropout(*ptrs, float(rate), float(scale), int(seed) & 0xFFFFFFFF, *tail))
    else:
        _lib.check(_lib.core().fa_mi355x_fwd_masked(*ptrs, *tail))
    return out, l, m


def core_bwd(layout, q, k, v, o, do, l, m, key_mask=None, dropout=None, causal=False, variant=2):
    """fa_mi355x_bwd_masked / _dropout through the C ABI (see core_fwd).  Returns (dq, dk, dv) in q's layout."""
    import torch
    from flash_attention_minitorch_amd import _lib, device_ops
    if layout == _lib.FA_LAYOUT_BNHD:
        B, N, H, d = q.shape
    else:
        B, H, N, d = q.shape
    ws = torch.empty((_lib.core().fa_mi355x_bwd_workspace_bytes(B * H, N, d) + 3) // 4, dtype=torch.float32, device=q.device)
    dq, dk, dv = (torch.empty(q.shape, dtype=torch.float32, device=q.device) for _ in range(3))
    p = device_ops._ptr
    ptrs = (p(q), p(k), p(v), p(o), p(do), p(dq), p(dk), p(dv), p(l), p(m), p(key_mask))
    tail = (p(ws), B, H, N, d, layout, int(causal), variant, device_ops._dtype_code(q), device_ops._stream_ptr())
    if dropout is not None:
        rate, scale, seed = dropout
        _lib.check(_lib.core().fa_mi355x_bwd_dropout(*ptrs, float(rate), float(scale), int(seed) & 0xFFFFFFFF, *tail))
    else:
        _lib.check(_lib.core().fa_mi355x_bwd_masked(*ptrs, *tail))
    return dq, dk, dv


def check_abort_hook(tmp_path):
    """tests/abort_trace.c (installed by conftest.py on GPU runs: a GPU-side fault reaches the process as abort() from a ROCm runtime
    thread, for which Python's faulthandler prints no frame) had never fired: a child process installs it, calls
    abort() from a NON-Python thread of a small C helper, and the native backtrace must land in the hook's log file with the helper's
    frame in it, before the process dies of SIGABRT."""
    import subprocess
    import sys
    import textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    helper = tmp_path / "abort_from_thread.c"
    helper.write_text(textwrap.dedent("""
        #include <pthread.h>
        #include <stdlib.h>
        void* fa_test_runtime_thread(void* p) { (void)p; abort(); return 0; }
        int fa_test_abort_from_thread(void) {
          pthread_t t;
          pthread_create(&t, 0, fa_test_runtime_thread, 0);
          pthread_join(t, 0);
          return 0;
        }
    """))
    so_h, so_t, log = tmp_path / "helper.so", tmp_path / "trace.so", tmp_path / "abort_trace.log"
    subprocess.run(["gcc", "-O0", "-fPIC", "-shared", "-rdynamic", "-pthread", str(helper), "-o", str(so_h)], check=True)
    subprocess.run(["gcc", "-O1", "-fPIC", "-shared", "-rdynamic", os.path.join(root, "tests", "abort_trace.c"), "-o", str(so_t)], check=True)
    code = textwrap.dedent(f"""
        import ctypes, faulthandler
        faulthandler.enable()
        t = ctypes.CDLL({str(so_t)!r})
        t.fa_install_abort_trace.argtypes = [ctypes.c_char_p]
        assert t.fa_install_abort_trace({str(log)!r}.encode()) == 0
        ctypes.CDLL({str(so_h)!r}).fa_test_abort_from_thread()
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert r.returncode == -6, (r.returncode, r.stderr[-500:])           # died of SIGABRT, after the hook
    text = log.read_text()
    assert "native backtrace (tests/abort_trace.c)" in text and "helper.so(" in text, text[-1500:]   # (the frame of the thread that aborted)
    assert "native backtrace" in r.stderr                                  # ... and on stderr, in front of faulthandler's dump
