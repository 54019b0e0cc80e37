"""CPU-side checks of the head-dim-256 entry points (include/flash_attn_mi355x_decode_d256.h): symbols and prototypes, builds without
scratch, refusals before any HIP call (fake non-null pointers), size queries, device_ops' refusals; the fp64 reference of the GPU tests."""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_decode_cpu import built  # noqa: F401  (the module-scoped build fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "flash_attn_mi355x_decode_d256.h"
TOL = 1e-3   # the project's bf16 figure, max-abs on out and lse


def reference(q, k, v, lens, causal=True, window=None, softcap=None, tau=1 / 16):
    """fp64 attention on the gathered cache: q (B, Nq, H, d), k / v (B, Ncap, Hkv, d), lens (B,).  Query i sits at len - Nq + i, admits
    the ``window`` keys up to its position, and the cap goes BEFORE the masks.  Returns (out, lse (B, H, Nq)); empty rows: 0, -inf."""
    B, Nq, H, d = q.shape
    G = H // k.shape[2]
    out, lse = torch.zeros(B, Nq, H, d, dtype=torch.float64), torch.full((B, H, Nq), -np.inf, dtype=torch.float64)
    for b in range(B):
        n = int(lens[b])
        kb, vb = (t[b, :n].double().repeat_interleave(G, 1).transpose(0, 1) for t in (k, v))   # (H, n, d)
        s = tau * q[b].double().transpose(0, 1) @ kb.transpose(1, 2)   # (H, Nq, n)
        if softcap:
            s = softcap * torch.tanh(s / softcap)
        pos, j = n - Nq + torch.arange(Nq)[:, None], torch.arange(n)[None, :]
        ok = torch.ones(Nq, n, dtype=torch.bool)
        if causal:
            ok &= j <= pos
        if window:
            ok &= j > pos - window
        s = s.masked_fill(~ok, -np.inf)
        some = ok.any(1)
        lse[b][:, some] = torch.logsumexp(s[:, some], -1)
        out[b][some] = (torch.exp(s[:, some] - lse[b][:, some, None]) @ vb).transpose(0, 1)
    return out, lse


def test_references_tell_the_builds_apart():
    """Capped / uncapped (0.25) and windowed / unwindowed (W = 100) differ by >= 10 tolerances on every case of tests/test_gpu_d256.py."""
    from test_gpu_d256 import CASE_SEEDS, LENS, NCAP, inputs
    cases = [(H, Hkv, Nq, LENS[Nq]) for H, Hkv in ((2, 2), (8, 2)) for Nq in LENS] + [(4, 2, Nq, (200, 700)) for Nq in (129, 200)]
    for H, Hkv, Nq, lens in cases:
        q, k, v = inputs(CASE_SEEDS[0], 2, NCAP, H, Hkv, Nq)
        plain = reference(q, k, v, lens)
        for kw in (dict(softcap=0.25), dict(window=100)):
            other = reference(q, k, v, lens, **kw)
            assert (other[0] - plain[0]).abs().max() >= 10 * TOL and (other[1] - plain[1]).abs().max() >= 10 * TOL, (H, Nq, kw)


def test_d256_symbols_are_declared_exported_and_bound(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    assert f'#include "{HEADER}"' in open(os.path.join(ROOT, "include", "flash_attn_mi355x_decode.h")).read()
    protos = _prototypes(HEADER)
    assert sorted(protos) == sorted(built.D256_ABI)
    lib = built.decode()
    for sym, (res, args) in built.D256_ABI.items():
        ret, kinds = protos[sym]
        assert [_ctypes_kind(a) for a in args] == kinds and _ctypes_kind(res) == ret, sym
        assert getattr(lib, sym).argtypes == args and getattr(lib, sym).restype is res, sym
    # the attention calls have their family's _softcap prototype, the size queries the _window ones
    soft, win = _prototypes("flash_attn_mi355x_decode_softcap.h"), _prototypes("flash_attn_mi355x_decode_window.h")
    for f in ("decode", "extend"):
        assert protos[f"fa_mi355x_fwd_{f}_d256"] == soft[f"fa_mi355x_fwd_{f}_softcap"]
        assert protos[f"fa_mi355x_{f}_d256_splits"] == win[f"fa_mi355x_{f}_window_splits"]
        assert protos[f"fa_mi355x_{f}_d256_workspace_bytes"] == win[f"fa_mi355x_{f}_window_workspace_bytes"]
    for sym, params in built.KV_D256_PARAMS.items():
        assert len(params) == len(built.D256_ABI[sym][1]) and built.KV_CALL_PARAMS[sym] == params, sym


_ONE = 16
_GOOD = dict(q=_ONE, kn=_ONE, vn=_ONE, k=_ONE, v=_ONE, out=_ONE, lse=_ONE, lens=_ONE, table=_ONE, ws=_ONE, B=2, H=4, Hkv=2, Nq=100,
             Ncap=2048, num_pages=40, page_size=128, max_pages=16, d_new=256, d=256, layout=1, scale=0.0, causal=1, window=300, softcap=30.0,
             dtype=1)
BAD_ARG, UNSUPPORTED_D = 1, 2


def _call(lib, family, **over):
    a = dict(_GOOD, **over)
    ptrs = [ctypes.c_void_p(a[n]) for n in ("q", "kn", "vn", "k", "v", "out", "lse", "lens", "table", "ws")]
    sizes = [a[n] for n in ("B", "H", "Hkv", "Nq", "Ncap", "num_pages", "page_size", "max_pages", "d_new", "d", "layout")]
    if family == "append":
        rc = lib.fa_mi355x_append_d256(*ptrs[1:5], *ptrs[7:9], a["B"], a["Hkv"], *sizes[3:], a["dtype"], None)
    else:
        rc = getattr(lib, f"fa_mi355x_fwd_{family}_d256")(*ptrs, *sizes, a["scale"], a["causal"], a["window"], a["softcap"], a["dtype"], None)
    return rc, lib.fa_mi355x_decode_last_error().decode()


@pytest.mark.parametrize("family,over,code,msg", [
    ("decode", dict(Nq=3, d=128, d_new=128), UNSUPPORTED_D, "d = 256 exactly"), ("extend", dict(d=64, d_new=64), UNSUPPORTED_D, "d = 256 exactly"),
    ("append", dict(d=128, d_new=128), UNSUPPORTED_D, "d = 256 exactly"), ("extend", dict(d=512), UNSUPPORTED_D, "d = 256 exactly"),
    ("decode", dict(Nq=3, d_new=257), BAD_ARG, "d_new = 257"), ("extend", dict(d_new=264), BAD_ARG, "d_new = 264"),
    ("append", dict(d_new=0), BAD_ARG, "d_new = 0"),
    ("decode", dict(Nq=3, dtype=0), BAD_ARG, "bf16 alone"), ("extend", dict(dtype=0), BAD_ARG, "bf16 alone"),
    ("append", dict(dtype=0), BAD_ARG, "bf16 alone"),
    ("decode", dict(Nq=129), BAD_ARG, "Nq > 128"),
    ("decode", dict(Nq=3, page_size=192), BAD_ARG, "multiple of 128"), ("extend", dict(page_size=64), BAD_ARG, "multiple of 128"),
    ("append", dict(page_size=200), BAD_ARG, "multiple of 128"),
    ("extend", dict(softcap=-1.0), BAD_ARG, "softcap"), ("decode", dict(Nq=3, causal=0), BAD_ARG, "causal"),
    ("extend", dict(H=3), BAD_ARG, "multiple of Hkv"), ("decode", dict(Nq=3, q=0), BAD_ARG, "null"),
])
def test_d256_forms_reject_each_bad_argument_before_any_hip_call(built, family, over, code, msg):
    rc, err = _call(built.decode(), family, **over)
    assert rc == code and msg in err, (rc, err)


def _policy(family, B, H, Hkv, Nq, Ncap, window):
    rows, waves = (32, 4) if family == "decode" else (128, 2)
    span = Ncap if not window or window >= Ncap else min(Ncap, window + min(Nq, rows) - 1 + 127)
    groups = B * Hkv * -(-(H // Hkv) * Nq // rows)
    per = -(-span // max(1, -(-256 * waves // groups)))
    chunk = max(256, -(-per // 256) * 256)
    ns = -(-span // chunk)
    return ns, 0 if ns == 1 else B * H * ns * Nq * (256 + 2) * 4


@pytest.mark.parametrize("family", ["decode", "extend"])
def test_d256_size_queries_agree_with_the_policy(built, family):
    lib = built.decode()
    splits, nbytes = getattr(lib, f"fa_mi355x_{family}_d256_splits"), getattr(lib, f"fa_mi355x_{family}_d256_workspace_bytes")
    for B, H, Hkv, Nq, Ncap in ((2, 2, 2, 1, 768), (2, 8, 2, 33, 768), (2, 4, 2, 200, 768), (32, 32, 8, 1, 2048), (64, 8, 8, 3, 768), (1, 4, 2, 64, 256)):
        for W in (0, 100, Ncap):
            want = _policy(family, B, H, Hkv, Nq, Ncap, W)
            assert (splits(B, H, Hkv, Nq, Ncap, 256, 1, W), nbytes(B, H, Hkv, Nq, Ncap, 256, W)) == want, (B, H, Hkv, Nq, Ncap, W)
    assert splits(2, 2, 2, 1, 768, 128, 1, 0) == 0 and nbytes(2, 2, 2, 1, 768, 128, 0) == 0 and splits(2, 3, 2, 1, 768, 256, 1, 0) == 0


def test_device_ops_refuses_by_name_what_is_not_built_at_256_and_picks_the_d256_symbols(built):
    from flash_attention_minitorch_amd import device_ops as ops
    q, kc = torch.zeros(2, 1, 4, 256, dtype=torch.bfloat16), torch.zeros(2, 512, 2, 256, dtype=torch.bfloat16)
    tab = torch.zeros(64, 8, dtype=torch.float32)
    for kw, msg in ((dict(window=8, sink=2), "sink tokens at head dim 256"), (dict(sink_logits=torch.zeros(4)), "sink_logits at head dim 256"),
                    (dict(rotary_cos=tab, rotary_sin=tab), "rotary keywords at head dim 256")):
        for attend in (ops.flash_attn_decode, ops.flash_attn_extend):
            with pytest.raises(ValueError, match=msg):
                attend(q, kc, kc, **kw)
    with pytest.raises(ValueError, match="float32 cache at head dim 256"):
        ops.flash_attn_decode(q.float(), kc.float(), kc.float())
    with pytest.raises(ValueError, match="fp8 .* cache at head dim 256"):
        ops.flash_attn_extend(q, kc.to(torch.float8_e4m3fn), kc.to(torch.float8_e4m3fn))
    with pytest.raises(ValueError, match="fp8 .* cache at head dim 256"):
        ops.decode_append(kc[:, :1], kc[:, :1], kc.to(torch.float8_e4m3fn), kc.to(torch.float8_e4m3fn))
    cu = torch.tensor([0, 1, 2], dtype=torch.int32)
    with pytest.raises(ValueError, match="flash_attn_ragged and ragged_append at head dim 256"):
        ops.flash_attn_ragged(q[:, 0], kc, kc, cu)
    for name in ("decode", "extend"):
        fam = ops._KV_FAMILIES[name]
        assert ops._kv_symbol(fam, "attend", True, True, 5, None, False, False, 0.5, False, True) == f"fa_mi355x_fwd_{name}_d256"
        assert ops._kv_symbol(fam, "append", d256=True) == "fa_mi355x_append_d256"
        assert ops._kv_symbol(fam, "size", d256=True) == f"fa_mi355x_{name}_d256_workspace_bytes"
        assert ops._kv_symbol(fam, "attend", True, True) == f"fa_mi355x_fwd_{name}_append_paged"
    assert ops._kv_symbol(ops._KV_FAMILIES["decode"], "attend", ungrouped=True) == "fa_mi355x_fwd_decode"
    assert ops.decode_workspace(q, kc) is not None and ops.decode_workspace(q, kc[:, :256]) is None   # (two splits of 256 keys; one)
