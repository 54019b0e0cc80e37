"""CPU-side checks of device_ops' Python call path: what every public entry point sends to the C libraries, what it returns, and
which arguments it rejects with which message.  No GPU and no built library: the tensors live on the CPU with ``is_cuda`` patched
to True, and ``_lib.core()`` / ``_lib.decode()`` are replaced by a recorder that logs every C call.  Pointers are logged by name:
the caller's tensors by their own names, the rest by order of first use within one public call (new0, new1, ...); every tensor whose
address is taken is kept alive until the next public call, so no address stands for two tensors."""
import ctypes
import math

import pytest
import torch

from flash_attention_minitorch_amd import _lib, device_ops as dev, modules_transformer as mt

F32, BF16 = torch.float32, torch.bfloat16
FA1, FA2 = _lib.FA_VARIANT_FA1, _lib.FA_VARIANT_FA2
GUARD_BYTES = 2048


class Recorder:
    """Stands in for both ctypes handles: every attribute is a C function that logs (symbol, arguments) and returns 0, or a size
    for the *_bytes queries."""

    def __init__(self):
        self.calls, self.names, self.alive = [], {}, []

    def reset(self, named):
        self.calls, self.alive = [], []
        self.names = {t.data_ptr(): n for n, t in named.items() if isinstance(t, torch.Tensor)}

    def name(self, ptr):
        if not ptr:
            return "null"
        if ptr not in self.names:
            self.names[ptr] = f"new{sum(n.startswith('new') for n in self.names.values())}"
        return self.names[ptr]

    def arg(self, a):
        if a is None:
            return "null"
        if isinstance(a, ctypes.c_void_p):
            return self.name(a.value)
        if isinstance(a, int) and a >= 1 << 32:   # an address passed as a plain int (no size or seed is this large)
            return self.name(a)
        if isinstance(a, ctypes.Array):
            return "[" + ",".join(str(x) for x in a) + "]"
        if isinstance(a, type(ctypes.byref(ctypes.c_int()))):
            return "&int"
        if isinstance(a, float):
            return repr(a)
        return str(int(a))

    def __getattr__(self, sym):
        def fn(*args):
            self.calls.append(f"{sym}({','.join(self.arg(a) for a in args)})")
            if sym == "fa_mi355x_guard_bytes":
                return GUARD_BYTES
            if sym == "fa_mi355x_bwd_workspace_bytes_ex":
                return 12 * args[0] * args[1]
            if sym == "fa_mi355x_decode_workspace_bytes":
                B, H, Nq, Ncap, d = args
                return 0 if Ncap < 1024 else B * H * 4 * Nq * (d + 2) * 4
            return 0
        return fn


def install_recorder(monkeypatch):
    r = Recorder()
    data_ptr = torch.Tensor.data_ptr

    def kept_data_ptr(t):   # every tensor whose address is taken lives until the next call: no address is reused
        r.alive.append(t)
        return data_ptr(t)
    monkeypatch.setattr(torch.Tensor, "data_ptr", kept_data_ptr)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: not getattr(self, "on_cpu", False)))
    monkeypatch.setattr(dev, "_stream_ptr", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(_lib, "core", lambda: r)
    monkeypatch.setattr(_lib, "decode", lambda: r)
    monkeypatch.setattr(_lib, "guard_elems", lambda: GUARD_BYTES // 4, raising=False)
    return r


@pytest.fixture
def rec(monkeypatch):
    return install_recorder(monkeypatch)


def _t(*shape, dtype=F32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(len(shape) + shape[-1])).to(dtype)


def _qkv(shape, dtype=F32, names="q k v do"):
    return {n: _t(*shape, dtype=dtype) for n in names.split()}


def _fwd(shape, dtype=F32, **kw):
    return _qkv(shape, dtype, "q k v"), lambda a: dev.flash_attn_fwd(a["q"], a["k"], a["v"], **kw)


def _bwd(shape, dtype=F32, **kw):
    a = _qkv(shape, dtype)
    a.update(o=_t(*shape), l=_t(*shape[:-1]), m=_t(*shape[:-1]))
    return a, lambda a: dev.flash_attn_bwd(a["q"], a["k"], a["v"], a["o"], a["do"], a["l"], **kw)


def _autograd(fn, shape, dtype):
    def run(a):
        q, k, v = (a[n].clone().requires_grad_() for n in "qkv")
        a.update(qg=q, kg=k, vg=v)
        o = fn(q, k, v)
        o.sum().backward()
        return o, q.grad, k.grad, v.grad
    return _qkv(shape, dtype, "q k v"), run


def _mha(shape, dtype=BF16, **kw):
    B, N, E, H = shape
    a = dict(x=_t(B, N, E, dtype=dtype), wq=_t(E, E, dtype=dtype), wk=_t(E, E, dtype=dtype), wv=_t(E, E, dtype=dtype),
             wo=_t(E, E, dtype=dtype))

    def run(a):
        x = a["x"].clone().requires_grad_()
        y = mt.multi_head_attention(x, a["wq"], a["wk"], a["wv"], a["wo"], H, **kw)
        y.sum().backward()
        return y, x.grad
    return a, run


def _kv_cache(d, steps):
    B, P, H, cap = 2, 16, 2, 64
    a = dict(x=_t(B, P, H * d, dtype=BF16), x1=_t(B, 1, H * d, dtype=BF16), w=_t(H * d, H * d, dtype=BF16))

    def run(a):
        cache = mt.KVCache(2, B, cap, H, d, BF16, a["x"].device)
        w = a["w"]
        layers = [(w, w, w, w)] * 2
        y = mt.attention_stack_prefill(a["x"], layers, H, cache)
        for _ in range(steps):
            y = mt.attention_stack_step(a["x1"], layers, H, cache)
        return y, cache.k[0], cache.lengths
    return a, run


def _decode(layout, d, dp, Ncap, dtype=BF16, **kw):
    B, H, Nq = 2, 3, 4
    qs, cs = ((B, Nq, H, d), (B, Ncap, H, dp)) if layout == "bnhd" else ((B, H, Nq, d), (B, H, Ncap, dp))
    a = dict(q=_t(*qs, dtype=dtype), kc=_t(*cs, dtype=dtype), vc=_t(*cs, dtype=dtype))
    for n, v in list(kw.items()):
        if v == "T":
            kw[n] = a[n] = {"cache_seqlens": torch.full((B,), 7, dtype=torch.int32), "out": _t(*qs), "lse": _t(B, H, Nq),
                            "workspace": torch.empty(B * H * 4 * Nq * (dp + 2))}[n]
    return a, lambda a: dev.flash_attn_decode(a["q"], a["kc"], a["vc"], layout=layout, **kw)


def _guard():
    return torch.empty(GUARD_BYTES // 4)


S4, S3 = (2, 3, 16, 64), (6, 16, 64)
CALLS = {
    # flash_attn_fwd
    "fwd_f32_4d_d64": lambda: _fwd(S4),
    "fwd_bf16_4d_d64_causal": lambda: _fwd(S4, BF16, causal=True),
    "fwd_bf16_3d_d128_fa1": lambda: _fwd((6, 16, 128), BF16, variant=FA1),
    "fwd_bf16_d32": lambda: _fwd((2, 3, 16, 32), BF16),
    "fwd_f32_3d_d64_fa1_causal": lambda: _fwd(S3, causal=True, variant=FA1),
    "fwd_bf16_d34_padded_fa1": lambda: _fwd((2, 3, 16, 34), BF16, variant=FA1),
    "fwd_f32_3d_d34_padded": lambda: _fwd((6, 16, 34)),
    "fwd_bf16_opts_phased": lambda: _fwd(S4, BF16, opts=dev.OPTS_PHASED),
    "fwd_bf16_opts_exact": lambda: _fwd(S4, BF16, opts=dev.OPTS_EXACT_SCALE),
    "fwd_bf16_opts_folded": lambda: _fwd(S4, BF16, opts=dev.OPTS_FOLDED_SCALE),
    "fwd_bf16_out_bf16": lambda: _fwd(S4, BF16, out_dtype=BF16),
    "fwd_bf16_out_bf16_opts": lambda: _fwd(S4, BF16, out_dtype=BF16, opts=dev.OPTS_PHASED),
    "fwd_bf16_out_bf16_long_opts": lambda: _fwd(S4, BF16, out_dtype=BF16, opts=(0,) * 11),
    "fwd_bf16_guard_none": lambda: _fwd(S4, BF16, guard=None),
    "fwd_f32_guard_none_produce": lambda: _fwd(S4, guard=None, produce_guard=True),
}


def _add(name, make):
    CALLS[name] = make


def _fwd_caller(shape, dtype, variant, **names):
    def make():
        a = _qkv(shape, dtype, "q k v")
        lead, N = shape[:-2], shape[-2]
        kw = {}
        for n, v in names.items():
            stats = (math.prod(lead) * N,) if v == "flat" else lead + (N,)   # (a flat view works as well)
            kw[n] = a[n] = {"out": lambda: torch.empty(shape, dtype=v), "l": lambda: torch.empty(stats),
                            "m": lambda: torch.empty(stats), "guard": _guard}[n]()
        if "guard" in names and names["guard"] == "produce":
            kw["produce_guard"] = True
        return a, lambda a: dev.flash_attn_fwd(a["q"], a["k"], a["v"], variant=variant, **kw)
    return make


_add("fwd_caller_out_l_m_fa1", _fwd_caller(S4, BF16, FA1, out=F32, l=1, m=1))
_add("fwd_caller_l_only", _fwd_caller(S3, F32, FA2, l=1))
_add("fwd_caller_flat_l_m", _fwd_caller(S4, BF16, FA1, l="flat", m="flat"))
_add("fwd_caller_guard_read", _fwd_caller(S4, BF16, FA2, guard="read"))
_add("fwd_caller_guard_produce", _fwd_caller(S4, BF16, FA2, guard="produce"))
_add("fwd_caller_padded_out_l_m", _fwd_caller((2, 3, 16, 34), F32, FA1, out=F32, l=1, m=1))
CALLS.update({
    # flash_attn_bwd
    "bwd_f32_4d_d64": lambda: _bwd(S4),
    "bwd_bf16_4d_d64_causal": lambda: _bwd(S4, BF16, causal=True),
    "bwd_bf16_3d_d128_fa1": lambda: _bwd((6, 16, 128), BF16, variant=FA1),
    "bwd_bf16_d32": lambda: _bwd((2, 3, 16, 32), BF16),
    "bwd_bf16_d34_padded": lambda: _bwd((2, 3, 16, 34), BF16, causal=True),
    "bwd_f32_3d_d34_padded_fa1": lambda: _bwd((6, 16, 34), variant=FA1),
    "bwd_bf16_opts": lambda: _bwd(S4, BF16, opts=dev.OPTS_PHASED),
    "bwd_bf16_opts_exact": lambda: _bwd(S4, BF16, opts=dev.OPTS_EXACT_SCALE),
    "bwd_bf16_stages": lambda: _bwd(S4, BF16, stages=dev.STAGE_DKDV),
    "bwd_bf16_guard_none": lambda: _bwd(S4, BF16, guard=None),
})


def _bwd_caller(shape, dtype, **names):
    def make():
        a, _ = _bwd(shape, dtype)
        kw = {}
        if "workspace" in names:
            kw["workspace"] = a["ws"] = torch.empty(3 * math.prod(shape[:-1]) + 5)
        if "grads" in names:
            kw["grads"] = tuple(a.setdefault(n, torch.empty(shape)) for n in ("dq", "dk", "dv"))
        if "guard" in names:
            kw["guard"] = a["g"] = _guard()
        if "m" in names:
            kw.update(m=a["m"], variant=FA1)
        return a, lambda a: dev.flash_attn_bwd(a["q"], a["k"], a["v"], a["o"], a["do"], a["l"], **kw)
    return make


_add("bwd_caller_ws_grads_guard", _bwd_caller(S4, BF16, workspace=1, grads=1, guard=1))
_add("bwd_caller_grads_m", _bwd_caller(S3, F32, grads=1, m=1))
_add("bwd_caller_padded_grads", _bwd_caller((2, 3, 16, 34), F32, grads=1, m=1))


def _bnhd(shape, dtype, variant=FA2, fwd_kw=(), bwd_kw=()):
    def make():
        B, N, H, d = shape
        a = _qkv(shape, dtype)
        a.update(o=_t(*shape), l=_t(B, H, N), m=_t(B, H, N) if variant == FA1 else None)
        fk, bk = dict(fwd_kw), dict(bwd_kw)
        for kw in (fk, bk):
            if kw.get("guard") == "T":
                kw["guard"] = a["g"] = _guard()

        def run(a):
            r1 = dev.flash_attn_fwd_bnhd(a["q"], a["k"], a["v"], variant=variant, **fk)
            r2 = dev.flash_attn_bwd_bnhd(a["q"], a["k"], a["v"], a["o"], a["do"], a["l"], a["m"], variant=variant, **bk)
            return r1 + r2
        return a, run
    return make


_add("bnhd_f32", _bnhd((2, 16, 3, 64), F32))
_add("bnhd_bf16_causal", _bnhd((2, 16, 3, 64), BF16, fwd_kw=dict(causal=True), bwd_kw=dict(causal=True)))
_add("bnhd_bf16_fa1_d128", _bnhd((2, 16, 3, 128), BF16, FA1))
_add("bnhd_bf16_scale", _bnhd((2, 16, 3, 64), BF16, fwd_kw=dict(softmax_scale=0.6931471805599453),
                              bwd_kw=dict(softmax_scale=0.6931471805599453)))
_add("bnhd_bf16_opts", _bnhd((2, 16, 3, 64), BF16, fwd_kw=dict(opts=dev.OPTS_EXACT_SCALE), bwd_kw=dict(opts=dev.OPTS_PHASED)))
_add("bnhd_bf16_guards", _bnhd((2, 16, 3, 64), BF16, fwd_kw=dict(guard="T", produce_guard=True), bwd_kw=dict(guard="T")))
_add("bnhd_bf16_guard_none", _bnhd((2, 16, 3, 64), BF16, fwd_kw=dict(guard=None), bwd_kw=dict(guard=None)))
_add("bnhd_bf16_guard_read", _bnhd((2, 16, 3, 64), BF16, fwd_kw=dict(guard="T")))


def _masked(dtype, variant, causal, mask=True, dropout=False):
    def make():
        B, H, N, d = S4
        a = _qkv(S4, dtype)
        a.update(o=_t(*S4), l=_t(B, H, N), m=_t(B, H, N), km=_t(B, N) if mask else None)

        def run(a):
            q, k, v = a["q"], a["k"], a["v"]
            if dropout:
                r1 = dev.flash_attn_fwd_dropout(q, k, v, 0.25, -3, 1.5, a["km"], causal, variant)
                r2 = dev.flash_attn_bwd_dropout(q, k, v, a["o"], a["do"], a["l"], a["m"], 0.25, -3, 1.5, a["km"], causal, variant)
            else:
                r1 = dev.flash_attn_fwd_masked(q, k, v, a["km"], causal, variant)
                r2 = dev.flash_attn_bwd_masked(q, k, v, a["o"], a["do"], a["l"], a["m"], a["km"], causal, variant)
            return r1 + r2
        return a, run
    return make


_add("masked_f32_fa2", _masked(F32, FA2, False))
_add("masked_bf16_fa1_causal", _masked(BF16, FA1, True))
_add("dropout_bf16_mask", _masked(BF16, FA2, True, dropout=True))
_add("dropout_f32_fa1_nomask", _masked(F32, FA1, False, mask=False, dropout=True))


def _helpers():
    a = _qkv(S4, BF16, "q k")
    a.update(g=_guard(), ws=torch.empty(100))

    def run(a):
        q, k = a["q"], a["k"]
        return (dev.bwd_workspace(q), dev.bwd_workspace(q, dev.OPTS_PHASED), dev.bwd_workspace(_t(6, 16, 34)), dev.bwd_status(a["ws"], q),
                dev.new_guard(q), dev.new_guard(q, dev.OPTS_EXACT_SCALE), dev.new_guard(q.float()), dev.new_guard(_t(6, 16, 32, dtype=BF16)),
                dev.scale_guard(q, k), dev.scale_guard(q, k, out=a["g"]), dev.pick_opts(q, k), dev.pick_opts(q.float(), k.float()),
                dev.pick_opts(q * 8, k * 8))
    return a, run


_add("helpers", _helpers)
CALLS.update({
    "autograd_flash_attn_bf16": lambda: _autograd(dev.flash_attn, S4, BF16),
    "autograd_flash_attn2_bf16_causal": lambda: _autograd(lambda q, k, v: dev.flash_attn2(q, k, v, True), S4, BF16),
    "autograd_flash_attn_causal_f32": lambda: _autograd(dev.flash_attn_causal, S3, F32),
    "autograd_flash_attn2_d34": lambda: _autograd(dev.flash_attn2, (2, 3, 16, 34), BF16),
    "autograd_flash_attn2_d32": lambda: _autograd(dev.flash_attn2, (2, 3, 16, 32), BF16),
    "mha_fused": lambda: _mha((2, 16, 128, 2)),
    "mha_fused_f32": lambda: _mha((2, 16, 128, 2), F32),
    "mha_fused_fold": lambda: _mha((2, 16, 128, 2), fold_scale=True),
    "mha_unfused_noncausal": lambda: _mha((2, 16, 128, 2), causal=False, fused_layout=False),
    "kv_cache_d64": lambda: _kv_cache(64, 2),
    "kv_cache_d48": lambda: _kv_cache(48, 1),
    "decode_bnhd": lambda: _decode("bnhd", 64, 64, 256),
    "decode_bhnd_f32_split": lambda: _decode("bhnd", 128, 128, 2048, F32, causal=False),
    "decode_bnhd_padded": lambda: _decode("bnhd", 48, 64, 256, cache_seqlens="T"),
    "decode_bhnd_padded_caller": lambda: _decode("bhnd", 20, 32, 2048, out="T", lse="T", workspace="T"),
    "decode_bnhd_caller_scale": lambda: _decode("bnhd", 32, 32, 1024, softmax_scale=0.5, out="T", lse="T", cache_seqlens="T"),
    "decode_workspace": lambda: ({"q": _t(2, 4, 3, 64), "kc": _t(2, 2048, 3, 64)},
                                 lambda a: (dev.decode_workspace(a["q"], a["kc"]), dev.decode_workspace(a["q"], a["kc"][:, :16].contiguous()))),
})


def _describe(rec, r):
    if isinstance(r, (tuple, list)):
        return "(" + ",".join(_describe(rec, x) for x in r) + ")"
    if isinstance(r, torch.Tensor):
        name = rec.names.get(r.data_ptr(), "fresh") if r.numel() else "empty"
        return f"{name}:{str(r.dtype)[6:]}{list(r.shape)}"
    return repr(r)


def run_call(rec, name):
    named, fn = CALLS[name]()
    rec.reset(named)
    r = fn(named)
    return rec.calls + ["-> " + _describe(rec, r)]


def _err_args(shape, dtype):
    bnhd = len(shape) == 4 and shape[2] == 3
    B, N = shape[0], shape[1] if bnhd else shape[-2]
    stats = (B, 3, N) if len(shape) == 4 else shape[:-1]
    a = _qkv(shape, dtype)
    a.update(o=_t(*shape), l=_t(*stats), m=_t(*stats), km=_t(B, N), kw={})
    return a


_ERR_CALLS = {
    "fwd": lambda a: dev.flash_attn_fwd(a["q"], a["k"], a["v"], **a["kw"]),
    "bwd": lambda a: dev.flash_attn_bwd(a["q"], a["k"], a["v"], a["o"], a["do"], a["l"], **a["kw"]),
    "fwd_bnhd": lambda a: dev.flash_attn_fwd_bnhd(a["q"], a["k"], a["v"], **a["kw"]),
    "bwd_bnhd": lambda a: dev.flash_attn_bwd_bnhd(a["q"], a["k"], a["v"], a["o"], a["do"], a["l"], **a["kw"]),
    "fwd_masked": lambda a: dev.flash_attn_fwd_masked(a["q"], a["k"], a["v"], a["km"], **a["kw"]),
    "bwd_masked": lambda a: dev.flash_attn_bwd_masked(a["q"], a["k"], a["v"], a["o"], a["do"], a["l"], a["m"], a["km"], **a["kw"]),
    "fwd_dropout": lambda a: dev.flash_attn_fwd_dropout(a["q"], a["k"], a["v"], 0.1, 1, key_mask=a["km"], **a["kw"]),
    "bwd_dropout": lambda a: dev.flash_attn_bwd_dropout(a["q"], a["k"], a["v"], a["o"], a["do"], a["l"], a["m"], 0.1, 1,
                                                        key_mask=a["km"], **a["kw"]),
    "scale_guard": lambda a: dev.scale_guard(a["q"], a["k"], **a["kw"]),
}


def _cpu(t):
    t.on_cpu = True
    return t


def _set(kw=(), **over):
    """A case's change to the arguments: a standard tensor's name -> function of that tensor; any other name, or a name in ``kw``, ->
    a keyword argument (a function of the standard tensors, or the value)."""
    def mod(a):
        for n, f in over.items():
            if n in kw or n not in a:
                a["kw"][n] = f(a) if callable(f) else f
            else:
                a[n] = f(a[n])
    return mod


_small = lambda t: t.flatten()[:-1].clone()
_f64 = lambda t: t.double()
_nc = lambda t: t.transpose(-1, -2).contiguous().transpose(-1, -2)
_short = lambda t: t[..., :8, :].contiguous()
BNHD = (2, 16, 3, 64)
# (function, shape, dtype, change)
ERRORS = {
    "fwd_cpu": ("fwd", S4, BF16, _set(q=_cpu)),
    "fwd_f64": ("fwd", S4, F32, _set(q=_f64, k=_f64, v=_f64)),
    "fwd_f16": ("fwd", S4, torch.float16, _set()),
    "fwd_shape_k": ("fwd", S4, BF16, _set(k=_short)),
    "fwd_dtype_v": ("fwd", S4, BF16, _set(v=lambda t: t.float())),
    "fwd_noncontig_q": ("fwd", S4, BF16, _set(q=_nc)),
    "fwd_2d": ("fwd", (16, 64), BF16, _set()),
    "fwd_5d": ("fwd", (1, 2, 3, 16, 64), BF16, _set()),
    "fwd_d160": ("fwd", (2, 3, 16, 160), BF16, _set()),
    "fwd_d160_3d": ("fwd", (6, 16, 160), F32, _set()),
    "fwd_d34_opts": ("fwd", (2, 3, 16, 34), BF16, _set(opts=dev.OPTS_PHASED)),
    "fwd_d34_out_bf16": ("fwd", (2, 3, 16, 34), BF16, _set(out_dtype=BF16)),
    "fwd_out_dtype_f16": ("fwd", S4, BF16, _set(out_dtype=torch.float16)),
    "fwd_out_shape": ("fwd", S4, BF16, _set(out=lambda a: torch.empty(6, 16, 64))),
    "fwd_out_dtype": ("fwd", S4, BF16, _set(out=lambda a: torch.empty(S4, dtype=BF16))),
    "fwd_out_noncontig": ("fwd", S4, BF16, _set(out=lambda a: _nc(torch.empty(S4)))),
    "fwd_cpu_and_f64": ("fwd", S4, F32, _set(q=lambda t: _cpu(t.double()))),
    "fwd_f64_and_shape": ("fwd", S4, F32, _set(q=_f64, k=_short)),
    "fwd_shape_and_noncontig": ("fwd", S4, BF16, _set(k=_short, v=_nc)),
    "fwd_d160_and_opts": ("fwd", (2, 3, 16, 160), BF16, _set(opts=dev.OPTS_PHASED)),
    "bwd_cpu": ("bwd", S4, BF16, _set(q=_cpu)),
    "bwd_f64": ("bwd", S4, F32, _set(q=_f64, k=_f64, v=_f64, do=_f64)),
    "bwd_shape_do": ("bwd", S4, BF16, _set(do=_short)),
    "bwd_dtype_do": ("bwd", S4, BF16, _set(do=lambda t: t.float())),
    "bwd_noncontig_do": ("bwd", S4, BF16, _set(do=_nc)),
    "bwd_out_bf16": ("bwd", S4, BF16, _set(o=lambda t: t.bfloat16())),
    "bwd_out_shape": ("bwd", S4, BF16, _set(o=_short)),
    "bwd_out_noncontig": ("bwd", S4, BF16, _set(o=_nc)),
    "bwd_d160": ("bwd", (2, 3, 16, 160), BF16, _set()),
    "bwd_d34_opts": ("bwd", (2, 3, 16, 34), BF16, _set(opts=dev.OPTS_PHASED)),
    "bwd_d34_stages": ("bwd", (2, 3, 16, 34), BF16, _set(stages=dev.STAGE_DQ)),
    "bwd_d34_workspace": ("bwd", (2, 3, 16, 34), BF16, _set(workspace=lambda a: torch.empty(1000))),
    "bwd_workspace_small": ("bwd", S4, BF16, _set(workspace=lambda a: torch.empty(3 * 96 - 1))),
    "bwd_workspace_small_opts": ("bwd", S4, BF16, _set(workspace=lambda a: torch.empty(3 * 96 - 1), opts=dev.OPTS_PHASED)),
    "bwd_out_bf16_and_shape_do": ("bwd", S4, BF16, _set(o=lambda t: t.bfloat16(), do=_short)),
    "bwd_out_bf16_and_workspace": ("bwd", S4, BF16, _set(o=lambda t: t.bfloat16(), workspace=lambda a: torch.empty(1))),
    "fwd_bnhd_3d": ("fwd_bnhd", (6, 16, 64), BF16, _set()),
    "fwd_bnhd_cpu": ("fwd_bnhd", BNHD, BF16, _set(v=_cpu)),
    "fwd_bnhd_shape": ("fwd_bnhd", BNHD, BF16, _set(k=lambda t: t[:, :8].contiguous())),
    "fwd_bnhd_dtype": ("fwd_bnhd", BNHD, BF16, _set(k=lambda t: t.float())),
    "fwd_bnhd_noncontig": ("fwd_bnhd", BNHD, BF16, _set(q=_nc)),
    "fwd_bnhd_3d_and_cpu": ("fwd_bnhd", (6, 16, 64), BF16, _set(q=_cpu)),
    "fwd_masked_cpu": ("fwd_masked", S4, BF16, _set(q=_cpu)),
    "fwd_masked_3d": ("fwd_masked", (6, 16, 64), BF16, _set()),
    "fwd_masked_shape": ("fwd_masked", S4, BF16, _set(v=_short)),
    "fwd_masked_mask_shape": ("fwd_masked", S4, BF16, _set(km=lambda t: t[:, :8].contiguous())),
    "fwd_masked_mask_dtype": ("fwd_masked", S4, BF16, _set(km=lambda t: t.bfloat16())),
    "fwd_masked_mask_cpu": ("fwd_masked", S4, BF16, _set(km=_cpu)),
    "fwd_masked_mask_noncontig": ("fwd_masked", S4, BF16, _set(km=lambda t: torch.empty(16, 2).t())),
    "fwd_masked_no_mask_cpu": ("fwd_masked", S4, BF16, _set(q=_cpu, km=lambda t: None)),
    "bwd_masked_no_mask_3d": ("bwd_masked", (6, 16, 64), BF16, _set(km=lambda t: None)),
    "fwd_masked_f64_and_mask": ("fwd_masked", S4, F32, _set(q=_f64, k=_f64, v=_f64, km=_f64)),
    "bwd_masked_shape_do": ("bwd_masked", S4, BF16, _set(do=_short)),
    "bwd_masked_mask_shape": ("bwd_masked", S4, BF16, _set(km=lambda t: t[:1].contiguous())),
    "bwd_masked_3d": ("bwd_masked", (6, 16, 64), BF16, _set()),
    "fwd_dropout_3d_nomask": ("fwd_dropout", (6, 16, 64), BF16, _set(km=lambda t: None)),
    "fwd_dropout_3d": ("fwd_dropout", (6, 16, 64), BF16, _set()),
    "fwd_dropout_mask_dtype": ("fwd_dropout", S4, BF16, _set(km=_f64)),
    "fwd_dropout_cpu": ("fwd_dropout", S4, BF16, _set(q=_cpu)),
    "bwd_dropout_mask_shape": ("bwd_dropout", S4, BF16, _set(km=lambda t: t[:, :8].contiguous())),
    "bwd_dropout_noncontig_do": ("bwd_dropout", S4, BF16, _set(do=_nc)),
    "bwd_dropout_3d": ("bwd_dropout", (6, 16, 64), BF16, _set()),
    "scale_guard_dtype": ("scale_guard", S4, BF16, _set(k=lambda t: t.float())),
    "scale_guard_rows": ("scale_guard", S4, BF16, _set(k=_short)),
    "scale_guard_row_length": ("scale_guard", S4, BF16, _set(k=lambda t: t[..., :32].contiguous())),
    "scale_guard_cpu": ("scale_guard", S4, BF16, _set(q=_cpu)),
    "scale_guard_noncontig": ("scale_guard", S4, BF16, _set(k=_nc)),
    # where earlier versions failed by accident (KeyError, AttributeError, an unpacking error) or let the kernels read or write past a
    # buffer's end: these are rejected up front now
    "fwd_bnhd_f64": ("fwd_bnhd", BNHD, F32, _set(q=_f64, k=_f64, v=_f64)),
    "bwd_bnhd_cpu": ("bwd_bnhd", BNHD, BF16, _set(q=_cpu)),
    "bwd_bnhd_f64": ("bwd_bnhd", BNHD, F32, _set(q=_f64, k=_f64, v=_f64, do=_f64)),
    "bwd_bnhd_shape_do": ("bwd_bnhd", BNHD, BF16, _set(do=lambda t: t[:, :8].contiguous())),
    "bwd_bnhd_out_bf16": ("bwd_bnhd", BNHD, BF16, _set(o=lambda t: t.bfloat16())),
    "bwd_bnhd_l_small": ("bwd_bnhd", BNHD, BF16, _set(l=_small)),
    "fwd_l_small": ("fwd", S4, BF16, _set(kw="lm", l=lambda a: torch.empty(95))),
    "fwd_m_small": ("fwd", S4, BF16, _set(kw="lm", variant=FA1, m=lambda a: torch.empty(2, 3, 15))),
    "fwd_l_f64": ("fwd", S4, BF16, _set(kw="lm", l=lambda a: torch.empty(2, 3, 16, dtype=torch.float64))),
    "fwd_l_noncontig": ("fwd", S4, BF16, _set(kw="lm", l=lambda a: torch.empty(16, 6).t())),
    "fwd_padded_l_small": ("fwd", (2, 3, 16, 34), BF16, _set(kw="lm", l=lambda a: torch.empty(10))),
    "fwd_guard_small": ("fwd", S4, BF16, _set(guard=lambda a: torch.empty(8), produce_guard=True)),
    "fwd_guard_bf16": ("fwd", S4, BF16, _set(guard=lambda a: torch.empty(GUARD_BYTES // 4, dtype=BF16))),
    "bwd_l_small": ("bwd", S4, BF16, _set(l=_small)),
    "bwd_m_small": ("bwd", S4, BF16, _set(kw="lm", variant=FA1, m=lambda a: torch.empty(3))),
    "bwd_grads_small": ("bwd", S4, BF16, _set(grads=lambda a: (torch.empty(S4), torch.empty(S4), torch.empty(10)))),
    "bwd_grads_bf16": ("bwd", S4, BF16, _set(grads=lambda a: tuple(torch.empty(S4, dtype=BF16) for _ in range(3)))),
    "bwd_guard_small": ("bwd", S4, BF16, _set(guard=lambda a: torch.empty(1))),
    "bwd_workspace_expanded": ("bwd", S4, BF16, _set(workspace=lambda a: torch.empty(1).expand(1000))),
    "fwd_masked_no_mask": ("fwd_masked", S4, BF16, _set(km=lambda t: None)),
    "bwd_masked_out_bf16": ("bwd_masked", S4, BF16, _set(o=lambda t: t.bfloat16())),
    "bwd_masked_m_small": ("bwd_masked", S4, BF16, _set(m=_small)),
    "bwd_dropout_l_small": ("bwd_dropout", S4, BF16, _set(l=_small)),
    "bwd_dropout_3d_nomask": ("bwd_dropout", (6, 16, 64), BF16, _set(km=lambda t: None)),
    "scale_guard_f64": ("scale_guard", S4, F32, _set(q=_f64, k=_f64)),
    "scale_guard_out_small": ("scale_guard", S4, BF16, _set(out=lambda a: torch.empty(4))),
}


def run_error(rec, name):
    fn, shape, dtype, mod = ERRORS[name]
    a = _err_args(shape, dtype)
    mod(a)
    rec.reset(a)
    try:
        _ERR_CALLS[fn](a)
    except Exception as e:
        return f"{type(e).__name__}: {e}"
    return "ok: " + ";".join(rec.calls)


# Recorded on the commit before the call path was consolidated, and unchanged by it, but for the cases below "where earlier versions
# failed" (which passed or raised KeyError / AttributeError / an unpacking error there).
EXPECTED_TRACES = {
    'autograd_flash_attn2_bf16_causal': [
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(new0,new1,new2,new3,new4,null,6,1,16,64,0,0.0,1,2,1,null,0,new5,1,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_guarded(new0,new1,new2,new3,new6,new7,new8,new9,new4,null,new10,6,1,16,64,0,0.0,1,2,1,7,null,0,new5,null)',
        '-> (new3:float32[2, 3, 16, 64],fresh:bfloat16[2, 3, 16, 64],fresh:bfloat16[2, 3, 16, 64],fresh:bfloat16[2, 3, 16, 64])',
    ],
    'autograd_flash_attn2_d32': [
        'fa_mi355x_fwd_guarded(new0,new1,new2,new3,new4,null,6,1,16,32,0,0.0,0,2,1,null,0,null,0,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,32,null,0)',
        'fa_mi355x_bwd_guarded(new0,new1,new2,new3,new5,new6,new7,new8,new4,null,new9,6,1,16,32,0,0.0,0,2,1,7,null,0,null,null)',
        '-> (new3:float32[2, 3, 16, 32],fresh:bfloat16[2, 3, 16, 32],fresh:bfloat16[2, 3, 16, 32],fresh:bfloat16[2, 3, 16, 32])',
    ],
    'autograd_flash_attn2_d34': [
        'fa_mi355x_fwd_padded(new0,new1,new2,new3,new4,null,6,16,34,64,0,2,1,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_padded(new5,new6,new7,new8,new9,new10,new11,new12,new4,null,new13,6,16,34,64,0,2,1,null)',
        '-> (fresh:float32[2, 3, 16, 34],fresh:bfloat16[2, 3, 16, 34],fresh:bfloat16[2, 3, 16, 34],fresh:bfloat16[2, 3, 16, 34])',
    ],
    'autograd_flash_attn_bf16': [
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(new0,new1,new2,new3,new4,new5,6,1,16,64,0,0.0,0,1,1,null,0,new6,1,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_guarded(new0,new1,new2,new3,new7,new8,new9,new10,new4,new5,new11,6,1,16,64,0,0.0,0,1,1,7,null,0,new6,null)',
        '-> (new3:float32[2, 3, 16, 64],fresh:bfloat16[2, 3, 16, 64],fresh:bfloat16[2, 3, 16, 64],fresh:bfloat16[2, 3, 16, 64])',
    ],
    'autograd_flash_attn_causal_f32': [
        'fa_mi355x_fwd_guarded(new0,new1,new2,new3,new4,new5,6,1,16,64,0,0.0,1,1,0,null,0,null,0,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_guarded(new0,new1,new2,new3,new6,new7,new8,new9,new4,new5,new10,6,1,16,64,0,0.0,1,1,0,7,null,0,null,null)',
        '-> (new3:float32[6, 16, 64],fresh:float32[6, 16, 64],fresh:float32[6, 16, 64],fresh:float32[6, 16, 64])',
    ],
    'bnhd_bf16_causal': [
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,2,3,16,64,1,0.0,1,2,1,null,0,new2,1,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_scale_guard(q,k,96,64,1,new3,null)',
        'fa_mi355x_bwd_guarded(q,k,v,o,do,new4,new5,new6,l,null,new7,2,3,16,64,1,0.0,1,2,1,7,null,0,new3,null)',
        '-> (new0:float32[2, 16, 3, 64],new1:float32[2, 3, 16],None,new4:float32[2, 16, 3, 64],new5:float32[2, 16, 3, 64],new6:float32[2, 16, 3, 64])',
    ],
    'bnhd_bf16_fa1_d128': [
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,new2,2,3,16,128,1,0.0,0,1,1,null,0,new3,1,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,128,null,0)',
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_scale_guard(q,k,96,128,1,new4,null)',
        'fa_mi355x_bwd_guarded(q,k,v,o,do,new5,new6,new7,l,m,new8,2,3,16,128,1,0.0,0,1,1,7,null,0,new4,null)',
        '-> (new0:float32[2, 16, 3, 128],new1:float32[2, 3, 16],new2:float32[2, 3, 16],new5:float32[2, 16, 3, 128],new6:float32[2, 16, 3, 128],new7:float32[2, 16, 3, 128])',
    ],
    'bnhd_bf16_guard_none': [
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,2,3,16,64,1,0.0,0,2,1,null,0,null,0,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_guarded(q,k,v,o,do,new2,new3,new4,l,null,new5,2,3,16,64,1,0.0,0,2,1,7,null,0,null,null)',
        '-> (new0:float32[2, 16, 3, 64],new1:float32[2, 3, 16],None,new2:float32[2, 16, 3, 64],new3:float32[2, 16, 3, 64],new4:float32[2, 16, 3, 64])',
    ],
    'bnhd_bf16_guard_read': [
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,2,3,16,64,1,0.0,0,2,1,null,0,g,0,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_scale_guard(q,k,96,64,1,new2,null)',
        'fa_mi355x_bwd_guarded(q,k,v,o,do,new3,new4,new5,l,null,new6,2,3,16,64,1,0.0,0,2,1,7,null,0,new2,null)',
        '-> (new0:float32[2, 16, 3, 64],new1:float32[2, 3, 16],None,new3:float32[2, 16, 3, 64],new4:float32[2, 16, 3, 64],new5:float32[2, 16, 3, 64])',
    ],
    'bnhd_bf16_guards': [
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,2,3,16,64,1,0.0,0,2,1,null,0,new2,1,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_guarded(q,k,v,o,do,new3,new4,new5,l,null,new6,2,3,16,64,1,0.0,0,2,1,7,null,0,g,null)',
        '-> (new0:float32[2, 16, 3, 64],new1:float32[2, 3, 16],None,new3:float32[2, 16, 3, 64],new4:float32[2, 16, 3, 64],new5:float32[2, 16, 3, 64])',
    ],
    'bnhd_bf16_opts': [
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,2,3,16,64,1,0.0,0,2,1,[0,0,0,0,0,0,0,0,2],9,null,0,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_scale_guard(q,k,96,64,1,new2,null)',
        'fa_mi355x_bwd_guarded(q,k,v,o,do,new3,new4,new5,l,null,new6,2,3,16,64,1,0.0,0,2,1,7,[4,2,2],3,new2,null)',
        '-> (new0:float32[2, 16, 3, 64],new1:float32[2, 3, 16],None,new3:float32[2, 16, 3, 64],new4:float32[2, 16, 3, 64],new5:float32[2, 16, 3, 64])',
    ],
    'bnhd_bf16_scale': [
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,2,3,16,64,1,0.6931471805599453,0,2,1,null,0,new2,1,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_scale_guard(q,k,96,64,1,new3,null)',
        'fa_mi355x_bwd_guarded(q,k,v,o,do,new4,new5,new6,l,null,new7,2,3,16,64,1,0.6931471805599453,0,2,1,7,null,0,new3,null)',
        '-> (new0:float32[2, 16, 3, 64],new1:float32[2, 3, 16],None,new4:float32[2, 16, 3, 64],new5:float32[2, 16, 3, 64],new6:float32[2, 16, 3, 64])',
    ],
    'bnhd_f32': [
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,2,3,16,64,1,0.0,0,2,0,null,0,null,0,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_guarded(q,k,v,o,do,new2,new3,new4,l,null,new5,2,3,16,64,1,0.0,0,2,0,7,null,0,null,null)',
        '-> (new0:float32[2, 16, 3, 64],new1:float32[2, 3, 16],None,new2:float32[2, 16, 3, 64],new3:float32[2, 16, 3, 64],new4:float32[2, 16, 3, 64])',
    ],
    'bwd_bf16_3d_d128_fa1': [
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,128,null,0)',
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_scale_guard(q,k,96,128,1,new0,null)',
        'fa_mi355x_bwd_guarded(q,k,v,o,do,new1,new2,new3,l,null,new4,6,1,16,128,0,0.0,0,1,1,7,null,0,new0,null)',
        '-> (new1:float32[6, 16, 128],new2:float32[6, 16, 128],new3:float32[6, 16, 128])',
    ],
    'bwd_bf16_4d_d64_causal': [
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_scale_guard(q,k,96,64,1,new0,null)',
        'fa_mi355x_bwd_guarded(q,k,v,o,do,new1,new2,new3,l,null,new4,6,1,16,64,0,0.0,1,2,1,7,null,0,new0,null)',
        '-> (new1:float32[2, 3, 16, 64],new2:float32[2, 3, 16, 64],new3:float32[2, 3, 16, 64])',
    ],
    'bwd_bf16_d32': [
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,32,null,0)',
        'fa_mi355x_bwd_guarded(q,k,v,o,do,new0,new1,new2,l,null,new3,6,1,16,32,0,0.0,0,2,1,7,null,0,null,null)',
        '-> (new0:float32[2, 3, 16, 32],new1:float32[2, 3, 16, 32],new2:float32[2, 3, 16, 32])',
    ],
    'bwd_bf16_d34_padded': [
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_padded(new0,new1,new2,new3,new4,new5,new6,new7,l,null,new8,6,16,34,64,1,2,1,null)',
        '-> (fresh:float32[2, 3, 16, 34],fresh:float32[2, 3, 16, 34],fresh:float32[2, 3, 16, 34])',
    ],
    'bwd_bf16_guard_none': [
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_guarded(q,k,v,o,do,new0,new1,new2,l,null,new3,6,1,16,64,0,0.0,0,2,1,7,null,0,null,null)',
        '-> (new0:float32[2, 3, 16, 64],new1:float32[2, 3, 16, 64],new2:float32[2, 3, 16, 64])',
    ],
    'bwd_bf16_opts': [
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,[4,2,2],3)',
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_scale_guard(q,k,96,64,1,new0,null)',
        'fa_mi355x_bwd_guarded(q,k,v,o,do,new1,new2,new3,l,null,new4,6,1,16,64,0,0.0,0,2,1,7,[4,2,2],3,new0,null)',
        '-> (new1:float32[2, 3, 16, 64],new2:float32[2, 3, 16, 64],new3:float32[2, 3, 16, 64])',
    ],
    'bwd_bf16_opts_exact': [
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,[0,0,0,0,0,0,0,0,2],9)',
        'fa_mi355x_bwd_guarded(q,k,v,o,do,new0,new1,new2,l,null,new3,6,1,16,64,0,0.0,0,2,1,7,[0,0,0,0,0,0,0,0,2],9,null,null)',
        '-> (new0:float32[2, 3, 16, 64],new1:float32[2, 3, 16, 64],new2:float32[2, 3, 16, 64])',
    ],
    'bwd_bf16_stages': [
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_scale_guard(q,k,96,64,1,new0,null)',
        'fa_mi355x_bwd_guarded(q,k,v,o,do,new1,new2,new3,l,null,new4,6,1,16,64,0,0.0,0,2,1,2,null,0,new0,null)',
        '-> (new1:float32[2, 3, 16, 64],new2:float32[2, 3, 16, 64],new3:float32[2, 3, 16, 64])',
    ],
    'bwd_caller_grads_m': [
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_guarded(q,k,v,o,do,dq,dk,dv,l,m,new0,6,1,16,64,0,0.0,0,1,0,7,null,0,null,null)',
        '-> (dq:float32[6, 16, 64],dk:float32[6, 16, 64],dv:float32[6, 16, 64])',
    ],
    'bwd_caller_padded_grads': [
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_padded(new0,new1,new2,new3,new4,new5,new6,new7,l,m,new8,6,16,34,64,0,1,0,null)',
        '-> (dq:float32[2, 3, 16, 34],dk:float32[2, 3, 16, 34],dv:float32[2, 3, 16, 34])',
    ],
    'bwd_caller_ws_grads_guard': [
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_guarded(q,k,v,o,do,dq,dk,dv,l,null,ws,6,1,16,64,0,0.0,0,2,1,7,null,0,g,null)',
        '-> (dq:float32[2, 3, 16, 64],dk:float32[2, 3, 16, 64],dv:float32[2, 3, 16, 64])',
    ],
    'bwd_f32_3d_d34_padded_fa1': [
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_padded(new0,new1,new2,new3,new4,new5,new6,new7,l,null,new8,6,16,34,64,0,1,0,null)',
        '-> (fresh:float32[6, 16, 34],fresh:float32[6, 16, 34],fresh:float32[6, 16, 34])',
    ],
    'bwd_f32_4d_d64': [
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_guarded(q,k,v,o,do,new0,new1,new2,l,null,new3,6,1,16,64,0,0.0,0,2,0,7,null,0,null,null)',
        '-> (new0:float32[2, 3, 16, 64],new1:float32[2, 3, 16, 64],new2:float32[2, 3, 16, 64])',
    ],
    'decode_bhnd_f32_split': [
        'fa_mi355x_decode_workspace_bytes(2,3,4,2048,128)',
        'fa_mi355x_fwd_decode(q,kc,vc,new0,new1,null,new2,2,3,4,2048,128,0,0.0,0,0,null)',
        '-> (new0:float32[2, 3, 4, 128],new1:float32[2, 3, 4])',
    ],
    'decode_bhnd_padded_caller': [
        'fa_mi355x_decode_workspace_bytes(2,3,4,2048,32)',
        'fa_mi355x_fwd_decode(new0,kc,vc,new1,lse,null,workspace,2,3,4,2048,32,0,0.22360679774997896,1,1,null)',
        '-> (out:float32[2, 3, 4, 20],lse:float32[2, 3, 4])',
    ],
    'decode_bnhd': [
        'fa_mi355x_decode_workspace_bytes(2,3,4,256,64)',
        'fa_mi355x_fwd_decode(q,kc,vc,new0,new1,null,null,2,3,4,256,64,1,0.0,1,1,null)',
        '-> (new0:float32[2, 4, 3, 64],new1:float32[2, 3, 4])',
    ],
    'decode_bnhd_caller_scale': [
        'fa_mi355x_decode_workspace_bytes(2,3,4,1024,32)',
        'fa_mi355x_fwd_decode(q,kc,vc,out,lse,cache_seqlens,new0,2,3,4,1024,32,1,0.5,1,1,null)',
        '-> (out:float32[2, 4, 3, 32],lse:float32[2, 3, 4])',
    ],
    'decode_bnhd_padded': [
        'fa_mi355x_decode_workspace_bytes(2,3,4,256,64)',
        'fa_mi355x_fwd_decode(new0,kc,vc,new1,new2,cache_seqlens,null,2,3,4,256,64,1,0.14433756729740643,1,1,null)',
        '-> (fresh:float32[2, 4, 3, 48],new2:float32[2, 3, 4])',
    ],
    'decode_workspace': [
        'fa_mi355x_decode_workspace_bytes(2,3,4,2048,64)',
        'fa_mi355x_decode_workspace_bytes(2,3,4,16,64)',
        '-> (fresh:float32[6336],None)',
    ],
    'dropout_bf16_mask': [
        'fa_mi355x_fwd_dropout(q,k,v,new0,new1,null,km,0.25,1.5,4294967293,2,3,16,64,0,1,2,1,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_dropout(q,k,v,o,do,new2,new3,new4,l,m,km,0.25,1.5,4294967293,new5,2,3,16,64,0,1,2,1,null)',
        '-> (new0:float32[2, 3, 16, 64],new1:float32[2, 3, 16],None,new2:float32[2, 3, 16, 64],new3:float32[2, 3, 16, 64],new4:float32[2, 3, 16, 64])',
    ],
    'dropout_f32_fa1_nomask': [
        'fa_mi355x_fwd_dropout(q,k,v,new0,new1,new2,null,0.25,1.5,4294967293,2,3,16,64,0,0,1,0,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_dropout(q,k,v,o,do,new3,new4,new5,l,m,null,0.25,1.5,4294967293,new6,2,3,16,64,0,0,1,0,null)',
        '-> (new0:float32[2, 3, 16, 64],new1:float32[2, 3, 16],new2:float32[2, 3, 16],new3:float32[2, 3, 16, 64],new4:float32[2, 3, 16, 64],new5:float32[2, 3, 16, 64])',
    ],
    'fwd_bf16_3d_d128_fa1': [
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,new2,6,1,16,128,0,0.0,0,1,1,null,0,new3,1,null)',
        '-> (new0:float32[6, 16, 128],new1:float32[6, 16],new2:float32[6, 16])',
    ],
    'fwd_bf16_4d_d64_causal': [
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,6,1,16,64,0,0.0,1,2,1,null,0,new2,1,null)',
        '-> (new0:float32[2, 3, 16, 64],new1:float32[2, 3, 16],None)',
    ],
    'fwd_bf16_d32': [
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,6,1,16,32,0,0.0,0,2,1,null,0,null,0,null)',
        '-> (new0:float32[2, 3, 16, 32],new1:float32[2, 3, 16],None)',
    ],
    'fwd_bf16_d34_padded_fa1': [
        'fa_mi355x_fwd_padded(new0,new1,new2,new3,new4,new5,6,16,34,64,0,1,1,null)',
        '-> (fresh:float32[2, 3, 16, 34],new4:float32[2, 3, 16],new5:float32[2, 3, 16])',
    ],
    'fwd_bf16_guard_none': [
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,6,1,16,64,0,0.0,0,2,1,null,0,null,0,null)',
        '-> (new0:float32[2, 3, 16, 64],new1:float32[2, 3, 16],None)',
    ],
    'fwd_bf16_opts_exact': [
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,6,1,16,64,0,0.0,0,2,1,[0,0,0,0,0,0,0,0,2],9,null,0,null)',
        '-> (new0:float32[2, 3, 16, 64],new1:float32[2, 3, 16],None)',
    ],
    'fwd_bf16_opts_folded': [
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,6,1,16,64,0,0.0,0,2,1,[0,0,0,0,0,0,0,0,1],9,null,0,null)',
        '-> (new0:float32[2, 3, 16, 64],new1:float32[2, 3, 16],None)',
    ],
    'fwd_bf16_opts_phased': [
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,6,1,16,64,0,0.0,0,2,1,[4,2,2],3,new2,1,null)',
        '-> (new0:float32[2, 3, 16, 64],new1:float32[2, 3, 16],None)',
    ],
    'fwd_bf16_out_bf16': [
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,6,1,16,64,0,0.0,0,2,1,[0,0,0,0,0,0,0,0,0,1],10,new2,1,null)',
        '-> (new0:bfloat16[2, 3, 16, 64],new1:float32[2, 3, 16],None)',
    ],
    'fwd_bf16_out_bf16_long_opts': [
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,6,1,16,64,0,0.0,0,2,1,[0,0,0,0,0,0,0,0,0,1,0],11,new2,1,null)',
        '-> (new0:bfloat16[2, 3, 16, 64],new1:float32[2, 3, 16],None)',
    ],
    'fwd_bf16_out_bf16_opts': [
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,6,1,16,64,0,0.0,0,2,1,[4,2,2,0,0,0,0,0,0,1],10,new2,1,null)',
        '-> (new0:bfloat16[2, 3, 16, 64],new1:float32[2, 3, 16],None)',
    ],
    'fwd_caller_flat_l_m': [
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(q,k,v,new0,l,m,6,1,16,64,0,0.0,0,1,1,null,0,new1,1,null)',
        '-> (new0:float32[2, 3, 16, 64],l:float32[96],m:float32[96])',
    ],
    'fwd_caller_guard_produce': [
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,6,1,16,64,0,0.0,0,2,1,null,0,guard,1,null)',
        '-> (new0:float32[2, 3, 16, 64],new1:float32[2, 3, 16],None)',
    ],
    'fwd_caller_guard_read': [
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,6,1,16,64,0,0.0,0,2,1,null,0,guard,0,null)',
        '-> (new0:float32[2, 3, 16, 64],new1:float32[2, 3, 16],None)',
    ],
    'fwd_caller_l_only': [
        'fa_mi355x_fwd_guarded(q,k,v,new0,l,null,6,1,16,64,0,0.0,0,2,0,null,0,null,0,null)',
        '-> (new0:float32[6, 16, 64],l:float32[6, 16],None)',
    ],
    'fwd_caller_out_l_m_fa1': [
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(q,k,v,out,l,m,6,1,16,64,0,0.0,0,1,1,null,0,new0,1,null)',
        '-> (out:float32[2, 3, 16, 64],l:float32[2, 3, 16],m:float32[2, 3, 16])',
    ],
    'fwd_caller_padded_out_l_m': [
        'fa_mi355x_fwd_padded(new0,new1,new2,new3,l,m,6,16,34,64,0,1,0,null)',
        '-> (out:float32[2, 3, 16, 34],l:float32[2, 3, 16],m:float32[2, 3, 16])',
    ],
    'fwd_f32_3d_d34_padded': [
        'fa_mi355x_fwd_padded(new0,new1,new2,new3,new4,null,6,16,34,64,0,2,0,null)',
        '-> (fresh:float32[6, 16, 34],new4:float32[6, 16],None)',
    ],
    'fwd_f32_3d_d64_fa1_causal': [
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,new2,6,1,16,64,0,0.0,1,1,0,null,0,null,0,null)',
        '-> (new0:float32[6, 16, 64],new1:float32[6, 16],new2:float32[6, 16])',
    ],
    'fwd_f32_4d_d64': [
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,6,1,16,64,0,0.0,0,2,0,null,0,null,0,null)',
        '-> (new0:float32[2, 3, 16, 64],new1:float32[2, 3, 16],None)',
    ],
    'fwd_f32_guard_none_produce': [
        'fa_mi355x_fwd_guarded(q,k,v,new0,new1,null,6,1,16,64,0,0.0,0,2,0,null,0,null,0,null)',
        '-> (new0:float32[2, 3, 16, 64],new1:float32[2, 3, 16],None)',
    ],
    'helpers': [
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,[4,2,2],3)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_status(ws,6,16,64,&int)',
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_scale_guard(q,k,96,64,1,new0,null)',
        'fa_mi355x_scale_guard(q,k,96,64,1,g,null)',
        '-> (fresh:float32[288],fresh:float32[288],fresh:float32[288],0,fresh:float32[512],None,None,None,new0:float32[512],g:float32[512],(0,0,0,0,0,0,0,0,2),None,(0,0,0,0,0,0,0,0,2))',
    ],
    'kv_cache_d48': [
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(new0,new1,new2,new3,new4,null,2,2,16,64,1,0.14433756729740643,1,2,1,null,0,new5,1,null)',
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(new6,new7,new8,new9,new10,null,2,2,16,64,1,0.14433756729740643,1,2,1,null,0,new11,1,null)',
        'fa_mi355x_decode_workspace_bytes(2,2,1,64,64)',
        'fa_mi355x_decode_workspace_bytes(2,2,1,64,64)',
        'fa_mi355x_fwd_decode(new12,new13,new14,new15,new16,new17,null,2,2,1,64,64,1,0.14433756729740643,1,1,null)',
        'fa_mi355x_decode_workspace_bytes(2,2,1,64,64)',
        'fa_mi355x_fwd_decode(new18,new19,new20,new21,new22,new17,null,2,2,1,64,64,1,0.14433756729740643,1,1,null)',
        '-> (fresh:bfloat16[2, 1, 96],new13:bfloat16[2, 64, 2, 64],fresh:int32[2])',
    ],
    'kv_cache_d64': [
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(new0,new1,new2,new3,new4,null,2,2,16,64,1,0.0,1,2,1,null,0,new5,1,null)',
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(new6,new7,new8,new9,new10,null,2,2,16,64,1,0.0,1,2,1,null,0,new11,1,null)',
        'fa_mi355x_decode_workspace_bytes(2,2,1,64,64)',
        'fa_mi355x_decode_workspace_bytes(2,2,1,64,64)',
        'fa_mi355x_fwd_decode(new12,new13,new14,new15,new16,new17,null,2,2,1,64,64,1,0.0,1,1,null)',
        'fa_mi355x_decode_workspace_bytes(2,2,1,64,64)',
        'fa_mi355x_fwd_decode(new18,new19,new20,new21,new22,new17,null,2,2,1,64,64,1,0.0,1,1,null)',
        'fa_mi355x_decode_workspace_bytes(2,2,1,64,64)',
        'fa_mi355x_fwd_decode(new23,new13,new14,new24,new25,new26,null,2,2,1,64,64,1,0.0,1,1,null)',
        'fa_mi355x_decode_workspace_bytes(2,2,1,64,64)',
        'fa_mi355x_fwd_decode(new27,new19,new20,new28,new29,new26,null,2,2,1,64,64,1,0.0,1,1,null)',
        '-> (fresh:bfloat16[2, 1, 128],new13:bfloat16[2, 64, 2, 64],fresh:int32[2])',
    ],
    'masked_bf16_fa1_causal': [
        'fa_mi355x_fwd_masked(q,k,v,new0,new1,new2,km,2,3,16,64,0,1,1,1,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_masked(q,k,v,o,do,new3,new4,new5,l,m,km,new6,2,3,16,64,0,1,1,1,null)',
        '-> (new0:float32[2, 3, 16, 64],new1:float32[2, 3, 16],new2:float32[2, 3, 16],new3:float32[2, 3, 16, 64],new4:float32[2, 3, 16, 64],new5:float32[2, 3, 16, 64])',
    ],
    'masked_f32_fa2': [
        'fa_mi355x_fwd_masked(q,k,v,new0,new1,null,km,2,3,16,64,0,0,2,0,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(6,16,64,null,0)',
        'fa_mi355x_bwd_masked(q,k,v,o,do,new2,new3,new4,l,m,km,new5,2,3,16,64,0,0,2,0,null)',
        '-> (new0:float32[2, 3, 16, 64],new1:float32[2, 3, 16],None,new2:float32[2, 3, 16, 64],new3:float32[2, 3, 16, 64],new4:float32[2, 3, 16, 64])',
    ],
    'mha_fused': [
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(new0,new1,new2,new3,new4,null,2,2,16,64,1,0.0,1,2,1,null,0,new5,1,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(4,16,64,null,0)',
        'fa_mi355x_bwd_guarded(new0,new1,new2,new3,new6,new7,new8,new9,new4,null,new10,2,2,16,64,1,0.0,1,2,1,7,null,0,new5,null)',
        '-> (fresh:bfloat16[2, 16, 128],fresh:bfloat16[2, 16, 128])',
    ],
    'mha_fused_f32': [
        'fa_mi355x_fwd_guarded(new0,new1,new2,new3,new4,null,2,2,16,64,1,0.0,1,2,0,null,0,null,0,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(4,16,64,null,0)',
        'fa_mi355x_bwd_guarded(new0,new1,new2,new3,new5,new6,new7,new8,new4,null,new9,2,2,16,64,1,0.0,1,2,0,7,null,0,null,null)',
        '-> (fresh:float32[2, 16, 128],fresh:float32[2, 16, 128])',
    ],
    'mha_fused_fold': [
        'fa_mi355x_fwd_guarded(new0,new1,new2,new3,new4,null,2,2,16,64,1,0.6931471805599453,1,2,1,null,0,null,0,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(4,16,64,null,0)',
        'fa_mi355x_bwd_guarded(new0,new1,new2,new3,new5,new6,new7,new8,new4,null,new9,2,2,16,64,1,0.6931471805599453,1,2,1,7,null,0,null,null)',
        '-> (fresh:bfloat16[2, 16, 128],fresh:bfloat16[2, 16, 128])',
    ],
    'mha_unfused_noncausal': [
        'fa_mi355x_guard_bytes()',
        'fa_mi355x_fwd_guarded(new0,new1,new2,new3,new4,null,4,1,16,64,0,0.0,0,2,1,null,0,new5,1,null)',
        'fa_mi355x_bwd_workspace_bytes_ex(4,16,64,null,0)',
        'fa_mi355x_bwd_guarded(new0,new1,new2,new3,new6,new7,new8,new9,new4,null,new10,4,1,16,64,0,0.0,0,2,1,7,null,0,new5,null)',
        '-> (fresh:bfloat16[2, 16, 128],fresh:bfloat16[2, 16, 128])',
    ],
}
EXPECTED_ERRORS = {
    'fwd_cpu': 'FlashAttnLibraryError: device_ops needs GPU tensors; there is no CPU fallback',
    'fwd_f64': 'TypeError: unsupported dtype torch.float64: use float32 or bfloat16',
    'fwd_f16': 'TypeError: unsupported dtype torch.float16: use float32 or bfloat16',
    'fwd_shape_k': 'ValueError: q, k, v (and out_grad) must share shape, dtype and device',
    'fwd_dtype_v': 'ValueError: q, k, v (and out_grad) must share shape, dtype and device',
    'fwd_noncontig_q': 'ValueError: tensors must be contiguous [.., N, d]',
    'fwd_2d': 'ValueError: expected (B, H, N, d) or (BH, N, d)',
    'fwd_5d': 'ValueError: expected (B, H, N, d) or (BH, N, d)',
    'fwd_d160': 'ValueError: head dimension d > 128 is not supported (the reference kernels assert d <= 128, src/flash_attn_fw.cu:43)',
    'fwd_d160_3d': 'ValueError: head dimension d > 128 is not supported (the reference kernels assert d <= 128, src/flash_attn_fw.cu:43)',
    'fwd_d34_opts': 'ValueError: per-call options and a bf16 output need a native head dim (32, 64, 128): other d run zero-padded through fa_mi355x_fwd_padded, which takes neither',
    'fwd_d34_out_bf16': 'ValueError: per-call options and a bf16 output need a native head dim (32, 64, 128): other d run zero-padded through fa_mi355x_fwd_padded, which takes neither',
    'fwd_out_dtype_f16': 'TypeError: out_dtype must be float32 or bfloat16',
    'fwd_out_shape': "ValueError: out must be a contiguous tensor of q's shape and of out_dtype",
    'fwd_out_dtype': "ValueError: out must be a contiguous tensor of q's shape and of out_dtype",
    'fwd_out_noncontig': "ValueError: out must be a contiguous tensor of q's shape and of out_dtype",
    'fwd_cpu_and_f64': 'FlashAttnLibraryError: device_ops needs GPU tensors; there is no CPU fallback',
    'fwd_f64_and_shape': 'TypeError: unsupported dtype torch.float64: use float32 or bfloat16',
    'fwd_shape_and_noncontig': 'ValueError: q, k, v (and out_grad) must share shape, dtype and device',
    'fwd_d160_and_opts': 'ValueError: per-call options and a bf16 output need a native head dim (32, 64, 128): other d run zero-padded through fa_mi355x_fwd_padded, which takes neither',
    'bwd_cpu': 'FlashAttnLibraryError: device_ops needs GPU tensors; there is no CPU fallback',
    'bwd_f64': 'TypeError: unsupported dtype torch.float64: use float32 or bfloat16',
    'bwd_shape_do': 'ValueError: q, k, v (and out_grad) must share shape, dtype and device',
    'bwd_dtype_do': 'ValueError: q, k, v (and out_grad) must share shape, dtype and device',
    'bwd_noncontig_do': 'ValueError: tensors must be contiguous [.., N, d]',
    'bwd_out_bf16': "ValueError: out must be the forward's contiguous float32 output",
    'bwd_out_shape': "ValueError: out must be the forward's contiguous float32 output",
    'bwd_out_noncontig': "ValueError: out must be the forward's contiguous float32 output",
    'bwd_d160': 'ValueError: head dimension d > 128 is not supported (the reference kernels assert d <= 128, src/flash_attn_fw.cu:43)',
    'bwd_d34_opts': "ValueError: per-call options, a stage mask and a caller's workspace need a native head dim (32, 64, 128): other d run zero-padded through fa_mi355x_bwd_padded, which takes none of them",
    'bwd_d34_stages': "ValueError: per-call options, a stage mask and a caller's workspace need a native head dim (32, 64, 128): other d run zero-padded through fa_mi355x_bwd_padded, which takes none of them",
    'bwd_d34_workspace': "ValueError: per-call options, a stage mask and a caller's workspace need a native head dim (32, 64, 128): other d run zero-padded through fa_mi355x_bwd_padded, which takes none of them",
    'bwd_workspace_small': 'ValueError: workspace too small for these options: size it with bwd_workspace(q, opts)',
    'bwd_workspace_small_opts': 'ValueError: workspace too small for these options: size it with bwd_workspace(q, opts)',
    'bwd_out_bf16_and_shape_do': 'ValueError: q, k, v (and out_grad) must share shape, dtype and device',
    'bwd_out_bf16_and_workspace': "ValueError: out must be the forward's contiguous float32 output",
    'fwd_bnhd_3d': 'ValueError: expected (B, N, H, d)',
    'fwd_bnhd_cpu': 'ValueError: q, k, v must be contiguous GPU tensors of one shape and dtype',
    'fwd_bnhd_shape': 'ValueError: q, k, v must be contiguous GPU tensors of one shape and dtype',
    'fwd_bnhd_dtype': 'ValueError: q, k, v must be contiguous GPU tensors of one shape and dtype',
    'fwd_bnhd_noncontig': 'ValueError: q, k, v must be contiguous GPU tensors of one shape and dtype',
    'fwd_bnhd_3d_and_cpu': 'ValueError: expected (B, N, H, d)',
    'fwd_masked_cpu': 'FlashAttnLibraryError: device_ops needs GPU tensors; there is no CPU fallback',
    'fwd_masked_3d': 'ValueError: a key mask needs (B, H, N, d) tensors: it is shared by the heads of a batch element',
    'fwd_masked_shape': 'ValueError: q, k, v (and out_grad) must share shape, dtype and device',
    'fwd_masked_mask_shape': 'ValueError: key_mask must be a contiguous float32 GPU tensor of shape (B, N)',
    'fwd_masked_mask_dtype': 'ValueError: key_mask must be a contiguous float32 GPU tensor of shape (B, N)',
    'fwd_masked_mask_cpu': 'ValueError: key_mask must be a contiguous float32 GPU tensor of shape (B, N)',
    'fwd_masked_mask_noncontig': 'ValueError: key_mask must be a contiguous float32 GPU tensor of shape (B, N)',
    'fwd_masked_no_mask_cpu': 'FlashAttnLibraryError: device_ops needs GPU tensors; there is no CPU fallback',
    'bwd_masked_no_mask_3d': 'ValueError: a key mask needs (B, H, N, d) tensors: it is shared by the heads of a batch element',
    'fwd_masked_f64_and_mask': 'TypeError: unsupported dtype torch.float64: use float32 or bfloat16',
    'bwd_masked_shape_do': 'ValueError: q, k, v (and out_grad) must share shape, dtype and device',
    'bwd_masked_mask_shape': 'ValueError: key_mask must be a contiguous float32 GPU tensor of shape (B, N)',
    'bwd_masked_3d': 'ValueError: a key mask needs (B, H, N, d) tensors: it is shared by the heads of a batch element',
    'fwd_dropout_3d_nomask': 'ValueError: expected (B, H, N, d)',
    'fwd_dropout_3d': 'ValueError: expected (B, H, N, d)',
    'fwd_dropout_mask_dtype': 'ValueError: key_mask must be a contiguous float32 GPU tensor of shape (B, N)',
    'fwd_dropout_cpu': 'FlashAttnLibraryError: device_ops needs GPU tensors; there is no CPU fallback',
    'bwd_dropout_mask_shape': 'ValueError: key_mask must be a contiguous float32 GPU tensor of shape (B, N)',
    'bwd_dropout_noncontig_do': 'ValueError: tensors must be contiguous [.., N, d]',
    'bwd_dropout_3d': 'ValueError: a key mask needs (B, H, N, d) tensors: it is shared by the heads of a batch element',
    'scale_guard_dtype': 'ValueError: q and k must be contiguous GPU tensors of one dtype and row length',
    'scale_guard_rows': 'ValueError: q and k must have the same number of rows',
    'scale_guard_row_length': 'ValueError: q and k must be contiguous GPU tensors of one dtype and row length',
    'scale_guard_cpu': 'ValueError: q and k must be contiguous GPU tensors of one dtype and row length',
    'scale_guard_noncontig': 'ValueError: q and k must be contiguous GPU tensors of one dtype and row length',
    'fwd_bnhd_f64': 'TypeError: unsupported dtype torch.float64: use float32 or bfloat16',
    'bwd_bnhd_cpu': 'ValueError: q, k, v must be contiguous GPU tensors of one shape and dtype',
    'bwd_bnhd_f64': 'TypeError: unsupported dtype torch.float64: use float32 or bfloat16',
    'bwd_bnhd_shape_do': 'ValueError: q, k, v must be contiguous GPU tensors of one shape and dtype',
    'bwd_bnhd_out_bf16': "ValueError: out must be the forward's contiguous float32 output",
    'bwd_bnhd_l_small': "ValueError: l must be a contiguous float32 tensor on q's device with at least 96 elements",
    'fwd_l_small': "ValueError: l must be a contiguous float32 tensor on q's device with at least 96 elements",
    'fwd_m_small': "ValueError: m must be a contiguous float32 tensor on q's device with at least 96 elements",
    'fwd_l_f64': "ValueError: l must be a contiguous float32 tensor on q's device with at least 96 elements",
    'fwd_l_noncontig': "ValueError: l must be a contiguous float32 tensor on q's device with at least 96 elements",
    'fwd_padded_l_small': "ValueError: l must be a contiguous float32 tensor on q's device with at least 96 elements",
    'fwd_guard_small': "ValueError: guard must be a contiguous float32 tensor on q's device with at least 512 elements",
    'fwd_guard_bf16': "ValueError: guard must be a contiguous float32 tensor on q's device with at least 512 elements",
    'bwd_l_small': "ValueError: l must be a contiguous float32 tensor on q's device with at least 96 elements",
    'bwd_m_small': "ValueError: m must be a contiguous float32 tensor on q's device with at least 96 elements",
    'bwd_grads_small': "ValueError: each of grads must be a contiguous float32 tensor on q's device with at least 6144 elements",
    'bwd_grads_bf16': "ValueError: each of grads must be a contiguous float32 tensor on q's device with at least 6144 elements",
    'bwd_guard_small': "ValueError: guard must be a contiguous float32 tensor on q's device with at least 512 elements",
    'bwd_workspace_expanded': "ValueError: workspace must be a contiguous tensor on q's device",
    'fwd_masked_no_mask': 'ValueError: key_mask must be a contiguous float32 GPU tensor of shape (B, N)',
    'bwd_masked_out_bf16': "ValueError: out must be the forward's contiguous float32 output",
    'bwd_masked_m_small': "ValueError: m must be a contiguous float32 tensor on q's device with at least 96 elements",
    'bwd_dropout_l_small': "ValueError: l must be a contiguous float32 tensor on q's device with at least 96 elements",
    'bwd_dropout_3d_nomask': 'ValueError: expected (B, H, N, d)',
    'scale_guard_f64': 'TypeError: unsupported dtype torch.float64: use float32 or bfloat16',
    'scale_guard_out_small': "ValueError: guard must be a contiguous float32 tensor on q's device with at least 512 elements",
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_call_trace(rec, name):
    """The C calls (symbol, arguments, which tensor each pointer is) and the returned tensors of one public call."""
    assert run_call(rec, name) == EXPECTED_TRACES[name]


@pytest.mark.parametrize("name", list(ERRORS))
def test_rejected_arguments(rec, name):
    """Each bad argument, alone and in a few combinations: the exception type and message (or, for a call that goes through, its C
    calls)."""
    assert run_error(rec, name) == EXPECTED_ERRORS[name]
