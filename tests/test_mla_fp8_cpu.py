"""The FP8 latent cache of MLA decode without a GPU (include/flash_attn_mi355x_mla_fp8.h, csrc/fa_mla_fp8.h): the format restated in
torch (quantise / dequantise, which tests/test_gpu_mla_fp8.py checks the kernels against), the inputs of those tests, the C ABI against
the header, every refusal in front of a HIP call, the kernels' registers, the Python operand checks."""
import os
import re

import pytest
import torch

import test_mla_cpu as dense
import test_mla_sparse_cpu as sparse
from test_abi_cpu import _device_kernels
from test_decode_cpu import built  # noqa: F401  (the module-scoped build fixture)
from test_mla_cpu import BAD_ARG, DQK, DV, ROOT, SCALE, inputs

HEADER, ROW = "flash_attn_mi355x_mla_fp8.h", 656
E4M3 = torch.float8_e4m3fn


def quantise(rows):
    """bf16 (..., 576) -> uint8 (..., 656), the header's append: per 128-column tile a = max |x| (NaN ignored, inf counts), the scale
    2^(e - 9) if m <= 0.875 else 2^(e - 8) for a = m 2^e, clamped to [2^-100, 2^120] (which is where a = 0 and a = inf land),
    code = rne_e4m3(clamp(x / s, -448, 448)), NaN -> 0x7F; then the four scales as fp32 and k_pe as it is."""
    x = rows[..., :DV].float().reshape(*rows.shape[:-1], 4, 128)
    a = torch.where(x.isnan(), 0.0, x.abs()).amax(-1)
    m, e = torch.frexp(a)
    e = torch.where(a == 0, -100, torch.where(a.isinf(), 120, torch.where(m <= 0.875, e - 9, e - 8))).clamp(-100, 120)
    s = torch.ldexp(torch.ones_like(a), e)
    codes = (x * (1.0 / s)[..., None]).clamp(-448.0, 448.0).to(E4M3).view(torch.uint8)
    codes[x.isnan()] = 0x7F
    return torch.cat([codes.reshape(*rows.shape[:-1], DV), s.contiguous().view(torch.uint8), rows[..., DV:].contiguous().view(torch.uint8)], -1)


def dequantise(cache):
    """uint8 (..., 656) -> bf16 (..., 576): s_{c >> 7} * e4m3(code_c), exact in bf16 for power-of-two scales, then k_pe."""
    s = cache[..., DV:DV + 16].contiguous().view(torch.float32)
    lat = cache[..., :DV].contiguous().view(E4M3).float().reshape(*cache.shape[:-1], 4, 128) * s[..., None]
    return torch.cat([lat.reshape(*cache.shape[:-1], DV).to(torch.bfloat16), cache[..., DV + 16:].contiguous().view(torch.bfloat16)], -1)


def fp8_inputs(seed, B, Ncap, H, Nq):
    """q and the QUANTISED cache (B, Ncap, 656) of the GPU tests: test_mla_cpu.inputs with every 128-column tile of every cache row
    scaled by a gain of {1, 1, 1/2, 1/4}, so that the tiles of a row carry different scales (2^-8, 2^-9, 2^-10)."""
    q, kv = inputs(seed, B, Ncap, H, Nq)
    gain = torch.tensor([1.0, 1.0, 0.5, 0.25])[torch.randint(0, 4, (B, Ncap, 4), generator=torch.Generator().manual_seed(seed + 100))]
    kv[..., :DV] = (kv[..., :DV].float().reshape(B, Ncap, 4, 128) * gain[..., None]).reshape(B, Ncap, DV).to(torch.bfloat16)
    return q, quantise(kv)


def edge_rows(B=2, Nq=3):
    """kv_new (B, Nq, 576) for the append test.  Token (0, 0): tile 0 all zeros, tile 1 with maximum exactly 448 * 2^3, tile 2 one bf16
    ulp above that (3600), tile 3 tiny (U(-1, 1) * 2^-40).  Token (0, 1): a NaN in tile 0, an infinity in tile 1."""
    kv = inputs(dense.SEED + 1, B, Nq, 1, 1)[1]
    kv[0, 0, :128] = 0
    kv[0, 0, 130], kv[0, 0, 300] = -3584.0, 3600.0
    kv[0, 0, 384:512] = (kv[0, 0, 384:512].float() * 2.0 ** -40).to(torch.bfloat16)
    kv[0, 1, 5], kv[0, 1, 200] = float("nan"), float("-inf")
    return kv


def test_the_restated_format_on_the_edge_rows():
    kv = edge_rows()
    b = quantise(kv)
    s = b[..., DV:DV + 16].contiguous().view(torch.float32)
    assert b.shape == (2, 3, ROW) and torch.equal(torch.frexp(s)[0], torch.full_like(s, 0.5))   # powers of two
    assert s[0, 0, 0] == 2.0 ** -100 and not b[0, 0, :128].any()
    assert s[0, 0, 1] == 8.0 and b[0, 0, 130] == 0xFE and s[0, 0, 2] == 16.0 and s[0, 0, 3] < 2.0 ** -45
    assert b[0, 1, 5] == 0x7F and s[0, 1, 1] == 2.0 ** 120 and b[0, 1, 200] == 0xFE
    assert torch.equal(b[..., DV + 16:].contiguous().view(torch.bfloat16), kv[..., DV:])
    clean = kv[1]   # U(-1, 1): the round trip is within half an e4m3 step of the tile's scale, and k_pe is exact
    back = dequantise(b[1])
    assert (back.float() - clean.float()).abs().max() <= 2.0 ** -8 * 16 and torch.equal(back[..., DV:], clean[..., DV:])


# ---- the C ABI ----
def test_fp8_abi_table_matches_the_header_and_the_library(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    protos, lib = _prototypes(HEADER), built.mla()
    assert sorted(protos) == sorted(built.MLA_FP8_ABI)
    assert not set(protos) & (set(built.MLA_ABI) | set(built.MLA_SPARSE_ABI) | set(built.MLA_INDEXER_ABI))
    for s, (res, args) in built.MLA_FP8_ABI.items():
        assert ([_ctypes_kind(x) for x in args], _ctypes_kind(res)) == (protos[s][1], protos[s][0]), s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s
    names = {}
    for h in (HEADER, dense.HEADER, sparse.HEADER):   # each fp8 entry point has its bf16 twin's parameter list
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        names.update({s: [re.findall(r"\w+", p)[-1] for p in ps.split(",")] for s, ps in re.findall(r"\b(fa_mi355x_\w+)\s*\(([^()]*)\)\s*;", text)})
    for twin in ("fa_mi355x_fwd_decode_mla", "fa_mi355x_fwd_decode_mla_sparse", "fa_mi355x_mla_append"):
        assert names[twin + "_fp8"] == names[twin]


def test_the_fp8_kernels_are_there_and_run_without_scratch(built):
    kernels = _device_kernels(built.lib_path(built.MLA_NAME))
    names = " ".join(k[0] for k in kernels)
    assert names.count("mla_fp8_split_kernel") == 2 and names.count("mla_fp8_sparse_split_kernel") == 2 and "mla_fp8_append_kernel" in names
    for name, scratch, vgpr in kernels:
        assert scratch == 0 and vgpr <= 512, (name, scratch, vgpr)


# ---- refusals, before any HIP call: the bf16 lists, with the 2 GiB bound at 656 bytes per row ----
_DENSE_BAD = [(o, m) for o, m in dense._BAD if m != "2 GiB"] + [(dict(Ncap=1 << 22), "2 GiB"), (dict(dense._PAGED, page_size=1 << 22), "2 GiB")]
_ids = lambda bad: [",".join(f"{k}={v}" for k, v in o.items()) for o, _ in bad]


@pytest.mark.parametrize("over,msg", _DENSE_BAD, ids=_ids(_DENSE_BAD))
def test_fp8_call_rejects_each_bad_argument_before_any_hip_call(built, over, msg):
    a, lib = dict(dense._GOOD, **over), built.mla()
    rc = lib.fa_mi355x_fwd_decode_mla_fp8(*[a[n] or None for n in ("q", "kv_new", "kv", "out", "lse", "lens", "table", "ws")], a["B"], a["H"],
                                          a["Nq"], a["Ncap"], a["num_pages"], a["page_size"], a["max_pages"], a["scale"], a["causal"], None)
    err = lib.fa_mi355x_mla_last_error().decode()
    assert rc == BAD_ARG and msg in err, (rc, err)


_SPARSE_BAD = sparse._BAD + [(dict(Ncap=1 << 22), "2 GiB")]


@pytest.mark.parametrize("over,msg", _SPARSE_BAD, ids=_ids(_SPARSE_BAD))
def test_fp8_sparse_call_rejects_each_bad_argument_before_any_hip_call(built, over, msg):
    a, lib = dict(sparse._GOOD, **over), built.mla()
    rc = lib.fa_mi355x_fwd_decode_mla_sparse_fp8(*[a[n] or None for n in ("q", "kv_new", "kv", "idx", "out", "lse", "lens", "table", "ws")],
                                                 *[a[n] for n in ("B", "H", "Nq", "topk", "Ncap", "num_pages", "page_size", "max_pages", "scale",
                                                                  "causal")], None)
    err = lib.fa_mi355x_mla_last_error().decode()
    assert rc == BAD_ARG and msg in err, (rc, err)


@pytest.mark.parametrize("over,msg", [(dict(kv_new=0), "null pointer"), (dict(kv=0), "null pointer"), (dict(kv=8), "aligned"), (dict(Nq=129), "Nq > 128"),
                                      (dict(Nq=0), "positive"), (dict(dense._PAGED, page_size=64), "multiple of 128"), (dict(Ncap=1 << 22), "2 GiB")])
def test_fp8_append_rejects_each_bad_argument_before_any_hip_call(built, over, msg):
    a, lib = dict(dict(dense._GOOD, kv_new=32), **over), built.mla()
    rc = lib.fa_mi355x_mla_append_fp8(*[a[n] or None for n in ("kv_new", "kv", "lens", "table")], a["B"], a["Nq"], a["Ncap"], a["num_pages"],
                                      a["page_size"], a["max_pages"], None)
    assert rc == BAD_ARG and msg in lib.fa_mi355x_mla_last_error().decode()


def test_python_checks_name_the_fp8_cache_before_the_library_is_called(monkeypatch):
    from flash_attention_minitorch_amd import _lib, device_ops as ops
    monkeypatch.setattr(_lib, "mla", lambda: pytest.fail("the library was called"))
    lens, q, new = torch.zeros(2, dtype=torch.int32), torch.zeros(2, 1, 4, DQK, dtype=torch.bfloat16), torch.zeros(2, 1, DQK, dtype=torch.bfloat16)
    z = lambda *shape: torch.zeros(*shape, dtype=torch.uint8)
    for cache, msg in [(z(2, 128, DQK), "rows of 656 bytes"), (z(256, ROW), "rows of 656 bytes"),
                       (z(2, 256, ROW)[:, ::2], "kv_cache must be contiguous"), (z(3, 128, ROW), "with B = 2")]:
        for call in (lambda: ops.flash_attn_decode_mla(q, cache, lens, SCALE), lambda: ops.mla_append(new, cache, lens),
                     lambda: ops.mla_workspace(q, cache)):
            with pytest.raises(ValueError, match=re.escape(msg)):
                call()
    with pytest.raises(ValueError, match="kv_new must be"):   # kv_new stays bf16 rows of 576
        ops.flash_attn_decode_mla(q, z(2, 128, ROW), lens, SCALE, kv_new=torch.zeros(2, 1, ROW, dtype=torch.bfloat16))
