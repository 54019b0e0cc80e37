"""_lib's argument-type tables against the C headers: every entry point the headers declare has an entry (but the host-pointer
launchers, which only the reference-named shims call), and every entry has its prototype's parameter count and, parameter by
parameter, its kind (pointer / int / unsigned / long / size_t / float / double).  No library is loaded."""
import ctypes
import os
import re

import pytest

from flash_attention_minitorch_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LAUNCHERS = {"fa_mi355x_launch_fw_host", "fa_mi355x_launch_bw_host"}


def _prototypes(header):
    """symbol -> (return kind, [parameter kind]) of every fa_mi355x_* function the header declares."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"(\w+\s*\**)\s*\b(fa_mi355x_\w+)\s*\(([^)]*)\)\s*;", text):
        params = [p.strip() for p in params.split(",")]
        protos[name] = (_c_kind(ret.strip() + " x"), [] if params == ["void"] else [_c_kind(p) for p in params])
    return protos


def _c_kind(decl):
    if "*" in decl:
        return "pointer"
    words = decl.split()[:-1]   # drop the parameter name
    words = [w for w in words if w not in ("const", "extern")]
    return {("int",): "int", ("bool",): "int", ("unsigned",): "unsigned", ("long",): "long", ("size_t",): "size_t",
            ("float",): "float", ("double",): "double", ("void",): "void"}[tuple(words)]


def _ctypes_kind(t):
    if t is None:
        return "void"
    if t is ctypes.c_void_p or t is ctypes.c_char_p or issubclass(t, ctypes._Pointer):
        return "pointer"
    return {ctypes.c_int: "int", ctypes.c_uint: "unsigned", ctypes.c_long: "long", ctypes.c_size_t: "size_t",
            ctypes.c_float: "float", ctypes.c_double: "double"}[t]


@pytest.mark.parametrize("header,table", [("flash_attn_mi355x.h", _lib.CORE_ABI), ("flash_attn_mi355x_decode.h", _lib.DECODE_ABI)])
def test_abi_table_matches_header(header, table):
    protos = _prototypes(header)
    assert set(protos) - HOST_LAUNCHERS == set(table)
    for sym, (res, args) in table.items():
        ret, params = protos[sym]
        assert [_ctypes_kind(a) for a in args] == params, sym
        assert _ctypes_kind(res) == ret, sym

