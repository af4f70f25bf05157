"""libqgtc_hip.so through ctypes, with every entry's calling signature derived from include/qgtc.h: the header is the one place a
signature is written. :func:`load` is what Python code in this tree uses to reach the C-ABI; it needs neither torch nor the
extension, and nothing is parsed or opened before its first call."""
from __future__ import annotations

import ctypes
import os
import re

from . import lib_path

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qgtc.h")
HEADS_HEADER = os.path.join(os.path.dirname(HEADER), "qgtc_heads.h")   # the multi-head entries, declared beside qgtc.h until the two are folded
ATTN_HEADS_HEADER = os.path.join(os.path.dirname(HEADER), "qgtc_attn_heads.h")   # the multi-head entries of the attention path, likewise
ADDSCORE_HEADER = os.path.join(os.path.dirname(HEADER), "qgtc_addscore.h")   # the additive edge score (GATv2) and its gradients, likewise

FANOUT_HEADER = os.path.join(os.path.dirname(HEADER), "qgtc_fanout.h")   # fixed-fanout sampling: the selection launches and the _fanout twins, likewise
BLOCKS_HEADER = os.path.join(os.path.dirname(HEADER), "qgtc_blocks.h")   # mini-batch sampling: masked selection, frontier and the _fanout_nodes twins, likewise
BITNODES_HEADER = os.path.join(os.path.dirname(HEADER), "qgtc_bitnodes.h")   # node masks on the bit products: the four _nodes entries, likewise
AFFINE_HEADER = os.path.join(os.path.dirname(HEADER), "qgtc_affine.h")   # affine quantisation: range, quantise + pack, dequantising epilogue, likewise
CODES_HEADER = os.path.join(os.path.dirname(HEADER), "qgtc_codes.h")   # the byte-code route: quantise to bytes, the uint8 gather on both views and its fused epilogue, likewise

_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "size_t": ctypes.c_size_t,
            "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p}
_PROTOTYPE = re.compile(r"^[ \t]*([A-Za-z_][\w \t]*?[ \t*]+)(qgtc_\w+)\s*\(([^()]*)\)\s*;", re.M)

_lib = None


def _argtype(entry: str, decl: str):
    if "*" in decl:
        return ctypes.c_void_p          # any pointer: accepts ints, None, byref(...), arrays and pointer objects
    kind = " ".join(decl.split()[:-1])  # the last word is the parameter's name
    if kind not in _SCALARS:
        raise ValueError(f"{entry}: argument '{decl}' has a type outside the header's vocabulary")
    return _SCALARS[kind]


def signatures(text: str | None = None) -> dict:
    """``{name: (restype, [argtypes])}`` for every prototype of include/qgtc.h (or of ``text``), in header order. A type outside the
    header's small vocabulary is an error naming the entry and the type, never a default."""
    if text is None:
        with open(HEADER) as f:
            text = f.read()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    out = {}
    for ret, name, params in _PROTOTYPE.findall(text):
        ret = " ".join(ret.replace("*", " * ").split())
        if ret not in _RETURNS:
            raise ValueError(f"{name}: return type '{ret}' is outside the header's vocabulary")
        decls = [" ".join(p.split()) for p in params.split(",")]
        out[name] = (_RETURNS[ret], [] if decls == ["void"] else [_argtype(name, d) for d in decls])
    return out


def load():
    """The library, opened once per process, with ``restype`` and ``argtypes`` set on every declared entry - those of include/qgtc.h
    and, through the same parser, those of include/qgtc_heads.h, include/qgtc_attn_heads.h, include/qgtc_addscore.h, include/qgtc_fanout.h, include/qgtc_blocks.h, include/qgtc_bitnodes.h, include/qgtc_affine.h and include/qgtc_codes.h. A declared entry the library does not
    export is an error naming it."""
    global _lib
    if _lib is None:
        lib = ctypes.CDLL(lib_path())
        with open(HEADS_HEADER) as f:
            heads = signatures(f.read())
        with open(ATTN_HEADS_HEADER) as f:
            attn_heads = signatures(f.read())
        with open(ADDSCORE_HEADER) as f:
            addscore = signatures(f.read())
        with open(FANOUT_HEADER) as f:
            fanout = signatures(f.read())
        with open(BLOCKS_HEADER) as f:
            blocks = signatures(f.read())
        with open(BITNODES_HEADER) as f:
            bitnodes = signatures(f.read())
        with open(AFFINE_HEADER) as f:
            affine = signatures(f.read())
        with open(CODES_HEADER) as f:
            codes = signatures(f.read())
        for header, table in (("qgtc.h", signatures()), ("qgtc_heads.h", heads), ("qgtc_attn_heads.h", attn_heads),
                              ("qgtc_addscore.h", addscore), ("qgtc_fanout.h", fanout), ("qgtc_blocks.h", blocks),
                              ("qgtc_bitnodes.h", bitnodes), ("qgtc_affine.h", affine), ("qgtc_codes.h", codes)):
            for name, (restype, argtypes) in table.items():
                try:
                    fn = getattr(lib, name)
                except AttributeError:
                    raise ImportError(f"{lib_path()} does not export {name}, which include/{header} declares") from None
                fn.restype, fn.argtypes = restype, argtypes
        _lib = lib
    return _lib
