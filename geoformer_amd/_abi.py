"""The C ABI as ctypes sees it, read from include/geoformer_hip.h and include/geoformer_hip_dev.h.

The two headers are the single source of every entry point's signature, every parameter struct's layout and every
``GF_*`` integer (``#define`` or enumerator with a written value) the host code uses: nothing of them is restated in
Python.  This is a regex pass over this project's own header style, not a C parser, and it is strict: a declaration
it does not understand is a GeoFormerHipError naming the header line, never a default type.
"""
from __future__ import annotations

import ctypes
import functools
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_uint, c_ulonglong, c_void_p
from typing import NamedTuple

from ._build import INCLUDE_DIR

HEADERS = ("geoformer_hip.h", "geoformer_hip_dev.h")  # in include order: the second uses the first's types

_SCALARS = {"int": c_int, "int32_t": c_int, "unsigned": c_uint, "uint32_t": c_uint, "float": c_float,
            "double": c_double, "size_t": c_size_t, "long long": c_longlong, "unsigned long long": c_ulonglong}


class Abi(NamedTuple):
    functions: dict  # name -> (restype, [argtypes]), header order
    structs: dict    # typedef name -> ctypes.Structure subclass, header order
    consts: dict     # GF_* -> int
    fnptrs: set      # names of function-pointer typedefs (passed as c_void_p)


def _blank(m):
    return " " + "\n" * m.group().count("\n")  # line numbers stay those of the header


def _unqualified(t):
    return " ".join(w for w in t.split() if w not in ("const", "volatile"))


def parse(text, label="<header>", abi=None):
    """Add the declarations of one header's text to `abi` (a new one when None) and return it."""
    abi = abi or Abi({}, {}, {}, set())

    def err(pos, what):
        from ._lib import GeoFormerHipError

        raise GeoFormerHipError(f"{label}:{text.count(chr(10), 0, pos) + 1}: {what}")

    text = re.sub(r"/\*.*?\*/|//[^\n]*", _blank, text, flags=re.S)
    text = re.sub(r"^#ifdef __cplusplus\n.*?^#endif", _blank, text, flags=re.S | re.M)  # extern "C" { / }
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(GF_\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", text, re.M):
        abi.consts[m[1]] = int(m[2], 0)
    text = re.sub(r"^[ \t]*#[^\n]*", _blank, text, flags=re.M)

    def field_type(base, is_ptr, dim, pos):
        key = _unqualified(base)
        t = c_void_p if is_ptr else _SCALARS.get(key) or abi.structs.get(key) or err(pos, f"unknown type {key!r}")
        if dim is None:
            return t
        n = int(dim) if dim.isdigit() else abi.consts.get(dim)
        return t * n if n is not None else err(pos, f"unknown array length {dim!r}")

    def fields(decl, pos):  # "const float *gamma, *beta" / "int M, ld" / "GfResBlockParams blocks[2]"
        first, *rest = decl.split(",")
        m = re.fullmatch(r"(.*?[\s*])(\w+)\s*(?:\[(\w+)\])?\s*", first, re.S) or \
            err(pos, f"struct member did not parse: {decl!r}")
        base = m[1].partition("*")[0]
        out = [(m[2], field_type(base, "*" in m[1], m[3], pos))]
        for d in rest:
            m = re.fullmatch(r"\s*(\**)\s*(\w+)\s*(?:\[(\w+)\])?\s*", d) or \
                err(pos, f"struct member did not parse: {decl!r}")
            out.append((m[2], field_type(base, bool(m[1]), m[3], pos)))
        return out

    def struct(m):
        body = m.start("body")
        fs = [f for d in re.finditer(r"[^;\s][^;]*", m["body"]) for f in fields(d[0], body + d.start())]
        abi.structs[m["name"]] = type(m["name"], (ctypes.Structure,), {"_fields_": fs})
        return _blank(m)

    def fnptr(m):
        abi.fnptrs.add(m[1])
        return _blank(m)

    text = re.sub(r"typedef\s+struct\s*\w*\s*\{(?P<body>[^{}]*)\}\s*(?P<name>\w+)\s*;", struct, text)
    def enum(m):  # enumerators with a written integer value are constants like the #defines
        for e in re.finditer(r"\b(GF_\w+)\s*=\s*(-?(?:0[xX][0-9a-fA-F]+|\d+))\s*(?=[,}])", m[0]):
            abi.consts[e[1]] = int(e[2], 0)
        return _blank(m)

    text = re.sub(r"(?:typedef\s+)?enum\s*\w*\s*\{[^{}]*\}\s*\w*\s*;", enum, text)
    text = re.sub(r"typedef\s+\w+\s*\(\s*\*\s*(\w+)\s*\)\s*\([^()]*\)\s*;", fnptr, text)

    # what is left is prototypes, one per ';'
    for d in re.finditer(r"[^;\s][^;]*", text):
        m = re.fullmatch(r"([\w\s*]+?)\s*\b(gf_\w+)\s*\(([^()]*)\)\s*", d[0]) or \
            err(d.start(), f"not a gf_* prototype: {d[0].splitlines()[0]!r}")
        ret, name, params = m.groups()
        if name in abi.functions:
            err(d.start(), f"{name} is declared twice")
        if "*" in ret:
            res = c_char_p if _unqualified(ret.replace("*", " ")) == "char" else c_void_p
        else:
            res = _SCALARS.get(_unqualified(ret)) or err(d.start(), f"{name}: unknown return type {ret!r}")
        args = []
        for p in params.split(",") if params.strip() != "void" else ():
            if "*" in p:
                args.append(c_void_p)
                continue
            pm = re.fullmatch(r"\s*(.*\S)\s+\w+\s*", p, re.S)  # every parameter is named
            key = _unqualified(pm[1]) if pm else ""
            args.append(_SCALARS.get(key) or (c_void_p if key in abi.fnptrs else None) or
                        err(d.start(), f"{name}: unknown parameter type in {p.strip()!r}"))
        abi.functions[name] = (res, args)
    return abi


@functools.lru_cache(maxsize=None)
def _headers():
    abi = None
    for h in HEADERS:
        with open(os.path.join(INCLUDE_DIR, h)) as f:
            abi = parse(f.read(), h, abi)
    return abi


def _lookup(table, name, kind):
    if name not in table:
        from ._lib import GeoFormerHipError

        raise GeoFormerHipError(f"include/{HEADERS[0]} and {HEADERS[1]} declare no {kind} {name}")
    return table[name]


def functions():
    """{name: (restype, [argtypes])} of every gf_* prototype of the two headers."""
    return _headers().functions


def struct(name):
    """The ctypes.Structure of `typedef struct { ... } name;` (one class per process)."""
    return _lookup(_headers().structs, name, "struct")


def const(name):
    """The integer of `#define name <integer>`."""
    return _lookup(_headers().consts, name, "constant")
