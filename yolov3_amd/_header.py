"""Reads the C ABI from the text of include/yolov3_hip.h: constants, ctypes Structures, (restype, argtypes) per export and the exports that launch nothing.
A pure function of the text -- the library is not loaded here.  It understands what the header uses (`#define Y3_NAME int`, enums with explicit values,
`typedef struct` of scalars / pointers / arrays / earlier structs, plain prototypes); anything else raises ValueError quoting the text, nothing is skipped.

Types: a scalar maps to the ctypes class of the same width; `char*` to c_char_p; a pointer to a struct the host passes by reference (BY_REFERENCE) to
POINTER(that class); every other pointer -- device memory, host arrays, `const void* const*`, every pointer field of a struct -- to c_void_p."""
from __future__ import annotations

import ctypes as C
import re
from typing import NamedTuple

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint16_t": C.c_uint16, "uint8_t": C.c_uint8, "size_t": C.c_size_t,
           "float": C.c_float, "double": C.c_double}
BY_REFERENCE = ("y3_tensor", "y3_conv_desc", "y3_nms_params", "y3_loss_params")
_DECL = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w+)((?:\s*\[\s*\d+\s*\])*)")   # [const] type [*...] name [dims]


class Header(NamedTuple):
    constants: dict     # Y3_ABI_VERSION and every enumerator -> int
    structs: dict       # typedef name -> ctypes.Structure subclass, header order
    signatures: dict    # export -> (restype, [argtypes]), header order
    queries: frozenset  # exports whose last parameter is not `void* stream`


def _declaration(text, structs, field=False):
    """`[const] type [*...] name [dims]` -> (name, ctypes class, is `void* stream`)"""
    d = _DECL.fullmatch(text.strip())
    if not d:
        raise ValueError(f"yolov3_hip.h: cannot parse {text!r}")
    base, stars, name = d.group(1), d.group(2).count("*"), d.group(3)
    if base not in SCALARS and base not in structs and base not in ("void", "char"):
        raise ValueError(f"yolov3_hip.h: unknown type {base!r} in {text!r}")
    if stars == 0:
        if base in ("void", "char"):
            raise ValueError(f"yolov3_hip.h: {base!r} by value in {text!r}")
        t = SCALARS.get(base) or structs[base]
    elif stars == 1 and base == "char" and not field:
        t = C.c_char_p
    elif stars == 1 and base in BY_REFERENCE and not field:
        t = C.POINTER(structs[base])
    else:
        t = C.c_void_p
    for dim in reversed(re.findall(r"\d+", d.group(4))):
        t = t * int(dim)
    return name, t, (base, stars, name) == ("void", 1, "stream")


def parse(text: str) -> Header:
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S).replace("\\\n", " ")
    constants = {m.group(1): int(m.group(2)) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(Y3_\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)
    m = re.fullmatch(r'\s*extern\s+"C"\s*\{(.*)\}\s*', text, flags=re.S)
    text = m.group(1) if m else text

    def enum(m):
        for item in filter(None, (s.strip() for s in m.group(1).split(","))):
            e = re.fullmatch(r"(\w+)\s*=\s*(-?\d+)", item)
            if not e:
                raise ValueError(f"yolov3_hip.h: enumerator without an explicit integer value: {item!r}")
            constants[e.group(1)] = int(e.group(2))
        return " "

    text = re.sub(r"\b(?:typedef\s+)?enum\s*\w*\s*\{([^{}]*)\}\s*\w*\s*;", enum, text)
    structs = {}

    def struct(m):
        fields = []
        for stmt in filter(None, (s.strip() for s in m.group(1).split(";"))):   # `int32_t h, w`: the type stands before the first declarator only
            base = re.match(r"(?:const\s+)?\w*", stmt).group(0)
            first, *more = stmt.split(",")
            fields += [_declaration(d, structs, field=True)[:2] for d in [first] + [f"{base} {d}" for d in more]]
        structs[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": fields})
        return " "

    text = re.sub(r"\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    signatures, queries = {}, set()
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        f = re.fullmatch(r"([^()]*)\(([^()]*)\)", stmt)   # a callback parameter brings parentheses of its own: no match
        if not f:
            raise ValueError(f"yolov3_hip.h: cannot parse {stmt!r}")
        if re.fullmatch(r"void\s+\w+\s*", f.group(1)):
            name, restype = f.group(1).split()[1], None
        else:
            name, restype, _ = _declaration(f.group(1), structs)
        params = [] if f.group(2).strip() == "void" else [_declaration(p, structs) for p in f.group(2).split(",")]
        signatures[name] = (restype, [t for _, t, _ in params])
        if not (params and params[-1][2]):
            queries.add(name)
    return Header(constants, structs, signatures, frozenset(queries))
