"""Reader of include/metaenc.h: the header is the one description of the C ABI, and _capi.py builds its ctypes structures,
signatures and constants from what this module returns.  Pure Python (neither torch nor the library is imported).

The header is plain C with a regular shape, and the reader takes exactly that shape: integer constants (``enum { NAME = int }``,
``#define ME_X int``), ``typedef struct me_x { ... } me_x;`` and prototypes ``ret me_x(args);``.  A declaration of any other form
raises HeaderError naming it -- nothing is skipped.
"""
from __future__ import annotations

import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "metaenc.h")
SCALARS = ("int", "int32_t", "int64_t", "uint64_t", "float", "size_t")


class HeaderError(ValueError):
    pass


def _ctype(spelling: str, decl: str) -> str:
    """'const  float *' -> 'const float*'; a type that is neither a pointer nor one of SCALARS raises."""
    t = re.sub(r"\*(?=\w)", "* ", re.sub(r"\s*\*", "*", " ".join(spelling.split())))
    if not re.fullmatch(r"(const )?\w+(\*( const)?)*", t) or ("*" not in t and t not in SCALARS):
        raise HeaderError(f"unknown type '{spelling.strip()}' in: {decl}")
    return t


def _split(text: str, sep: str) -> list:
    """pieces of text between separators that stand outside every brace"""
    out, depth, start = [], 0, 0
    for i, ch in enumerate(text):
        depth += (ch == "{") - (ch == "}")
        if ch == sep and depth == 0:
            out.append(text[start:i].strip())
            start = i + 1
    if depth != 0 or text[start:].strip():
        raise HeaderError(f"unterminated declaration: {' '.join(text[start:].split())[:120]}")
    return out


def _int(value: str, constants: dict, decl: str) -> int:
    try:
        return constants[value] if value in constants else int(value, 0)
    except ValueError:
        raise HeaderError(f"'{value}' is not an integer constant in: {decl}") from None


def _fields(body: str, constants: dict, decl: str) -> list:
    """members of a struct body -> [(name, C type)]; a nested ``struct { ... } name[N]`` gives (name, ([members], N))"""
    out = []
    for member in _split(body, ";"):
        nested = re.fullmatch(r"struct\s*\{(.*)\}\s*(\w+)\s*\[\s*(\w+)\s*\]", member, re.S)
        if nested:
            inner = _fields(nested.group(1), constants, decl)
            if any(not isinstance(t, str) for _, t in inner):
                raise HeaderError(f"more than one level of nested struct in: {decl}")
            out.append((nested.group(2), (inner, _int(nested.group(3), constants, decl))))
            continue
        m = re.fullmatch(r"((?:const\s+)?\w+)\b(.*)", member, re.S)
        if not m:
            raise HeaderError(f"cannot read member '{member}' of: {decl}")
        for d in m.group(2).split(","):
            dm = re.fullmatch(r"\s*([\s*]*)(\w+)\s*", d)
            if not dm:
                raise HeaderError(f"cannot read member '{member}' of: {decl}")
            out.append((dm.group(2), _ctype(m.group(1) + dm.group(1), decl)))
    return out


def parse(text: str):
    """C text -> (constants {name: int}, structs {name: [(field, type)]}, prototypes {name: (return type, [(type, arg name)])})"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b[^\n]*", " ", text, flags=re.S | re.M)   # (read as C)
    constants, structs, protos, code = {}, {}, {}, []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        m = re.fullmatch(r"\s*#\s*define\s+(\w+)(.*)", line)
        if m and m.group(2).strip():
            constants[m.group(1)] = _int(m.group(2).strip(), constants, line.strip())
    for decl in _split("\n".join(code), ";"):
        flat = " ".join(decl.split())
        m = re.fullmatch(r"enum\s*\{(.*)\}", decl, re.S)
        if m:
            for entry in m.group(1).split(","):
                e = re.fullmatch(r"\s*(\w+)\s*=\s*(\S+)\s*", entry)
                if not e:
                    raise HeaderError(f"enum entry '{entry.strip()}' is not NAME = int in: {flat}")
                constants[e.group(1)] = _int(e.group(2), constants, flat)
            continue
        if re.fullmatch(r"typedef\s+struct\s+(\w+)\s+\1", decl):       # opaque handle (me_comm): nothing to mirror
            continue
        m = re.fullmatch(r"typedef\s+struct\s+(\w+)\s*\{(.*)\}\s*\1", decl, re.S)
        if m:
            structs[m.group(1)] = _fields(m.group(2), constants, flat)
            continue
        m = re.fullmatch(r"([\w\s*]+?)\b(\w+)\s*\(([^(){}]*)\)", decl, re.S)
        if not m:
            raise HeaderError(f"cannot read declaration: {flat[:200]}")
        args = []
        if m.group(3).strip() != "void":
            for a in m.group(3).split(","):
                am = re.fullmatch(r"(.*?)\b(\w+)\s*", a, re.S)
                if not am or not am.group(1).strip():
                    raise HeaderError(f"cannot read argument '{a.strip()}' of: {flat}")
                args.append((_ctype(am.group(1), flat), am.group(2)))
        protos[m.group(2)] = (_ctype(m.group(1), flat), args)
    return constants, structs, protos


def read():
    with open(HEADER_PATH) as f:
        return parse(f.read())
