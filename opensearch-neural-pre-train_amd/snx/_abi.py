"""The C ABI as ctypes, read from include/snx.h: the header is the only statement of the prototypes, the structs and
the constants.

The reader knows the forms the header uses and no more.  A declaration it cannot type raises at import and names the
declaration; it never guesses a type."""
from __future__ import annotations

import ctypes as C
import os
import re


class SnxLibraryError(RuntimeError):
    pass


# ROOT/include, as snx/build.py locates it
_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HEADER = os.path.join(_ROOT, "include", "snx.h")

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double,
            "size_t": C.c_size_t, "hipStream_t": C.c_void_p}
_NAME = re.compile(r"\b\w+$")          # the declared name that ends a parameter or field


def _ctype(ctype: str, where: str):
    t = " ".join(ctype.replace("*", " * ").split())
    if t == "const char *":
        return C.c_char_p
    if t.endswith("*"):
        return C.c_void_p
    if t not in _SCALARS:
        raise SnxLibraryError(f"include/snx.h, {where}: no ctypes mapping for the type {t!r}")
    return _SCALARS[t]


def parse(text: str):
    """Header text -> (prototypes: name -> (restype, argtypes), structs: name -> ctypes.Structure subclass,
    constants: name -> int)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    define = r"^[ \t]*#[ \t]*define[ \t]+(SNX_\w+)[ \t]+\(?[ \t]*(-?\d+)[ \t]*\)?[ \t]*$"
    constants = {m[1]: int(m[2]) for m in re.finditer(define, text, flags=re.M)}
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{', "", text, flags=re.M)

    structs = {}

    def struct(m):
        fields = []
        for decl in filter(None, (d.strip() for d in m[2].split(";"))):
            first, *more = (s.strip() for s in decl.split(","))
            ctype = _ctype(_NAME.sub("", first), f"struct {m[1]}")
            fields += [(n, ctype) for n in (_NAME.search(first)[0], *more)]
        structs[m[1]] = type(m[1], (C.Structure,), {"_fields_": fields})
        return ""
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", struct, text, flags=re.S)

    prototypes = {}
    for stmt in text.split(";"):
        if "(" not in stmt:
            continue
        m = re.fullmatch(r"\s*(.*?)\b(\w+)\s*\((.*)\)\s*", stmt, flags=re.S)
        if not m:
            raise SnxLibraryError(f"include/snx.h: not a prototype: {' '.join(stmt.split())!r}")
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        prototypes[name] = (_ctype(ret, name), [_ctype(_NAME.sub("", p.strip()), name) for p in params])
    return prototypes, structs, constants


def load(path: str = HEADER):
    try:
        with open(path, encoding="utf-8") as f:
            text = f.read()
    except OSError as e:
        raise SnxLibraryError(f"{path} not found: the Python layer binds libsnx.so from this header") from e
    return parse(text)


PROTOTYPES, STRUCTS, CONSTANTS = load()
