"""The C ABI as include/fv3_mi355x.h declares it: the header is the single source of the Python binding.

``parse`` reads the prototypes and the ``typedef struct``s; ``ROUTINES`` / ``STRUCTS`` hold them for the header of this tree,
``CLASSES`` the ctypes.Structure classes generated from the structs, and ``bind`` sets ``restype`` / ``argtypes`` on a loaded
library.  A declaration the reader cannot classify raises ``AbiError``: nothing is skipped.

Kinds: a by-value parameter or field is ``int``, ``double``, ``size_t`` or ``long``; everything passed by address (data
pointers, handles, struct pointers, array parameters such as ``size_t elems[8]``) keeps its C spelling with the name taken out
(``const double *``, ``fv3_ctx *``, ``size_t [8]``) and binds as ``c_void_p``, which takes byref(...), ctypes arrays and
pointers, ``ndarray.ctypes``, an address, None and any object with ``_as_parameter_``.
"""
from __future__ import annotations

import ctypes as C
import keyword
import os
import re
from typing import NamedTuple

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fv3_mi355x.h")
SCALARS = {"int": C.c_int, "double": C.c_double, "size_t": C.c_size_t, "long": C.c_long}
RETURNS = dict(SCALARS, **{"const char *": C.c_char_p})
_POINTEES = {"void", "char", "unsigned char", "long long"} | set(SCALARS)


class AbiError(RuntimeError):
    pass


class Param(NamedTuple):
    name: str
    kind: str      # a key of SCALARS, or the C type of something passed by address

    @property
    def by_address(self):
        return self.kind not in SCALARS


class Routine(NamedTuple):
    name: str
    returns: str   # a key of RETURNS
    params: tuple


class Field(NamedTuple):
    name: str
    kind: str      # a key of SCALARS, the name of an earlier struct (nested by value), or a pointer type
    count: int     # 0, or the length of an array member


def _declarator(base, text, types, where):
    """'*const sendbuf[8]' after the base type 'double' -> ('sendbuf', 'double *const [8]'); the base type must be known"""
    m = re.fullmatch(r"((?:\*\s*(?:const\b\s*)?)*)(\w+)\s*(\[\d+\])?", text.strip())
    if not m or base.replace("const ", "") not in types:
        raise AbiError(f"{where}: cannot classify '{base} {text.strip()}'")
    stars, name, dim = re.sub(r"\s+", "", m.group(1)), m.group(2), m.group(3) or ""
    return name, " ".join(p for p in (base, stars, dim) if p)


def _split(decl, where):
    """'const double *area' -> ('const double', '*area'): the base type and the (first) declarator of a declaration"""
    m = re.fullmatch(r"([\w ]+?)\s*(\*.*|\w+\s*(?:\[\d+\])?)", decl.strip())
    if not m:
        raise AbiError(f"{where}: cannot read '{decl.strip()}'")
    return re.sub(r"\s+", " ", m.group(1)), m.group(2)


def parse(text):
    """-> ({name: Routine}, {name: (Field, ...)}) of every prototype and every typedef struct with a body in the header text"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    routines, structs, opaque = {}, {}, set()
    for stmt in re.split(r";(?![^{]*\})", text):          # the ';' that end a statement, not those inside a struct body
        stmt = " ".join(stmt.split())
        if stmt in ("", "}"):
            continue
        types = _POINTEES | opaque | set(structs)
        if m := re.fullmatch(r"typedef struct (\w+) (\w+)", stmt):
            opaque.add(m.group(2))
        elif m := re.fullmatch(r"typedef struct (\w+) \{(.*)\} (\w+)", stmt):
            fields = []
            for decl in filter(None, (d.strip() for d in m.group(2).split(";"))):
                first, *more = decl.split(",")
                base, d0 = _split(first, m.group(1))
                for d in [d0] + more:
                    name, kind = _declarator(base, d, types, m.group(1))
                    n = re.search(r"\[(\d+)\]$", kind)
                    kind = kind[:n.start()].strip() if n else kind
                    if "*" not in kind and kind not in SCALARS and kind not in structs:
                        raise AbiError(f"{m.group(1)}.{name}: a '{kind}' member by value")
                    fields.append(Field(name, kind, int(n.group(1)) if n else 0))
            structs[m.group(3)] = tuple(fields)
        elif m := re.fullmatch(r"(const char \*|int |long )(\w+) ?\((.*)\)", stmt):
            params = []
            for p in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
                name, kind = _declarator(*_split(p, m.group(2)), types, m.group(2))
                if "*" not in kind and "[" not in kind and kind not in SCALARS:
                    raise AbiError(f"{m.group(2)}: parameter '{name}' of the type '{kind}' by value")
                params.append(Param(name, kind))
            routines[m.group(2)] = Routine(m.group(2), m.group(1).strip(), tuple(params))
        else:
            raise AbiError(f"cannot classify the declaration '{stmt[:80]}'")
    return routines, structs


def struct_classes(structs):
    """{name: ctypes.Structure class} in the header's layout; a member whose name Python reserves gets a trailing '_' (is -> is_)"""
    out = {}
    for name, fields in structs.items():
        fs = []
        for f in fields:
            t = SCALARS.get(f.kind) or out.get(f.kind) or C.c_void_p
            fs.append((f.name + "_" * keyword.iskeyword(f.name), t * f.count if f.count else t))
        out[name] = type(name, (C.Structure,), {"_fields_": fs})
    return out


def bind(dll, routines=None):
    """restype and argtypes of every declared routine the loaded object has -> {name: the bound function}"""
    fns = {}
    for r in (routines or ROUTINES).values():
        if hasattr(dll, r.name):
            fn = fns[r.name] = getattr(dll, r.name)
            fn.restype = RETURNS[r.returns]
            fn.argtypes = [C.c_void_p if p.by_address else SCALARS[p.kind] for p in r.params]
    return fns


with open(HEADER) as _f:
    ROUTINES, STRUCTS = parse(_f.read())
CLASSES = struct_classes(STRUCTS)
