"""The Python binding takes its signatures and structs from include/fv3_mi355x.h (gfdl_atmos_cubed_sphere_amd/abi.py): the reader
against a cruder regex, the generated ctypes classes against the C compiler's own layout, what Fv3Lib.call refuses before the
library sees it, and a variant build loaded with a shorter EXPORTS.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from gfdl_atmos_cubed_sphere_amd import abi
from gfdl_atmos_cubed_sphere_amd import lib as L
from gfdl_atmos_cubed_sphere_amd.layout import Bounds
from gfdl_atmos_cubed_sphere_amd.grid import doubly_periodic

from parity_phys import emu  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fv3_mi355x.h")
# every spelling of a parameter the header uses today, by value and by address; a new one is looked at before it is added here
KINDS = set(abi.SCALARS) | {
    "fv3_ctx *", "const fv3_ctx *", "fv3_ctx **", "fv3_ctx *const*", "fv3_group *", "fv3_group **", "fv3_gather *", "const fv3_gather *",
    "fv3_gather **", "void *", "const void *", "void **", "double *", "const double *", "double *const*", "int *", "const int *", "long *",
    "long long *", "const size_t *", "char *", "unsigned char *", "const unsigned char *", "size_t [8]", "double [3]", "double *const [8]",
    "const double *const [8]"}


def test_reader_finds_what_a_cruder_regex_finds():
    hdr = open(HEADER).read()
    assert abi.HEADER == HEADER
    declared = set(re.findall(r"\b(fv3_[a-z0-9_]+)\s*\(", hdr))                    # the regex of test_product_isolation.py
    structs = set(re.findall(r"^\}\s*(fv3_[a-z0-9_]+)\s*;", hdr, flags=re.M))       # the line that closes a typedef struct
    assert len(declared) > 100 and len(structs) > 10
    assert set(abi.ROUTINES) == declared == set(L.EXPORTS)
    assert set(abi.STRUCTS) == structs == set(abi.CLASSES)
    for r in abi.ROUTINES.values():
        assert r.returns in abi.RETURNS, r
        for p in r.params:
            assert p.kind in KINDS or re.fullmatch(r"const (fv3_\w+) \*", p.kind).group(1) in structs, (r.name, p)
            assert p.by_address == ("*" in p.kind or "[" in p.kind)
    assert sum(len(f) for f in abi.STRUCTS.values()) == sum(len(c._fields_) for c in abi.CLASSES.values()) > 100


@pytest.mark.parametrize("text", [
    "int fv3_x(fv3_ctx *ctx, float y);",                       # a type the binding has no scalar for
    "int fv3_x(unknown_t *p);",                                # a pointer to something never declared
    "int fv3_x(fv3_domain d);\n",                              # a struct by value
    "short fv3_x(void);",                                      # a return type
    "typedef struct fv3_s { float a; } fv3_s;",
    "typedef struct fv3_s { int (*fn)(int); } fv3_s;",
    "#define FV3_X 1\nenum fv3_e { A, B };",
])
def test_reader_refuses_what_it_cannot_classify(text):
    with pytest.raises(abi.AbiError):
        abi.parse("typedef struct fv3_ctx fv3_ctx;\ntypedef struct fv3_domain { int a; } fv3_domain;\n" + text)


def test_struct_layout_is_the_compilers(tmp_path):
    """sizeof and every offsetof as the host C compiler lays the header's structs out, against the generated ctypes classes: the check
    that does not depend on the reader (the member lists come from it; a member it lost shifts a size or an offset)"""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {"]
    for s, fields in abi.STRUCTS.items():
        lines.append(f'  printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'  printf("{s}.{f.name} %zu\\n", offsetof({s}, {f.name}));' for f in fields]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.check_call([cc, str(src), "-o", str(tmp_path / "layout")])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    want = {}
    for s, cls in abi.CLASSES.items():
        want[s] = str(C.sizeof(cls))
        for (n, _), f in zip(cls._fields_, abi.STRUCTS[s]):
            want[f"{s}.{f.name}"] = str(getattr(cls, n).offset)
    assert len(abi.CLASSES) == 19 and got == want
    k = abi.CLASSES["fv3_reed_params"]().k                    # nested by value, an array member
    assert isinstance(k, abi.CLASSES["fv3_reed_consts"]) and len(abi.CLASSES["fv3_grid_cubed"]().corner_f) == 12


@pytest.fixture()
def ctx(emu):  # noqa: F811
    bd = Bounds(1, 8, 1, 8)
    c = L.Context(doubly_periodic(bd, 9, 9, dx_const=1.0, dy_const=1.0), 4, lib=emu)
    yield c
    c.close()


def test_none_for_a_required_field_never_reaches_the_library(ctx, monkeypatch):
    reached = []
    monkeypatch.setitem(ctx.lib.fn, "fv3_update_dz_c", lambda *a: reached.append(a) or 0)
    f = [ctx.zeros("A", 5) for _ in range(5)]
    with pytest.raises(L.Fv3Error, match=r"fv3_update_dz_c: argument 2 \(zs\) is None"):
        ctx.update_dz_c(1.0, None, *f)             # fv3_update_dz_c takes zs unchecked
    with pytest.raises(L.Fv3Error, match=r"fv3_update_dz_c: argument 7 \(ws\) is None"):
        ctx.update_dz_c(1.0, *f, None)
    assert not reached
    ctx.update_dz_c(1.0, *f, f[0])
    assert len(reached) == 1 and None not in reached[0]


def test_an_optional_pointer_arrives_as_null(ctx):
    q = ctx.zeros("A", 4)
    ctx.set_condensate(q, q)
    ctx.set_condensate(None, None)                                   # _pp(None): the entry takes NULL as "off"
    ctx.set_dp_ref(np.ones(4))
    with pytest.raises(L.Fv3Error, match="fv3_set_dp_ref: null argument"):
        ctx.call("fv3_set_dp_ref", L._pp(None))                      # ... and this one refuses the NULL it is handed
    with pytest.raises(L.Fv3Error, match=r"fv3_set_dp_ref: argument 1 \(dp0\) is None"):
        ctx.call("fv3_set_dp_ref", None)
    assert q._as_parameter_ == q.ptr == C.cast(q.p, C.c_void_p).value


def test_a_wrapper_takes_any_array_with_a_p(ctx):
    """a caller's own view of a device array has DeviceArray's .p and nothing else, as tests/parity_diag.py's Slab"""
    class View:
        def __init__(self, a, elems):
            self.p = C.cast(C.c_void_p(a.ptr + 8 * elems), C.POINTER(C.c_double))

    a = ctx.zeros("A", 2)
    n = a.shape[0] * a.shape[1]
    a.upload(np.arange(2.0 * n).reshape(a.shape, order="F"))
    for level1 in (View(a, n), L._pp(View(a, n))):                   # required, and marked optional
        host = np.empty(n)
        ctx.call("fv3_memcpy_d2h", host.ctypes, level1, 8 * n)
        ctx.sync()
        assert np.array_equal(host, np.arange(n, 2.0 * n))
    with pytest.raises(C.ArgumentError):
        ctx.call("fv3_memcpy_d2h", host.ctypes, object(), 8 * n)


def test_direct_calls_take_what_the_tests_and_bench_pass(ctx):
    """byref, ctypes arrays and pointers, ndarray.ctypes, ctypes scalars, bare sizes and None on the bound functions themselves"""
    dll, h = ctx.lib.dll, ctx.h
    a, host = ctx.zeros("A", 1), np.arange(4.0)
    assert dll.fv3_memcpy_h2d(h, C.c_void_p(a.ptr), host.ctypes.data_as(C.POINTER(C.c_double)), C.c_size_t(32)) == 0
    out = (C.c_double * 4)()
    assert dll.fv3_memcpy_d2h(h, out, a.p, 32) == 0 and dll.fv3_sync(h) == 0 and list(out) == [0.0, 1.0, 2.0, 3.0]
    assert dll.fv3_memcpy_d2h(h, host[::-1].copy().ctypes, a, 32) == 0
    assert dll.fv3_registry_forget(h, None, C.c_int(0)) == 0
    assert dll.fv3_set_condensate(h, None, None) == 0
    with pytest.raises(C.ArgumentError):
        dll.fv3_memcpy_d2h(h, out, a.p, 32.0)                        # a float where the header says size_t
    assert dll.fv3_last_error.restype is C.c_char_p and dll.fv3_cube_table.restype is C.c_long


def test_variant_loading_binds_what_exists(emu, monkeypatch):  # noqa: F811
    monkeypatch.setattr(L, "EXPORTS", ["fv3_last_error", "fv3_create"])
    lib = L.Fv3Lib(emu.path)
    assert set(lib.fn) == set(abi.ROUTINES)               # the object has all of the header: all of it is bound
    assert lib.dll.fv3_d_sw.argtypes == [C.c_void_p] * 30 and lib.dll.fv3_malloc.argtypes == [C.c_void_p, C.c_size_t]
    del lib.fn["fv3_sync"]                                 # a routine a variant build does not have is an error where it is called
    with pytest.raises(L.Fv3Error, match="has no fv3_sync"):
        lib.call("fv3_sync", C.c_void_p())
    monkeypatch.setattr(L, "EXPORTS", ["fv3_last_error", "fv3_no_such_entry"])
    with pytest.raises(L.Fv3Error, match="does not export"):
        L.Fv3Lib(emu.path)
