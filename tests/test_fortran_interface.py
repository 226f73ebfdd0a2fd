"""The ISO_C_BINDING interface module compiles with the image's Fortran compiler and
declares a binding for every compute entry point of the C ABI."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOD = os.path.join(ROOT, "gfdl_atmos_cubed_sphere_amd", "fortran", "fv3_mi355x_mod.F90")


def test_bindings_cover_the_header():
    src = open(MOD).read()
    bound = set(re.findall(r'bind\(C, name="(fv3_[a-z0-9_]+)"\)', src))
    hdr = open(os.path.join(ROOT, "include", "fv3_mi355x.h")).read()
    declared = set(re.findall(r"^(?:int|const char \*)\s*(fv3_[a-z0-9_]+)\(", hdr, flags=re.M))
    # everything the header declares is bound, except the two profiling helpers and memset (host-tool only)
    missing = declared - bound - {"fv3_profile", "fv3_profile_report", "fv3_memset"}
    assert not missing, missing


def test_module_compiles(tmp_path):
    fc = shutil.which("amdflang") or "/opt/rocm/bin/amdflang"
    if not os.path.exists(fc):
        pytest.skip("no Fortran compiler in this image")
    subprocess.check_call([fc, "-c", MOD, "-o", str(tmp_path / "m.o"), "-module-dir", str(tmp_path)])


_BY_VALUE = {"integer(c_int)": "int", "real(c_double)": "double", "integer(c_size_t)": "size_t", "integer(c_long)": "long"}
# what a dummy argument passed by reference points at, as the header spells the pointee
_POINTEE = {"integer(c_int)": "int", "real(c_double)": "double", "integer(c_size_t)": "size_t", "integer(c_long)": "long",
            "integer(c_long_long)": "long long", "integer(c_signed_char)": "unsigned char", "character(kind=c_char)": "char"}


def fortran_interfaces(src):
    """{C name: [kind of each dummy argument, in order]} of every bind(C, name="fv3_*") interface: 'int' / 'double' / 'size_t' /
    'long' by value, 'c_ptr' by value, or 'ref <type>' by reference"""
    src = re.sub(r"&\s*\n\s*&?", " ", re.sub(r"!.*", "", src))
    out = {}
    for m in re.finditer(r'function\s+\w+\s*\(([^)]*)\)\s*bind\(C, name="(fv3_[a-z0-9_]+)"\)(.*?)end function', src, flags=re.S):
        kinds = {}
        for decl in m.group(3).splitlines():
            d = re.fullmatch(r"\s*([^:]+?)\s*::\s*(.+?)\s*", decl)
            if not d or d.group(1).startswith("import"):
                continue
            typ, *attrs = [a.strip() for a in re.split(r",\s*(?![^()]*\))", d.group(1))]
            typ = re.sub(r"\s+", "", typ) if not typ.startswith("type(") else typ
            for name in re.split(r",\s*(?![^()]*\))", d.group(2)):
                name = re.sub(r"\(.*\)", "", name).strip()
                if "value" in attrs:
                    kinds[name] = "c_ptr" if typ == "type(c_ptr)" else _BY_VALUE[typ]
                else:
                    kinds[name] = "ref " + typ
        out[m.group(2)] = [kinds[a.strip()] for a in m.group(1).split(",") if a.strip()]
    return out


def kinds_agree(fortran, c_kind):
    """a dummy argument's kind against the header's parameter"""
    from gfdl_atmos_cubed_sphere_amd import abi
    levels = c_kind.count("*") + c_kind.count("[")
    if fortran in abi.SCALARS:
        return c_kind == fortran
    if fortran == "c_ptr":
        return levels >= 1
    typ = fortran[4:]
    if typ == "type(c_ptr)":                        # an address by reference: a pointer to pointers, or an array of them
        return levels == 2
    base = re.sub(r"\bconst\b|[*\s]|\[\d+\]", "", c_kind)
    want = typ[5:-1] if typ.startswith("type(") else _POINTEE[typ].replace(" ", "")
    return levels == 1 and base == want


def mismatches(mod_src):
    from gfdl_atmos_cubed_sphere_amd import abi
    bad = []
    for name, kinds in fortran_interfaces(mod_src).items():
        params = abi.ROUTINES[name].params
        if len(kinds) != len(params):
            bad.append((name, len(kinds), len(params)))
        bad += [(name, n, f, p.kind) for n, (f, p) in enumerate(zip(kinds, params)) if not kinds_agree(f, p.kind)]
    return bad


def test_dummy_arguments_agree_with_the_header_in_kind():
    """every bind(C) interface against the header's prototype: the number of arguments, and position by position by value as c_int /
    c_double / c_size_t / c_long / c_ptr or by reference (then to the same type) -- a dropped `value` sends an address's address"""
    src = open(MOD).read()
    bound = fortran_interfaces(src)
    assert len(bound) == len(set(re.findall(r'bind\(C, name="(fv3_[a-z0-9_]+)"\)', src))) >= 117
    assert not mismatches(src)
    dropped = src.replace("type(c_ptr), value :: ctx, pe, delp_before, omga", "type(c_ptr) :: ctx, pe, delp_before, omga", 1)
    assert dropped != src and {m[0] for m in mismatches(dropped)} == {"fv3_omga_update"}
