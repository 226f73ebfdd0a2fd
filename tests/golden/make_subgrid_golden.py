"""Golden fixtures of fv_subgrid_z from the REFERENCE's own compiled Fortran:

    python tests/golden/make_subgrid_golden.py

compiles the reference's model/fv_sg.F90, and model/fv_arrays.F90 with model/fv_grid_utils.F90, from where they lie (FV3_REFERENCE) with
REF_FFLAGS of oracle/Makefile, beside this project's stand-ins and bind(C) drivers (tests/golden/subgrid_ref/), into a temporary directory,
runs fv_sg_SHiELD on the cases of tests/subgrid_inputs.SG_CASES and update_dwinds_phys on DW_CASES (grid_type 4; a whole C12 face with
the oracle's geometry) and records their outputs:

    tests/golden/subgrid_<group>.npz:  "<case>|out|<field>" (compute domain) and "<case>|sha" = the checksum of the inputs
    tests/golden/subgrid_dwinds.npz:   "<case>|out|u", "|out|v" (whole arrays) and "<case>|sha" (inputs and geometry)

Data only.  The inputs are not stored: the tests form them again from the seeds and compare the checksum.  Runs only where the
reference tree and amdflang are present; no test reads the reference.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import subgrid_inputs as SI  # noqa: E402

# the reference tree: FV3_REFERENCE, or a directory `reference` beside this repository
REFERENCE = os.environ.get("FV3_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "reference"))
LIMIT = 213341        # the largest golden committed before (ppm1d_golden.npz)


def ref_fflags():
    mk = open(os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "Makefile")).read()
    return re.search(r"^REF_FFLAGS \?= (.*)$", mk, flags=re.M).group(1).split()


def build(tmp, name, files):
    """the files, in order, into <tmp>/<name>/lib<name>.so (a directory of its own: the two libraries have stand-in modules of the same names)"""
    fc = shutil.which("amdflang") or "/opt/rocm/bin/amdflang"
    src = os.path.join(HERE, "subgrid_ref")
    fl = ref_fflags() + ["-I" + src]
    d = os.path.join(tmp, name)
    os.makedirs(d)
    objs = []
    for f in files:
        f = os.path.join(src, f) if os.sep not in f else f
        o = os.path.join(d, os.path.basename(f)[:-4] + ".o")
        subprocess.check_call([fc, *fl, "-c", f, "-o", o], cwd=d)
        objs.append(o)
    so = os.path.join(d, f"lib{name}.so")
    subprocess.check_call([fc, "-shared", "-o", so, *objs], cwd=d)
    return C.CDLL(so)


def build_sg(tmp):
    return build(tmp, "sgref", ("sg_standins.F90", os.path.join(REFERENCE, "model", "fv_sg.F90"), "sg_driver.F90"))


def build_dw(tmp):
    return build(tmp, "dwref", ("gu_standins.F90", os.path.join(REFERENCE, "model", "fv_arrays.F90"),
                                os.path.join(REFERENCE, "model", "fv_grid_utils.F90"), "dw_driver.F90"))


def dw_checksum(t, geom):
    return SI.checksum(dict(t, **{"geom_" + k: v for k, v in (geom or {}).items()}))


def run_dw(dll, name):
    import grid_oracle as GO
    c = SI.DW_CASES[name]
    bd, npx, npy, t, geom = SI.dw_case_inputs(name)
    sha = dw_checksum(t, geom)
    npz = c["npz"]
    if geom is None:
        z = lambda *shape: np.zeros(shape, order="F")      # noqa: E731
        nid, njd = bd.shape("A")
        full = dict(vlon=z(nid, njd, 3), vlat=z(nid, njd, 3), es=z(3, nid, njd + 1, 2), ew=z(3, nid + 1, njd, 2), edge_vect_w=z(njd),
                    edge_vect_e=z(njd), edge_vect_s=z(nid), edge_vect_n=z(nid))
    else:
        full = SI.oracle_dwinds_reference_shapes(GO.ref_sphere(c["npx"]), c["face"])
    full = {k: np.asfortranarray(v, dtype=np.float64) for k, v in full.items()}
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    i = C.c_int
    dll.dw_run(i(bd.is_), i(bd.ie), i(bd.js), i(bd.je), i(bd.ng), i(npx), i(npy), i(npz), i(c["grid_type"]), C.c_double(SI.DW_DT),
               *(p(t[n]) for n in ("u_dt", "v_dt", "u", "v")),
               *(p(full[n]) for n in ("vlon", "vlat", "es", "ew", "edge_vect_w", "edge_vect_e", "edge_vect_s", "edge_vect_n")))
    return {f"{name}|out|u": t["u"], f"{name}|out|v": t["v"], f"{name}|sha": np.array(sha)}


def run_sg(dll, name):
    c = SI.SG_CASES[name]
    bd, st = SI.sg_case_inputs(name)
    sha = SI.checksum(st)
    sp = SI.SPECIES_OF[c["nwat"]]
    idx = (C.c_int * 7)(*[sp.get(n, 0) for n in SI.SPECIES], 0)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    for n in st:
        assert st[n].flags.f_contiguous and st[n].dtype == np.float64, n
    i = C.c_int
    dll.sg_run(i(bd.is_), i(bd.ie), i(bd.js), i(bd.je), i(bd.ng), i(c["km"]), i(c["nq"]), i(c["nqa"]), C.c_double(SI.DT), i(SI.FV_SG_ADJ),
               i(c["fv_sg_adj_weak"]), i(c["nwat"]), idx, i(int(c["hydrostatic"])), i(c["k_bot_full"]),
               *(p(st[n]) for n in ("delp", "pe", "peln", "pkz", "ta", "qa", "ua", "va", "w", "delz", "u_dt", "v_dt")))
    r = (bd.is_, bd.ie, bd.js, bd.je)
    out = {f"{name}|out|{n}": np.ascontiguousarray(bd.view(st[n], "A", *r)) for n in SI.SG_OUT}
    out[f"{name}|sha"] = np.array(sha)
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        dll = build_sg(tmp)
        files = {}
        for name, c in SI.SG_CASES.items():
            files.setdefault(c["group"], {}).update(run_sg(dll, name))
        dw = build_dw(tmp)
        files["dwinds"] = {}
        for name in SI.DW_CASES:
            files["dwinds"].update(run_dw(dw, name))
        for group, d in files.items():
            path = os.path.join(HERE, f"subgrid_{group}.npz")
            np.savez_compressed(path, **d)
            print(f"{os.path.basename(path)}: {len(d)} arrays, {os.path.getsize(path)} bytes")
            assert os.path.getsize(path) <= LIMIT, "larger than the largest golden committed before"


if __name__ == "__main__":
    main()
