"""Golden fixtures of fv_update_phys from the REFERENCE's own compiled Fortran:

    python tests/golden/make_update_phys_golden.py [--measure]

compiles, from where they lie (FV3_REFERENCE) and unmodified, with REF_FFLAGS of oracle/Makefile: this project's stand-ins
(tests/golden/update_phys_ref/up_standins.F90), the reference's tools/fv_eta.F90 (get_eta_level), model/fv_arrays.F90,
model/fv_grid_utils.F90, the stand-ins that need fv_arrays_mod (up_standins_post.F90), model/fv_thermodynamics.F90 (moist_cp,
moist_cv), model/fv_update_phys.F90 and the bind(C) driver up_driver.F90, into a temporary directory; runs the WHOLE fv_update_phys
on the cases of tests/update_phys_inputs.CASES -- a one-rank doubly periodic domain (grid_type 4), where a periodic fill is an honest
start_group_halo_update, so update_dwinds_phys is part of what is recorded -- and records the outputs:

    tests/golden/update_phys_<group>.npz:  "<case>|out|<field>" (the range the routine writes) and "<case>|sha" = the checksum of the inputs

Data only.  The inputs are not stored: the tests form them again from the seeds and compare the checksum.  The gfs_phys form of the
routine (the reference's GFS_PHYS build) is not recorded: its cubed_to_latlon needs a vector halo update no stand-in can give.
--measure: nothing is written; the library of the CPU harness (tests/hostemu) is run on every case and the relative RMS and max norm
of peln, pk, pkz (include/fv3_math.h against the compiled reference's libm) are printed -- the figures the tests' bounds come from.
Runs only where the reference tree and amdflang are present; no test reads the reference.
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

import update_phys_inputs as UI  # noqa: E402

# the reference tree: FV3_REFERENCE, or a directory `reference` beside this repository
REFERENCE = os.environ.get("FV3_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "reference"))
LIMIT = 213341        # the largest golden committed before (ppm1d_golden.npz)


def ref_fflags():
    mk = open(os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "Makefile")).read()
    return re.search(r"^REF_FFLAGS \?= (.*)$", mk, flags=re.M).group(1).split()


def build(tmp):
    fc = shutil.which("amdflang") or "/opt/rocm/bin/amdflang"
    src = os.path.join(HERE, "update_phys_ref")
    ref = lambda *p: os.path.join(REFERENCE, *p)      # noqa: E731
    fl = ref_fflags() + ["-I" + src, "-I" + ref("tools")]
    files = ("up_standins.F90", ref("tools", "fv_eta.F90"), ref("model", "fv_arrays.F90"), ref("model", "fv_grid_utils.F90"),
             "up_standins_post.F90", ref("model", "fv_thermodynamics.F90"), ref("model", "fv_update_phys.F90"), "up_driver.F90")
    objs = []
    for f in files:
        f = os.path.join(src, f) if os.sep not in f else f
        o = os.path.join(tmp, os.path.basename(f)[:-4] + ".o")
        subprocess.check_call([fc, *fl, "-c", f, "-o", o], cwd=tmp)
        objs.append(o)
    so = os.path.join(tmp, "libupref.so")
    subprocess.check_call([fc, "-shared", "-o", so, *objs], cwd=tmp)
    return C.CDLL(so)


def written(bd, name, a):
    """the range of a field the routine may write: the compute domain; u on (is:ie, js:je+1), v on (is:ie+1, js:je)"""
    r = (bd.is_, bd.ie, bd.js, bd.je)
    if name == "u":
        return bd.view(a, "U", bd.is_, bd.ie, bd.js, bd.je + 1)
    if name == "v":
        return bd.view(a, "V", bd.is_, bd.ie + 1, bd.js, bd.je)
    if name == "pe":
        return a[1:-1, :, 1:-1]
    if name in ("q", "qdiag", "delp", "pt", "ua", "va", "ps"):
        return bd.view(a, "A", *r)
    return a


def run_ref(dll, name):
    """the compiled reference on a copy of the case's inputs -> (bd, inputs, outputs)"""
    c = UI.CASES[name]
    bd, st = UI.case_inputs(name)
    o = {n: a.copy(order="F") for n, a in st.items()}
    sp = UI.species_of(c)
    # get_tracer_index's order in up_standins.F90; absent = -1 (NO_TRACER)
    idx = (C.c_int * 8)(*[sp.get(n, 0) or -1 for n in ("sphum", "liq_wat", "ice_wat", "rainwat", "snowwat", "graupel", "cld_amt", "w_diff")])
    adj = np.ascontiguousarray(UI.adjust_mass_of(c), dtype=np.int32)
    ak, bk = (np.ascontiguousarray(a) for a in UI.eta_levels(c["km"]))
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    for n in o:
        assert o[n].flags.f_contiguous and o[n].dtype == np.float64, n
    phis, ts = bd.zeros("A"), np.zeros((bd.nx, bd.ny), order="F")
    i = C.c_int
    dll.up_run(i(bd.is_), i(bd.ie), i(bd.js), i(bd.je), i(bd.ng), i(c["km"]), i(c["nq"]), i(c["ncnst"]), i(c["nwat"]), idx,
               adj.ctypes.data_as(C.POINTER(C.c_int)), i(int(c["hydrostatic"])), i(int(c["phys_hydrostatic"])), i(int(c["has_qdt"])),
               C.c_double(c["dt"]), C.c_double(c["ptop"]), C.c_double(c["tau_h2o"]), p(ak), p(bk),
               *(p(o[n]) for n in ("u", "v", "w", "delp", "pt", "q", "qdiag", "ua", "va", "ps", "pe", "peln", "pk", "pkz")), p(phis),
               p(o["u_srf"]), p(o["v_srf"]), p(ts), *(p(o[n]) for n in ("delz", "u_dt", "v_dt", "t_dt", "q_dt")))
    assert not ts.any() and not phis.any()
    return bd, st, o


def record(dll, name):
    bd, st, o = run_ref(dll, name)
    out = {f"{name}|sha": np.array(UI.checksum(st))}
    for n in UI.OUT:
        w = written(bd, n, o[n])
        if np.array_equal(w, written(bd, n, st[n])):      # a field the case leaves alone is not stored: the tests demand its input bits
            continue
        out[f"{name}|out|{n}"] = np.ascontiguousarray(w)
    # nothing outside the written ranges, and no pure input, may have changed -- u_dt, v_dt get their halo from the periodic fill
    for n in UI.OUT:
        m = np.ones(o[n].shape, dtype=bool)
        written(bd, n, m)[...] = False
        assert np.array_equal(o[n][m], st[n][m]), f"{name}: the reference wrote {n} outside the range the recorder keeps"
    for n in ("t_dt", "w"):
        assert np.array_equal(o[n], st[n]), n
    return out


def measure(dll):
    """the library of the CPU harness against the compiled reference: relative RMS and max norm of the fields behind a transcendental"""
    import parity_update_phys as S
    from gfdl_atmos_cubed_sphere_amd.lib import Fv3Lib
    subprocess.check_call(["make", "-C", os.path.join(os.path.dirname(HERE), "hostemu"), "-s"])
    emu = Fv3Lib(os.path.join(os.path.dirname(HERE), "hostemu", "libfv3_hostemu.so"))
    worst = {}
    for name, c in UI.CASES.items():
        bd, st, o = run_ref(dll, name)
        got = S.run_whole_tile(emu, bd, st, S.params_of(c))
        for n in UI.TRANSCENDENTAL:
            if n == "pkz" and not c["hydrostatic"]:
                continue
            a, b = written(bd, n, got[n]), written(bd, n, o[n])
            rms = float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))
            mx = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
            w = worst.setdefault(n, [0.0, 0.0])
            w[0], w[1] = max(w[0], rms), max(w[1], mx)
    for n, (rms, mx) in worst.items():
        print(f"{n}: relative RMS {rms:.3e}, max norm {mx:.3e} (worst of {len(UI.CASES)} cases)")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        dll = build(tmp)
        if "--measure" in sys.argv:
            return measure(dll)
        files = {}
        for name, c in UI.CASES.items():
            files.setdefault(c["group"], {}).update(record(dll, name))
        for group, d in files.items():
            path = os.path.join(HERE, f"update_phys_{group}.npz")
            np.savez_compressed(path, **d)
            print(f"{os.path.basename(path)}: {len(d)} arrays, {os.path.getsize(path)} bytes")
            assert os.path.getsize(path) <= LIMIT, "larger than the largest golden committed before"


if __name__ == "__main__":
    main()
