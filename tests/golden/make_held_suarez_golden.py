"""Golden fixtures of Held_Suarez_Tend and age_of_air from the REFERENCE's own compiled Fortran:

    python tests/golden/make_held_suarez_golden.py [--measure]

compiles, from where they lie (FV3_REFERENCE) and unmodified, with REF_FFLAGS of oracle/Makefile: the stand-ins of
tests/golden/update_phys_ref/up_standins.F90, this directory's held_suarez_ref/hs_standins.F90 (constants_mod with pi and RADIAN,
time_manager_mod with get_date / get_time, diag_manager_mod), the reference's tools/fv_eta.F90, model/fv_arrays.F90 (radius) and
model/fv_grid_utils.F90 (g_sum), driver/solo/hswf.F90 and the bind(C) driver held_suarez_ref/hs_driver.F90 -- and, for the chained case,
the rest of the fv_update_phys recipe (up_standins_post.F90, model/fv_thermodynamics.F90, model/fv_update_phys.F90, up_driver.F90) --
into a temporary directory; runs Held_Suarez_Tend on the cases of tests/held_suarez_inputs.CASES, age_of_air on AGE_CASES and the chain
Held_Suarez_Tend -> fv_update_phys of tests/held_suarez_inputs.CHAIN, and records the outputs:

    tests/golden/held_suarez_<set>.npz:  "<case>|out|<field>" (the compute domain) and "<case>|sha" = the checksum of the inputs

Data only.  The inputs are not stored: the tests form them again from the seeds and compare the checksum.  The conditions the cases
are there for are asserted here, with the numpy restatement's branch counts, before anything is written.
--measure: nothing is written; the library of the CPU harness (tests/hostemu) is run on every case and the relative RMS and max norm
of t_dt per branch set (include/fv3_math.h against the compiled reference's libm), the bit-identity of u_dt, v_dt and of the
host-formed latitude planes are printed -- the figures the tests' bounds come from.
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

import held_suarez_inputs as HI  # noqa: E402
import ref_held_suarez as R  # noqa: E402

REFERENCE = os.environ.get("FV3_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "reference"))
LIMIT = 213341        # the largest golden committed before (ppm1d_golden.npz)


def ref_fflags():
    mk = open(os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "Makefile")).read()
    return re.search(r"^REF_FFLAGS \?= (.*)$", mk, flags=re.M).group(1).split()


def build(tmp):
    fc = shutil.which("amdflang") or "/opt/rocm/bin/amdflang"
    up, hs = os.path.join(HERE, "update_phys_ref"), os.path.join(HERE, "held_suarez_ref")
    ref = lambda *p: os.path.join(REFERENCE, *p)      # noqa: E731
    fl = ref_fflags() + ["-I" + up, "-I" + ref("tools")]
    files = (os.path.join(up, "up_standins.F90"), os.path.join(hs, "hs_standins.F90"), ref("tools", "fv_eta.F90"), ref("model", "fv_arrays.F90"),
             ref("model", "fv_grid_utils.F90"), os.path.join(up, "up_standins_post.F90"), ref("model", "fv_thermodynamics.F90"),
             ref("model", "fv_update_phys.F90"), ref("driver", "solo", "hswf.F90"), os.path.join(up, "up_driver.F90"), os.path.join(hs, "hs_driver.F90"))
    objs = []
    for f in files:
        o = os.path.join(tmp, os.path.basename(f)[:-4] + ".o")
        subprocess.check_call([fc, *fl, "-c", f, "-o", o], cwd=tmp)
        objs.append(o)
    so = os.path.join(tmp, "libhsref.so")
    # hs_standins.F90 states constants_mod and time_manager_mod again, as supersets with the same values: the linker keeps the first
    subprocess.check_call([fc, "-shared", "-Wl,--allow-multiple-definition", "-o", so, *objs], cwd=tmp)
    return C.CDLL(so)


def params_of(c):
    return dict(pdt=c["pdt"], strat=c["strat"], zurita=c["zurita"], rd_zur=c["rd_zur"], radius=c["radius"], pi=HI.PI)


def run_ref(dll, name):
    """the compiled reference on a copy of the case's inputs -> (bd, inputs, outputs)"""
    c = HI.CASES[name]
    bd, st = HI.case_inputs(name)
    o = {n: a.copy(order="F") for n, a in st.items()}
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    for n in o:
        assert o[n].flags.f_contiguous and o[n].dtype == np.float64, n
    i, f = C.c_int, C.c_double
    dll.hs_run(i(bd.is_), i(bd.ie), i(bd.js), i(bd.je), i(bd.ng), i(c["km"]), f(c["pdt"]), i(int(c["strat"])), i(int(c["zurita"])),
               f(c["rd_zur"]), f(c["radius"]), *(p(o[n]) for n in ("agrid", "pt", "pe", "delp", "peln", "pkz", "ua", "va", "u_dt", "v_dt", "t_dt")))
    return bd, st, o


def run_age(dll, name):
    c = HI.AGE_CASES[name]
    bd, st = HI.age_inputs(name)
    o = {n: a.copy(order="F") for n, a in st.items()}
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    i = C.c_int
    dll.hs_age(i(bd.is_), i(bd.ie), i(bd.js), i(bd.je), i(c["km"]), i(bd.ng), C.c_double(c["time"]), p(o["pe"]), p(o["q"]))
    return bd, st, o


def compute(bd, a):
    return bd.view(a, "A", bd.is_, bd.ie, bd.js, bd.je)


def record(dll, name, seen):
    c = HI.CASES[name]
    bd, st, o = run_ref(dll, name)
    # ---- the conditions
    chk = {n: a.copy(order="F") for n, a in st.items()}
    cnt = R.held_suarez_tend(bd, c["km"], params_of(c), chk)
    if c["strat"] and c["km"] >= 12:
        assert cnt["meso"] > 0 and cnt["strat"] > 0 and cnt["tropo"] > 0, (name, cnt)
        pl = compute(bd, st["delp"]) / np.transpose(st["peln"][:, 1:, :] - st["peln"][:, :-1, :], (0, 2, 1))
        per_col = [(pl <= 1.0e2).any(axis=2), ((pl > 1.0e2) & (pl <= 1.0e4)).any(axis=2), (pl > 1.0e4).any(axis=2)]
        assert all(m.all() for m in per_col), f"{name}: a column misses one of the three branches"
    assert cnt["friction"] > 0 and cnt["no_friction"] > 0, (name, cnt)
    plb = compute(bd, st["delp"])[:, :, -1] / (st["peln"][:, -1, :] - st["peln"][:, -2, :])
    assert plb.min() > 2.0e4, f"{name}: a bottom layer near 100 hPa"
    for n in ("teq_t0", "teq_free"):
        seen[(c["group"], n)] = seen.get((c["group"], n), 0) + cnt[n]
    # nothing but t_dt and the compute domain of u_dt, v_dt may have changed in the reference's run
    for n in st:
        if n == "t_dt":
            continue
        m = np.ones(o[n].shape, dtype=bool)
        if n in ("u_dt", "v_dt"):
            compute(bd, m)[...] = False
        assert np.array_equal(o[n][m].view(np.uint64), st[n][m].view(np.uint64)), f"{name}: the reference wrote {n} outside the range the recorder keeps"
    out = {f"{name}|sha": np.array(HI.checksum(st)), f"{name}|out|t_dt": np.ascontiguousarray(o["t_dt"])}
    for n in ("u_dt", "v_dt"):
        out[f"{name}|out|{n}"] = np.ascontiguousarray(compute(bd, o[n]))
    return out


def record_age(dll, name):
    bd, st, o = run_age(dll, name)
    m = np.ones(o["q"].shape, dtype=bool)
    compute(bd, m)[...] = False
    assert np.array_equal(o["q"][m].view(np.uint64), st["q"][m].view(np.uint64)) and np.array_equal(o["pe"], st["pe"]), name
    src = st["pe"][1:-1, :-1, 1:-1] >= 75000.0
    assert src.any() and not src.all(), f"{name}: the source level is not crossed"
    return {f"{name}|sha": np.array(HI.checksum(st)), f"{name}|out|q": np.ascontiguousarray(compute(bd, o["q"]))}


def written(bd, name, a):
    """the range of a field of the chained case that the recorder keeps (make_update_phys_golden.written; u_dt, v_dt whole: the
    periodic fill writes their halo)"""
    if name == "u":
        return bd.view(a, "U", bd.is_, bd.ie, bd.js, bd.je + 1)
    if name == "v":
        return bd.view(a, "V", bd.is_, bd.ie + 1, bd.js, bd.je)
    if name == "pe":
        return a[1:-1, :, 1:-1]
    if name in ("pt", "ua", "va", "ps"):
        return compute(bd, a)
    return a


def run_chain(dll):
    """Held_Suarez_Tend, then the reference's whole fv_update_phys (up_driver.F90 of the fv_update_phys recipe), on one state"""
    c = HI.CHAIN
    bd, st = HI.chain_inputs()
    o = {n: a.copy(order="F") for n, a in st.items()}
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    i, f = C.c_int, C.c_double
    km, nq = c["km"], c["nq"]
    dll.hs_run(i(bd.is_), i(bd.ie), i(bd.js), i(bd.je), i(bd.ng), i(km), f(c["pdt"]), i(int(c["strat"])), i(int(c["zurita"])),
               f(c["rd_zur"]), f(c["radius"]), *(p(o[n]) for n in ("agrid", "pt", "pe", "delp", "peln", "pkz", "ua", "va", "u_dt", "v_dt", "t_dt")))
    idx = (C.c_int * 8)(1, -1, -1, -1, -1, -1, -1, -1)
    adj = np.ones(nq, dtype=np.int32)
    ak, bk = (np.ascontiguousarray(a) for a in HI.eta_levels(km))
    qdiag, phis, ts = np.zeros((1,), order="F"), bd.zeros("A"), np.zeros((bd.nx, bd.ny), order="F")
    dll.up_run(i(bd.is_), i(bd.ie), i(bd.js), i(bd.je), i(bd.ng), i(km), i(nq), i(nq), i(0), idx, adj.ctypes.data_as(C.POINTER(C.c_int)),
               i(1), i(1), i(1), f(c["pdt"]), f(c["ptop"]), f(0.0), p(ak), p(bk),
               *(p(o[n]) for n in ("u", "v", "w", "delp", "pt", "q")), p(qdiag), *(p(o[n]) for n in ("ua", "va", "ps", "pe", "peln", "pk", "pkz")),
               p(phis), p(o["u_srf"]), p(o["v_srf"]), p(ts), *(p(o[n]) for n in ("delz", "u_dt", "v_dt", "t_dt", "q_dt")))
    assert not ts.any() and not phis.any()
    return bd, st, o


def record_chain(dll):
    bd, st, o = run_chain(dll)
    out = {"chain|sha": np.array(HI.checksum(st))}
    for n in st:
        m = np.ones(o[n].shape, dtype=bool)
        if n in HI.CHAIN_OUT:
            written(bd, n, m)[...] = False
            out[f"chain|out|{n}"] = np.ascontiguousarray(written(bd, n, o[n]))
            assert not np.array_equal(written(bd, n, o[n]), written(bd, n, st[n])) or n in ("pe", "peln", "pk", "pkz"), f"chain: {n} did not change"      # (rebuilt from an unchanged delp)
        assert np.array_equal(o[n][m].view(np.uint64), st[n][m].view(np.uint64)), f"chain: the reference wrote {n} outside the range the recorder keeps"
    return out


def measure(dll):
    """the library of the CPU harness against the compiled reference"""
    import parity_held_suarez as S
    from gfdl_atmos_cubed_sphere_amd.lib import Fv3Lib
    subprocess.check_call(["make", "-C", os.path.join(os.path.dirname(HERE), "hostemu"), "-s"])
    emu = Fv3Lib(os.path.join(os.path.dirname(HERE), "hostemu", "libfv3_hostemu.so"))
    worst, exact = {}, {}
    for name, c in HI.CASES.items():
        bd, st, o = run_ref(dll, name)
        got = S.run_lib(emu, bd, st, params_of(c))
        masks = S.branch_masks(bd, c["km"], params_of(c), st)
        for bs, m in masks.items():
            if not m.any():
                continue
            a, b = got["t_dt"][m], o["t_dt"][m]
            rms = float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))
            mx = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
            w = worst.setdefault(bs, [0.0, 0.0, 0])
            w[0], w[1], w[2] = max(w[0], rms), max(w[1], mx), w[2] + 1
        for n in ("u_dt", "v_dt"):
            exact[n] = exact.get(n, True) and bool(np.array_equal(got[n].view(np.uint64), o[n].view(np.uint64)))
    for bs, (rms, mx, n) in worst.items():
        print(f"t_dt, {bs}: relative RMS {rms:.3e}, max norm {mx:.3e} (worst of {n} cases)")
    print("bit-identical in every case:", exact)
    lats = np.concatenate([HI.case_inputs(name)[1]["lat"].reshape(-1) for name in HI.CASES])
    planes = np.zeros((lats.size, 4), order="F")
    dll.hs_lat_planes(C.c_int(lats.size), lats.ctypes.data_as(C.POINTER(C.c_double)), planes.ctypes.data_as(C.POINTER(C.c_double)))
    tab = R.lat_table(lats)
    for k, n in enumerate(("cos", "tey", "tez", "cos4")):
        same = np.array_equal(tab[n].view(np.uint64), planes[:, k].view(np.uint64))
        print(f"latitude plane {n}: host libm against the reference's compiler, {lats.size} latitudes: bit-identical {same}, "
              f"max relative difference {float(np.max(np.abs(tab[n] - planes[:, k]) / np.maximum(np.abs(planes[:, k]), 1e-300))):.3e}")
    for name in HI.AGE_CASES:
        bd, st, o = run_age(dll, name)
        got = S.run_age(emu, bd, st, HI.AGE_CASES[name])
        print(f"{name}: q bit-identical {bool(np.array_equal(got.view(np.uint64), o['q'].view(np.uint64)))}")


def save(path, d):
    """np.savez_compressed with the archive's time stamps fixed, so that the file regenerates byte for byte"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, a in d.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


def main():
    with tempfile.TemporaryDirectory() as tmp:
        dll = build(tmp)
        if "--measure" in sys.argv:
            return measure(dll)
        files, seen = {}, {}
        for name, c in HI.CASES.items():
            files.setdefault(c["group"], {}).update(record(dll, name, seen))
        for key, n in seen.items():
            assert n > 0, f"{key}: an arm of max(t0, .) no recorded case of the set reaches"
        for name in HI.AGE_CASES:
            files.setdefault("age", {}).update(record_age(dll, name))
        files["chain"] = record_chain(dll)
        for group, d in files.items():
            path = os.path.join(HERE, f"held_suarez_{group}.npz")
            save(path, d)
            print(f"{os.path.basename(path)}: {len(d)} arrays, {os.path.getsize(path)} bytes")
            assert os.path.getsize(path) <= LIMIT, "larger than the largest golden committed before"


if __name__ == "__main__":
    main()
