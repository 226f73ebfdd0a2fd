"""Golden fixtures of the Kessler warm-rain microphysics from the REFERENCE's own compiled Fortran:

    python tests/golden/make_kessler_golden.py [--measure]

compiles driver/solo/qs_tables.F90 where it lies (FV3_REFERENCE) and unmodified, and cuts from driver/solo/fv_phys.F90, unmodified,
by anchors: K_warm_rain and kessler_imp, each from its `subroutine` line to its `end subroutine` line, and the module parameters
e0 .. Lv0 (:74-85).  The cuts go into ONE module, kessler_cut_mod, in a temporary directory and nowhere else; it is compiled with
REF_FFLAGS of oracle/Makefile between this directory's kessler_ref/kessler_standins.F90 (constants_mod and gfdl_mp_mod's c_liq with
the reference's values, time_type, send_data, prt_maxmin, the namelist switches and tracer indices K_warm_rain reads of its
module) and the bind(C) driver kessler_ref/kessler_driver.F90.  For the chained case the fv_update_phys recipe of
tests/golden/make_update_phys_golden.py is built beside it, as a library of its own (both recipes define a constants_mod).  It runs
K_warm_rain on tests/kessler_inputs.CASES and the chain K_warm_rain -> fv_update_phys of CHAIN, and records the outputs:

    tests/golden/kessler/<group>[_a|_b|_c].npz:  "<case>|out|<field>" (the range the routine writes) and "<case>|sha" = the
                                                checksum of the inputs; the fields of parity_kessler.stored(case): the winds only
                                                where the routine adds to them -- elsewhere the recorder asserts that the reference
                                                left their bits (u_dt, v_dt: the incoming value + 0.) -- and no pe: the recorder
                                                asserts that the reference's pe is the running sum of its delp, bit for bit
    tests/golden/kessler/table.npz:             table_w and des_w of qs_tables_mod, what fv3_qs_wat_init is held to, bit for bit
    tests/golden/kessler/chain.npz, chain_b.npz (the winds)

Data only.  The inputs are not stored: the tests form them again from the seeds and compare the checksum.  The branches the inputs
are there for are asserted here, with the numpy restatement's counts over the recorded set, before anything is written.
--measure: nothing is written.  (1) the unperturbed restatement tests/ref_kessler.py against the compiled reference; (2) the
restatement with every log, exp, power and sqrt perturbed in its last place (ref_kessler.Math(seed), 8 seeds) against the
unperturbed one: per output field and flag set the worst relative RMS change, the figures MEASURED of tests/parity_kessler.py, of
which the tests assert ten times; (3) the library of the CPU harness (tests/hostemu) against the compiled reference, printed beside
them; (4) the table against the compiler's.
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
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import kessler_inputs as KI  # noqa: E402
import ref_kessler as R  # noqa: E402

REFERENCE = os.environ.get("FV3_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "reference"))
LIMIT = 121503        # the largest golden of tests/golden/reed
OUT_DIR = os.path.join(HERE, "kessler")
SEEDS = 8
PARTS = {"_a": ("pt", "delp", "q_sphum", "q_liq", "q_rain", "rain", "ps"), "_b": ("peln", "pk"), "_c": ("ua", "va", "w", "u_dt", "v_dt")}


def ref_fflags():
    mk = open(os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "Makefile")).read()
    return re.search(r"^REF_FFLAGS \?= (.*)$", mk, flags=re.M).group(1).split()


def cut(lines, first, last, start=0):
    """the lines from the first one matching `first` (at or after `start`) to the first one after it matching `last`, inclusive"""
    a = next(n for n in range(start, len(lines)) if re.search(first, lines[n]))
    b = next(n for n in range(a, len(lines)) if re.search(last, lines[n]))
    return lines[a:b + 1], a, b


def write_cut_module(tmp):
    src = open(os.path.join(REFERENCE, "driver", "solo", "fv_phys.F90")).read().split("\n")
    params, _, _ = cut(src, r"^\s*real, parameter:: e0 =", r"^\s*real, parameter:: Lv0 =")
    kwr, _, _ = cut(src, r"^\s*subroutine K_warm_rain\(", r"^\s*end subroutine K_warm_rain")
    kimp, _, _ = cut(src, r"^\s*subroutine kessler_imp\(", r"^\s*end subroutine kessler_imp")
    body = ["module kessler_cut_mod", "  use constants_mod, only: rdgas, rvgas, cp_air, cp_vapor, hlv, grav, kappa", "  use gfdl_mp_mod, only: c_liq",
            "  use qs_tables_mod, only: qs_wat_init, qs_wat", "  use kessler_standins_mod", "  implicit none", *params, "contains", *kwr, *kimp,
            "end module kessler_cut_mod", ""]
    path = os.path.join(tmp, "kessler_cut.F90")
    with open(path, "w") as f:
        f.write("\n".join(body))
    return path


def build(tmp):
    fc = shutil.which("amdflang") or "/opt/rocm/bin/amdflang"
    kr = os.path.join(HERE, "kessler_ref")
    files = (os.path.join(kr, "kessler_standins.F90"), os.path.join(REFERENCE, "driver", "solo", "qs_tables.F90"), write_cut_module(tmp),
             os.path.join(kr, "kessler_driver.F90"))
    objs = []
    for f in files:
        o = os.path.join(tmp, os.path.basename(f)[:-4] + ".o")
        subprocess.check_call([fc, *ref_fflags(), "-c", f, "-o", o], cwd=tmp)
        objs.append(o)
    so = os.path.join(tmp, "libkesslerref.so")
    subprocess.check_call([fc, "-shared", "-o", so, *objs], cwd=tmp)
    return C.CDLL(so)


def p(a):
    assert a.flags.f_contiguous and a.dtype == np.float64
    return a.ctypes.data_as(C.POINTER(C.c_double))


def run_ref(dll, pr, bd, st, km):
    """the compiled K_warm_rain on a copy of the inputs -> outputs"""
    o = {n: a.copy(order="F") for n, a in st.items()}
    i = C.c_int
    dll.kessler_run(i(bd.is_), i(bd.ie), i(bd.js), i(bd.je), i(bd.ng), i(km), i(pr["nq"]), C.c_double(pr["pdt"]), i(pr["K_cycle"]),
                    i(int(pr["K_sedi_transport"])), i(int(pr["do_K_sedi_w"])), i(int(pr["do_K_sedi_heat"])), i(int(pr["hydrostatic"])),
                    i(int(pr["moist_kappa"])), i(pr["sphum"]), i(pr["liq_wat"]), i(pr["rainwat"]),
                    *(p(o[n]) for n in ("ua", "va", "w", "u_dt", "v_dt", "q", "pt", "delp", "delz", "pe", "peln", "pk", "ps", "rain")))
    return o


def ref_table(dll):
    tw, dw = np.zeros(R.QS_LENGTH), np.zeros(R.QS_LENGTH)
    dll.qs_table_run(C.c_int(R.QS_LENGTH), p(tw), p(dw))
    return tw, dw


def same(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def record(dll, name, total):
    import parity_kessler as S
    c = KI.CASES[name]
    bd, st = KI.case_inputs(name)
    pr = KI.params_of(c)
    o = run_ref(dll, pr, bd, st, c["km"])
    chk, cnt = S.run_checker(bd, st, pr)
    for k, v in cnt.items():
        total[k] = total.get(k, 0) + v
    # nothing but what the recorder keeps may have changed in the reference's run, and pe is the running sum of delp
    S.assert_untouched(bd, st, {n: o[n] for n in KI.STATE}, pr, what=f"{name}: the reference: ")
    vo, vi = S.views(bd, pr, o), S.views(bd, pr, st)
    for n in S.FIELDS:
        assert np.all(np.isfinite(vo[n])), f"{name}: {n} is not finite in the reference's output"
        if n not in S.stored(c):
            assert same(vo[n], vi[n] + 0.0 if n in ("u_dt", "v_dt") else vi[n]), f"{name}: the reference changed {n}, which the recorder does not keep"
    out = {f"{name}|sha": np.array(KI.checksum(st))}
    for n in S.stored(c):
        out[f"{name}|out|{n}"] = np.ascontiguousarray(vo[n])
    return out


def written(bd, name, a):
    """the range of a field of the chained case that the recorder keeps (make_held_suarez_golden.written)"""
    if name == "u":
        return bd.view(a, "U", bd.is_, bd.ie, bd.js, bd.je + 1)
    if name == "v":
        return bd.view(a, "V", bd.is_, bd.ie + 1, bd.js, bd.je)
    if name == "pe":
        return a[1:-1, :, 1:-1]
    if name in ("pt", "ua", "va", "w", "ps", "delp", "q", "u_dt", "v_dt"):
        return bd.view(a, "A", bd.is_, bd.ie, bd.js, bd.je)
    return a


def run_chain(dll, tmp):
    """K_warm_rain, then the reference's whole fv_update_phys (up_driver.F90 of the fv_update_phys recipe), on one state"""
    import held_suarez_inputs as HI
    import make_update_phys_golden as MU
    up = os.path.join(tmp, "up")
    os.makedirs(up)
    udll = MU.build(up)
    c = KI.CHAIN
    bd, st = KI.chain_inputs()
    pr = KI.params_of(c)
    km, nq = c["km"], c["nq"]
    o = run_ref(dll, pr, bd, st, km)
    i, f = C.c_int, C.c_double
    idx = (C.c_int * 8)(1, 2, 3, 4, -1, -1, -1, -1)
    adj = np.ones(nq, dtype=np.int32)
    ak, bk = (np.ascontiguousarray(a) for a in HI.eta_levels(km))
    qdiag, ts = np.zeros((1,), order="F"), np.zeros((bd.nx, bd.ny), order="F")
    udll.up_run(i(bd.is_), i(bd.ie), i(bd.js), i(bd.je), i(bd.ng), i(km), i(nq), i(nq), i(4), idx, adj.ctypes.data_as(C.POINTER(C.c_int)),
                i(int(c["hydrostatic"])), i(1), i(1), f(c["pdt"]), f(c["ptop"]), f(0.0), p(ak), p(bk),
                *(p(o[n]) for n in ("u", "v", "w", "delp", "pt", "q")), p(qdiag), *(p(o[n]) for n in ("ua", "va", "ps", "pe", "peln", "pk", "pkz")),
                p(o["phis"]), p(o["u_srf"]), p(o["v_srf"]), p(ts), *(p(o[n]) for n in ("delz", "u_dt", "v_dt", "t_dt", "q_dt")))
    assert not ts.any() and not o["t_dt"].any() and not o["q_dt"].any()
    return bd, st, o


def record_chain(dll, tmp):
    bd, st, o = run_chain(dll, tmp)
    out = {"chain|sha": np.array(KI.checksum(st))}
    for n in st:
        m = np.ones(o[n].shape, dtype=bool)
        if n in KI.CHAIN_OUT:
            written(bd, n, m)[...] = False
            out[f"chain|out|{n}"] = np.ascontiguousarray(written(bd, n, o[n]))
            assert np.all(np.isfinite(out[f"chain|out|{n}"])), n
            assert not np.array_equal(written(bd, n, o[n]), written(bd, n, st[n])), f"chain: {n} did not change"
        if n in ("u_dt", "v_dt", "u_srf", "v_srf"):      # (the halo of u_dt, v_dt: fv_update_phys' exchange; the bottom winds are not compared)
            continue
        assert same(o[n][m], st[n][m]), f"chain: the reference wrote {n} outside the range the recorder keeps"
    return out


def rel_rms(a, b):
    d = float(np.sqrt(np.mean((a - b) ** 2)))
    s = float(np.sqrt(np.mean(b ** 2)))
    return d / s if s > 0.0 else (0.0 if d == 0.0 else np.inf)


def measure(dll):
    import parity_kessler as S
    from gfdl_atmos_cubed_sphere_amd.lib import Fv3Lib
    subprocess.check_call(["make", "-C", os.path.join(os.path.dirname(HERE), "hostemu"), "-s"])
    emu = Fv3Lib(os.path.join(os.path.dirname(HERE), "hostemu", "libfv3_hostemu.so"))
    base, spread, libd = {}, {}, {}

    def up(d, key, v):
        d[key] = max(d.get(key, 0.0), v)
    for name, c in KI.CASES.items():
        bd, st = KI.case_inputs(name)
        pr = KI.params_of(c)
        fam = c["flags"]
        vo = S.views(bd, pr, run_ref(dll, pr, bd, st, c["km"]))
        vp = S.views(bd, pr, S.run_checker(bd, st, pr)[0])
        vl = S.views(bd, pr, S.run_lib(emu, bd, st, pr))
        for n in S.FIELDS:
            up(base, (fam, n), rel_rms(vp[n], vo[n]))
            up(libd, (fam, n), rel_rms(vl[n], vo[n]))
        for seed in range(SEEDS):
            vs = S.views(bd, pr, S.run_checker(bd, st, pr, M=R.Math(9000 + seed))[0])
            for n in S.FIELDS:
                up(spread, (fam, n), rel_rms(vs[n], vp[n]))
    print("flag set, field: perturbed restatement vs restatement (MEASURED) | restatement vs compiled reference | library (CPU harness) vs compiled reference")
    for key in sorted(spread):
        print(f"  {key[0]:5s} {key[1]:8s}: {spread[key]:.3e} | {base[key]:.3e} | {libd[key]:.3e}")
    for key in sorted(spread):
        assert base[key] <= 10.0 * spread[key], f"{key}: the unperturbed restatement is not within the spread of the compiled reference"
    print("MEASURED = {" + ", ".join(f'("{k[0]}", "{k[1]}"): {v:.3e}' for k, v in sorted(spread.items())) + "}")
    print("LIBRARY = {" + ", ".join(f'("{k[0]}", "{k[1]}"): {v:.3e}' for k, v in sorted(libd.items())) + "}")
    tw, dw = ref_table(dll)
    mine = S.lib_table(emu)
    for n, a, b in (("table_w", mine[0], tw), ("des_w", mine[1], dw)):
        print(f"{n}: host libm against the reference's compiler, {a.size} entries: bit-identical {bool(same(a, b))}, "
              f"max relative difference {float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))):.3e}")


def save(path, d):
    """np.savez_compressed with the archive's time stamps fixed, so that the file regenerates byte for byte"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, a in d.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            zi = zipfile.ZipInfo(k.replace("/", "%") + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


def main():
    import parity_kessler as S
    with tempfile.TemporaryDirectory() as tmp:
        dll = build(tmp)
        if "--measure" in sys.argv:
            return measure(dll)
        files, total = {}, {}
        for name, c in KI.CASES.items():
            out = record(dll, name, total)
            for s in S.parts_of(c):
                keep = {k: v for k, v in out.items() if k.endswith("|sha") or not s or k.rsplit("|", 1)[1] in PARTS[s]}
                files.setdefault(c["group"] + s, {}).update(keep)
        print("branch counts over the recorded set:", total)
        assert all(total[k] > 0 for k in R.COUNTS), {k: v for k, v in total.items() if v == 0}
        tw, dw = ref_table(dll)
        files["table"] = {"table_w": tw, "des_w": dw}
        chain = record_chain(dll, tmp)      # two files: the winds apart
        winds = tuple(f"chain|out|{n}" for n in ("u", "v", "ua", "va", "w", "u_dt", "v_dt"))
        files["chain"] = {k: v for k, v in chain.items() if k not in winds}
        files["chain_b"] = {k: v for k, v in chain.items() if k in winds}
        os.makedirs(OUT_DIR, exist_ok=True)
        size = 0
        for group, d in files.items():
            path = os.path.join(OUT_DIR, f"{group}.npz")
            save(path, d)
            size += os.path.getsize(path)
            assert os.path.getsize(path) <= LIMIT, f"{path}: {os.path.getsize(path)} bytes, larger than the largest golden of tests/golden/reed"
        print(f"{len(files)} files, {size} bytes")


if __name__ == "__main__":
    main()
