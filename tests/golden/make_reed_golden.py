"""Golden fixtures of the Reed-Jablonowski simple physics and the terminator chemistry from the REFERENCE's own compiled Fortran:

    python tests/golden/make_reed_golden.py [--measure]

cuts from driver/solo/fv_phys.F90, where it lies (FV3_REFERENCE) and unmodified, by anchors: reed_sim_physics and
DCMIP2016_terminator_advance, each from its `subroutine` line to its `end subroutine` line; the module parameters e0 .. Lv0 (:74-85); the
lines of the do_reed_sim_phys branch that set zvir and rgrav (:548-549) and its column loop (:551-602), which go into a subroutine
whose declarations this generator writes; and, for the host-formed planes, the constants of :2508-2551, the Tsurf block (:2571-2586)
and the five lines that form k1 (:2840-2841, :2845-2846, :2873).  The cuts go into ONE module, reed_cut_mod, in a temporary directory
and nowhere else; it is compiled with REF_FFLAGS of oracle/Makefile between this directory's reed_ref/reed_standins.F90 (the
constants with the reference's values, the tracer lookup, the namelist switch) and the bind(C) driver reed_ref/reed_driver.F90 -- and,
for the chained case, with the fv_update_phys recipe of tests/golden/make_update_phys_golden.py.  It runs the column loop on
tests/reed_inputs.CASES, the terminator on TERM_CASES and the chain column loop -> fv_update_phys of CHAIN, and records the outputs:

    tests/golden/reed/<group>.npz:  "<case>|out|<field>" (the compute domain) and "<case>|sha" = the checksum of the inputs
    tests/golden/reed/planes.npz:   Tsurf and the SST factor of qsats for reed_test 0 and 1 on the recorded latitudes, k1 on the
                                    terminator cases' agrid: what the host-formed planes of the library are held to, bit for bit

Data only.  The inputs are not stored: the tests form them again from the seeds and compare the checksum.  The conditions the cases
are there for are asserted here, with the numpy restatement's branch counts, before anything is written.
--measure: nothing is written.  (1) the unperturbed restatement tests/ref_reed.py against the compiled reference; (2) the restatement
with every log, exp and power perturbed in its last place (ref_reed.Math(seed), 8 seeds) against the unperturbed one: per output
field and branch family the worst relative RMS change -- what one last bit of the reference's own libm is worth, the figures
MEASURED of tests/parity_reed.py, of which the tests assert ten times; (3) the library of the CPU harness (tests/hostemu) against the
compiled reference, printed beside them; (4) the host-formed planes against the compiler's.
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

import reed_inputs as RI  # noqa: E402
import ref_reed as R  # noqa: E402

REFERENCE = os.environ.get("FV3_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "reference"))
LIMIT = 213341        # the largest golden committed before (ppm1d_golden.npz)
OUT_DIR = os.path.join(HERE, "reed")
SEEDS = 8


def ref_fflags():
    mk = open(os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "Makefile")).read()
    return re.search(r"^REF_FFLAGS \?= (.*)$", mk, flags=re.M).group(1).split()


def cut(lines, first, last, start=0):
    """the lines from the first one matching `first` (at or after `start`) to the first one after it matching `last`, inclusive"""
    a = next(n for n in range(start, len(lines)) if re.search(first, lines[n]))
    b = next(n for n in range(a, len(lines)) if re.search(last, lines[n]))
    return lines[a:b + 1], a, b


WRAP_HEAD = """
  subroutine reed_wrap(is, ie, js, je, ng, npz, nq, sphum, pdt, hydrostatic, reed_test, do_reed_cond, reed_cond_only, reed_alt_mxg, &
                       agrid_in, delp, pt, ua, va, q, pe, peln, phis, delz, u_dt, v_dt, t_dt, q_dt, rain)
    integer, intent(in) :: is, ie, js, je, ng, npz, nq, sphum, reed_test
    real, intent(in) :: pdt
    logical, intent(in) :: hydrostatic, do_reed_cond, reed_cond_only, reed_alt_mxg
    real, intent(in) :: agrid_in(is-ng:ie+ng, js-ng:je+ng, 2), delp(is-ng:ie+ng, js-ng:je+ng, npz), pt(is-ng:ie+ng, js-ng:je+ng, npz)
    real, intent(in) :: ua(is-ng:ie+ng, js-ng:je+ng, npz), va(is-ng:ie+ng, js-ng:je+ng, npz), q(is-ng:ie+ng, js-ng:je+ng, npz, nq)
    real, intent(in) :: pe(is-1:ie+1, npz+1, js-1:je+1), peln(is:ie, npz+1, js:je), phis(is-ng:ie+ng, js-ng:je+ng), delz(is:ie, js:je, npz)
    real, intent(inout) :: u_dt(is-ng:ie+ng, js-ng:je+ng, npz), v_dt(is-ng:ie+ng, js-ng:je+ng, npz), t_dt(is:ie, js:je, npz)
    real, intent(inout) :: q_dt(is:ie, js:je, npz, nq), rain(is:ie, js:je)
    type reed_grid_type
      real, allocatable :: agrid(:, :, :)
    end type
    type(reed_grid_type) :: gridstruct
    real, dimension(is:ie, npz) :: dp2, rdelp, u2, v2, t2, q2, pm, du2, dv2, dt2, dq2
    real :: zint(is:ie, npz+1), rain2(is:ie), zvir, rgrav
    integer :: i, j, k
    allocate(gridstruct%agrid(is-ng:ie+ng, js-ng:je+ng, 2))
    gridstruct%agrid = agrid_in
"""

PLANES_HEAD = """
  subroutine reed_planes(pcols, lat, test, Tsurf, sstf)
    integer, parameter :: r8 = selected_real_kind(12)
    integer, intent(in) :: pcols, test
    real, intent(in) :: lat(pcols)
    real, intent(out) :: Tsurf(pcols), sstf(pcols)
    real :: gravit, rair, cpair, latvap, rh2o, epsilo, zvir, a, omega_r
    real :: SST_tc, T0, rhow, p0, Cd0, Cd1, Cm, v20, C, sqC, T00, u0, latw, eta0, etav, q0, pbltop, pbltopz, pblconst
    integer :: i
"""
PLANES_TAIL = """
    do i = 1, pcols
      sstf(i) = exp((dc_vap*log(Tsurf(i)/tice) + Lv0*(Tsurf(i) - tice)/(Tsurf(i)*tice))/rvgas)
    enddo
  end subroutine
"""
K1_HEAD = """
  subroutine term_k1(n, lon, lat, k1out)
    integer, intent(in) :: n
    real, intent(in) :: lon(n, 1), lat(n, 1)
    real, intent(out) :: k1out(n)
    real :: sinthc, costhc, k1
    integer :: i, j
"""


def write_cut_module(tmp):
    src = open(os.path.join(REFERENCE, "driver", "solo", "fv_phys.F90")).read().split("\n")
    params, _, _ = cut(src, r"^\s*real, parameter:: e0 =", r"^\s*real, parameter:: Lv0 =")
    branch = next(n for n in range(len(src)) if re.search(r"^\s*if \( do_reed_sim_phys \) then", src[n]))
    scal, _, b = cut(src, r"^\s*zvir = rvgas/rdgas - 1\.", r"^\s*rgrav = 1\./grav", start=branch)
    loop_first = next(n for n in range(b, len(src)) if re.search(r"^\s*do j=js,je", src[n]))
    _, _, rain_line = cut(src, r"^\s*do j=js,je", r"rain\(i,j\) = rain2\(i\) \* 8\.64e7", start=loop_first)
    ends = [n for n in range(rain_line, len(src)) if re.search(r"^\s*enddo", src[n])]
    loop = src[loop_first:ends[1] + 1]                                    # the enddo of the i-loop, the endif, the enddo of the j-loop
    assert re.search(r"^\s*endif", src[ends[0] + 1]) and ends[1] == ends[0] + 2, "the tail of the column loop is not the one expected"
    reed, ra, _ = cut(src, r"^\s*subroutine reed_sim_physics", r"^\s*end subroutine reed_sim_physics")
    term, _, _ = cut(src, r"^\s*subroutine DCMIP2016_terminator_advance", r"^\s*end subroutine DCMIP2016_terminator_advance")
    consts, _, cb = cut(src, r"^#ifdef USE_REED_CONST", r"^\s*q0\s+= 0\.021", start=next(n for n in range(ra, len(src)) if "if ( test .eq. 2 ) return" in src[n]))
    tsurf, _, _ = cut(src, r"^\s*if \(test \.eq\. 1\) then", r"^\s*end if", start=cb)
    k1 = []
    for first in (r"^\s*real, parameter :: lc\s+=", r"^\s*real, parameter :: thc\s+=", r"^\s*sinthc = sin\(thc\)", r"^\s*costhc = cos\(thc\)"):
        k1 += cut(term, first, first)[0]
    k1line = cut(term, r"^\s*k1 = max\(0\.,", r"^\s*k1 = max\(0\.,")[0]
    body = ["module reed_cut_mod", "  use reed_standins_mod", "  implicit none", *params, "contains", *reed, *term,
            WRAP_HEAD, *scal, *loop, "  end subroutine",
            PLANES_HEAD, *consts, *tsurf, PLANES_TAIL,
            K1_HEAD.replace("    real :: sinthc", "\n".join(k1[:2]) + "\n    real :: sinthc"), *k1[2:], "    do j = 1, 1", "    do i = 1, n", *k1line,
            "      k1out(i) = k1", "    enddo", "    enddo", "  end subroutine", "end module reed_cut_mod", ""]
    path = os.path.join(tmp, "reed_cut.F90")
    with open(path, "w") as f:
        f.write("\n".join(body))
    return path


def build(tmp):
    fc = shutil.which("amdflang") or "/opt/rocm/bin/amdflang"
    up, rr = os.path.join(HERE, "update_phys_ref"), os.path.join(HERE, "reed_ref")
    ref = lambda *p: os.path.join(REFERENCE, *p)      # noqa: E731
    fl = ref_fflags() + ["-I" + up, "-I" + ref("tools")]
    files = (os.path.join(up, "up_standins.F90"), ref("tools", "fv_eta.F90"), ref("model", "fv_arrays.F90"), ref("model", "fv_grid_utils.F90"),
             os.path.join(up, "up_standins_post.F90"), ref("model", "fv_thermodynamics.F90"), ref("model", "fv_update_phys.F90"),
             os.path.join(up, "up_driver.F90"), os.path.join(rr, "reed_standins.F90"), write_cut_module(tmp), os.path.join(rr, "reed_driver.F90"))
    objs = []
    for f in files:
        o = os.path.join(tmp, os.path.basename(f)[:-4] + ".o")
        subprocess.check_call([fc, *fl, "-c", f, "-o", o], cwd=tmp)
        objs.append(o)
    so = os.path.join(tmp, "libreedref.so")
    subprocess.check_call([fc, "-shared", "-o", so, *objs], cwd=tmp)
    return C.CDLL(so)


def p(a):
    assert a.flags.f_contiguous and a.dtype == np.float64
    return a.ctypes.data_as(C.POINTER(C.c_double))


def run_ref(dll, c, bd, st):
    """the compiled column loop on a copy of the inputs -> outputs"""
    o = {n: a.copy(order="F") for n, a in st.items()}
    i, f = C.c_int, C.c_double
    dll.reed_run(i(bd.is_), i(bd.ie), i(bd.js), i(bd.je), i(bd.ng), i(c["km"]), f(c["pdt"]), i(int(c["hydrostatic"])), i(c["reed_test"]),
                 i(int(c["do_reed_cond"])), i(int(c["reed_cond_only"])), i(int(c["reed_alt_mxg"])),
                 *(p(o[n]) for n in ("agrid", "delp", "pt", "ua", "va", "q", "pe", "peln", "phis", "delz", "u_dt", "v_dt", "t_dt", "q_dt", "rain")))
    return o


def run_term(dll, c, bd, st):
    q = np.asfortranarray(np.stack([st["cl"], st["cl2"]], axis=3))
    agrid = st["agrid"].copy(order="F")
    i = C.c_int
    dll.term_run(i(bd.is_), i(bd.ie), i(bd.js), i(bd.je), i(bd.ng), i(c["km"]), C.c_double(c["pdt"]), i(int(c["fill"])), p(agrid), p(q))
    assert np.array_equal(agrid, st["agrid"])
    return dict(cl=np.asfortranarray(q[..., 0]), cl2=np.asfortranarray(q[..., 1]))


def compute(bd, a):
    return bd.view(a, "A", bd.is_, bd.ie, bd.js, bd.je)


def conditions(name, c, cnt):
    """every branch the case has is taken"""
    assert cnt["q_neg"] > 0, (name, "no negative q")
    if c["do_reed_cond"]:
        assert cnt["sat"] > 0 and cnt["unsat"] > 0, (name, cnt)
        assert cnt["qsat_edge"] == 0, (name, "a cell within 4 ulp of saturation")
    if not c["reed_cond_only"]:
        assert cnt["wind_lt_v20"] > 0 and cnt["wind_ge_v20"] > 0, (name, cnt)
        if c["km"] >= 2:
            if c["reed_alt_mxg"]:
                assert cnt["z_above"] > 0 and cnt["z_below"] > 0, (name, cnt)
            else:
                assert cnt["p_above"] > 0 and cnt["p_below"] > 0, (name, cnt)


def record(dll, name):
    c = RI.CASES[name]
    bd, st = RI.case_inputs(name)
    o = run_ref(dll, c, bd, st)
    chk = {n: a.copy(order="F") for n, a in st.items()}
    conditions(name, c, R.reed_wrapper(bd, c["km"], RI.params_of(c), chk))
    if c["reed_test"] == 1:
        assert 0.5 * RI.PI - st["lat"].max() <= 1.0e-12 and 0.5 * RI.PI + st["lat"].min() <= 1.0e-12, f"{name}: the latitudes do not reach the poles"
    # nothing but the compute domain of the tendencies and rain may have changed in the reference's run
    for n in st:
        if n in ("t_dt", "q_dt", "rain"):
            continue
        m = np.ones(o[n].shape, dtype=bool)
        if n in ("u_dt", "v_dt"):
            compute(bd, m)[...] = False
        assert np.array_equal(o[n][m].view(np.uint64), st[n][m].view(np.uint64)), f"{name}: the reference wrote {n} outside the range the recorder keeps"
    if not c["do_reed_cond"]:
        assert np.array_equal(o["rain"].view(np.uint64), st["rain"].view(np.uint64)), f"{name}: rain written without do_reed_cond"
    out = {f"{name}|sha": np.array(RI.checksum(st))}
    for n in ("t_dt", "q_dt", "rain"):
        out[f"{name}|out|{n}"] = np.ascontiguousarray(o[n])
    for n in ("u_dt", "v_dt"):
        out[f"{name}|out|{n}"] = np.ascontiguousarray(compute(bd, o[n]))
    return out


def record_term(dll, name):
    c = RI.TERM_CASES[name]
    bd, st = RI.term_inputs(name)
    o = run_term(dll, c, bd, st)
    k1 = R.term_k1(st["agrid"], RI.PI)
    chk = {n: st[n].copy(order="F") for n in ("cl", "cl2")}
    night = R.terminator_advance(c["pdt"], c["fill"], k1, chk["cl"], chk["cl2"])
    assert night > 0 and (k1 > 0.0).any(), (name, "no night / no day cell")
    assert (st["cl"] < 0.0).any() and (st["cl2"] < 0.0).any(), name
    assert np.all(np.isfinite(o["cl"])) and np.all(np.isfinite(o["cl2"])), name
    return {f"{name}|sha": np.array(RI.checksum(st)), f"{name}|out|cl": np.ascontiguousarray(o["cl"]), f"{name}|out|cl2": np.ascontiguousarray(o["cl2"])}


def ref_planes(dll, lat, test):
    lat = np.ascontiguousarray(lat.reshape(-1))
    ts, sf = np.zeros(lat.size), np.zeros(lat.size)
    dll.reed_planes_run(C.c_int(lat.size), p(np.asfortranarray(lat)), C.c_int(test), p(ts), p(sf))
    return ts, sf


def ref_k1(dll, agrid):
    lon, lat = (np.ascontiguousarray(agrid[..., n].reshape(-1)) for n in (0, 1))
    k1 = np.zeros(lon.size)
    dll.term_k1_run(C.c_int(lon.size), p(lon), p(lat), p(k1))
    return k1.reshape(agrid.shape[:2])


def record_planes(dll):
    lat = RI.latitude()
    out = {"lat": lat}
    for test in (0, 1):
        ts, sf = ref_planes(dll, lat, test)
        out[f"t{test}|tsurf"], out[f"t{test}|sstf"] = ts.reshape(lat.shape), sf.reshape(lat.shape)
    for name in RI.TERM_CASES:
        out[f"{name}|k1"] = ref_k1(dll, RI.term_inputs(name)[1]["agrid"])
    return out


def written(bd, name, a):
    """the range of a field of the chained case that the recorder keeps (make_held_suarez_golden.written)"""
    if name == "u":
        return bd.view(a, "U", bd.is_, bd.ie, bd.js, bd.je + 1)
    if name == "v":
        return bd.view(a, "V", bd.is_, bd.ie + 1, bd.js, bd.je)
    if name == "pe":
        return a[1:-1, :, 1:-1]
    if name in ("pt", "ua", "va", "ps", "delp", "q"):
        return compute(bd, a)
    return a


def run_chain(dll):
    """the column loop, then the reference's whole fv_update_phys (up_driver.F90 of the fv_update_phys recipe), on one state"""
    import held_suarez_inputs as HI
    c = RI.CHAIN
    bd, st = RI.chain_inputs()
    o = {n: a.copy(order="F") for n, a in st.items()}
    i, f = C.c_int, C.c_double
    km, nq = c["km"], c["nq"]
    dll.reed_run_nq(i(bd.is_), i(bd.ie), i(bd.js), i(bd.je), i(bd.ng), i(km), i(nq), f(c["pdt"]), i(int(c["hydrostatic"])), i(c["reed_test"]),
                    i(int(c["do_reed_cond"])), i(int(c["reed_cond_only"])), i(int(c["reed_alt_mxg"])),
                    *(p(o[n]) for n in ("agrid", "delp", "pt", "ua", "va", "q", "pe", "peln", "phis", "delz", "u_dt", "v_dt", "t_dt", "q_dt", "rain")))
    idx = (C.c_int * 8)(1, -1, -1, -1, -1, -1, -1, -1)
    adj = np.ones(nq, dtype=np.int32)
    ak, bk = (np.ascontiguousarray(a) for a in HI.eta_levels(km))
    qdiag, ts = np.zeros((1,), order="F"), np.zeros((bd.nx, bd.ny), order="F")
    dll.up_run(i(bd.is_), i(bd.ie), i(bd.js), i(bd.je), i(bd.ng), i(km), i(nq), i(nq), i(1), idx, adj.ctypes.data_as(C.POINTER(C.c_int)),
               i(1), i(1), i(1), f(c["pdt"]), f(c["ptop"]), f(0.0), p(ak), p(bk),
               *(p(o[n]) for n in ("u", "v", "w", "delp", "pt", "q")), p(qdiag), *(p(o[n]) for n in ("ua", "va", "ps", "pe", "peln", "pk", "pkz")),
               p(o["phis"]), p(o["u_srf"]), p(o["v_srf"]), p(ts), *(p(o[n]) for n in ("delz", "u_dt", "v_dt", "t_dt", "q_dt")))
    assert not ts.any()
    return bd, st, o


def record_chain(dll):
    bd, st, o = run_chain(dll)
    out = {"chain|sha": np.array(RI.checksum(st))}
    for n in st:
        m = np.ones(o[n].shape, dtype=bool)
        if n in RI.CHAIN_OUT:
            written(bd, n, m)[...] = False
            out[f"chain|out|{n}"] = np.ascontiguousarray(written(bd, n, o[n]))
            assert not np.array_equal(written(bd, n, o[n]), written(bd, n, st[n])), f"chain: {n} did not change"
        assert np.array_equal(o[n][m].view(np.uint64), st[n][m].view(np.uint64)), f"chain: the reference wrote {n} outside the range the recorder keeps"
    return out


def rel_rms(a, b):
    d = float(np.sqrt(np.mean((a - b) ** 2)))
    s = float(np.sqrt(np.mean(b ** 2)))
    return d / s if s > 0.0 else (0.0 if d == 0.0 else np.inf)


def measure(dll):
    import parity_reed as S
    from gfdl_atmos_cubed_sphere_amd.lib import Fv3Lib
    subprocess.check_call(["make", "-C", os.path.join(os.path.dirname(HERE), "hostemu"), "-s"])
    emu = Fv3Lib(os.path.join(os.path.dirname(HERE), "hostemu", "libfv3_hostemu.so"))
    base, spread, libd = {}, {}, {}

    def up(d, key, v):
        d[key] = max(d.get(key, 0.0), v)
    for name, c in RI.CASES.items():
        bd, st = RI.case_inputs(name)
        pr = RI.params_of(c)
        o = run_ref(dll, c, bd, st)
        fam = S.family(c)
        plain = {n: a.copy(order="F") for n, a in st.items()}
        R.reed_wrapper(bd, c["km"], pr, plain)
        got = S.run_lib(emu, bd, st, pr)
        for n in S.fields_of(c):
            cv = (lambda a: compute(bd, a)) if n in ("u_dt", "v_dt") else (lambda a: a)      # noqa: E731
            up(base, (fam, n), rel_rms(cv(plain[n]), cv(o[n])))
            up(libd, (fam, n), rel_rms(cv(got[n]), cv(o[n])))
        for seed in range(SEEDS):
            pert = {n: a.copy(order="F") for n, a in st.items()}
            R.reed_wrapper(bd, c["km"], pr, pert, M=R.Math(9000 + seed))
            for n in S.fields_of(c):
                cv = (lambda a: compute(bd, a)) if n in ("u_dt", "v_dt") else (lambda a: a)      # noqa: E731
                up(spread, (fam, n), rel_rms(cv(pert[n]), cv(plain[n])))
    print("family, field: perturbed restatement vs restatement (MEASURED) | restatement vs compiled reference | library (CPU harness) vs compiled reference")
    for key in sorted(spread):
        print(f"  {key[0]:10s} {key[1]:5s}: {spread[key]:.3e} | {base[key]:.3e} | {libd[key]:.3e}")
        assert base[key] <= 10.0 * spread[key], f"{key}: the unperturbed restatement is not within the spread of the compiled reference"
    print("MEASURED = {" + ", ".join(f'("{k[0]}", "{k[1]}"): {v:.3e}' for k, v in sorted(spread.items())) + "}")
    tspread, tbase, tlib = {}, {}, {}
    for name, c in RI.TERM_CASES.items():
        bd, st = RI.term_inputs(name)
        o = run_term(dll, c, bd, st)
        k1 = R.term_k1(st["agrid"], RI.PI)
        plain = {n: st[n].copy(order="F") for n in ("cl", "cl2")}
        R.terminator_advance(c["pdt"], c["fill"], k1, plain["cl"], plain["cl2"])
        got = S.run_term(emu, bd, st, c)
        for n in ("cl", "cl2"):
            up(tbase, n, rel_rms(plain[n], o[n]))
            up(tlib, n, rel_rms(got[n], o[n]))
        for seed in range(SEEDS):
            pert = {n: st[n].copy(order="F") for n in ("cl", "cl2")}
            R.terminator_advance(c["pdt"], c["fill"], k1, pert["cl"], pert["cl2"], M=R.Math(9100 + seed))
            for n in ("cl", "cl2"):
                up(tspread, n, rel_rms(pert[n], plain[n]))
    for n in ("cl", "cl2"):
        print(f"  terminator {n}: {tspread[n]:.3e} | {tbase[n]:.3e} | {tlib[n]:.3e}")
        assert tbase[n] <= 10.0 * tspread[n], n
    print("TERM_MEASURED = {" + ", ".join(f'"{n}": {tspread[n]:.3e}' for n in ("cl", "cl2")) + "}")
    lat = RI.latitude()
    for test in (0, 1):
        ts, sf = ref_planes(dll, lat, test)
        mine = S.lib_planes(emu, lat, test)
        for n, a, b in (("Tsurf", mine[0], ts.reshape(lat.shape)), ("sstf", mine[1], sf.reshape(lat.shape))):
            print(f"reed_test {test} plane {n}: host libm against the reference's compiler, {lat.size} latitudes: bit-identical "
                  f"{bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))}, max relative difference {float(np.max(np.abs(a - b) / np.abs(b))):.3e}")
    for name in RI.TERM_CASES:
        bd, st = RI.term_inputs(name)
        a, b = S.lib_k1(emu, bd, st["agrid"]), ref_k1(dll, st["agrid"])
        print(f"{name} k1: bit-identical {bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))}, max difference {float(np.max(np.abs(a - b))):.3e}")


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
    with tempfile.TemporaryDirectory() as tmp:
        dll = build(tmp)
        if "--measure" in sys.argv:
            return measure(dll)
        files = {}
        for name, c in RI.CASES.items():
            files.setdefault(c["group"], {}).update(record(dll, name))
        for name in RI.TERM_CASES:
            files.setdefault("terminator", {}).update(record_term(dll, name))
        files["planes"] = record_planes(dll)
        files["chain"] = record_chain(dll)
        os.makedirs(OUT_DIR, exist_ok=True)
        total = 0
        for group, d in files.items():
            path = os.path.join(OUT_DIR, f"{group}.npz")
            save(path, d)
            total += os.path.getsize(path)
            assert os.path.getsize(path) <= LIMIT, f"{path}: larger than the largest golden committed before"
        print(f"{len(files)} files, {total} bytes")


if __name__ == "__main__":
    main()
