"""Seeded inputs of the Kessler warm-rain tests (driver/solo/fv_phys.F90:1992-2291, driver/solo/qs_tables.F90), shared by the recorder
of the reference goldens (tests/golden/make_kessler_golden.py), the numpy restatement's own test and the library tests.  Pure numpy.

The columns.  ps uniform in 9.5e4 .. 1.02e5; pure sigma interfaces pe = sigma ps.  km >= 12: sigma spaced geometrically from 0.005
to 0.7, then 0.82, 0.92, 0.98, 1.  km = 1: ONE layer from a seeded top of 0.2 .. 0.8 ps (every k = 2 .. km loop is empty).  km = 2:
a top at 0.05 .. 0.3 ps and one interface at 0.78 .. 0.98 ps.  peln = log(pe), pk = exp(kappa peln); the ring of pe is noise.
T = 210 .. 300 K rising with pressure + 3 K N(0, 1).  Water, per cell from one uniform draw each:
  sphum    rh x an approximate saturation value, rh uniform in 0.2 .. 1.4 (saturated and subsaturated levels); 6 % of the cells
           negative (clamped by qv_min);
  liq_wat  30 % zero (clamped by qc_min), 25 % 1e-6 .. 1e-4 (cloud below the autoconversion threshold), 25 % 1.2e-3 .. 4e-3 (above
           it), 10 % -1e-5 .. -1e-6 with rain of 1e-4 .. 1e-3 (q2 < 0, qcon > 0), 10 % -1e-4 .. -1e-5 with rain zero or negative
           (qcon <= 0: left alone, then clamped);
  rainwat  where liq_wat did not decide it: 35 % zero, 15 % 1e-9 .. 1e-8 (rain that evaporates completely in one cycle), 35 %
           1e-5 .. 2e-3, 15 % -1e-6 .. -1e-7 (q3 < 0; qcon > 0 wherever there is cloud).
Planted, the same (i, j) in every case and every level of those columns: T = 100 K (ta < tmin: ap1 = 1, the first entries of the
table) and T = 380 K (ap1 capped at 2621).  Not hydrostatic only: delz of ONE column x 1e-11 on the levels above the bottom one -- a
dry density 1e11 times the bottom level's, the only way vr = 36.34 sqrt(rho(nz)/rho) (r qr)**0.1364 falls below vr_min = 1e-3.
Winds 12 m/s N(0, 1), w 0.5 m/s N(0, 1); delz = the hydrostatic thickness x (1 + 0.02 N(0, 1)), negative; u_dt, v_dt 1e-3 m/s2
N(0, 1) in every cell, halo included; rain, ps outside what the routine writes, and two tracer planes the routine does not read
are noise.
"""
from __future__ import annotations

import numpy as np

from gfdl_atmos_cubed_sphere_amd.layout import Bounds
from parity_phys import checksum  # noqa: F401

KAPPA = 2.0 / 7.0
# the reference's constants_mod (GFDL defaults) and gfdl_mp_mod's c_liq: what tests/golden/kessler_ref/kessler_standins.F90 states
CONSTS = dict(rdgas=287.04, rvgas=461.50, cp_air=287.04 / KAPPA, cp_vapor=4.0 * 461.50, hlv=2.500e6, c_liq=4.218e3, grav=9.80, kappa=KAPPA)
STATE = ("ua", "va", "w", "u_dt", "v_dt", "q", "pt", "delp", "delz", "pe", "peln", "pk", "ps", "rain")
NX, NY = 12, 7
NQ = 5
# (K_sedi_transport, do_K_sedi_w, do_K_sedi_heat)
FLAGS = {"none": (False, False, False), "tr": (True, False, False), "trw": (True, True, False), "trwh": (True, True, True), "heat": (False, False, True)}
COLD, HOT, DENSE = (2, 3), (9, 5), (5, 1)      # 0-based (i, j) of the planted columns


def sigma_levels(km):
    return np.concatenate([np.geomspace(0.005, 0.7, km - 3), [0.82, 0.92, 0.98, 1.0]])


def state(nx, ny, km, seed, hydrostatic=False, nq=NQ, tracers=(1, 2, 3)):
    """-> (bd, dict of arrays in the library's layouts)"""
    bd = Bounds(1, nx, 1, ny)
    ng = bd.ng
    rng = np.random.default_rng(seed)
    ps = rng.uniform(9.5e4, 1.02e5, (nx, ny))
    pe3 = np.empty((nx, ny, km + 1))
    if km >= 12:
        pe3[...] = sigma_levels(km)[None, None, :] * ps[:, :, None]
    elif km == 1:
        pe3[:, :, 0] = ps * rng.uniform(0.2, 0.8, (nx, ny))
        pe3[:, :, 1] = ps
    else:
        pe3[:, :, 0] = ps * rng.uniform(0.05, 0.3, (nx, ny))
        lo = np.sort(rng.uniform(0.78, 0.98, (nx, ny, km - 1)), axis=2)
        pe3[:, :, 1:km] = ps[:, :, None] * lo
        pe3[:, :, km] = ps
    peln_c = np.log(pe3)
    dl = peln_c[:, :, 1:] - peln_c[:, :, :-1]
    dpc = pe3[:, :, 1:] - pe3[:, :, :-1]
    pm = dpc / dl
    T = 210.0 + 90.0 * (pm / 1.0e5) + 3.0 * rng.standard_normal((nx, ny, km))
    qs = 0.622 * 610.71 / pm * np.exp(-5417.0 * (1.0 / T - 1.0 / 273.16))
    shp = (nx, ny, km)
    qv = qs * rng.uniform(0.2, 1.4, shp)
    neg = rng.uniform(0.0, 1.0, shp) < 0.06
    neg.reshape(-1)[rng.integers(0, neg.size, 3)] = True
    qv[neg] = -1.0e-5 * rng.uniform(0.1, 1.0, int(neg.sum()))
    U = lambda lo, hi: rng.uniform(lo, hi, shp)      # noqa: E731
    pl, pr_ = U(0.0, 1.0), U(0.0, 1.0)
    ql = np.zeros(shp)
    ql = np.where((pl >= 0.30) & (pl < 0.55), U(1.0e-6, 1.0e-4), ql)
    ql = np.where((pl >= 0.55) & (pl < 0.80), U(1.2e-3, 4.0e-3), ql)
    ql = np.where((pl >= 0.80) & (pl < 0.90), -U(1.0e-6, 1.0e-5), ql)
    ql = np.where(pl >= 0.90, -U(1.0e-5, 1.0e-4), ql)
    qr = np.zeros(shp)
    qr = np.where((pr_ >= 0.35) & (pr_ < 0.50), U(1.0e-9, 1.0e-8), qr)
    qr = np.where((pr_ >= 0.50) & (pr_ < 0.85), U(1.0e-5, 2.0e-3), qr)
    qr = np.where(pr_ >= 0.85, -U(1.0e-7, 1.0e-6), qr)
    qr = np.where((pl >= 0.80) & (pl < 0.90), U(1.0e-4, 1.0e-3), qr)
    qr = np.where(pl >= 0.90, np.where(pr_ < 0.5, 0.0, -U(1.0e-7, 1.0e-6)), qr)
    if nx > max(COLD[0], HOT[0]) and ny > max(COLD[1], HOT[1]):
        T[COLD[0], COLD[1], :] = 100.0
        T[HOT[0], HOT[1], :] = 380.0
    dz = -(287.04 / 9.80) * T * (1.0 + 0.608 * np.maximum(qv, 0.0)) * dl * (1.0 + 0.02 * rng.standard_normal(shp))
    if not hydrostatic and km >= 2 and nx > DENSE[0] and ny > DENSE[1]:
        dz[DENSE[0], DENSE[1], :km - 1] *= 1.0e-11

    def halo(c):
        full = bd.shape("A") + c.shape[2:]
        a = np.asfortranarray(rng.uniform(-1.0, 1.0, full))
        a[ng:ng + nx, ng:ng + ny] = c
        return a
    pe = np.asfortranarray(rng.uniform(1.0, 2.0, (nx + 2, km + 1, ny + 2)))
    pe[1:-1, :, 1:-1] = np.transpose(pe3, (0, 2, 1))
    q4 = rng.uniform(0.0, 1.0e-3, shp + (nq,))
    sp, lw, rw = (t - 1 for t in tracers)
    q4[..., sp], q4[..., lw], q4[..., rw] = qv, ql, qr
    F = np.asfortranarray
    st = dict(ua=halo(12.0 * rng.standard_normal(shp)), va=halo(12.0 * rng.standard_normal(shp)), w=halo(0.5 * rng.standard_normal(shp)),
              u_dt=F(1.0e-3 * rng.standard_normal(bd.shape("A", km))), v_dt=F(1.0e-3 * rng.standard_normal(bd.shape("A", km))),
              q=halo(q4), pt=halo(T), delp=halo(dpc), delz=F(dz), pe=pe, peln=F(np.transpose(peln_c, (0, 2, 1))),
              pk=F(np.exp(KAPPA * peln_c)), ps=halo(ps), rain=F(rng.uniform(1.0, 2.0, (nx, ny))))
    return bd, st


# ---- the recorded cases: 12 x 7 columns; km 1, 2, 12 x (hydrostatic, not) x moist_kappa (on, off) x the five flag sets, and km 32 x
# the five flag sets x ((hydrostatic, moist_kappa off), (not, on)).  K_cycle and pdt alternate down the list so that at km 12 and at
# km 32 every flag set runs with K_cycle 1 and 3 and with both pdt, K_cycle = 0 (nint(pdt/30.)) once per km <= 12; the tracer planes are
# (1, 2, 3) or (4, 1, 3) of nq = 5.  A golden file holds the cases of one (km, flag set) for km <= 2, one case's fields for km 12, and
# part of one case's fields for km 32, so that every file stays under the recorder's LIMIT.
PDTS = (30.0, 75.0)
CASES = {}
for _km in (1, 2, 12, 32):
    _n = 0
    for _fn in FLAGS:
        for _hyd, _mk in (((True, True), (True, False), (False, True), (False, False)) if _km < 32 else ((True, False), (False, True))):
            _kc = 0 if (_fn == "trwh" and not _hyd and _mk and _km < 32) else (1, 3)[_n % 2]
            _pdt = PDTS[(_n // 2) % 2] if _km < 32 else PDTS[(_n + list(FLAGS).index(_fn)) % 2]
            _name = f"km{_km}/{_fn}/{'hyd' if _hyd else 'nh'}/{'mk' if _mk else 'dry'}"
            CASES[_name] = dict(km=_km, flags=_fn, hydrostatic=_hyd, moist_kappa=_mk, K_cycle=_kc, pdt=_pdt, seed=7100 + len(CASES),
                                tracers=(4, 1, 3) if _n % 3 == 2 else (1, 2, 3),
                                group=(f"km{_km}_{_fn}" if _km <= 2 else _name.replace("/", "_")))
            _n += 1


def case_inputs(name):
    c = CASES[name]
    return state(NX, NY, c["km"], c["seed"], hydrostatic=c["hydrostatic"], tracers=c["tracers"])


def params_of(c, consts=None):
    tr, sw, sh = FLAGS[c["flags"]]
    sp, lw, rw = c.get("tracers", (1, 2, 3))
    return dict(pdt=c["pdt"], K_cycle=c["K_cycle"], K_sedi_transport=tr, do_K_sedi_w=sw, do_K_sedi_heat=sh, hydrostatic=c["hydrostatic"],
                moist_kappa=c["moist_kappa"], nq=c.get("nq", NQ), sphum=sp, liq_wat=lw, rainwat=rw, consts=dict(CONSTS, **(consts or {})))


# ---- the chained case: K_warm_rain with K_sedi_transport, then the reference's WHOLE fv_update_phys with the arguments of
# driver/solo/fv_phys.F90:677-684 (moist_phys true, q_dt present and zero, t_dt zero) on the one-rank doubly periodic domain of
# tests/golden/make_update_phys_golden.py: what FvDynamics.k_warm_rain is held to.  nwat = 4, the reference's "K_warm_rain with fake
# ice" (fv_thermodynamics.F90:295, :374): the fourth tracer stands for it
CHAIN = dict(km=12, seed=7901, pdt=75.0, K_cycle=3, flags="trw", hydrostatic=False, moist_kappa=False, nq=4, tracers=(1, 2, 3), ptop=1.0)
CHAIN_OUT = ("u", "v", "w", "pt", "ua", "va", "delp", "delz", "q", "pe", "peln", "pk", "ps", "u_dt", "v_dt", "rain")


def chain_inputs():
    c = CHAIN
    km, nq = c["km"], c["nq"]
    bd, st = state(NX, NY, km, c["seed"], hydrostatic=c["hydrostatic"], nq=nq, tracers=c["tracers"])
    rng = np.random.default_rng(c["seed"] + 1)
    F = np.asfortranarray
    peln_c = np.transpose(st["peln"], (0, 2, 1))
    pk = st["pk"]
    st.update(u=F(10.0 * rng.standard_normal(bd.shape("U", km))), v=F(10.0 * rng.standard_normal(bd.shape("V", km))),
              pkz=F((pk[:, :, 1:] - pk[:, :, :-1]) / (KAPPA * (peln_c[:, :, 1:] - peln_c[:, :, :-1]))),
              phis=F(rng.uniform(0.0, 3000.0, bd.shape("A"))), u_srf=F(rng.uniform(1.0, 2.0, (NX, NY))), v_srf=F(rng.uniform(1.0, 2.0, (NX, NY))),
              t_dt=np.zeros((NX, NY, km), order="F"), q_dt=np.zeros((NX, NY, km, nq), order="F"),
              u_dt=np.zeros(bd.shape("A", km), order="F"), v_dt=np.zeros(bd.shape("A", km), order="F"))      # fv_phys.F90:292-313
    return bd, st
