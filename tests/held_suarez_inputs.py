"""Seeded inputs of the Held_Suarez_Tend / age_of_air tests (driver/solo/hswf.F90), shared by the recorder of the reference goldens
(tests/golden/make_held_suarez_golden.py), the numpy restatement's own test and the library tests.  Pure numpy.

The columns.  ps uniform in 9.5e4 .. 1.02e5.  The interfaces: km >= 12 ("deep"): pe = ak + bk ps with ak, bk of eta_levels(km) --
interfaces spaced geometrically from 1 Pa to 500 hPa, then 800 and 1000 hPa, so that with strat every column has layers with pl <= 1e2 (mesosphere),
1e2 < pl <= 100e2 (stratosphere) and above (troposphere), and the bottom layers lie beyond sigma = 0.7 (friction).  km = 1: ONE layer
from a seeded top of 0.2 .. 0.8 ps -- pl / ps crosses 0.7 near a top of 0.49 ps, so some columns have friction and some have none;
km = 2: interfaces at 0.05 .. 0.3 ps and 0.5 .. 0.9 ps.  No bottom layer is anywhere near 100 hPa (the reference reads pl(npz+1)
there).  peln = log(pe) and pkz = (pk(k+1) - pk(k)) / (kappa (peln(k+1) - peln(k))) are the hydrostatic model's; the ring of pe
(is-1, ie+1, js-1, je+1) is noise.  T = 210 .. 300 K rising with pressure + 3 K N(0, 1), winds 10 m/s N(0, 1); the incoming
tendencies t_dt 2e-3 K/s N(0, 1), u_dt, v_dt 1e-3 m/s2 N(0, 1) in every cell, halo included (zero_tendencies: all three zero).

The latitude is a seeded FIELD, not the constant a doubly periodic grid has (the routine is pointwise in it): uniform in
(-pi/2, pi/2), with cells planted at pi/2 - 10^-n and -(pi/2 - 10^-n), n = 2 .. 12, at 0 and at +-1e-9; the halo of agrid and its
longitudes are noise.
"""
from __future__ import annotations

import numpy as np

from gfdl_atmos_cubed_sphere_amd.layout import Bounds
from parity_phys import checksum  # noqa: F401

KAPPA = 2.0 / 7.0
PI = 3.14159265358979323846       # constants_mod's pi
RADIUS = 6.3712e6                 # constants_mod's radius, fv_arrays_mod's unless a small earth scales it
IN = ("delp", "peln", "pe", "pkz", "pt", "ua", "va")
OUT = ("t_dt", "u_dt", "v_dt")
DEVICE = IN + OUT
SETS = {"std": (False, False), "strat": (True, False), "zurita": (False, True), "strat_zurita": (True, True)}   # name -> (strat, zurita)


def eta_levels(km):
    """ak, bk (km + 1 each) of the deep columns: interfaces spaced geometrically from 1 Pa to 500 hPa, then 800 and 1000 hPa (the
    bottom layer lies beyond sigma = 0.7, the one above it does not); pure pressure above 50 hPa"""
    ph = np.concatenate([np.geomspace(1.0, 5.0e4, km - 1), [8.0e4, 1.0e5]])
    bk = np.where(ph > 5.0e3, (ph - 5.0e3) / (1.0e5 - 5.0e3), 0.0)
    return ph - bk * 1.0e5, bk


def latitude(rng, nx, ny):
    lat = rng.uniform(-0.5 * PI, 0.5 * PI, (nx, ny))
    flat = lat.reshape(-1)
    plant = [0.5 * PI - 10.0 ** -n for n in range(2, 13)] + [-(0.5 * PI - 10.0 ** -n) for n in range(2, 13)] + [0.0, 1.0e-9, -1.0e-9]
    where = rng.permutation(flat.size)[:min(len(plant), flat.size // 2)]
    flat[where] = rng.permutation(plant)[:len(where)]
    return flat.reshape(nx, ny)


def state(nx, ny, km, seed, zero_tendencies=False):
    """-> (bd, dict of arrays in the library's layouts; "agrid" (A x 2) and "lat" (is:ie, js:je) among them)"""
    bd = Bounds(1, nx, 1, ny)
    ng = bd.ng
    rng = np.random.default_rng(seed)
    ps = rng.uniform(9.5e4, 1.02e5, (nx, ny))
    pe3 = np.empty((nx, ny, km + 1))
    if km >= 12:
        ak, bk = eta_levels(km)
        pe3[...] = ak[None, None, :] + bk[None, None, :] * ps[:, :, None]
    elif km == 1:
        pe3[:, :, 0] = ps * rng.uniform(0.2, 0.8, (nx, ny))
        pe3[:, :, 1] = ps
    else:
        frac = np.sort(rng.uniform(0.0, 1.0, (nx, ny, km - 1)), axis=2)
        pe3[:, :, 0] = ps * rng.uniform(0.05, 0.3, (nx, ny))
        lo = 0.5 + 0.4 * frac
        pe3[:, :, 1:km] = ps[:, :, None] * lo
        pe3[:, :, km] = ps
    peln_c = np.log(pe3)
    pk = np.exp(KAPPA * peln_c)
    dl = peln_c[:, :, 1:] - peln_c[:, :, :-1]
    dpc = pe3[:, :, 1:] - pe3[:, :, :-1]
    pkz = (pk[:, :, 1:] - pk[:, :, :-1]) / (KAPPA * dl)
    pm = dpc / dl
    T = 210.0 + 90.0 * (pm / 1.0e5) + 3.0 * rng.standard_normal((nx, ny, km))

    def halo(c):
        a = np.asfortranarray(rng.uniform(-1.0, 1.0, bd.shape("A", c.shape[2])))
        a[ng:ng + nx, ng:ng + ny] = c
        return a
    pe = np.asfortranarray(rng.uniform(1.0, 2.0, (nx + 2, km + 1, ny + 2)))
    pe[1:-1, :, 1:-1] = np.transpose(pe3, (0, 2, 1))
    lat = latitude(rng, nx, ny)
    agrid = np.asfortranarray(rng.uniform(-1.0, 1.0, bd.shape("A") + (2,)))
    agrid[ng:ng + nx, ng:ng + ny, 1] = lat
    st = dict(delp=halo(dpc), pt=halo(T), ua=halo(10.0 * rng.standard_normal((nx, ny, km))), va=halo(10.0 * rng.standard_normal((nx, ny, km))),
              pe=pe, peln=np.asfortranarray(np.transpose(peln_c, (0, 2, 1))), pkz=np.asfortranarray(pkz),
              u_dt=np.asfortranarray(1.0e-3 * rng.standard_normal(bd.shape("A", km))), v_dt=np.asfortranarray(1.0e-3 * rng.standard_normal(bd.shape("A", km))),
              t_dt=np.asfortranarray(2.0e-3 * rng.standard_normal((nx, ny, km))), agrid=agrid, lat=np.asfortranarray(lat))
    if zero_tendencies:
        for n in OUT:
            st[n][...] = 0.0
    return bd, st


# ---- the recorded cases: 6 x 4 columns.  Per (strat, zurita) set -- the golden file tests/golden/held_suarez_<set>.npz --: km 1, 2, 12,
# 32 with non-zero incoming tendencies at pdt = 225 s on the earth; at km = 12 also zero incoming tendencies (the pair of fresh), a
# second pdt (1800 s), and a small earth (radius / 10, pdt = 60 s)
NX, NY = 6, 4
CASES = {}
for _g, (_s, _z) in SETS.items():
    _base = dict(group=_g, strat=_s, zurita=_z, rd_zur=1.0 / 25.0, pdt=225.0, radius=RADIUS, zero=False)
    for _m, _km in enumerate((1, 2, 12, 32)):
        CASES[f"{_g}/km{_km}"] = dict(_base, km=_km, seed=1100 + 10 * len(CASES) + _m)
    CASES[f"{_g}/zero_incoming"] = dict(_base, km=12, zero=True, seed=1100 + 10 * len(CASES))
    CASES[f"{_g}/pdt1800"] = dict(_base, km=12, pdt=1800.0, seed=1100 + 10 * len(CASES))
    CASES[f"{_g}/small_earth"] = dict(_base, km=12, pdt=60.0, radius=RADIUS / 10.0, rd_zur=1.0 / 10.0, seed=1100 + 10 * len(CASES))
# age_of_air: the tracer is noise, halo included; time = 0 zeroes it, time > 0 sets it at and below 750 hPa
AGE_CASES = {"age/time0": dict(km=12, time=0.0, seed=1501), "age/tiny": dict(km=12, time=5.0e-7, seed=1502),
             "age/time_1d": dict(km=12, time=86400.0, seed=1503), "age/km2": dict(km=2, time=3.0e7, seed=1504)}


def case_inputs(name):
    c = CASES[name]
    return state(NX, NY, c["km"], c["seed"], zero_tendencies=c["zero"])


def age_inputs(name, nx=NX, ny=NY):
    c = AGE_CASES[name]
    bd, st = state(nx, ny, c["km"], c["seed"])
    q = np.asfortranarray(np.random.default_rng(c["seed"] + 1).uniform(-1.0, 1.0, bd.shape("A", c["km"])))
    return bd, dict(pe=st["pe"], q=q)


# ---- the chained case: Held_Suarez_Tend on zeroed tendencies, then the reference's WHOLE fv_update_phys with the arguments of
# driver/solo/fv_phys.F90:677-684 (hydrostatic, moist_phys false, q_dt present and zero) on the one-rank doubly periodic domain of
# tests/golden/make_update_phys_golden.py: what FvDynamics.held_suarez is held to.  Deep columns with strat: all three branches
CHAIN = dict(km=12, seed=1601, pdt=225.0, strat=True, zurita=False, rd_zur=1.0 / 25.0, radius=RADIUS, nq=2, ptop=1.0)
CHAIN_OUT = ("u", "v", "pt", "ua", "va", "pe", "peln", "pk", "pkz", "ps", "u_srf", "v_srf", "t_dt", "u_dt", "v_dt")


def chain_inputs():
    c = CHAIN
    km, nq = c["km"], c["nq"]
    bd, st = state(NX, NY, km, c["seed"], zero_tendencies=True)
    rng = np.random.default_rng(c["seed"] + 1)
    F = np.asfortranarray
    st.update(u=F(10.0 * rng.standard_normal(bd.shape("U", km))), v=F(10.0 * rng.standard_normal(bd.shape("V", km))),
              w=F(0.5 * rng.standard_normal(bd.shape("A", km))), q=F(rng.uniform(0.0, 1.0, bd.shape("A", km) + (nq,))),
              ps=F(rng.uniform(1.0, 2.0, bd.shape("A"))), pk=F(np.exp(KAPPA * np.transpose(st["peln"], (0, 2, 1)))),
              u_srf=F(rng.uniform(1.0, 2.0, (NX, NY))), v_srf=F(rng.uniform(1.0, 2.0, (NX, NY))), delz=F(-rng.uniform(1.0, 2.0, (NX, NY, km))),
              q_dt=np.zeros((NX, NY, km, nq), order="F"))
    return bd, st
