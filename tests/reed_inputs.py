"""Seeded inputs of the Reed-Jablonowski simple-physics and terminator tests (driver/solo/fv_phys.F90:551-602, :2332-2894), shared by
the recorder of the reference goldens (tests/golden/make_reed_golden.py), the numpy restatement's own test and the library tests.
Pure numpy.

The columns.  ps uniform in 9.5e4 .. 1.02e5; pure sigma interfaces pe = sigma ps.  km >= 12 ("deep"): sigma spaced geometrically
from 0.005 to 0.7, then 0.82, 0.92, 0.98, 1 -- interfaces on both sides of pbltop = 85000 Pa, and the two lowest interfaces below
1000 m, the rest above.  km = 1: ONE layer from a seeded top of 0.2 .. 0.8 ps (both k-loops of the solve are empty).  km = 2: a top
at 0.05 .. 0.3 ps and ONE interface at 0.78 .. 0.98 ps, on either side of 85000 Pa and of 1000 m.  peln = log(pe); the ring of pe
(is-1, ie+1, js-1, je+1) is noise.  T = 210 .. 300 K rising with pressure + 3 K N(0, 1); q = rh x an approximate saturation value
with rh uniform in 0.3 .. 1.3 (saturated and unsaturated cells), 6 % of the cells negative; winds 12 m/s N(0, 1) (bottom wind on
both sides of v20 = 20); phis 0 .. 3000 m2/s2; delz = the hydrostatic thickness x (1 + 0.02 N(0, 1)), negative.  The incoming
tendencies: t_dt 2e-3 K/s N(0, 1), u_dt, v_dt 1e-3 m/s2 N(0, 1) in every cell, halo included, q_dt 1e-8 1/s N(0, 1)
(zero_tendencies: all four zero); rain is noise.

The latitude is ONE seeded field for every case, not the constant a doubly periodic grid has (the routine is pointwise in it):
uniform in (-pi/2, pi/2) with cells planted at +-(pi/2 - 10^-n), n = 2 .. 13, at 0 and at +-1e-9 (held_suarez_inputs.latitude, one
decade closer to the poles).
"""
from __future__ import annotations

import numpy as np

import held_suarez_inputs as HI
from gfdl_atmos_cubed_sphere_amd.layout import Bounds
from parity_phys import checksum  # noqa: F401

PI = HI.PI
# the reference's constants_mod (GFDL defaults) and gfdl_mp_mod's c_liq: what tests/golden/reed_ref/reed_consts.F90 states
CONSTS = dict(grav=9.80, rdgas=287.04, rvgas=461.50, cp_air=287.04 / (2.0 / 7.0), cp_vapor=4.0 * 461.50, c_liq=4.218e3, hlv=2.500e6,
              radius=6.3712e6, omega=7.2921e-5, pi=PI)
IN = ("delp", "pt", "ua", "va", "q", "pe", "peln", "phis", "delz")
OUT = ("u_dt", "v_dt", "t_dt", "q_dt", "rain")
DEVICE = IN + OUT
# (do_reed_cond, reed_cond_only, reed_alt_mxg)
FLAGS = {"cond": (True, False, False), "nocond": (False, False, False), "condonly": (True, True, False), "alt": (True, False, True)}
NX, NY = 12, 7
LAT_SEED = 3001


def sigma_levels(km):
    return np.concatenate([np.geomspace(0.005, 0.7, km - 3), [0.82, 0.92, 0.98, 1.0]])


def latitude(nx=NX, ny=NY, seed=LAT_SEED):
    """held_suarez_inputs.latitude with the planted cells going on to 10^-13 from either pole"""
    rng = np.random.default_rng(seed)
    flat = rng.uniform(-0.5 * PI, 0.5 * PI, nx * ny)
    plant = [0.5 * PI - 10.0 ** -n for n in range(2, 14)] + [-(0.5 * PI - 10.0 ** -n) for n in range(2, 14)] + [0.0, 1.0e-9, -1.0e-9]
    where = rng.permutation(flat.size)[:min(len(plant), flat.size // 2)]
    flat[where] = plant[:len(where)] if len(where) == len(plant) else rng.permutation(plant)[:len(where)]
    return flat.reshape(nx, ny)


def state(nx, ny, km, seed, zero_tendencies=False, lat_seed=LAT_SEED):
    """-> (bd, dict of arrays in the library's layouts; "agrid" (A x 2) and "lat" (is:ie, js:je) among them)"""
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
    qv = qs * rng.uniform(0.3, 1.3, (nx, ny, km))
    neg = rng.uniform(0.0, 1.0, (nx, ny, km)) < 0.06
    neg.reshape(-1)[rng.integers(0, neg.size, 3)] = True                   # (km = 1 has 84 cells: never none)
    qv[neg] = -1.0e-5 * rng.uniform(0.1, 1.0, int(neg.sum()))
    dz = -(287.04 / 9.80) * T * (1.0 + 0.608 * np.maximum(qv, 0.0)) * dl * (1.0 + 0.02 * rng.standard_normal((nx, ny, km)))

    def halo(c):
        shp = bd.shape("A", c.shape[2]) if c.ndim == 3 else bd.shape("A")
        a = np.asfortranarray(rng.uniform(-1.0, 1.0, shp))
        a[ng:ng + nx, ng:ng + ny] = c
        return a
    pe = np.asfortranarray(rng.uniform(1.0, 2.0, (nx + 2, km + 1, ny + 2)))
    pe[1:-1, :, 1:-1] = np.transpose(pe3, (0, 2, 1))
    lat = latitude(nx, ny, lat_seed)
    agrid = np.asfortranarray(rng.uniform(-1.0, 1.0, bd.shape("A") + (2,)))
    agrid[ng:ng + nx, ng:ng + ny, 1] = lat
    F = np.asfortranarray
    st = dict(delp=halo(dpc), pt=halo(T), ua=halo(12.0 * rng.standard_normal((nx, ny, km))), va=halo(12.0 * rng.standard_normal((nx, ny, km))),
              q=halo(qv), pe=pe, peln=F(np.transpose(peln_c, (0, 2, 1))), phis=halo(rng.uniform(0.0, 3000.0, (nx, ny))), delz=F(dz),
              u_dt=F(1.0e-3 * rng.standard_normal(bd.shape("A", km))), v_dt=F(1.0e-3 * rng.standard_normal(bd.shape("A", km))),
              t_dt=F(2.0e-3 * rng.standard_normal((nx, ny, km))), q_dt=F(1.0e-8 * rng.standard_normal((nx, ny, km))),
              rain=F(rng.uniform(1.0, 2.0, (nx, ny))), agrid=agrid, lat=F(lat))
    if zero_tendencies:
        for n in ("u_dt", "v_dt", "t_dt", "q_dt"):
            st[n][...] = 0.0
    return bd, st


# ---- the recorded cases: 12 x 7 columns; km 1, 2, 12, 32 x (hydrostatic, not) x reed_test 0, 1 x the four flag sets x two pdt x
# (non-zero, zero) incoming tendencies.  A golden file holds the cases of one (km, hydrostatic, reed_test, flag set) -- of km = 32 one
# pdt of them, so that every file stays under the recorder's LIMIT
PDTS = (225.0, 1800.0)
CASES = {}
for _km in (1, 2, 12, 32):
    for _hyd in (True, False):
        for _t in (0, 1):
            for _fn, (_c, _o, _a) in FLAGS.items():
                for _pdt in PDTS:
                    for _zero in (False, True):
                        _g = f"km{_km}_{'hyd' if _hyd else 'nh'}_t{_t}_{_fn}" + (f"_pdt{int(_pdt)}" if _km == 32 else "")
                        CASES[f"km{_km}/{'hyd' if _hyd else 'nh'}/t{_t}/{_fn}/pdt{int(_pdt)}/{'zero' if _zero else 'in'}"] = dict(
                            group=_g, km=_km, hydrostatic=_hyd, reed_test=_t, flags=_fn, do_reed_cond=_c, reed_cond_only=_o, reed_alt_mxg=_a,
                            pdt=_pdt, zero=_zero, seed=4100 + len(CASES))
GROUPS = sorted({c["group"] for c in CASES.values()})


def case_inputs(name):
    c = CASES[name]
    return state(NX, NY, c["km"], c["seed"], zero_tendencies=c["zero"])


def params_of(c, consts=None):
    return dict(pdt=c["pdt"], hydrostatic=c["hydrostatic"], reed_test=c["reed_test"], do_reed_cond=c["do_reed_cond"],
                reed_cond_only=c["reed_cond_only"], reed_alt_mxg=c["reed_alt_mxg"], consts=dict(CONSTS, **(consts or {})))


# ---- the terminator: Cl, Cl2 of 1e-6-ish on the whole A layout x km; negative values planted so that Cl + 2 Cl2 stays positive
# (the reference takes the square root of r*r + 2 r (Cl + 2 Cl2)); the longitudes cover day and night (k1 = 0) cells, halo included
TERM_CASES = {"term/fill": dict(km=12, pdt=225.0, fill=True, seed=5001), "term/nofill": dict(km=12, pdt=225.0, fill=False, seed=5002),
              "term/fill_pdt1800_km2": dict(km=2, pdt=1800.0, fill=True, seed=5003), "term/nofill_km1": dict(km=1, pdt=900.0, fill=False, seed=5004)}


def term_state(nx, ny, km, seed):
    bd = Bounds(1, nx, 1, ny)
    rng = np.random.default_rng(seed)
    shp = bd.shape("A", km)
    agrid = np.asfortranarray(np.stack([rng.uniform(0.0, 2.0 * PI, bd.shape("A")), rng.uniform(-0.5 * PI, 0.5 * PI, bd.shape("A"))], axis=2))
    cl = rng.uniform(0.0, 4.0e-6, shp)
    cl2 = rng.uniform(0.0, 2.0e-6, shp)
    pick = rng.uniform(0.0, 1.0, shp)
    a = pick < 0.1                      # Cl negative, Cl2 large enough
    cl[a] = -rng.uniform(1.0e-8, 1.0e-6, int(a.sum()))
    cl2[a] = rng.uniform(1.0e-6, 2.0e-6, int(a.sum()))
    b = (pick >= 0.1) & (pick < 0.2)    # Cl2 negative, Cl large enough
    cl2[b] = -rng.uniform(1.0e-8, 5.0e-7, int(b.sum()))
    cl[b] = rng.uniform(2.0e-6, 4.0e-6, int(b.sum()))
    return bd, dict(agrid=agrid, cl=np.asfortranarray(cl), cl2=np.asfortranarray(cl2))


def term_inputs(name, nx=NX, ny=NY):
    c = TERM_CASES[name]
    return term_state(nx, ny, c["km"], c["seed"])


# ---- the chained case: the wrapper with reed_sim_physics on zeroed tendencies, then the reference's WHOLE fv_update_phys with the
# arguments of driver/solo/fv_phys.F90:677-684 (moist_phys true, q_dt present) on the one-rank doubly periodic domain of
# tests/golden/make_update_phys_golden.py: what FvDynamics.reed_sim_phys is held to
CHAIN = dict(km=12, seed=5101, pdt=225.0, hydrostatic=True, reed_test=0, do_reed_cond=True, reed_cond_only=False, reed_alt_mxg=False, nq=2, ptop=1.0)
CHAIN_OUT = ("u", "v", "pt", "ua", "va", "delp", "q", "pe", "peln", "pk", "pkz", "ps", "u_srf", "v_srf", "t_dt", "u_dt", "v_dt", "q_dt", "rain")


def chain_inputs():
    c = CHAIN
    km, nq = c["km"], c["nq"]
    bd, st = state(NX, NY, km, c["seed"], zero_tendencies=True)
    rng = np.random.default_rng(c["seed"] + 1)
    F = np.asfortranarray
    q4 = F(rng.uniform(0.0, 1.0e-3, bd.shape("A", km) + (nq,)))
    q4[..., 0] = st["q"]
    peln_c = np.transpose(st["peln"], (0, 2, 1))
    pk = np.exp(HI.KAPPA * peln_c)
    st.update(u=F(10.0 * rng.standard_normal(bd.shape("U", km))), v=F(10.0 * rng.standard_normal(bd.shape("V", km))),
              w=F(0.5 * rng.standard_normal(bd.shape("A", km))), q=q4, ps=F(rng.uniform(1.0, 2.0, bd.shape("A"))), pk=F(pk),
              pkz=F((pk[:, :, 1:] - pk[:, :, :-1]) / (HI.KAPPA * (peln_c[:, :, 1:] - peln_c[:, :, :-1]))),
              u_srf=F(rng.uniform(1.0, 2.0, (NX, NY))), v_srf=F(rng.uniform(1.0, 2.0, (NX, NY))), q_dt=np.zeros((NX, NY, km, nq), order="F"))
    return bd, st
