"""Seeded inputs of the fv_subgrid_z tests (fv_sg_SHiELD, update_dwinds_phys), shared by the recorder of the reference goldens
(tests/golden/make_subgrid_golden.py), the numpy checker's own test and the library tests.  Pure numpy.

The columns: sigma = linspace(0, 1, km+1)^1.5, ps uniform in 9.5e4 .. 1.02e5, theta = 290 (1e5 / pm)^0.05 + 3 K N(0, 1), winds
10 m/s N(0, 1), w 0.5 N(0, 1), qv <= 1.5e-2 (pm / 1e5)^3, condensates <= 2e-4, delz hydrostatic from T_v.  With dt = 225 and
fv_sg_adj = 600 the compiled reference mixes 30 % (k_bot_full 5 of 12) to 76 % (full depth) of the cells and its top levels are
colder than t_min.  The warm-top branch (fv_sg.F90:322-324) never fires by itself: it is planted in columns of their own, 5 K and
more beyond 315 K and 325 K (the routine mixes the planted heat away at the full mass flux, ri = 0, so the larger excesses are what
is still above t_max in the second and third sweep), and every other cell stays 5 K clear of t_max -- that test is the routine's
one discontinuity.  Shapes with fewer than 12 levels take km MIDDLE layers of the 12-level grid, so that their layers are as
thin as the recipe's and mix at its rate; nothing there is colder than t_min, so the cold branch (:325-326) is planted as well, in
columns of their own, 5 K and more below 160 K.
"""
from __future__ import annotations

import numpy as np

from gfdl_atmos_cubed_sphere_amd.layout import Bounds
from parity_phys import checksum  # noqa: F401

RDGAS, RVGAS, GRAV, KAPPA = 287.04, 461.50, 9.80, 2.0 / 7.0
ZVIR = RVGAS / RDGAS - 1.0
DT, FV_SG_ADJ = 225.0, 600
SPECIES = ("sphum", "liq_wat", "rainwat", "ice_wat", "snowwat", "graupel")
# species indices (1-based) per nwat, as a field_table of that microphysics orders them
SPECIES_OF = {
    0: dict(sphum=1),
    1: dict(sphum=1),
    2: dict(sphum=1, liq_wat=2),
    3: dict(sphum=1, liq_wat=2, ice_wat=3),
    4: dict(sphum=1, liq_wat=2, rainwat=3),
    6: dict(sphum=1, liq_wat=2, rainwat=3, ice_wat=4, snowwat=5, graupel=6),
}
WARM_EXCESS = (5.0, 15.0, 300.0, 600.0)    # K beyond t_max of the planted layers (one column each, for 315 and for 325)
COLD_DEFICIT = (5.0, 40.0, 80.0, 110.0, 110.0, 120.0, 120.0, 130.0)    # K below 160 K of the planted lower layers (km < 12; one column each)


def columns(nx, ny, km, nqa, nwat, seed, ptop=300.0, plant=True):
    """-> (bd, dict of arrays in the library's layouts).  nqa: tracers of the array (those beyond the water species are passive)."""
    bd = Bounds(1, nx, 1, ny)
    ng = bd.ng
    rng = np.random.default_rng(seed)
    lo = max(0, 12 - km) // 2
    sig = (np.linspace(0.0, 1.0, max(km, 12) + 1) ** 1.5)[lo:lo + km + 1]
    ps = rng.uniform(9.5e4, 1.02e5, (nx + 2, ny + 2))
    pe = np.asfortranarray(np.transpose(ptop * (1.0 - sig)[None, None, :] + sig[None, None, :] * ps[:, :, None], (0, 2, 1)))   # (nx+2, km+1, ny+2)
    pec = np.transpose(pe[1:-1, :, 1:-1], (0, 2, 1))        # (nx, ny, km+1)
    peln_c = np.log(pec)
    dpc = pec[:, :, 1:] - pec[:, :, :-1]
    dl = peln_c[:, :, 1:] - peln_c[:, :, :-1]
    pm = dpc / dl
    pk = np.exp(KAPPA * peln_c)
    pkz = (pk[:, :, 1:] - pk[:, :, :-1]) / (KAPPA * dl)
    theta = 290.0 * (1.0e5 / pm) ** 0.05 + 3.0 * rng.standard_normal((nx, ny, km))
    T = theta * pkz * (1.0e5 ** -KAPPA)
    sp = SPECIES_OF[nwat]
    q = rng.uniform(0.0, 1.0, (nx, ny, km, nqa))
    q[..., sp["sphum"] - 1] *= 1.5e-2 * (pm / 1.0e5) ** 3
    for n in SPECIES[1:]:
        if n in sp:
            q[..., sp[n] - 1] *= 2.0e-4
    qv = q[..., sp["sphum"] - 1] if nwat else np.zeros_like(T)
    planted = np.zeros((nx, ny), dtype=bool)
    if plant:
        cols = rng.permutation(nx * ny)[:2 * len(WARM_EXCESS) + len(COLD_DEFICIT)]
        if km < 12:
            for m, ex in enumerate(COLD_DEFICIT):
                c = int(cols[2 * len(WARM_EXCESS) + m])
                i, j = c % nx, c // nx
                T[i, j, 1 + m % (km - 1)] = 160.0 - ex
                planted[i, j] = True
        n = 0
        for t_max in (315.0, 325.0):
            for ex in WARM_EXCESS:
                i, j = int(cols[n]) % nx, int(cols[n]) // nx
                k = 1 + n % max(1, min(km - 1, 4) - 1) if km > 2 else 0      # the upper layer of a pair inside every kbot the tests use
                qcon = sum(q[i, j, k, sp[s] - 1] for s in SPECIES[1:] if s in sp) if nwat >= 2 else 0.0
                T[i, j, k] = (t_max + ex) / (1.0 + (ZVIR if nwat else 0.0) * qv[i, j, k] - qcon)
                planted[i, j] = True
                n += 1
    tv_like = T * (1.0 + (ZVIR if nwat else 0.0) * qv)
    assert tv_like[~planted].max() < 315.0 - 5.0, "an unplanted cell is within 5 K of t_max"
    delz = -RDGAS * T * (1.0 + ZVIR * qv) * dl / GRAV

    def halo(c, noise=None):
        a = np.asfortranarray(rng.uniform(-1.0, 1.0, bd.shape("A", km) + c.shape[3:]) if noise is None else np.full(bd.shape("A", km) + c.shape[3:], noise))
        a[ng:ng + nx, ng:ng + ny] = c
        return a
    st = dict(
        delp=halo(dpc, 1.0e3), ta=halo(T), qa=halo(q), ua=halo(10.0 * rng.standard_normal((nx, ny, km))),
        va=halo(10.0 * rng.standard_normal((nx, ny, km))), w=halo(0.5 * rng.standard_normal((nx, ny, km))),
        pe=pe, peln=np.asfortranarray(np.transpose(peln_c, (0, 2, 1))), pkz=np.asfortranarray(pkz), delz=np.asfortranarray(delz))
    st["planted"] = planted
    return bd, st


def tile_tendencies(nx, ny, npz, seed):
    """update_dwinds_phys on grid_type = 4: u_dt, v_dt with every halo cell filled, u, v"""
    bd = Bounds(1, nx, 1, ny)
    rng = np.random.default_rng(seed)
    f = lambda kind: np.asfortranarray(rng.standard_normal(bd.shape(kind, npz)))      # noqa: E731
    return bd, dict(u_dt=1.0e-3 * f("A"), v_dt=1.0e-3 * f("A"), u=10.0 * f("U"), v=10.0 * f("V"))


# ---- the recorded cases of fv_sg_SHiELD: 8 x 4 columns; name -> parameters.  group = the golden file the case is kept in
# (tests/golden/subgrid_<group>.npz), so that no file outgrows the largest golden committed before
SG_NX, SG_NY = 8, 4


def _sg_case(group, hyd, nwat, nq, kbf=5, weak=0, ptop=300.0, km=12, nqa=None, seed=11):
    return dict(group=group, hydrostatic=hyd, nwat=nwat, nq=nq, nqa=nqa or nq, k_bot_full=kbf, fv_sg_adj_weak=weak, ptop=ptop, km=km, seed=seed)


SG_CASES = {}
for _nwat, _nq in ((0, 1), (1, 1), (2, 2), (3, 4), (4, 4), (6, 7)):
    SG_CASES[f"nh/nwat{_nwat}"] = _sg_case("sg_nh", False, _nwat, _nq, seed=11 + _nwat)
for _nwat, _nq in ((0, 1), (3, 4), (6, 7)):
    SG_CASES[f"hydro/nwat{_nwat}"] = _sg_case("sg_hydro", True, _nwat, _nq, seed=21 + _nwat)
SG_CASES["nh/full_depth"] = _sg_case("sg_depth", False, 6, 7, kbf=12, seed=31)
SG_CASES["hydro/full_depth"] = _sg_case("sg_depth", True, 6, 7, kbf=12, seed=32)
SG_CASES["nh/weak900"] = _sg_case("sg_depth", False, 6, 7, weak=900, seed=33)
SG_CASES["hydro/weak900"] = _sg_case("sg_hydro", True, 0, 1, weak=900, seed=34)
SG_CASES["nh/ptop1"] = _sg_case("sg_misc", False, 6, 7, ptop=1.0, seed=35)
SG_CASES["nh/km2"] = _sg_case("sg_misc", False, 6, 7, kbf=2, km=2, seed=36)
SG_CASES["hydro/km2"] = _sg_case("sg_misc", True, 2, 2, kbf=2, km=2, seed=37)
SG_CASES["nh/nq_below_array"] = _sg_case("sg_misc", False, 6, 6, nqa=8, seed=38)
SG_OUT = ("ta", "qa", "ua", "va", "w", "u_dt", "v_dt")


def sg_case_inputs(name):
    c = SG_CASES[name]
    bd, st = columns(SG_NX, SG_NY, c["km"], c["nqa"], c["nwat"], c["seed"], ptop=c["ptop"])
    st.pop("planted")
    st["u_dt"], st["v_dt"] = bd.zeros("A", c["km"]), bd.zeros("A", c["km"])
    return bd, st


# ---- update_dwinds_phys: the geometry it reads, from the ORACLE's sphere, and the recorded cases ------------------------------------
def oracle_dwinds_geom(ref, t):
    """what fv3_grid_upload_dwinds takes, from tests/grid_oracle.RefSphere (oracle/fv_grid.c): vlon, vlat from agrid by unit_vect_latlon
    (fv_grid_utils.F90:2220-2243), es(:,i,j,1), ew(:,i,j,2) on the compute domain, edge_vect_*"""
    o, N = ref.ng, ref.N
    ag = ref.f("agrid", t)
    lon, lat = ag[..., 0], ag[..., 1]
    F = np.asfortranarray
    return dict(vlon=F(np.stack([-np.sin(lon), np.cos(lon), np.zeros_like(lon)], axis=-1)),
                vlat=F(np.stack([-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)], axis=-1)),
                es1=F(ref.f("es", t)[o:o + N, o:o + N + 1, 0:3].copy()), ew2=F(ref.f("ew", t)[o:o + N + 1, o:o + N, 3:6].copy()),
                **{n: np.ascontiguousarray(ref.f(n, t)) for n in ("edge_vect_w", "edge_vect_e", "edge_vect_s", "edge_vect_n")})


def oracle_dwinds_reference_shapes(ref, t):
    """the same members in the shapes the reference's gridstruct has: es (3, isd:ied, jsd:jed+1, 2), ew (3, isd:ied+1, jsd:jed, 2)"""
    g = oracle_dwinds_geom(ref, t)
    four = lambda a: np.asfortranarray(np.transpose(a.reshape(a.shape[0], a.shape[1], 2, 3), (3, 0, 1, 2)))      # noqa: E731
    return dict(vlon=g["vlon"], vlat=g["vlat"], es=four(ref.f("es", t)), ew=four(ref.f("ew", t)),
                **{n: g[n] for n in ("edge_vect_w", "edge_vect_e", "edge_vect_s", "edge_vect_n")})


DW_DT = 225.0
DW_CASES = {"tile": dict(grid_type=4, nx=9, ny=7, npz=2, seed=51), "c12_face": dict(grid_type=0, npx=13, npz=2, face=2, seed=52)}


def dw_case_inputs(name):
    """-> (bd, npx, npy, fields, geometry or None): u_dt, v_dt with every halo cell filled from the seed, u, v"""
    c = DW_CASES[name]
    if c["grid_type"] == 4:
        bd, t = tile_tendencies(c["nx"], c["ny"], c["npz"], c["seed"])
        return bd, c["nx"] + 1, c["ny"] + 1, t, None
    import grid_oracle as GO
    n = c["npx"] - 1
    bd, t = tile_tendencies(n, n, c["npz"], c["seed"])
    return bd, c["npx"], c["npx"], t, oracle_dwinds_geom(GO.ref_sphere(c["npx"]), c["face"])
