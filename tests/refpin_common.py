"""Cases that pin the oracle and the kernels to the REFERENCE's compiled Fortran (tests/ref_lib.py over
oracle/_ref/libfv3ref.so).  Shared by tests/test_reference_pin.py (oracle vs reference, live and against the goldens),
tests/golden/make_refpin_golden.py (records reference outputs), tests/test_reference_pin_hostemu.py and
tests/test_reference_pin_gpu.py (kernels vs reference, no oracle in between).

A case is (grid, inputs, parameters).  `run(M, routine, g, inp, par)` runs it through a backend M that has oracle_lib's
signatures -- oracle_lib itself or ref_lib -- and returns the outputs on the index ranges where the reference defines
them.  `run_lib(lib, ...)` does the same through a library that exports the fv3_* C ABI (the product or the host emulation).

Inputs are seeded, from the generators the parity checks use (smooth_state, nh_state, _courant, default_levels, the cubed
sphere's face metrics).
"""
from __future__ import annotations

import dataclasses

import numpy as np

import oracle_lib as O
import parity_common as P
from fields import smooth_state
from gfdl_atmos_cubed_sphere_amd.grid import METRIC_KINDS, GridStruct
from gfdl_atmos_cubed_sphere_amd.layout import Bounds, periodic_fill
from gfdl_atmos_cubed_sphere_amd.lib import GRAV, Context, nh_consts
from gfdl_atmos_cubed_sphere_amd.synthetic import CSW_OUT, DSW_PAR, PTOP, nh_state
from test_oracle_properties import _courant, default_levels

F = np.asfortranarray
NORTH_STAR = 1e-12          # BASELINE.json: the project's bound on any fp64 field
ALL_HORD = (1, 2, 3, 4, 5, -5, 6, -6, 7, 8, 9, 10, 11, 12, 13)

# ---- measured oracle-vs-reference bounds -----------------------------------------------------------------------------
# Where the oracle is bit-identical to the reference the tests assert np.array_equal (bound 0).  Where exp / log / ** go through
# libm in the reference and through include/fv3_math.h in the oracle they assert, FIELD BY FIELD, 10 x the worst relative
# difference measured over the cases of tests/test_reference_pin.py (floor 1e-15, ceiling NORTH_STAR).
#
# The metric is the one the project's bound is stated in (BASELINE.json north_star, parity_common.rel_rms): the RMS difference
# of a field relative to the field's RMS.  The largest difference over the field's largest magnitude (rel_max below) is the
# stricter reading of "worst relative difference"; it is written beside each figure.  In that norm ppe of Riem_Solver3 reaches
# 1.01e-12 at km = 127 (9.2e-13 at km = 79), i.e. the ceiling: ppe is the small nonhydrostatic part (of order 1e2 Pa) of a
# pressure of order 1e5 Pa, so the last bit of the pressure powers (6.6e-10 Pa) is 1e-12 of it, and the tridiagonal solve
# carries that into w (2e-12 m/s).  It is libm against fv3_math.h amplified by cancellation, not a transcription slip; RMS is
# asserted because a max norm over such a field measures its one worst cell.  README carries both figures.
MEASURED = {                                   # relative RMS              (rel_max)
    "riem_solver_c": {"gz": 5.8e-16,           #                            5.3e-15
                      "pef": 2.5e-16},         #                            2.9e-15
    "riem_solver3": {"w": 2.1e-13,             # km = 127                   4.4e-13
                     "ppe": 1.5e-13,           #                            1.01e-12
                     "delz": 4.7e-15,          #                            1.5e-14
                     "zh": 8.4e-16,            #                            3.6e-15
                     "pk": 7.8e-17, "pk3": 7.8e-17,   #                     9.3e-16
                     "peln": 1.9e-17,          #                            1.6e-16
                     "pe": 0.0},               # hydrostatic sums only: bit-identical
}
BIT_IDENTICAL = ("fv_tp_2d", "copy_corners", "c_sw", "d_sw", "a2b_ord4", "update_dz_c", "update_dz_d", "remap", "fillz")


def bound(routine, field=None):
    """the asserted oracle-versus-reference bound of one output field (field None: the routine's largest)"""
    if routine in BIT_IDENTICAL:
        return 0.0
    m = max(MEASURED[routine].values()) if field is None else MEASURED[routine][field]
    return 0.0 if m == 0.0 else min(NORTH_STAR, max(1e-15, 10.0 * m))


def rel_max(a, b):
    """worst difference relative to the field's largest magnitude"""
    s = float(np.max(np.abs(b))) if b.size else 0.0
    d = float(np.max(np.abs(a - b))) if b.size else 0.0
    return d / s if s > 0 else d


def compare(routine, got, ref, extra=0.0, what="", figures=None):
    """every output field of `got` against `ref`: bit equality when the field's bound (+ extra) is 0, else rel_rms <= bound.
    Returns the worst difference; figures (a dict) collects {field: (rel_rms, rel_max)} for the callers that measure."""
    worst = 0.0
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for n in sorted(ref):
        tol = bound(routine, n) + extra
        a, b = np.asarray(got[n]), np.asarray(ref[n])
        assert a.shape == b.shape, f"{routine} {what} {n}: shape {a.shape} != {b.shape}"
        assert np.all(np.isfinite(a)), f"{routine} {what} {n}: non-finite values"
        e = P.rel_rms(a, b) if tol > 0.0 else rel_max(a, b)
        worst = max(worst, e)
        if figures is not None:
            figures[n] = (float(P.rel_rms(a, b)), rel_max(a, b))
        if tol == 0.0:
            assert np.array_equal(a, b), f"{routine} {what} {n}: not bit-identical to the reference (rel max {e:.3e}, {int(np.sum(a != b))} of {a.size} differ)"
        else:
            assert e <= tol, f"{routine} {what} {n}: rel rms {e:.3e} > {tol:.1e}"
    return worst


# ---- grids -----------------------------------------------------------------------------------------------------------
def periodic_grid(nx, ny, perturb=True):
    return P.make_grid(Bounds(1, nx, 1, ny), perturb)


TILES = {                      # of a face with 24 x 24 cells (npx = 25): name -> (is, ie, js, je)
    "interior": (9, 16, 9, 16), "west": (1, 8, 9, 16), "east": (17, 24, 9, 16), "south": (9, 16, 1, 8),
    "north": (9, 16, 17, 24), "corner_sw": (1, 8, 1, 8), "corner_ne": (17, 24, 17, 24),
}


def subtile(g, i0, i1, j0, j1):
    """the fv_grid_type of the rank that owns cells (i0:i1, j0:j1) of face tile g (whole face, one tile)"""
    fb = g.bd
    bd = Bounds(i0, i1, j0, j1, ng=fb.ng)
    out = GridStruct(bd=bd, npx=g.npx, npy=g.npy, grid_type=g.grid_type, da_min=g.da_min, da_min_c=g.da_min_c,
                     lim_fac=g.lim_fac, do_diss_est=g.do_diss_est, prevent_diss_cooling=g.prevent_diss_cooling, do_f3d=g.do_f3d)
    for n, kind in METRIC_KINDS.items():
        out.m[n] = F(fb.view(g.m[n], kind, *bd.limits(kind)).copy())
    for n in ("sin_sg", "cos_sg"):
        out.m[n] = F(fb.view(g.m[n], "A", *bd.limits("A")).copy())
    for n in ("edge_w", "edge_e", "edge_s", "edge_n", "corner_f"):
        out.m[n] = g.m[n]
    out.sw_corner, out.se_corner = (i0 == 1 and j0 == 1), (i1 == g.npx - 1 and j0 == 1)
    out.nw_corner, out.ne_corner = (i0 == 1 and j1 == g.npy - 1), (i1 == g.npx - 1 and j1 == g.npy - 1)
    return out


def cut(g_face, g_tile, a, kind):
    """the tile's part (halo included) of a face field of stagger `kind`"""
    return F(g_face.bd.view(a, kind, *g_tile.bd.limits(kind)).copy())


_SPHERE = {}


def face_state(npx, npz, face=1, hydrostatic=False):
    """(g, st): gridstruct and smooth state (halos exchanged) of one whole face of the cubed sphere"""
    import cubed_common as CC
    key = (npx, npz, hydrostatic)
    if key not in _SPHERE:
        _SPHERE[key] = CC.global_state(npx, npz, hydrostatic)
    cs, gs, st = _SPHERE[key]
    return gs[face], {k: v.copy(order="F") for k, v in st[face].items()}


def tile_state(tile, npz, hydrostatic=False, npx=25, face=1):
    """(g, st) of a sub-tile of a face (TILES), or of the whole face for tile == "face" (all four corners, npx as given)"""
    gf, st = face_state(npx, npz, face, hydrostatic)
    if tile == "face":
        return dataclasses.replace(gf, m=dict(gf.m)), st      # the cached gridstruct stays as built: tests set flags on theirs
    g = subtile(gf, *TILES[tile])
    kinds = dict(u="U", v="V")
    return g, {k: cut(gf, g, v, kinds.get(k, "A")) for k, v in st.items()}


def grid_to_arrays(g, prefix="g_"):
    """a GridStruct as a flat dict of arrays (for an .npz)"""
    b = g.bd
    d = {prefix + "meta": np.array([b.is_, b.ie, b.js, b.je, b.ng, g.npx, g.npy, g.grid_type, int(g.bounded_domain),
                                    int(g.stretched_grid), int(g.sw_corner), int(g.se_corner), int(g.ne_corner), int(g.nw_corner),
                                    int(g.do_diss_est), int(g.prevent_diss_cooling), int(g.do_f3d)], dtype=np.int64),
         prefix + "real": np.array([g.da_min, g.da_min_c, g.lim_fac])}
    for n, a in g.m.items():
        if n in METRIC_KINDS or n in ("sin_sg", "cos_sg", "edge_w", "edge_e", "edge_s", "edge_n", "corner_f"):
            d[prefix + "m_" + n] = np.asarray(a)
    return d


def grid_from_arrays(d, prefix="g_"):
    mt, rl = [int(x) for x in d[prefix + "meta"]], [float(x) for x in d[prefix + "real"]]
    g = GridStruct(bd=Bounds(mt[0], mt[1], mt[2], mt[3], ng=mt[4]), npx=mt[5], npy=mt[6], grid_type=mt[7],
                   bounded_domain=bool(mt[8]), stretched_grid=bool(mt[9]), sw_corner=bool(mt[10]), se_corner=bool(mt[11]),
                   ne_corner=bool(mt[12]), nw_corner=bool(mt[13]), do_diss_est=bool(mt[14]), prevent_diss_cooling=bool(mt[15]),
                   do_f3d=bool(mt[16]), da_min=rl[0], da_min_c=rl[1], lim_fac=rl[2])
    for k in d:
        if k.startswith(prefix + "m_"):
            n = k[len(prefix) + 2:]
            g.m[n] = d[k] if n.startswith("edge_") or n == "corner_f" else F(d[k])
    return g


# ---- fv_tp_2d --------------------------------------------------------------------------------------------------------
TP_MODES = {"plain": dict(), "mass_flux": dict(mf=True), "damp0": dict(mf=True, mass=True, nord=0, damp_c=0.05),
            "damp1": dict(mf=True, mass=True, nord=1, damp_c=0.05), "damp2": dict(mf=True, mass=True, nord=2, damp_c=0.05)}
# nord = 3 is not a case: the reference's deln_flux indexes (is-1-nord : ie+1+nord) of arrays with a halo of 3 ("del-8 -->
# requires more ghosting than current", tp_core.F90:1273), i.e. it overruns its own arrays; dyn_core caps nord_v / nord_t /
# nord_w at 2 (dyn_core.F90:679).


def tp_inputs(g, q=None, seed=5, spikes=True):
    """one slab of fv_tp_2d inputs on grid g; q: a field with its halo (default: seeded, periodic halo)"""
    bd = g.bd
    rng = np.random.default_rng(seed)
    if q is None:
        q = 1.0 + rng.uniform(0, 1, bd.shape("A")) + spikes * 5.0 * (rng.uniform(0, 1, bd.shape("A")) > 0.7)
        periodic_fill(bd, q, "A")
    inp = dict(q=F(q))
    for n, a in zip(("crx", "cry", "xfx", "yfx", "ra_x", "ra_y"), _courant(bd, g, rng)):
        inp[n] = F(a)
    inp["mfx"] = F(rng.uniform(-1, 1, bd.shape("FX")) * 1e5)
    inp["mfy"] = F(rng.uniform(-1, 1, bd.shape("FY")) * 1e5)
    mass = 500.0 + 50 * rng.uniform(0, 1, bd.shape("A"))
    if g.grid_type == 4:
        periodic_fill(bd, mass, "A")
    inp["mass"] = F(mass)
    return inp


def run_fv_tp_2d(M, g, inp, hord, mode):
    md = TP_MODES[mode]
    q = inp["q"].copy(order="F")      # copy_corners writes the corner halos of q
    fx, fy = M.fv_tp_2d(g, q, inp["crx"], inp["cry"], hord, inp["xfx"], inp["yfx"], inp["ra_x"], inp["ra_y"],
                        inp["mfx"] if md.get("mf") else None, inp["mfy"] if md.get("mf") else None,
                        inp["mass"] if md.get("mass") else None, md.get("nord", -1), md.get("damp_c", 0.0))
    return dict(fx=fx, fy=fy)


def lib_fv_tp_2d(lib, g, inp, hord, mode):
    md = TP_MODES[mode]
    ctx = Context(g, 1, lib=lib)
    try:
        d = {n: ctx.from_host(F(a[:, :, None])) for n, a in inp.items()}
        dfx, dfy = ctx.zeros("FX", 1), ctx.zeros("FY", 1)
        ctx.fv_tp_2d(d["q"], d["crx"], d["cry"], hord, dfx, dfy, d["xfx"], d["yfx"], d["ra_x"], d["ra_y"],
                     d["mfx"] if md.get("mf") else None, d["mfy"] if md.get("mf") else None,
                     d["mass"] if md.get("mass") else None, md.get("nord", -1), md.get("damp_c", 0.0), nk=1)
        return dict(fx=dfx.download()[:, :, 0], fy=dfy.download()[:, :, 0])
    finally:
        ctx.close()


def run_copy_corners(M, g, q, dir_):
    q = q.copy(order="F")
    if M is O:
        gs = O.make_grid(g)
        O.lib().fvo_copy_corners.restype = None
        O.lib().fvo_copy_corners(O.C.byref(gs), O.p(q), O.C.c_int(dir_))
    else:
        M.copy_corners(g, q, dir_)
    return dict(q=q)


# ---- a2b_ord4 --------------------------------------------------------------------------------------------------------
def run_a2b_ord4(M, g, qin, replace=False):
    bd = g.bd
    qi, qo = qin.copy(order="F"), bd.zeros("A")
    if M is O:
        gs = O.make_grid(g)
        assert O.lib().fvo_a2b_ord4(O.C.byref(gs), O.p(qi), O.p(qo), O.C.c_int(int(replace))) == 0
    else:
        M.a2b_ord4(g, qi, qo, replace)
    r = (bd.is_, bd.ie + 1, bd.js, bd.je + 1)
    return dict(qout=bd.view(qi if replace else qo, "A", *r).copy())


# ---- c_sw ------------------------------------------------------------------------------------------------------------
def run_c_sw(M, g, st, npz, dt2, hydrostatic, nord=1):
    bd = g.bd
    f = {k: v.copy(order="F") for k, v in st.items() if k in ("u", "v", "w", "delp", "pt")}
    for n, kind in CSW_OUT:
        f[n] = bd.zeros(kind, npz)
    M.c_sw_3d(g, npz, f, nord=nord, dt2=dt2, hydrostatic=hydrostatic)
    rng_ = P.csw_valid_ranges(bd)
    return {n: bd.view(f[n], kind, *rng_[n]).copy() for n, kind in CSW_OUT if not (hydrostatic and n == "wc")}, f


def lib_c_sw(lib, g, st, npz, dt2, hydrostatic, nord=1):
    bd = g.bd
    ctx = Context(g, npz, lib=lib)
    try:
        d = {k: ctx.from_host(v) for k, v in st.items() if k in ("u", "v", "w", "delp", "pt")}
        for n, kind in CSW_OUT:
            d[n] = ctx.zeros(kind, npz)
        ctx.c_sw(d["delpc"], d["delp"], d["ptc"], d["pt"], d["u"], d["v"], d.get("w"), d["uc"], d["vc"], d["ua"], d["va"],
                 None if hydrostatic else d["wc"], d["ut"], d["vt"], d["divg_d"], nord, dt2, hydrostatic)
        rng_ = P.csw_valid_ranges(bd)
        return {n: bd.view(d[n].download(), kind, *rng_[n]).copy() for n, kind in CSW_OUT if not (hydrostatic and n == "wc")}
    finally:
        ctx.close()


# ---- d_sw ------------------------------------------------------------------------------------------------------------
DSW_CASES = {          # the branches tests/test_gpu_parity.py and tests/test_hostemu_parity.py parametrise check_d_sw with
    "defaults": dict(),
    "nord0": dict(lev_over=dict(nord=0)),
    "nord2_vort_dcon": dict(par_over=dict(dddmp=0.2, kgb=1e-3), lev_over=dict(nord=2, do_vort_damp=True, vtdm4=0.06, d_con=1.0, d2_bg=0.0075)),
    "nord3_diss_est": dict(lev_over=dict(nord=3, do_vort_damp=True, vtdm4=0.03, d_con=0.5),
                           flags=dict(prevent_diss_cooling=False, do_diss_est=True)),
    "nord1_dcon": dict(lev_over=dict(nord=1, d_con=1.0)),
    "use_cond_low_order": dict(use_cond=True, par_over=dict(hord_mt=6, hord_vt=6, hord_tm=5, hord_dp=-5)),
    "hord8_mt6": dict(par_over=dict(hord_dp=8, hord_tm=8, hord_vt=8, hord_mt=6)),
    "hord5": dict(par_over=dict(hord_dp=5, hord_tm=5, hord_vt=5, hord_mt=5)),
    "hord-5_mt8": dict(par_over=dict(hord_dp=-5, hord_tm=-5, hord_vt=-5, hord_mt=8)),
    "hord6_mt8": dict(par_over=dict(hord_dp=6, hord_tm=6, hord_vt=6, hord_mt=8)),
    "hord9": dict(par_over=dict(hord_mt=9)),
    "hord_lin": dict(par_over=dict(hord_dp=1, hord_tm=2, hord_vt=3, hord_mt=4, hord_tr=-6)),
    "hord_hi": dict(par_over=dict(hord_dp=11, hord_tm=12, hord_vt=13, hord_mt=7, hord_tr=9)),
    "inline_q": dict(inline_q=2),
    "lim_fac": dict(flags=dict(lim_fac=0.85), par_over=dict(hord_dp=1, hord_tm=-1, hord_vt=1, hord_mt=1, hord_tr=1)),
    # outside the library's table (hord_mt: 1 .. 11): the reference runs a hord_mt <= 0 through its 5, 6, 7 branch
    # (sw_core.F90:2337).  The pin found the oracle's cubed-sphere line taking the iord == 3 branch there; fixed in oracle/sw_core.c.
    "hord_mt_neg": dict(flags=dict(lim_fac=0.85), par_over=dict(hord_dp=-6, hord_tm=-6, hord_vt=-6, hord_mt=-6)),
}
# a tile with a cube corner runs every case, with nord = 0 on every level (dsw_inputs(nord0=True)): nord > 0 there needs
# fill_corners / great_circle_dist, which the stand-ins stop at.  nord_v / nord_w / nord_t follow as min(2, nord) = 0.
DSW_NOT_IN_LIB = ("inline_q", "hord_mt_neg")   # forms the library's d_sw does not have (tracers go through tracer_2d) or refuses


def dsw_inputs(g, st, npz, hydrostatic, case, periodic=None, c_sw_backend=None, nord0=False):
    """inputs of d_sw: c_sw (by the oracle) of the state, halo of uc, vc, divg_d (periodic grids), seeded accumulators.
    Returns (g with the case's flags, par, lev, f)."""
    bd = g.bd
    kw = DSW_CASES[case]
    for k, v in (kw.get("flags") or {}).items():
        setattr(g, k, v)
    lev_over = dict(kw.get("lev_over") or {})
    if nord0 or case == "inline_q":
        lev_over["nord"] = 0
    par = dict(DSW_PAR)
    par.update(kw.get("par_over") or {})
    use_cond = bool(kw.get("use_cond"))
    par["hydrostatic"], par["use_cond"] = int(hydrostatic), int(use_cond)
    par.update(nord=1, nord_v=1, nord_w=1, nord_t=1, d2_bg=0.0, damp_v=0.0, damp_w=0.0, damp_t=0.0, d_con=0.0)
    _, f = run_c_sw(c_sw_backend or O, g, st, npz, 0.5 * par["dt"], hydrostatic)
    periodic = (g.grid_type == 4) if periodic is None else periodic
    if periodic:
        for n, kind in (("uc", "V"), ("vc", "U"), ("divg_d", "B")):
            for k in range(npz):
                periodic_fill(bd, f[n][:, :, k], kind, fill_edge=True)
    rng = np.random.default_rng(99)
    if use_cond:
        f["q_con"] = F(0.01 * rng.uniform(0, 1, bd.shape("A", npz)))
        if periodic:
            for k in range(npz):
                periodic_fill(bd, f["q_con"][:, :, k], "A")
    for n, kind in (("mfx", "FX"), ("mfy", "FY"), ("cx", "CX"), ("cy", "CY")):
        f[n] = F(rng.uniform(-1, 1, bd.shape(kind, npz)))
    for n, kind in (("crx", "CX"), ("cry", "CY"), ("xfx", "CX"), ("yfx", "CY"), ("heat_source", "CC"), ("diss_est", "CC")):
        f[n] = bd.zeros(kind, npz)
    if kw.get("inline_q"):
        nq = kw["inline_q"]
        q = np.empty(bd.shape("A", npz) + (nq,), order="F")
        for iq in range(nq):
            q[..., iq] = f["pt"] * (0.01 + 0.002 * iq) * (1.0 + 0.1 * rng.uniform(0, 1, bd.shape("A", npz)))
            if periodic:
                for k in range(npz):
                    periodic_fill(bd, q[:, :, k, iq], "A")
        f["inline_q"] = F(q)
    f.pop("wc", None), f.pop("ut", None), f.pop("vt", None)
    lev = default_levels(npz, **lev_over)
    return g, par, lev, f


def dsw_outputs(bd, f, hydrostatic, use_cond):
    i0, i1, j0, j1 = bd.is_, bd.ie, bd.js, bd.je
    cmp = [("crx", "CX", None), ("cry", "CY", None), ("xfx", "CX", None), ("yfx", "CY", None), ("cx", "CX", None),
           ("cy", "CY", None), ("mfx", "FX", None), ("mfy", "FY", None), ("delp", "A", (i0, i1, j0, j1)),
           ("pt", "A", (i0, i1, j0, j1)), ("u", "U", (i0, i1, j0, j1 + 1)), ("v", "V", (i0, i1 + 1, j0, j1)),
           ("heat_source", "CC", None), ("diss_est", "CC", None), ("delpc", "A", (i0, i1 + 1, j0, j1 + 1))]
    if not hydrostatic:
        cmp.append(("w", "A", (i0, i1, j0, j1)))
    if use_cond:
        cmp.append(("q_con", "A", (i0, i1, j0, j1)))
    out = {n: (f[n] if r is None else bd.view(f[n], kind, *r)).copy() for n, kind, r in cmp}
    if f.get("inline_q") is not None:
        out["inline_q"] = bd.view(f["inline_q"], "A", i0, i1, j0, j1).copy()
    return out


def run_d_sw(M, g, par, lev, f, npz):
    f = {k: v.copy(order="F") for k, v in f.items()}
    M.d_sw_3d(g, npz, par, lev, f)
    return dsw_outputs(g.bd, f, bool(par["hydrostatic"]), bool(par["use_cond"]))


def lib_d_sw(lib, g, par, lev, f, npz):
    """d_sw through the C ABI (out-of-place outputs, as tests/parity_common.check_d_sw drives it).  inline_q is not a form
    of the library's d_sw (tracers go through tracer_2d), so such cases are the oracle's only."""
    assert f.get("inline_q") is None
    bd = g.bd
    hydrostatic, use_cond = bool(par["hydrostatic"]), bool(par["use_cond"])
    ctx = Context(g, npz, lib=lib)
    try:
        ctx.dsw_levels(lev)
        d = {k: ctx.from_host(v) for k, v in f.items() if k not in ("heat_source", "diss_est")}
        out = {n: ctx.zeros(kind, npz) for n, kind in (("delp_out", "A"), ("pt_out", "A"), ("u_out", "U"), ("v_out", "V"),
                                                       ("w_out", "A"), ("q_con_out", "A"), ("heat_s", "CC"), ("diss_e", "CC"),
                                                       ("delpc_o", "A"))}
        lpar = dict(par)
        ctx.d_sw(lpar, out["delpc_o"], d["delp"], d["pt"], d["u"], d["v"], d.get("w"), d["uc"], d["vc"], d["ua"], d["va"],
                 d["divg_d"], d["mfx"], d["mfy"], d["cx"], d["cy"], d["crx"], d["cry"], d["xfx"], d["yfx"], d.get("q_con"),
                 out["delp_out"], out["pt_out"], out["u_out"], out["v_out"], None if hydrostatic else out["w_out"],
                 out["q_con_out"] if use_cond else None, out["heat_s"], out["diss_e"])
        g_ = {n: d[n].download() for n in ("crx", "cry", "xfx", "yfx", "cx", "cy", "mfx", "mfy")}
        g_.update(delp=out["delp_out"].download(), pt=out["pt_out"].download(), u=out["u_out"].download(),
                  v=out["v_out"].download(), heat_source=out["heat_s"].download(), diss_est=out["diss_e"].download(),
                  delpc=out["delpc_o"].download())
        if not hydrostatic:
            g_["w"] = out["w_out"].download()
        if use_cond:
            g_["q_con"] = out["q_con_out"].download()
        return dsw_outputs(bd, g_, hydrostatic, use_cond)
    finally:
        ctx.close()


# ---- nonhydrostatic column path ------------------------------------------------------------------------------------------
def nh_inputs(g, km, seed=3):
    bd = g.bd
    s = nh_state(bd, km)
    rng = np.random.default_rng(seed)
    s["ws_a"] = F(0.1 * rng.uniform(-1, 1, bd.shape("A")))
    s["ws_cc"] = F(0.1 * rng.uniform(-1, 1, bd.shape("CC")))
    rng2 = np.random.default_rng(17)
    s["q_con"] = F(0.02 * rng2.uniform(0, 1, bd.shape("A", km)))
    s["cappa"] = F((2.0 / 7.0) * (1.0 - 0.1 * rng2.uniform(0, 1, bd.shape("A", km))))
    return s


def run_update_dz_c(M, g, s, km, ut, vt, dt=3.0):
    bd = g.bd
    gz, ws = s["zh"].copy(order="F"), bd.zeros("A")
    M.update_dz_c(g, km, dt, s["dp0"], s["zs"], ut, vt, gz, ws)
    r = (bd.is_ - 1, bd.ie + 1, bd.js - 1, bd.je + 1)
    return dict(gz=bd.view(gz, "A", *r).copy(), ws=bd.view(ws, "A", *r).copy())


def lib_update_dz_c(lib, g, s, km, ut, vt, dt=3.0):
    bd = g.bd
    ctx = Context(g, km, lib=lib)
    try:
        ctx.set_dp_ref(s["dp0"])
        d_gz, d_ws = ctx.zeros("A", km + 1), ctx.zeros("A")
        ctx.update_dz_c(dt, ctx.from_host(s["zs"]), ctx.from_host(ut), ctx.from_host(vt), ctx.from_host(s["zh"]), d_gz, d_ws)
        r = (bd.is_ - 1, bd.ie + 1, bd.js - 1, bd.je + 1)
        return dict(gz=bd.view(d_gz.download(), "A", *r).copy(), ws=bd.view(d_ws.download(), "A", *r).copy())
    finally:
        ctx.close()


def dz_d_inputs(g, km, seed=8, lev_over=None):
    bd = g.bd
    rng = np.random.default_rng(seed)
    arr = {n: bd.zeros(k, km) for n, k in (("crx", "CX"), ("xfx", "CX"), ("cry", "CY"), ("yfx", "CY"))}
    for k in range(km):
        c = _courant(bd, g, rng, cmax=0.4)
        for n, a in zip(("crx", "cry", "xfx", "yfx"), c[:4]):
            arr[n][:, :, k] = a
    lev = default_levels(km, **(lev_over or {}))
    arr["ndif"] = np.concatenate([lev["nord_v"], lev["nord_v"][-1:]]).astype(np.int32)
    arr["damp"] = np.concatenate([lev["damp_vt"], lev["damp_vt"][-1:]])
    return arr, lev


def run_update_dz_d(M, g, s, km, arr, hord, rdt=1.0 / 6.0):
    bd = g.bd
    zh, ws = s["zh"].copy(order="F"), bd.zeros("CC")
    a = {n: arr[n].copy(order="F") for n in ("crx", "cry", "xfx", "yfx")}
    M.update_dz_d(g, km, arr["ndif"].copy(), arr["damp"].copy(), hord, s["dp0"], s["zs"], zh, a["crx"], a["cry"], a["xfx"], a["yfx"],
                  ws, rdt)
    return dict(zh=bd.view(zh, "A", bd.is_, bd.ie, bd.js, bd.je).copy(), ws=ws)


def lib_update_dz_d(lib, g, s, km, arr, lev, hord, rdt=1.0 / 6.0):
    bd = g.bd
    ctx = Context(g, km, lib=lib)
    try:
        ctx.set_dp_ref(s["dp0"])
        ctx.dsw_levels(lev)
        d_out, d_ws = ctx.zeros("A", km + 1), ctx.zeros("CC")
        ctx.update_dz_d(hord, ctx.from_host(s["zs"]), ctx.from_host(s["zh"]), d_out, ctx.from_host(arr["crx"]),
                        ctx.from_host(arr["cry"]), ctx.from_host(arr["xfx"]), ctx.from_host(arr["yfx"]), d_ws, rdt)
        return dict(zh=bd.view(d_out.download(), "A", bd.is_, bd.ie, bd.js, bd.je).copy(), ws=d_ws.download())
    finally:
        ctx.close()


def run_riem_solver_c(M, g, s, km, a_imp=1.0, use_cond=False, moist_kappa=False, dt=3.0):
    bd = g.bd
    cn = nh_consts(PTOP, a_imp=a_imp)
    hs = F(s["zs"] * GRAV)
    gz, pef = s["zh"].copy(order="F"), bd.zeros("A", km + 1)
    M.riem_solver_c(g, km, dt, cn, hs, s["w"], s["pt"], s["delp"], gz, pef, s["ws_a"], s["q_con"] if use_cond else None,
                    s["cappa"] if moist_kappa else None)
    r = (bd.is_ - 1, bd.ie + 1, bd.js - 1, bd.je + 1)
    return dict(gz=bd.view(gz, "A", *r).copy(), pef=bd.view(pef, "A", *r).copy())


def lib_riem_solver_c(lib, g, s, km, a_imp=1.0, use_cond=False, moist_kappa=False, dt=3.0):
    bd = g.bd
    cn = nh_consts(PTOP, a_imp=a_imp)
    hs = F(s["zs"] * GRAV)
    ctx = Context(g, km, lib=lib)
    try:
        d_gz, d_pef = ctx.from_host(s["zh"]), ctx.zeros("A", km + 1)
        ctx.set_condensate(ctx.from_host(s["q_con"]) if use_cond else None, ctx.from_host(s["cappa"]) if moist_kappa else None)
        ctx.riem_solver_c(dt, cn, ctx.from_host(hs), ctx.from_host(s["w"]), ctx.from_host(s["pt"]), ctx.from_host(s["delp"]),
                          d_gz, d_pef, ctx.from_host(s["ws_a"]))
        r = (bd.is_ - 1, bd.ie + 1, bd.js - 1, bd.je + 1)
        return dict(gz=bd.view(d_gz.download(), "A", *r).copy(), pef=bd.view(d_pef.download(), "A", *r).copy())
    finally:
        ctx.close()


def _riem3_fields(bd, s, km):
    nx, ny = bd.nx, bd.ny
    return dict(w=s["w"].copy(order="F"), zh=s["zh"].copy(order="F"), delz=bd.zeros("CC", km), ppe=bd.zeros("A", km + 1),
                pk3=bd.full("A", 1e40, km + 1), pk=bd.zeros("CC", km + 1), pe=np.zeros((nx + 2, km + 1, ny + 2), order="F"),
                peln=np.zeros((nx, km + 1, ny), order="F"))


def _riem3_outputs(bd, o, last_call):
    r = (bd.is_, bd.ie, bd.js, bd.je)
    out = {n: bd.view(o[n], "A", *r).copy() for n in ("w", "zh", "ppe", "pk3")}
    out["delz"] = o["delz"].copy()
    if last_call:
        out.update(pk=o["pk"].copy(), peln=o["peln"].copy(), pe=o["pe"][1:-1, :, 1:-1].copy())
    return out


def run_riem_solver3(M, g, s, km, a_imp=1.0, use_logp=False, last_call=True, use_cond=False, moist_kappa=False, dt=6.0):
    bd = g.bd
    cn = nh_consts(PTOP, a_imp=a_imp)
    o = _riem3_fields(bd, s, km)
    M.riem_solver3(g, km, dt, cn, s["zs"], o["w"], o["delz"], s["pt"], s["delp"], o["zh"], o["pe"], o["ppe"], o["pk3"], o["pk"],
                   o["peln"], s["ws_cc"], use_logp, last_call, False, s["q_con"] if use_cond else None,
                   s["cappa"] if moist_kappa else None)
    return _riem3_outputs(bd, o, last_call)


def lib_riem_solver3(lib, g, s, km, a_imp=1.0, use_logp=False, last_call=True, use_cond=False, moist_kappa=False, dt=6.0):
    bd = g.bd
    cn = nh_consts(PTOP, a_imp=a_imp)
    ctx = Context(g, km, lib=lib)
    try:
        ctx.set_condensate(ctx.from_host(s["q_con"]) if use_cond else None, ctx.from_host(s["cappa"]) if moist_kappa else None)
        d = {k: ctx.from_host(v) for k, v in _riem3_fields(bd, s, km).items()}
        ctx.riem_solver3(dt, cn, ctx.from_host(s["zs"]), d["w"], d["delz"], ctx.from_host(s["pt"]), ctx.from_host(s["delp"]),
                         d["zh"], d["pe"], d["ppe"], d["pk3"], d["pk"], d["peln"], ctx.from_host(s["ws_cc"]), use_logp, last_call,
                         False)
        return _riem3_outputs(bd, {k: v.download() for k, v in d.items()}, last_call)
    finally:
        ctx.close()


# ---- remap operators and fillz -------------------------------------------------------------------------------------------
KORDS = (4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)   # what the project accepts: ppm_profile (<= 7), scalar_ / cs_profile (8..15)
REMAP_OPS = {0: "map_scalar", 1: "map1_ppm", 2: "map1_q2", 3: "mapn_tracer"}


def remap_columns(km, seed):
    """(pe1, pe2, q) of one column: a stretched source grid, a target grid with the same ends, a field with structure"""
    rng = np.random.default_rng(seed)
    d1 = 200.0 + 1800.0 * rng.uniform(0.2, 1.0, km) * np.linspace(0.3, 1.0, km)
    pe1 = 300.0 + np.concatenate([[0.0], np.cumsum(d1)])
    w = rng.uniform(0.6, 1.4, km)
    pe2 = 300.0 + np.concatenate([[0.0], np.cumsum(w / w.sum() * (pe1[-1] - 300.0))])
    pe2[-1] = pe1[-1]
    z = np.linspace(0, 1, km)
    q = 280.0 + 30.0 * z + 4.0 * np.sin(9.0 * z + seed) + 3.0 * (rng.uniform(0, 1, km) > 0.8)
    return pe1, pe2, q


def fillz_inputs(im, km, nq, seed=11):
    rng = np.random.default_rng(seed)
    q = F(rng.uniform(-0.3, 1.0, (im, km, nq)) * 1e-3)
    q[0, :, :] = np.abs(q[0, :, :])                 # one column without negatives
    q[1, 0, :] = -1e-4                              # negative top layer
    q[2, km - 1, :] = -2e-4                         # negative bottom layer
    if im > 3:
        q[3, :, :] = -np.abs(q[3, :, :])            # a column with nothing to borrow
    dp = F(500.0 + 1500.0 * rng.uniform(0, 1, (im, km)))
    return q, dp


# ---- kernels against the reference, live: the shapes where kernels go wrong ------------------------------------------------
def live_kernel_cases(small=False):
    """(name, bound key, run(M) -> outputs through a backend with oracle_lib's signatures, run(lib) -> outputs through the C ABI).
    Shapes: widths that are no multiple of the wavefront / segment size, one strip and several strips, km that is no multiple
    of the column kernels' chunk; doubly periodic tiles (the LDS-tile and the marching kernels) and a whole cube face (the pass
    / frame kernels).  small: the subset the host emulation runs in reasonable time.  Which kernel FORM serves a case is the
    library's choice at context creation (FV3_MI355X_MARCH, FV3_MI355X_FUSED, docs/SWITCHES.md): the callers run the whole
    list under KERNEL_FORMS."""
    out = []
    tp_shapes = [("dp", 40, 19), ("dp", 130, 100)] if not small else [("dp", 40, 19), ("dp", 67, 5)]
    for _, nx, ny in tp_shapes:
        g = periodic_grid(nx, ny, True)
        inp = tp_inputs(g)
        for hord in (ALL_HORD if not small else (5, -5, 6, 8, 10, 1, 3)):
            for mode in ("plain", "damp2"):
                out.append((f"fv_tp_2d dp {nx}x{ny} hord {hord} {mode}", "fv_tp_2d",
                            lambda M, g=g, i=inp, h=hord, m=mode: run_fv_tp_2d(M, g, i, h, m),
                            lambda lib, g=g, i=inp, h=hord, m=mode: lib_fv_tp_2d(lib, g, i, h, m)))
    for npx in ((13, 41) if not small else (13,)):
        g, st = tile_state("face", 2, npx=npx)
        inp = tp_inputs(g, q=st["delp"][:, :, 0])
        for hord in (ALL_HORD if not small else (5, 6, 8, 10, 2)):
            out.append((f"fv_tp_2d face C{npx - 1} hord {hord}", "fv_tp_2d", lambda M, g=g, i=inp, h=hord: run_fv_tp_2d(M, g, i, h, "mass_flux"),
                        lambda lib, g=g, i=inp, h=hord: lib_fv_tp_2d(lib, g, i, h, "mass_flux")))
    sw_shapes = [(40, 19, 3), (130, 70, 3), (61, 4, 2), (6, 5, 2)] if not small else [(40, 19, 3), (67, 5, 2)]
    for nx, ny, npz in sw_shapes:
        for hyd in (False, True):
            g = periodic_grid(nx, ny, True)
            st = smooth_state(g.bd, npz, hydrostatic=hyd)
            out.append((f"c_sw dp {nx}x{ny}x{npz} hyd={hyd}", "c_sw", lambda M, g=g, st=st, n=npz, h=hyd: run_c_sw(M, g, st, n, 3.0, h)[0],
                        lambda lib, g=g, st=st, n=npz, h=hyd: lib_c_sw(lib, g, st, n, 3.0, h)))
            for case in (("defaults", "nord2_vort_dcon", "nord3_diss_est", "use_cond_low_order", "hord5", "hord_lin", "hord_hi", "lim_fac")
                         if (nx, ny) == (40, 19) else ("defaults", "hord6_mt8")):
                g2, par, lev, f = dsw_inputs(periodic_grid(nx, ny, True), st, npz, hyd, case)
                out.append((f"d_sw dp {nx}x{ny}x{npz} hyd={hyd} {case}", "d_sw",
                            lambda M, g=g2, p_=par, l=lev, f=f, n=npz: run_d_sw(M, g, p_, l, f, n),
                            lambda lib, g=g2, p_=par, l=lev, f=f, n=npz: lib_d_sw(lib, g, p_, l, f, n)))
    for npx in ((13, 41) if not small else (13,)):
        for hyd in (False, True):
            g, st = tile_state("face", 3, hydrostatic=hyd, npx=npx)
            out.append((f"c_sw face C{npx - 1} hyd={hyd}", "c_sw", lambda M, g=g, st=st, h=hyd: run_c_sw(M, g, st, 3, 3.0, h)[0],
                        lambda lib, g=g, st=st, h=hyd: lib_c_sw(lib, g, st, 3, 3.0, h)))
            # a whole face owns four cube corners: every case with nord = 0 (the reference's stand-ins stop at nord > 0 there)
            for case in (("nord0", "hord5", "hord6_mt8", "hord8_mt6", "hord_lin", "hord_hi", "lim_fac", "use_cond_low_order", "nord2_vort_dcon")
                         if npx == 13 else ("nord0", "hord5")):
                g2, par, lev, f = dsw_inputs(tile_state("face", 3, hydrostatic=hyd, npx=npx)[0], st, 3, hyd, case, nord0=True)
                out.append((f"d_sw face C{npx - 1} hyd={hyd} {case} nord=0", "d_sw", lambda M, g=g2, p_=par, l=lev, f=f: run_d_sw(M, g, p_, l, f, 3),
                            lambda lib, g=g2, p_=par, l=lev, f=f: lib_d_sw(lib, g, p_, l, f, 3)))
    for nx, ny, km in ([(24, 13, 8), (24, 13, 79), (37, 5, 127), (24, 13, 3)] if not small else [(24, 13, 8), (19, 3, 79)]):
        g = periodic_grid(nx, ny, True)
        s = nh_inputs(g, km)
        _, f = run_c_sw(O, g, smooth_state(g.bd, km), km, 3.0, False)
        out.append((f"update_dz_c {nx}x{ny}x{km}", "update_dz_c", lambda M, g=g, s=s, k=km, f=f: run_update_dz_c(M, g, s, k, f["ut"], f["vt"]),
                    lambda lib, g=g, s=s, k=km, f=f: lib_update_dz_c(lib, g, s, k, f["ut"], f["vt"])))
        for hord, lo in ((10, dict(nord=2, do_vort_damp=True, vtdm4=0.06)), (5, dict(nord=2, do_vort_damp=True, vtdm4=0.06)), (8, None)):
            arr, lev = dz_d_inputs(g, km, lev_over=lo)       # damped levels (the transport kernel with deln_flux) and undamped ones
            out.append((f"update_dz_d {nx}x{ny}x{km} hord {hord} {'damped' if lo else 'undamped'}", "update_dz_d",
                        lambda M, g=g, s=s, k=km, a=arr, h=hord: run_update_dz_d(M, g, s, k, a, h),
                        lambda lib, g=g, s=s, k=km, a=arr, l=lev, h=hord: lib_update_dz_d(lib, g, s, k, a, l, h)))
        for uc, mk in ((False, False), (True, True)):
            kw = dict(use_cond=uc, moist_kappa=mk)
            out.append((f"riem_solver_c {nx}x{ny}x{km} {kw}", "riem_solver_c", lambda M, g=g, s=s, k=km, kw=kw: run_riem_solver_c(M, g, s, k, **kw),
                        lambda lib, g=g, s=s, k=km, kw=kw: lib_riem_solver_c(lib, g, s, k, **kw)))
            for ulp, lc in ((False, True), (True, False)):
                kw3 = dict(kw, use_logp=ulp, last_call=lc)
                out.append((f"riem_solver3 {nx}x{ny}x{km} {kw3}", "riem_solver3",
                            lambda M, g=g, s=s, k=km, kw=kw3: run_riem_solver3(M, g, s, k, **kw),
                            lambda lib, g=g, s=s, k=km, kw=kw3: lib_riem_solver3(lib, g, s, k, **kw)))
    return out


# the environment a context is created under -> the kernel forms that serve c_sw / d_sw / fv_tp_2d / update_dz_d (docs/SWITCHES.md)
KERNEL_FORMS = {"default": {}, "unfused_march": {"FV3_MI355X_FUSED": "0"}, "tile": {"FV3_MI355X_MARCH": "0"}}
_LIVE_REF = {}


def check_live(lib, ref_backend, small, cache_key):
    """every live case through `lib` against the reference's outputs (computed once a process, `cache_key`); all failures are
    collected before the assertion, so that one failing case does not hide the rest.  Returns the printed figures."""
    cases = live_kernel_cases(small=small)
    refs = _LIVE_REF.setdefault(cache_key, {})
    lines, failures = [], []
    for name, key, run, lib_run in cases:
        if name not in refs:
            refs[name] = run(ref_backend)
        try:
            w = compare(key, lib_run(lib), refs[name], extra=P.TOL, what=name)
            lines.append(f"{name}: {w:.3e}")
        except AssertionError as e:
            failures.append(f"{name}: {str(e).splitlines()[0]}")
    assert not failures, f"{len(failures)} of {len(cases)} live cases fail:\n" + "\n".join(failures)
    return lines, len(cases)
