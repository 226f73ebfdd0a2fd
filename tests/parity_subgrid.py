"""Check bodies of fv_subgrid_z -- fv3_fv_subgrid_z (fv_sg_SHiELD, model/fv_sg.F90:76-505) and fv3_update_dwinds_phys
(model/fv_grid_utils.F90:3291-3475) -- shared by tests/test_subgrid_hostemu.py (CPU) and tests/test_subgrid_gpu.py: the library
against the outputs of the reference's compiled Fortran (tests/golden/subgrid_*.npz), against the numpy restatement
tests/ref_fv_sg.py at larger shapes, and properties that need no restatement.  The inputs (tests/subgrid_inputs.py) are conditions:
every check asserts that both the mixing and the non-mixing branch run, and what else it relies on, before it compares anything."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import parity_common as P
import parity_phys as H
import ref_fv_sg as R
import subgrid_inputs as SI
from gfdl_atmos_cubed_sphere_amd.lib import Context, Fv3Error
from parity_phys import same_bits

SHAPES = ((40, 19, 12), (130, 100, 5), (21, 7, 2), (21, 7, 3))
NWATS = ((0, 1), (1, 1), (2, 2), (3, 4), (4, 4), (6, 7))
OUT = SI.SG_OUT
IN = ("delp", "pe", "peln", "pkz", "delz")
golden = functools.partial(H.golden, "subgrid_")


def params_of(c):
    """the call's parameters from a case dict (subgrid_inputs.SG_CASES) or keywords of the same names"""
    return dict(hydrostatic=c["hydrostatic"], nwat=c["nwat"], nq=c["nq"], k_bot_full=c["k_bot_full"], fv_sg_adj_weak=c.get("fv_sg_adj_weak", 0),
                ptop=c.get("ptop", 300.0), fv_sg_adj=c.get("fv_sg_adj", SI.FV_SG_ADJ), dt=c.get("dt", SI.DT))


def run_checker(bd, st, pr):
    """the numpy restatement on a copy of the state -> ({field: array with halos}, counts)"""
    o = {n: st[n].copy(order="F") for n in OUT}
    km = st["ta"].shape[2]
    cnt = R.fv_sg_shield(bd, km, pr["nq"], pr["dt"], pr["fv_sg_adj"], pr["fv_sg_adj_weak"], pr["nwat"], SI.SPECIES_OF[pr["nwat"]], st["delp"],
                         st["pe"], st["peln"], st["pkz"], o["ta"], o["qa"], o["ua"], o["va"], pr["hydrostatic"], o["w"], st["delz"],
                         o["u_dt"], o["v_dt"], pr["k_bot_full"], pr["ptop"])
    return o, cnt


def call_lib(ctx, d, pr, species=None):
    hyd = pr["hydrostatic"]
    ctx.fv_subgrid_z(hyd, pr["nq"], pr["nwat"], SI.SPECIES_OF[pr["nwat"]] if species is None else species, pr["k_bot_full"], pr["fv_sg_adj"],
                     pr["fv_sg_adj_weak"], pr["dt"], pr["ptop"], d["delp"], d["pe"] if hyd else None, d["peln"], d["pkz"], d["ta"], d["qa"],
                     d["ua"], d["va"], None if hyd else d["w"], None if hyd else d["delz"], d["u_dt"], d["v_dt"], consts=R.CONSTS)


def upload(ctx, st):
    return H.upload(ctx, st, IN + OUT)


def run_lib(lib, bd, st, pr, ctx=None, grid=None):
    """fv3_fv_subgrid_z on a copy of the state -> {field: array with halos}; the inputs must come back as they went"""
    with H.own_or_borrowed(lib, bd, st["ta"].shape[2], ctx, grid) as ctx:
        d = upload(ctx, st)
        call_lib(ctx, d, pr)
        for n in IN:
            assert same_bits(d[n].download(), st[n]), f"{n}: an input was written"
        return H.download(d, OUT)


def written_mask(bd, st, pr, name):
    """True where the header says the routine writes the field"""
    km = st["ta"].shape[2]
    kbot = R.kbot_of(km, pr["k_bot_full"], pr["fv_sg_adj_weak"])
    m = np.zeros(st[name].shape, dtype=bool)
    if name == "w" and pr["hydrostatic"]:
        return m
    v = bd.view(m, "A", bd.is_, bd.ie, bd.js, bd.je)
    if name == "qa":
        v[:, :, :kbot, :pr["nq"]] = True
    else:
        v[:, :, :kbot] = True
    return m


def assert_conditions(bd, st, ref, cnt, pr):
    """what the comparisons rely on, per sweep: pairs mixed and not mixed, pairs with ri < 0, warm-top pairs, cold pairs, mixing at
    each of the boosted levels k = 2, 3, 4 that the call reaches -- every count positive in every sweep; and, from five levels on, the
    share of u cells that change (of all levels of the array) within 0.2 .. 0.8"""
    km = st["ta"].shape[2]
    kbot = R.kbot_of(km, pr["k_bot_full"], pr["fv_sg_adj_weak"])
    need = ["mixed", "not_mixed", "ri_negative", "warm_top", "cold"] + [f"mixed_k{k}" for k in (2, 3, 4) if k <= kbot]
    for n in need:
        assert all(c > 0 for c in cnt[n]), (n, cnt[n])
    if km >= 5:
        r = (bd.is_, bd.ie, bd.js, bd.je)
        share = float((bd.view(ref["ua"], "A", *r) != bd.view(st["ua"], "A", *r)).mean())
        assert 0.2 <= share <= 0.8, share


def compare(bd, st, got, ref, pr, tol=P.TOL):
    """every written field at `tol` on the range the header gives; everything else keeps its bits"""
    worst = 0.0
    for n in OUT:
        m = written_mask(bd, st, pr, n)
        if m.any():
            worst = max(worst, P.assert_close(n, got[n][m], ref[n][m], tol))
        assert same_bits(got[n][~m], st[n][~m]), f"{n}: written outside the compute domain / levels 1..kbot / tracers 1..nq"
    return worst


def bit_identical(bd, st, got, ref, pr):
    return {n: bool(np.array_equal(got[n][written_mask(bd, st, pr, n)], ref[n][written_mask(bd, st, pr, n)])) for n in OUT}


# ---- the recorded outputs of the reference's compiled Fortran ----------------------------------------------------------------------
def golden_case(name):
    c = SI.SG_CASES[name]
    bd, st = SI.sg_case_inputs(name)
    g = golden(c["group"])
    assert str(g[f"{name}|sha"]) == SI.checksum(st), f"{name}: the inputs formed from the seed are not those the golden was recorded with"
    ref = {n: st[n].copy(order="F") for n in OUT}
    r = (bd.is_, bd.ie, bd.js, bd.je)
    for n in OUT:
        bd.view(ref[n], "A", *r)[...] = g[f"{name}|out|{n}"]
    return c, bd, st, ref


def check_checker_against_golden(name):
    """the numpy restatement = the compiled reference, bit for bit; and the recorded case meets the conditions"""
    c, bd, st, ref = golden_case(name)
    pr = params_of(c)
    got, cnt = run_checker(bd, st, pr)
    assert_conditions(bd, st, ref, cnt, pr)
    for n in OUT:
        assert same_bits(got[n], ref[n]), f"{name}: {n} of the restatement is not the reference's, max diff {np.max(np.abs(got[n] - ref[n])):.3e}"
    if c["ptop"] < 2.0:      # t_min = 160 decides something in this case: with 165 the restatement gives other bits
        other, _ = run_checker(bd, st, dict(pr, ptop=300.0))
        assert not np.array_equal(other["ta"], ref["ta"]), "t_min 160 / 165 makes no difference in the ptop = 1 Pa case"


def check_lib_against_golden(lib, name):
    """the library against the recorded outputs with nothing in between -> (worst relative difference, {field: bit-identical})"""
    c, bd, st, ref = golden_case(name)
    pr = params_of(c)
    got = run_lib(lib, bd, st, pr)
    return compare(bd, st, got, ref, pr), bit_identical(bd, st, got, ref, pr)


# ---- the restatement at larger shapes ----------------------------------------------------------------------------------------------
def check_against_checker(lib, shape, hydrostatic, nwat, nq, k_bot_full=None, weak=0, nqa=None, seed=101):
    nx, ny, km = shape
    kbf = k_bot_full if k_bot_full is not None else km
    pr = params_of(dict(hydrostatic=hydrostatic, nwat=nwat, nq=nq, k_bot_full=kbf, fv_sg_adj_weak=weak))
    bd, st = SI.columns(nx, ny, km, nqa or nq, nwat, seed + nwat + 10 * int(hydrostatic))
    st.pop("planted")
    st["u_dt"], st["v_dt"] = bd.zeros("A", km), bd.zeros("A", km)
    ref, cnt = run_checker(bd, st, pr)
    assert_conditions(bd, st, ref, cnt, pr)
    return compare(bd, st, run_lib(lib, bd, st, pr), ref, pr)


# ---- properties that need no restatement -------------------------------------------------------------------------------------------
def check_properties(lib, shape, hydrostatic, nwat=6, nq=7):
    nx, ny, km = shape
    r = (1, nx, 1, ny)
    eps = np.finfo(float).eps
    # (a) fra = 1 (dt = fv_sg_adj): the column keeps its tracer mass and its momentum, to the rounding of km exchanges per sweep
    pr = params_of(dict(hydrostatic=hydrostatic, nwat=nwat, nq=nq, k_bot_full=km, dt=600.0, fv_sg_adj=600))
    bd, st = SI.columns(nx, ny, km, nq, nwat, seed=211)
    st.pop("planted")
    st["u_dt"], st["v_dt"] = bd.zeros("A", km), bd.zeros("A", km)
    got = run_lib(lib, bd, st, pr)
    v = lambda a: bd.view(a, "A", *r)      # noqa: E731
    dp = v(st["delp"])
    assert np.any(v(got["ua"]) != v(st["ua"]))
    fields = [("ua", v(st["ua"]), v(got["ua"])), ("va", v(st["va"]), v(got["va"]))]
    fields += [(f"q{iq + 1}", v(st["qa"])[..., iq], v(got["qa"])[..., iq]) for iq in range(nq)]
    if not hydrostatic:
        fields.append(("w", v(st["w"]), v(got["w"])))
    for n, a, b in fields:
        m0, m1 = (a * dp).sum(axis=2), (b * dp).sum(axis=2)
        scale = (np.abs(a) * dp).sum(axis=2)
        assert np.all(np.abs(m1 - m0) <= 8 * 3 * km * eps * scale), (n, float(np.max(np.abs(m1 - m0) / scale)))
    # (b) u_dt = (ua_out - ua_in) / dt, with the routine's own rdt = 1 / dt, whatever fra is
    pr = params_of(dict(hydrostatic=hydrostatic, nwat=nwat, nq=nq, k_bot_full=km))
    got = run_lib(lib, bd, st, pr)
    rdt = 1.0 / pr["dt"]
    for t, a in (("u_dt", "ua"), ("v_dt", "va")):
        assert np.array_equal(v(got[t]), rdt * (v(got[a]) - v(st[a]))), t
    # (c) columns in which no pair mixes: a strongly stable, calm column (theta rising fast with height, no shear) beside ordinary ones
    calm = np.zeros((nx, ny), dtype=bool)
    calm[::3, ::2] = True
    kk = np.arange(km)[None, None, :]
    pkz = st["pkz"]
    T = v(st["ta"])
    T[calm] = ((300.0 + 40.0 * (km - 1 - kk)) * pkz * (1.0e5 ** -SI.KAPPA))[calm]
    T[calm] = np.minimum(T[calm], 300.0)      # (stays 5 K clear of t_max; theta still rises with height where the cap acts)
    for n in ("ua", "va", "w"):
        v(st[n])[calm] = 1.0
    ref, cnt = run_checker(bd, st, pr)
    got = run_lib(lib, bd, st, pr)
    still = calm & np.all(v(ref["ua"]) == v(st["ua"]), axis=2) & np.all(v(ref["qa"]) == v(st["qa"]), axis=(2, 3))
    assert still.sum() >= calm.sum() // 2 > 0, "the calm columns mix: the test shows nothing"
    for n in ("ua", "va", "qa") + (() if hydrostatic else ("w",)):
        assert same_bits(v(got[n])[still], v(st[n])[still]), f"{n}: a column without mixing came back different"
    for n in ("u_dt", "v_dt"):
        assert np.all(v(got[n])[still] == 0.0), n


# ---- the memory contract -----------------------------------------------------------------------------------------------------------
def check_contract(lib, shape=(40, 19, 12), hydrostatic=False):
    """outputs prefilled with the pattern; halos, levels below kbot, tracers beyond nq bit-unchanged (compare); and a call made after
    another kind of call in the same context gives the bits of a fresh context.  Meant to run under memory_contract.run_case."""
    import memory_contract as MC
    nx, ny, km = shape
    pr = params_of(dict(hydrostatic=hydrostatic, nwat=6, nq=6, k_bot_full=5))
    bd, st = SI.columns(nx, ny, km, 8, 6, seed=307)
    st.pop("planted")
    st["u_dt"], st["v_dt"] = MC.pattern_array(bd.shape("A", km)), MC.pattern_array(bd.shape("A", km))
    ref, cnt = run_checker(bd, st, pr)
    assert all(c > 0 for c in cnt["mixed"]) and all(c > 0 for c in cnt["not_mixed"])
    fresh = run_lib(lib, bd, st, pr)
    worst = compare(bd, st, fresh, ref, pr)
    ctx = Context(P.make_grid(bd, False), km, lib=lib)
    try:
        # another kind of call first, on other data and with another work-array size: the full depth, hydrostatic or not the other way round
        other = params_of(dict(hydrostatic=not hydrostatic, nwat=3, nq=8, k_bot_full=km))
        bd2, st2 = SI.columns(nx, ny, km, 8, 3, seed=311)
        st2.pop("planted")
        st2["u_dt"], st2["v_dt"] = bd.zeros("A", km), bd.zeros("A", km)
        call_lib(ctx, upload(ctx, st2), other)
        t = SI.tile_tendencies(nx, ny, km, seed=5)[1]
        ctx.update_dwinds_phys(pr["dt"], *(ctx.from_host(t[n]) for n in ("u_dt", "v_dt", "u", "v")))
        again = run_lib(lib, bd, st, pr, ctx=ctx)
    finally:
        ctx.close()
    H.same_as_fresh_context(OUT, fresh, again, "another call")
    return worst


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    nx, ny, km = 12, 9, 6
    bd, st = SI.columns(nx, ny, km, 7, 6, seed=401)
    st.pop("planted")
    st["u_dt"], st["v_dt"] = bd.zeros("A", km), bd.zeros("A", km)
    good = params_of(dict(hydrostatic=False, nwat=6, nq=7, k_bot_full=4))
    ctx = Context(P.make_grid(bd, False), km, lib=lib)
    try:
        d = upload(ctx, st)
        refused = H.refusals(functools.partial(call_lib, ctx), d, good)

        for n in ("delp", "peln", "pkz", "ta", "qa", "ua", "va", "u_dt", "v_dt"):
            refused("null", drop=(n,))
        refused("w and delz", drop=("w",))          # (call_lib hands w, delz only when nonhydrostatic)
        refused("fv_sg_adj", dict(good, fv_sg_adj=0))
        refused("fv_sg_adj", dict(good, fv_sg_adj=-600))
        refused("k_bot_full", dict(good, k_bot_full=0))
        refused("k_bot_full", dict(good, k_bot_full=km + 1))
        six = SI.SPECIES_OF[6]
        refused("graupel", species=dict(six, graupel=0))
        refused("graupel", species=dict(six, graupel=8))
        refused("sphum", dict(good, nwat=1), species={})
        refused("liq_wat", dict(good, nwat=2), species=dict(sphum=1))
        refused("ice_wat", dict(good, nwat=3), species=dict(sphum=1, liq_wat=2))
        refused("rainwat", dict(good, nwat=4), species=dict(sphum=1, liq_wat=2))
        refused("snowwat", dict(good, nwat=5), species=dict(sphum=1, liq_wat=2, rainwat=3, ice_wat=4))
        refused("nwat", dict(good, nwat=-1), species=six)
        H.assert_nothing_written(d, st, IN + OUT)
        # what is NOT refused, and why: k_bot_full > npz with fv_sg_adj_weak > 0 (kbot = npz, fv_sg.F90:123-128); nwat = 5 and 7 with all
        # five condensates (the reference's `else` branches, :242-248, :302-307, :358-361, :436-442: the arithmetic of nwat = 6)
        call_lib(ctx, upload(ctx, st), dict(good, k_bot_full=km + 1, fv_sg_adj_weak=900))
        outs = []
        for nwat in (6, 5, 7):
            dd = upload(ctx, st)
            call_lib(ctx, dd, dict(good, nwat=nwat), species=six)
            outs.append({n: dd[n].download() for n in OUT})
        for o in outs[1:]:
            for n in OUT:
                assert np.array_equal(o[n], outs[0][n]), n
        bdh, sth = SI.columns(nx, ny, km, 1, 0, seed=402)
        sth["u_dt"], sth["v_dt"] = bd.zeros("A", km), bd.zeros("A", km)
        dh = upload(ctx, {k: v for k, v in sth.items() if k != "planted"})
        refused("pe", call=lambda: call_lib(ctx, dict(dh, pe=None), params_of(dict(hydrostatic=True, nwat=0, nq=1, k_bot_full=4))))
        # update_dwinds_phys: null fields
        t = SI.tile_tendencies(nx, ny, km, seed=5)[1]
        dt_ = {n: ctx.from_host(t[n]) for n in t}
        for n in t:
            refused("null", call=lambda: ctx.update_dwinds_phys(1.0, *(None if m == n else dt_[m] for m in ("u_dt", "v_dt", "u", "v"))))
    finally:
        ctx.close()


# ---- update_dwinds_phys on the doubly periodic tile --------------------------------------------------------------------------------
def run_dwinds_lib(lib, bd, t, dt, npz, grid=None, ctx=None):
    with H.own_or_borrowed(lib, bd, npz, ctx, grid) as ctx:
        d = H.upload(ctx, t, ("u_dt", "v_dt", "u", "v"))
        ctx.update_dwinds_phys(dt, d["u_dt"], d["v_dt"], d["u"], d["v"])
        for n in ("u_dt", "v_dt"):
            assert same_bits(d[n].download(), t[n]), n
        return d["u"].download(), d["v"].download()


def compare_dwinds(bd, t, u, v, ru, rv):
    """u on (is:ie, js:je+1), v on (is:ie+1, js:je) at P.TOL; the rest of both arrays keeps its bits"""
    worst = 0.0
    for n, got, ref, kind, rg in (("u", u, ru, "U", (bd.is_, bd.ie, bd.js, bd.je + 1)), ("v", v, rv, "V", (bd.is_, bd.ie + 1, bd.js, bd.je))):
        m = np.zeros(got.shape, dtype=bool)
        bd.view(m, kind, *rg)[...] = True
        assert np.any(ref[m] != t[n][m])
        worst = max(worst, P.assert_close(n, got[m], ref[m], P.TOL))
        assert same_bits(got[~m], t[n][~m]), f"{n}: written outside its range"
    return worst


@functools.lru_cache(maxsize=None)
def dwinds_golden_case(name):
    """(bd, npx, npy, grid_type, inputs, geometry, u and v of the reference's compiled update_dwinds_phys)"""
    bd, npx, npy, t, geom = SI.dw_case_inputs(name)
    g = golden("dwinds")
    sha = SI.checksum(dict(t, **{"geom_" + k: v for k, v in (geom or {}).items()}))
    assert str(g[f"{name}|sha"]) == sha, f"{name}: the inputs formed from the seed are not those the golden was recorded with"
    return bd, npx, npy, SI.DW_CASES[name]["grid_type"], t, geom, np.asfortranarray(g[f"{name}|out|u"]), np.asfortranarray(g[f"{name}|out|v"])


def check_dwinds_checker_against_golden(name):
    """the numpy restatement = the compiled reference, bit for bit, over the whole arrays"""
    bd, npx, npy, gt, t, geom, ru, rv = dwinds_golden_case(name)
    u, v = t["u"].copy(order="F"), t["v"].copy(order="F")
    R.update_dwinds_phys(bd, npx, npy, gt, SI.DW_DT, t["u_dt"], t["v_dt"], u, v, geom)
    assert np.any(ru != t["u"]) and np.any(rv != t["v"])
    for n, a, b in (("u", u, ru), ("v", v, rv)):
        assert same_bits(a, b), f"{name}: {n} of the restatement is not the reference's, max diff {np.max(np.abs(a - b)):.3e}"


def check_dwinds_lib_against_golden(lib, name):
    """the library against the recorded outputs with nothing in between -> (worst relative difference, bit-identical)"""
    bd, npx, npy, gt, t, geom, ru, rv = dwinds_golden_case(name)
    npz = t["u"].shape[2]
    if gt == 4:
        ctx = Context(P.make_grid(bd, False), npz, lib=lib)
    else:
        import cubed_common as CC
        ctx = Context(CC.sphere(npx)[1][SI.DW_CASES[name]["face"]], npz, lib=lib)
    try:
        if geom is not None:
            ctx.upload_dwinds(geom)
        u, v = run_dwinds_lib(lib, bd, t, SI.DW_DT, npz, ctx=ctx)
    finally:
        ctx.close()
    return compare_dwinds(bd, t, u, v, ru, rv), bool(np.array_equal(u, ru) and np.array_equal(v, rv))


def check_dwinds_tile(lib, shape=(40, 19, 3), dt=225.0):
    nx, ny, npz = shape
    bd, t = SI.tile_tendencies(nx, ny, npz, seed=17)
    ru, rv = t["u"].copy(order="F"), t["v"].copy(order="F")
    R.update_dwinds_phys(bd, nx + 1, ny + 1, 4, dt, t["u_dt"], t["v_dt"], ru, rv)
    u, v = run_dwinds_lib(lib, bd, t, dt, npz)
    return compare_dwinds(bd, t, u, v, ru, rv)


# ---- update_dwinds_phys on the sphere ----------------------------------------------------------------------------------------------
oracle_dwinds_geom = SI.oracle_dwinds_geom


def sphere_tendencies(cs, bd, npz, seed):
    """u_dt, v_dt on the six faces after a real exchange as two scalars; u, v"""
    import cubed_common as CC
    rng = np.random.default_rng(seed)
    st = []
    for t in range(6):
        f = lambda kind, s: np.asfortranarray(s * rng.standard_normal(bd.shape(kind, npz)))      # noqa: E731
        st.append(dict(u_dt=f("A", 1.0e-3), v_dt=f("A", 1.0e-3), u=f("U", 10.0), v=f("V", 10.0)))
    CC.exchange(cs, st, ("u_dt", "v_dt"), "A")
    return st


def check_dwinds_sphere(lib, npx=13, npz=2, dt=225.0):
    """all six C12 faces with the oracle's geometry: the library against the restatement"""
    import cubed_common as CC
    cs, gs = CC.sphere(npx)
    bd = gs[0].bd
    st = sphere_tendencies(cs, bd, npz, seed=23)
    worst = 0.0
    for t in range(6):
        geom = oracle_dwinds_geom(cs, t)
        ru, rv = st[t]["u"].copy(order="F"), st[t]["v"].copy(order="F")
        R.update_dwinds_phys(bd, npx, npx, 0, dt, st[t]["u_dt"], st[t]["v_dt"], ru, rv, geom)
        ctx = Context(gs[t], npz, lib=lib)
        try:
            d = {n: ctx.from_host(st[t][n]) for n in ("u_dt", "v_dt", "u", "v")}
            try:                                              # refused on the sphere without the upload
                ctx.lib.check(ctx.lib.dll.fv3_update_dwinds_phys(ctx.h, C.c_double(dt), d["u_dt"].p, d["v_dt"].p, d["u"].p, d["v"].p),
                              "fv3_update_dwinds_phys")
            except Fv3Error as e:
                assert "fv3_grid_upload_dwinds" in str(e)
            else:
                raise AssertionError("fv3_update_dwinds_phys ran on a cubed-sphere face without its geometry")
            assert np.array_equal(d["u"].download(), st[t]["u"])
            ctx.upload_dwinds(geom)
            u, v = run_dwinds_lib(lib, bd, st[t], dt, npz, ctx=ctx)
        finally:
            ctx.close()
        worst = max(worst, compare_dwinds(bd, st[t], u, v, ru, rv))
    return worst


def solid_body_error(npx):
    """the tendency of a solid-body rotation, given analytically in (east, north) components at the cell centres, through the
    restatement with the PRODUCT's geometry (cubed_sphere.py) and dt = 1 on zero winds: the D-grid increments against that wind's
    analytic components along the cell edges at their mid-points.  -> the largest error over the six faces / the wind's strength"""
    from gfdl_atmos_cubed_sphere_amd.cubed_sphere import CubedSphere, _mid, _unit
    cs = CubedSphere(npx)
    axis = _unit(np.array([0.3, -0.5, 0.8]))
    wind = lambda p: 30.0 * np.cross(axis, p)      # noqa: E731
    worst = 0.0
    for t in range(6):
        gs = cs.gridstruct(t)
        bd, m = gs.bd, gs.m
        a3 = cs.grids[t]["agrid3"]
        w = wind(a3)
        ud = np.asfortranarray(np.sum(w * m["vlon"], -1)[:, :, None])
        vd = np.asfortranarray(np.sum(w * m["vlat"], -1)[:, :, None])
        u, v = bd.zeros("U", 1), bd.zeros("V", 1)
        R.update_dwinds_phys(bd, npx, npx, 0, 1.0, ud, vd, u, v, m)
        o, N = bd.ng, npx - 1
        c0 = cs.grids[t]["grid3"][o:o + N + 1, o:o + N + 1]
        ue = np.sum(wind(_mid(c0[:-1, :], c0[1:, :])) * m["es1"], -1)
        ve = np.sum(wind(_mid(c0[:, :-1], c0[:, 1:])) * m["ew2"], -1)
        worst = max(worst, float(np.max(np.abs(bd.view(u, "U", 1, N, 1, N + 1)[:, :, 0] - ue))), float(np.max(np.abs(bd.view(v, "V", 1, N + 1, 1, N)[:, :, 0] - ve))))
    return worst / 30.0


def check_geometry_against_oracle(npx=13, tol=1.0e-11):
    """vlon, vlat, es1, ew2, edge_vect_* of cubed_sphere.py against oracle/fv_grid.c, member by member, every face"""
    import grid_oracle as GO
    from gfdl_atmos_cubed_sphere_amd.cubed_sphere import CubedSphere
    cs, ref = CubedSphere(npx), GO.ref_sphere(npx)
    o, N = ref.ng, ref.N
    worst = {}
    for t in range(6):
        m, want = cs.gridstruct(t).m, oracle_dwinds_geom(ref, t)
        for n in want:
            a, b = np.asarray(m[n]), np.asarray(want[n])
            assert a.shape == b.shape, (n, a.shape, b.shape)
            if n in ("vlon", "vlat"):                         # the corner halo cells do not exist
                a, b = a[o:o + N, o:o + N], b[o:o + N, o:o + N]
            if n.startswith("edge_vect"):                     # set on 0 .. npx
                a, b = a[o - 1:o + npx], b[o - 1:o + npx]
            worst[n] = max(worst.get(n, 0.0), float(np.max(np.abs(a - b))))
    bad = {k: v for k, v in worst.items() if v > tol}
    assert not bad, bad
    return worst


# ---- six faces as one group ------------------------------------------------------------------------------------------------------
def check_six_faces(lib, npx=13, npz=6, hydrostatic=False):
    """the six faces as one fv3_group: the bits of face-by-face runs, and ONE merged launch for the column kernel"""
    import cubed_common as CC
    cs, gs = CC.sphere(npx)
    n = npx - 1
    pr = params_of(dict(hydrostatic=hydrostatic, nwat=6, nq=7, k_bot_full=4))
    sts = []
    for t in range(6):
        bd, st = SI.columns(n, n, npz, 7, 6, seed=500 + t)
        st.pop("planted")
        st["u_dt"], st["v_dt"] = bd.zeros("A", npz), bd.zeros("A", npz)
        sts.append(st)
    bd = gs[0].bd
    alone = [run_lib(lib, bd, st, pr, grid=gs[t]) for t, st in enumerate(sts)]
    for t, st in enumerate(sts):
        ref, cnt = run_checker(bd, st, pr)
        assert cnt["mixed"][0] > 0 and cnt["not_mixed"][0] > 0
        compare(bd, st, alone[t], ref, pr)
    alone = [dict({n: st[n] for n in IN}, **a) for st, a in zip(sts, alone)]      # the inputs come back as they went
    H.six_faces(lib, gs, npz, sts, IN + OUT, lambda mctx, d: call_lib(mctx, d, pr), alone, label="fv_subgrid_z")


# ---- the Python host: FvDynamics.atmosphere_step ---------------------------------------------------------------------------------
HOST_FIELDS = ("u", "v", "w", "delp", "pt", "ua", "va", "q", "delz")
SG_OPTS = dict(fv_sg_adj=600, fv_sg_adj_weak=0, sg_nq=6)


def run_host(lib, where, sg_opts, use_atmosphere_step=True):
    """parity_negadj.run_tile / run_sphere (24 x 16 x 10 on the doubly periodic tile, C12 L8 from the Jablonowski-Williamson state, moist,
    nq = 7) with the FvDynamics they build taking sg_opts and n_sponge = npz (the full depth), and atmosphere_step in the place of
    step_from_temperature -> their outputs + pe, peln, pkz, bdt"""
    import dataclasses

    import gfdl_atmos_cubed_sphere_amd.fv_dynamics as M
    import parity_negadj as NA
    orig, kept = M.FvDynamics, {}

    class SgFvDynamics(orig):
        def __init__(self, *a, **kw):
            super().__init__(*a, **dict(kw, **sg_opts))
            self.fl = dataclasses.replace(self.fl, n_sponge=self.ctx.npz)      # (k_bot_full of fv_subgrid_z; dyn_core keeps its own flags)
            self._inside = False
            if where == "sphere":      # the tests' gridstructs are the oracle's: what update_dwinds_phys reads comes from there as well
                import cubed_common as CC
                cs, _ = CC.sphere(self.ctx.grid.npx)
                for t, c in enumerate(self.ctx.ctxs):
                    c.upload_dwinds(oracle_dwinds_geom(cs, t))

        def _roughen(self):
            """the runs' states are smooth and stably stratified: nothing would mix.  2 % noise on T (halos consistent), the same in
            every run, leaves layer pairs on either side of the Richardson-number test after the step"""
            from gfdl_atmos_cubed_sphere_amd.layout import periodic_fill
            d, bd = self.dc.d, self.ctx.bd
            pt = d["pt"].download()
            lst = pt if isinstance(pt, list) else [pt]
            for t, a in enumerate(lst):
                rng = np.random.default_rng(700 + t)
                bd.view(a, "A", bd.is_, bd.ie, bd.js, bd.je)[...] *= 1.0 + 0.02 * rng.standard_normal((bd.nx, bd.ny, a.shape[2]))
            if where == "tile":
                for k in range(lst[0].shape[2]):
                    periodic_fill(bd, lst[0][:, :, k], "A")
            else:
                import cubed_common as CC
                CC.exchange(CC.sphere(self.ctx.grid.npx)[0], [dict(pt=a) for a in lst], ("pt",), "A")
            d["pt"].upload(pt)

        def step_from_temperature(self, bdt):
            if not self._inside:
                self._roughen()
            if self._inside or not use_atmosphere_step:
                super().step_from_temperature(bdt)
            else:
                self._inside = True
                self.atmosphere_step(bdt)
                self._inside = False
            kept.update({n: self.dc.d[n].download() for n in ("pe", "peln", "pkz")}, bdt=bdt, consts=self.neg_adj_consts, ptop=self.fl.ptop)

    M.FvDynamics = SgFvDynamics
    try:
        out = (NA.run_tile if where == "tile" else NA.run_sphere)(lib)
    finally:
        M.FvDynamics = orig
    out.update(kept)
    return out


def check_atmosphere_step(lib, where):
    """atmosphere_step = step_from_temperature, then the restatement's column routine, a real exchange of u_dt, v_dt and the
    restatement's wind update, at P.TOL; with fv_sg_adj = 0 it is step_from_temperature bit for bit"""
    import parity_negadj as NA
    import parity_remap as PR
    from gfdl_atmos_cubed_sphere_amd.layout import periodic_fill
    base = run_host(lib, where, dict(fv_sg_adj=0), use_atmosphere_step=False)
    off = run_host(lib, where, dict(fv_sg_adj=0))
    NA.assert_same_fields(base, off, HOST_FIELDS, "atmosphere_step with fv_sg_adj = 0")
    got = run_host(lib, where, SG_OPTS)
    bd = base["bd"]
    faces = NA._faces
    nf = len(faces(base["pt"]))
    npz = faces(base["pt"])[0].shape[2]
    sp = {n: PR.MOIST6[n] for n in SI.SPECIES if n != "sphum"}
    sp["sphum"] = 1
    ref, total = [], {n: 0 for n in R.COUNTS}
    for t in range(nf):
        f = {n: faces(base[n])[t].copy(order="F") for n in HOST_FIELDS}
        f["u_dt"], f["v_dt"] = bd.zeros("A", npz), bd.zeros("A", npz)
        cnt = R.fv_sg_shield(bd, npz, SG_OPTS["sg_nq"], base["bdt"], SG_OPTS["fv_sg_adj"], SG_OPTS["fv_sg_adj_weak"], PR.MOIST6["nwat"], sp, f["delp"],
                             faces(base["pe"])[t], faces(base["peln"])[t], faces(base["pkz"])[t], f["pt"], f["q"], f["ua"], f["va"], False, f["w"],
                             f["delz"], f["u_dt"], f["v_dt"], npz, base["ptop"], consts=base["consts"])
        for n in cnt:
            total[n] += sum(cnt[n])
        ref.append(f)
    print(where, total)
    assert total["mixed"] > 0 and total["not_mixed"] > 0, total
    if where == "tile":
        for n in ("u_dt", "v_dt"):
            for k in range(npz):
                periodic_fill(bd, ref[0][n][:, :, k], "A")
        geoms = [None]
    else:
        import cubed_common as CC
        cs, _ = CC.sphere(base["gs"][0].npx)
        CC.exchange(cs, ref, ("u_dt", "v_dt"), "A")
        geoms = [oracle_dwinds_geom(cs, t) for t in range(6)]
    worst, moved = 0.0, False
    r = (bd.is_, bd.ie, bd.js, bd.je)
    for t in range(nf):
        g = base["g"] if where == "tile" else base["gs"][t]
        R.update_dwinds_phys(bd, g.npx, g.npy, g.grid_type, base["bdt"], ref[t]["u_dt"], ref[t]["v_dt"], ref[t]["u"], ref[t]["v"], geoms[t])
        for n, kind, rg in (("u", "U", (bd.is_, bd.ie, bd.js, bd.je + 1)), ("v", "V", (bd.is_, bd.ie + 1, bd.js, bd.je)), ("pt", "A", r),
                            ("ua", "A", r), ("va", "A", r), ("w", "A", r), ("q", "A", r)):
            a, b = bd.view(faces(got[n])[t], kind, *rg), bd.view(ref[t][n], kind, *rg)
            worst = max(worst, P.assert_close(f"face {t + 1} {n}", a, b, P.TOL))
        moved = moved or bool(np.any(bd.view(faces(got["u"])[t], "U", *r) != bd.view(faces(base["u"])[t], "U", *r)))
        assert np.array_equal(faces(got["q"])[t][..., 6], faces(base["q"])[t][..., 6]), "a tracer beyond sg_nq moved"
    assert moved, "fv_subgrid_z moved no wind"
    NA.assert_same_fields(base, got, ["delp", "delz"], "fv_subgrid_z")
    return worst

