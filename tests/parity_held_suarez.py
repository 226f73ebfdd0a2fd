"""Check bodies of the Held-Suarez forcing -- fv3_held_suarez_tend, fv3_age_of_air, fv3_grid_upload_lat (driver/solo/hswf.F90) and
FvDynamics.held_suarez -- shared by tests/test_held_suarez_hostemu.py (CPU) and tests/test_held_suarez_gpu.py, and by the contract
tests of both: the library against the outputs of the reference's compiled Fortran (tests/golden/held_suarez_*.npz), against the numpy
restatement tests/ref_held_suarez.py at larger shapes, and properties that need no restatement.

Bounds.  u_dt, v_dt have no transcendental on their path (peln is an input): bit-identical with the compiled reference and with the
restatement, everywhere.  t_dt goes through include/fv3_math.h where the reference calls its libm, per branch set; measured with
`python tests/golden/make_held_suarez_golden.py --measure` (the library of the CPU harness against the compiled reference, worst of the
recorded cases, relative RMS / max norm): see MEASURED below.  Each bound is ten times the measured relative RMS; a set measured
bit-identical is asserted bit-identical."""
from __future__ import annotations

import functools

import numpy as np

import held_suarez_inputs as HI
import parity_common as P
import parity_phys as H
import ref_held_suarez as R
from gfdl_atmos_cubed_sphere_amd.lib import Context
from parity_phys import compute, same_bits  # noqa: F401

SHAPES = ((21, 7, 1), (21, 7, 2), (40, 19, 12), (130, 100, 32))
IDS = ["21x7x1", "21x7x2", "40x19x12", "130x100x32"]
DEVICE = HI.DEVICE
# branch set -> (relative RMS, max norm) of t_dt, library (CPU harness) against the compiled reference, worst recorded case
MEASURED = {"standard": (2.095e-17, 8.561e-17), "zurita": (4.126e-16, 1.338e-15), "strat_meso": (9.463e-17, 2.371e-16)}
BOUND = {n: 10.0 * v[0] for n, v in MEASURED.items()}
assert max(BOUND.values()) <= 1.0e-12


golden = functools.partial(H.golden, "held_suarez_")


def params_of(c):
    return dict(pdt=c["pdt"], strat=c["strat"], zurita=c["zurita"], rd_zur=c["rd_zur"], radius=c.get("radius", HI.RADIUS), pi=HI.PI)


def set_params(name, pdt=225.0):
    s, z = HI.SETS[name]
    return dict(pdt=pdt, strat=s, zurita=z, rd_zur=1.0 / 25.0, radius=HI.RADIUS, pi=HI.PI)


def call_lib(ctx, d, pr, fresh=False):
    ctx.held_suarez_tend(pr["pdt"], d["delp"], d["peln"], d["pe"], d["pkz"], d["pt"], d["ua"], d["va"], d["u_dt"], d["v_dt"], d["t_dt"],
                         strat=pr["strat"], zurita=pr["zurita"], rd_zur=pr["rd_zur"], fresh=fresh, radius=pr["radius"], pi=pr["pi"])


def upload(ctx, st):
    return H.upload(ctx, st, DEVICE)


def download(d):
    return H.download(d, DEVICE)


def run_lib(lib, bd, st, pr, fresh=False, ctx=None):
    """fv3_held_suarez_tend on a copy of the state -> {field: whole array}"""
    with H.own_or_borrowed(lib, bd, st["pt"].shape[2], ctx) as ctx:
        ctx.upload_lat(st["lat"])
        d = upload(ctx, st)
        call_lib(ctx, d, pr, fresh)
        return download(d)


def run_checker(bd, st, pr, teq_out=None):
    o = {n: st[n].copy(order="F") for n in st}
    cnt = R.held_suarez_tend(bd, st["pt"].shape[2], pr, o, teq_out=teq_out)
    return o, cnt


def branch_masks(bd, km, pr, st):
    """{branch set: True on the cells of t_dt (is:ie, js:je, km) its bound covers}"""
    pl = compute(bd, st["delp"]) / np.transpose(st["peln"][:, 1:, :] - st["peln"][:, :-1, :], (0, 2, 1))
    upper = (pl <= 100.0e2) if pr["strat"] else np.zeros(pl.shape, dtype=bool)
    return {"strat_meso": upper, ("zurita" if pr["zurita"] else "standard"): ~upper}


def compare(bd, st, got, ref, pr):
    """u_dt, v_dt bit for bit (whole arrays: the halo keeps its bits), t_dt per branch set at its bound, every input unchanged
    -> {branch set: relative RMS}"""
    km = st["pt"].shape[2]
    for n in HI.IN:
        assert same_bits(got[n], st[n]), f"{n}: an input was written"
    for n in ("u_dt", "v_dt"):
        assert same_bits(got[n], ref[n]), \
            f"{n}: not bit-identical, max diff {np.max(np.abs(got[n] - ref[n])):.3e}"
    out = {}
    for bs, m in branch_masks(bd, km, pr, st).items():
        if not m.any():
            continue
        out[bs] = H.assert_bounded(f"t_dt ({bs})", got["t_dt"][m], ref["t_dt"][m], BOUND[bs])      # per branch set: each has its own bound
    return out


# ---- the recorded outputs of the reference's compiled Fortran ----------------------------------------------------------------------
def golden_case(name):
    """-> (case, bd, inputs, the reference's outputs as whole arrays)"""
    c = HI.CASES[name]
    bd, st = HI.case_inputs(name)
    g = golden(c["group"])
    assert str(g[f"{name}|sha"]) == HI.checksum(st), f"{name}: the inputs formed from the seed are not those the golden was recorded with"
    ref = {n: st[n].copy(order="F") for n in DEVICE}
    ref["t_dt"][...] = g[f"{name}|out|t_dt"]
    for n in ("u_dt", "v_dt"):
        compute(bd, ref[n])[...] = g[f"{name}|out|{n}"]
    return c, bd, st, ref


def check_checker_against_golden(name):
    c, bd, st, ref = golden_case(name)
    pr = params_of(c)
    got, cnt = run_checker(bd, st, pr)
    assert cnt["friction"] > 0 and cnt["no_friction"] > 0, cnt
    if c["strat"] and c["km"] >= 12:
        assert cnt["meso"] > 0 and cnt["strat"] > 0 and cnt["tropo"] > 0, cnt
    for n in ("u_dt", "v_dt"):
        assert same_bits(got[n], ref[n]), f"{name}: {n} of the restatement is not the reference's"
    for bs, m in branch_masks(bd, c["km"], pr, st).items():
        if m.any():
            P.assert_close(f"{name} t_dt ({bs})", got["t_dt"][m], ref["t_dt"][m], max(BOUND[bs], 10.0 * np.finfo(float).eps))
    return cnt


def check_lib_against_golden(lib, name):
    """the library against the recorded outputs with nothing in between -> {branch set: relative RMS}"""
    c, bd, st, ref = golden_case(name)
    pr = params_of(c)
    got = run_lib(lib, bd, st, pr)
    for bs, m in branch_masks(bd, c["km"], pr, st).items():
        if m.any():
            a, b = got["t_dt"][m], ref["t_dt"][m]
            print(name, bs, "rel-rms", float(P.rel_rms(a, b)), "max norm", float(np.max(np.abs(a - b)) / np.max(np.abs(b))))
    out = compare(bd, st, got, ref, pr)
    if c["zero"]:      # the pair of fresh: the same outputs without reading the three
        import memory_contract as MC
        st2 = dict(st, **{n: MC.pattern_array(st[n].shape) for n in HI.OUT})
        got2 = run_lib(lib, bd, st2, pr, fresh=True)
        assert same_bits(got2["t_dt"], got["t_dt"]), "t_dt with fresh"
        for n in ("u_dt", "v_dt"):
            assert same_bits(compute(bd, got2[n]), compute(bd, got[n])), f"{n} with fresh"
    return out


# ---- the restatement at larger shapes ----------------------------------------------------------------------------------------------
def generic_case(shape, set_name, seed=1701, zero=False, pdt=225.0):
    nx, ny, km = shape
    bd, st = HI.state(nx, ny, km, seed + 13 * list(HI.SETS).index(set_name) + km, zero_tendencies=zero)
    return set_params(set_name, pdt), bd, st


def assert_conditions(pr, cnt, km):
    assert cnt["friction"] > 0 and cnt["no_friction"] > 0, cnt
    if pr["strat"] and km >= 12:
        assert cnt["meso"] > 0 and cnt["strat"] > 0 and cnt["tropo"] > 0, cnt
    if km >= 12:
        assert cnt["teq_t0"] > 0 and cnt["teq_free"] > 0, cnt


def check_against_checker(lib, shape, set_name):
    pr, bd, st = generic_case(shape, set_name)
    ref, cnt = run_checker(bd, st, pr)
    assert_conditions(pr, cnt, shape[2])
    return compare(bd, st, run_lib(lib, bd, st, pr), ref, pr)


# ---- fresh -------------------------------------------------------------------------------------------------------------------------
def check_fresh(lib, shape, set_name):
    """fresh is bit-identical, the sign of zero included, with zero-then-call, and writes every cell: with the three outputs
    prefilled with the contract pattern nothing of it survives on the compute domain, and the halo of u_dt, v_dt keeps it"""
    import memory_contract as MC
    pr, bd, st = generic_case(shape, set_name, seed=1801, zero=True)
    zeroed = run_lib(lib, bd, st, pr)
    pat = {n: MC.pattern_array(st[n].shape) for n in HI.OUT}
    got = run_lib(lib, bd, dict(st, **pat), pr, fresh=True)
    assert same_bits(got["t_dt"], zeroed["t_dt"]), "t_dt: fresh differs from zero-then-call"
    assert np.any(np.signbit(zeroed["t_dt"])) and np.any(zeroed["t_dt"] != 0.0)
    for n in ("u_dt", "v_dt"):
        a, b = compute(bd, got[n]), compute(bd, zeroed[n])
        assert same_bits(a, b), f"{n}: fresh differs from zero-then-call"
        assert np.any(b != 0.0) and np.any(b == 0.0), f"{n}: the case has no cell with / without friction"
        halo = H.halo_mask(bd, got[n].shape)
        assert same_bits(got[n][halo], pat[n][halo]), f"{n}: fresh wrote the halo"
    for n in HI.OUT:
        a = got[n] if n == "t_dt" else compute(bd, got[n])
        assert np.all(np.abs(a) < 1.0e29), f"{n}: the pattern survives on the compute domain"


# ---- physical checks ---------------------------------------------------------------------------------------------------------------
def check_equilibrium(lib, shape, set_name):
    """pt = the restatement's teq, winds and incoming tendencies zero.  u_dt, v_dt come back exactly zero everywhere.  t_dt comes
    back exactly zero wherever the restatement's teq IS the library's to the bit: the troposphere cells on the t0 arm of max(t0, .),
    where both hold 200 exactly.  Elsewhere a log or an exp stands between the inputs and teq, the library's is include/fv3_math.h
    and the restatement's is numpy's, and the two teq differ in their last bits, so (teq - pt) is a few ulp of teq and not zero --
    a property of the check, which takes teq from the restatement, not of the library.  The bound there, from the formats: log and
    exp of either side within 1 ulp; standard form, teq = (tey - tez (log pkz + algpk)) pkz with |log pkz| < 4 and tez pkz < 35 K:
    35 K x 2 ulp(4) = 6e-14 K = 1.4 eps x 200 K, and four roundings of teq, 2 eps: under 4 eps teq; zurita form, exp(akap log sigl)
    with |log sigl| < 12: the argument is off by akap x 2 ulp(12) = 4.6 eps, exp adds 2 eps and three roundings 1.5: under 9 eps
    teq; the stratosphere and mesosphere add per level 2.25 x 7 x 2 ulp(log(pl1 / pl)) and two roundings, under 0.3 eps teq each,
    32 levels: under 10 eps teq: 19 eps teq in all, taken as 32 eps.  t_dt is that times rk / (1 + rk) rdt with rk <= rks (rka,
    rks and the stratosphere's pdt / (relx sday) <= rms < rks).  The mesosphere's implicit form ((pt + rms teq) rmr - pt) rdt is
    at pt = teq itself (teq (1 + rms)) / (1 + rms) - teq in floating point, not zero in the reference either: four roundings,
    2 eps teq rdt more.  teq of a level depends on the levels below, not on pt, so one pass of the restatement gives it."""
    pr, bd, st = generic_case(shape, set_name, seed=1901, zero=True)
    km = shape[2]
    teq = np.zeros((bd.nx, bd.ny, km))
    run_checker(bd, st, pr, teq_out=teq)
    compute(bd, st["pt"])[...] = teq
    for n in ("ua", "va"):
        st[n][...] = 0.0
    eps = np.finfo(float).eps
    rks = R.scalars(pr["pdt"], pr["radius"], pr["rd_zur"], pr["pi"])["rks"]
    pl = compute(bd, st["delp"]) / np.transpose(st["peln"][:, 1:, :] - st["peln"][:, :-1, :], (0, 2, 1))
    meso = (pl <= 1.0e2) if pr["strat"] else np.zeros(pl.shape, dtype=bool)
    upper = (pl <= 100.0e2) if pr["strat"] else np.zeros(pl.shape, dtype=bool)
    exact = ~upper & (teq == R.T0)
    if km >= 12:
        assert exact.any() and (~upper & ~exact).any()
    bound = 32.0 * eps * np.abs(teq) * rks / pr["pdt"] + np.where(meso, 2.0 * eps * np.abs(teq) / pr["pdt"], 0.0)
    for fresh in (False, True):
        got = run_lib(lib, bd, st, pr, fresh=fresh)
        for n in ("u_dt", "v_dt"):
            assert not compute(bd, got[n]).any(), f"{n}: not zero at equilibrium (fresh = {fresh})"
        assert not got["t_dt"][exact].any(), f"t_dt: not zero at equilibrium on the t0 arm (fresh = {fresh})"
        print("equilibrium", shape, set_name, "max |t_dt| / bound", float(np.max(np.abs(got["t_dt"]) / bound)))
        assert np.all(np.abs(got["t_dt"]) <= bound), f"t_dt at equilibrium (fresh = {fresh})"


def check_friction_bits(lib, shape, set_name):
    """u_dt, v_dt keep their bits wherever sigl <= sigb or the cell is not in the troposphere branch, and change where the friction acts"""
    pr, bd, st = generic_case(shape, set_name, seed=2001)
    km = shape[2]
    m = R.friction_mask(bd, km, pr, st)
    assert m.any() and not m.all()
    got = run_lib(lib, bd, st, pr)
    for n in ("u_dt", "v_dt"):
        a, b = compute(bd, got[n]), compute(bd, st[n])
        assert same_bits(a[~m], b[~m]), f"{n}: written where no friction acts"
        assert np.all(a[m] != b[m]), f"{n}: unchanged where the friction acts"


# ---- age_of_air --------------------------------------------------------------------------------------------------------------------
def run_age(lib, bd, st, c, ctx=None):
    with H.own_or_borrowed(lib, bd, c["km"], ctx) as ctx:
        pe, q = ctx.from_host(st["pe"]), ctx.from_host(st["q"])
        ctx.age_of_air(c["km"], c["time"], pe, q)
        assert same_bits(pe.download(), st["pe"]), "pe was written"
        return q.download()


def check_age_against_golden(lib, name):
    c = HI.AGE_CASES[name]
    bd, st = HI.age_inputs(name)
    g = golden("age")
    assert str(g[f"{name}|sha"]) == HI.checksum(st), name
    ref = st["q"].copy(order="F")
    compute(bd, ref)[...] = g[f"{name}|out|q"]
    chk = st["q"].copy(order="F")
    R.age_of_air(bd, c["km"], c["time"], st["pe"], chk)
    assert same_bits(chk, ref), f"{name}: the restatement is not the reference's"
    if lib is not None:
        got = run_age(lib, bd, st, c)
        assert same_bits(got, ref), f"{name}: q is not the reference's (the halo included)"


def check_age_against_checker(lib, shape, time):
    nx, ny, km = shape
    bd, s = HI.state(nx, ny, km, 2101 + km)
    st = dict(pe=s["pe"], q=np.asfortranarray(np.random.default_rng(2102).uniform(-1.0, 1.0, bd.shape("A", km))))
    ref = st["q"].copy(order="F")
    R.age_of_air(bd, km, time, st["pe"], ref)
    got = run_age(lib, bd, st, dict(km=km, time=time))
    assert same_bits(got, ref)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    pr, bd, st = generic_case((12, 9, 12), "strat_zurita", seed=2201)
    ctx = Context(P.make_grid(bd, False), 12, lib=lib)
    try:
        d = upload(ctx, st)
        refused = H.refusals(functools.partial(call_lib, ctx), d, pr)

        ctx.lat_ready = True                     # (the wrapper would upload the gridstruct's on first use)
        refused("no latitude table")
        ctx.upload_lat(st["lat"])
        for n in ("delp", "peln", "pe", "pt", "ua", "va", "u_dt", "v_dt", "t_dt"):
            refused("null", drop=(n,))
        refused("pkz", dict(pr, zurita=False), drop=("pkz",))
        refused("pdt", dict(pr, pdt=0.0))
        refused("pdt", dict(pr, pdt=-225.0))
        refused("rd_zur", dict(pr, rd_zur=0.0))
        refused("rd_zur", dict(pr, rd_zur=-1.0))
        refused("radius", dict(pr, radius=0.0))
        refused("null", call=lambda: ctx.age_of_air(12, 1.0, None, d["pt"]))
        refused("null", call=lambda: ctx.age_of_air(12, 1.0, d["pe"], None))
        refused("km", call=lambda: ctx.age_of_air(0, 1.0, d["pe"], d["pt"]))
        H.assert_nothing_written(d, st, DEVICE)
        # npz < 1 cannot be reached: fv3_create refuses such a domain.  NOT refused: pkz left out with zurita
        call_lib(ctx, dict(d, pkz=None), pr)
    finally:
        ctx.close()


# ---- six faces as one group ------------------------------------------------------------------------------------------------------
def check_six_faces(lib, set_name, npx=13, npz=12):
    """the six faces as one fv3_group: the bits of six single launches, and ONE merged launch"""
    import cubed_common as CC
    cs, gs = CC.sphere(npx)
    n = npx - 1
    sts = []
    for t in range(6):
        pr, bd, st = generic_case((n, n, npz), set_name, seed=2301 + t)
        sts.append(st)
    alone = [run_lib(lib, bd, st, pr, fresh=bool(t % 2)) for t, st in enumerate(sts)]
    def prepare(mctx):
        for c, st in zip(mctx.ctxs, sts):
            c.upload_lat(st["lat"])
    for fresh in (False, True):      # fresh is one flag of the group's call: the faces run alone with it are compared
        H.six_faces(lib, gs, npz, sts, DEVICE, lambda mctx, d: call_lib(mctx, d, pr, fresh), alone, prepare, "held_suarez_tend",
                    faces=[t for t in range(6) if bool(t % 2) == fresh])


# ---- the memory contract -----------------------------------------------------------------------------------------------------------
def check_contract(lib, shape, set_name):
    """meant to run under memory_contract.run_case (every device array between guard bands, FV3_MI355X_POISON=1): the five layouts
    between their bands; with fresh the outputs prefilled with the pattern; inputs, halos and q_dt -- an array of fv_update_phys'
    that lies beside the three and is no argument of this call -- bit-unchanged; a call made after an fv3_fv_update_phys in the same
    context gives the bits of a fresh context"""
    import memory_contract as MC
    import parity_update_phys as UP
    pr, bd, st = generic_case(shape, set_name, seed=2401)
    km = shape[2]
    ref, cnt = run_checker(bd, st, pr)
    assert_conditions(pr, cnt, km)
    first = run_lib(lib, bd, st, pr)
    worst = compare(bd, st, first, ref, pr)
    check_fresh(lib, shape, set_name)
    ctx = Context(P.make_grid(bd, False), km, lib=lib)
    try:
        upr, _, ust = UP.generic_case(shape, True, True, 6, seed=2403)
        ud = UP.upload(ctx, ust)
        UP.call_lib(ctx, ud, upr)
        q_dt = ud["q_dt"].download()
        again = run_lib(lib, bd, st, pr, ctx=ctx)
        assert same_bits(ud["q_dt"].download(), q_dt), "q_dt was written"
        age = np.asfortranarray(np.random.default_rng(2404).uniform(-1.0, 1.0, bd.shape("A", km)))
        ref_age = age.copy(order="F")
        R.age_of_air(bd, km, 86400.0, st["pe"], ref_age)
        got_age = run_age(lib, bd, dict(pe=st["pe"], q=age), dict(km=km, time=86400.0), ctx=ctx)
        assert same_bits(got_age, ref_age), "age_of_air"
    finally:
        ctx.close()
    H.same_as_fresh_context(DEVICE, first, again, "fv3_fv_update_phys")
    return max(worst.values())


# ---- the Python host: FvDynamics.held_suarez -----------------------------------------------------------------------------------------
def check_host(lib, where, set_name="strat", age_tracer=7, time_total=3600.0):
    """FvDynamics.held_suarez on the state a step of parity_negadj.run_tile / run_sphere leaves (24 x 16 x 10 on the doubly periodic
    tile, C12 L8, moist, nq = 7, nonhydrostatic) against restatement-then-fv_update_phys: the restatement of Held_Suarez_Tend on
    zeroed tendencies, the restatement of the column routine of fv_update_phys, a real exchange of u_dt, v_dt and the restatement
    of update_dwinds_phys; the age tracer against age_of_air's restatement on the pe fv_update_phys leaves"""
    import parity_update_phys as UP
    fields = ("u", "v", "w", "delp", "pt", "ua", "va", "q", "delz", "pe", "peln", "pk", "ps", "pkz")
    strat, zurita = HI.SETS[set_name]
    base, kept = H.host_step(lib, where, fields, ("u_srf", "v_srf", "t_dt"),
                             lambda fv, bdt: fv.held_suarez(bdt, strat=strat, zurita=zurita, age_tracer=age_tracer, time_total=time_total))
    bd = base["bd"]
    before, after = kept["before"], kept["after"]
    nf = len(before["pt"])
    npz = before["pt"][0].shape[2]
    upr = H.update_phys_params(kept, before["q"][0].shape[3], hydrostatic=False, has_qdt=False)
    hpr = dict(pdt=kept["bdt"], strat=strat, zurita=zurita, rd_zur=1.0 / 25.0, radius=kept["radius"], pi=HI.PI)
    r = (bd.is_, bd.ie, bd.js, bd.je)
    ref = []
    for t in range(nf):
        s = {n: before[n][t].copy(order="F") for n in fields}
        s.update(t_dt=np.zeros((bd.nx, bd.ny, npz), order="F"), u_dt=bd.zeros("A", npz), v_dt=bd.zeros("A", npz),
                 lat=np.asfortranarray(compute(bd, kept["agrids"][t][..., 1])))
        cnt = R.held_suarez_tend(bd, npz, hpr, s)
        assert cnt["friction"] > 0 and cnt["no_friction"] > 0, cnt
        P.assert_close(f"face {t + 1} t_dt", after["t_dt"][t], s["t_dt"], max(BOUND.values()) or 10.0 * np.finfo(float).eps)
        ref.append(s)
    H.update_phys_reference(where, base, kept, ref, upr)
    worst = 0.0
    for t in range(nf):
        if age_tracer:
            qa = np.asfortranarray(ref[t]["q"][..., age_tracer - 1])
            R.age_of_air(bd, npz, time_total, ref[t]["pe"], qa)
            ref[t]["q"][..., age_tracer - 1] = qa
        rows = [("u", "U", (bd.is_, bd.ie, bd.js, bd.je + 1)), ("v", "V", (bd.is_, bd.ie + 1, bd.js, bd.je)), ("pt", "A", r), ("ua", "A", r),
                ("va", "A", r), ("q", "A", r)]
        for n, kind, rg in rows:
            a, b = bd.view(after[n][t], kind, *rg), bd.view(ref[t][n], kind, *rg)
            assert np.any(b != bd.view(before[n][t], kind, *rg)), n
            worst = max(worst, P.assert_close(f"face {t + 1} {n}", a, b, P.TOL))
        for n in ("delp", "w"):
            assert same_bits(after[n][t], before[n][t]), f"{n}: the forcing has no such tendency"
        P.assert_close(f"face {t + 1} delz", after["delz"][t], ref[t]["delz"], P.TOL)
        P.assert_close(f"face {t + 1} pe", after["pe"][t][1:-1, :, 1:-1], ref[t]["pe"][1:-1, :, 1:-1], P.TOL)
        for n in ("peln", "pk"):
            P.assert_close(f"face {t + 1} {n}", after[n][t], ref[t][n], UP.BOUND[n])
    return worst


def check_chain(lib):
    """the chained golden -- the reference's Held_Suarez_Tend followed by its whole fv_update_phys -- through FvDynamics.held_suarez
    on the doubly periodic tile: the recorded state is laid into the resident fields of a hydrostatic FvDynamics (the constants of
    the recipe's constants_mod), one call, and the fields the reference wrote are compared on the ranges it wrote.  u, v, ua, va,
    u_dt, v_dt, pe, ps, u_srf, v_srf have no transcendental on their path: bit-identical.  t_dt at the bounds of its branch sets; pt =
    pt + t_dt dt cp_air / cpm inherits t_dt's last bits: P.TOL; peln, pk, pkz at fv_update_phys' own bounds."""
    import parity_update_phys as UP
    from gfdl_atmos_cubed_sphere_amd.dyn_core import DynFlags
    from gfdl_atmos_cubed_sphere_amd.fv_dynamics import FvDynamics
    c = HI.CHAIN
    bd, st = HI.chain_inputs()
    g = golden("chain")
    assert str(g["chain|sha"]) == HI.checksum(st), "chain: the inputs formed from the seed are not those the golden was recorded with"
    km, nq = c["km"], c["nq"]
    ak, bk = HI.eta_levels(km)
    fl = DynFlags(hydrostatic=True, ptop=c["ptop"], akap=2.0 / 7.0, grav=9.80, rdgas=287.04, cp_air=287.04 / (2.0 / 7.0))
    ctx = Context(P.make_grid(bd, False), km, lib=lib)
    try:
        fv = FvDynamics(ctx, fl, ak, bk, nq=nq, radius=c["radius"])
        d = H.lay_state(fv, ctx, st, ("u", "v", "w", "delp", "pt", "ua", "va", "q", "ps", "pe", "peln", "pk", "pkz"))
        ctx.upload_lat(st["lat"])
        fv.held_suarez(c["pdt"], strat=c["strat"], zurita=c["zurita"], rd_zur=c["rd_zur"])
        got = {n: d[n].download() for n in HI.CHAIN_OUT + ("delp", "q")}
    finally:
        ctx.close()
    for n in HI.CHAIN_OUT:
        a, b = H.written_range(bd, n, got[n], ("pt", "ua", "va", "ps")), g[f"chain|out|{n}"]
        if n == "t_dt":
            pr = params_of(dict(c))
            for bs, m in branch_masks(bd, km, pr, st).items():
                assert m.any(), bs
                P.assert_close(f"chain t_dt ({bs})", a[m], b[m], BOUND[bs])
        elif n == "pt":
            P.assert_close("chain pt", a, b, P.TOL)
        elif n in UP.BOUND:
            P.assert_close(f"chain {n}", a, b, UP.BOUND[n])
        else:
            assert same_bits(a, b), f"chain: {n} is not the reference's, max diff {np.max(np.abs(a - b)):.3e}"
    for n in ("delp", "q"):      # the reference's q_dt is zero there: the air mass and the tracers keep their bits
        assert same_bits(got[n], st[n]), n
