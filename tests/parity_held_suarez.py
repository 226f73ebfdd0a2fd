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
import os

import numpy as np

import held_suarez_inputs as HI
import parity_common as P
import ref_held_suarez as R
from gfdl_atmos_cubed_sphere_amd.lib import Context, Fv3Error

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ((21, 7, 1), (21, 7, 2), (40, 19, 12), (130, 100, 32))
IDS = ["21x7x1", "21x7x2", "40x19x12", "130x100x32"]
DEVICE = HI.DEVICE
# branch set -> (relative RMS, max norm) of t_dt, library (CPU harness) against the compiled reference, worst recorded case
MEASURED = {"standard": (2.095e-17, 8.561e-17), "zurita": (4.126e-16, 1.338e-15), "strat_meso": (9.463e-17, 2.371e-16)}
BOUND = {n: 10.0 * v[0] for n, v in MEASURED.items()}
assert max(BOUND.values()) <= 1.0e-12


@functools.lru_cache(maxsize=None)
def golden(group):
    return dict(np.load(os.path.join(HERE, "golden", f"held_suarez_{group}.npz")))


def params_of(c):
    return dict(pdt=c["pdt"], strat=c["strat"], zurita=c["zurita"], rd_zur=c["rd_zur"], radius=c.get("radius", HI.RADIUS), pi=HI.PI)


def set_params(name, pdt=225.0):
    s, z = HI.SETS[name]
    return dict(pdt=pdt, strat=s, zurita=z, rd_zur=1.0 / 25.0, radius=HI.RADIUS, pi=HI.PI)


def call_lib(ctx, d, pr, fresh=False):
    ctx.held_suarez_tend(pr["pdt"], d["delp"], d["peln"], d["pe"], d["pkz"], d["pt"], d["ua"], d["va"], d["u_dt"], d["v_dt"], d["t_dt"],
                         strat=pr["strat"], zurita=pr["zurita"], rd_zur=pr["rd_zur"], fresh=fresh, radius=pr["radius"], pi=pr["pi"])


def upload(ctx, st):
    return {n: ctx.from_host(st[n]) for n in DEVICE}


def download(d):
    return {n: d[n].download() for n in DEVICE}


def run_lib(lib, bd, st, pr, fresh=False, ctx=None):
    """fv3_held_suarez_tend on a copy of the state -> {field: whole array}"""
    km = st["pt"].shape[2]
    own = ctx is None
    if own:
        ctx = Context(P.make_grid(bd, False), km, lib=lib)
    try:
        ctx.upload_lat(st["lat"])
        d = upload(ctx, st)
        call_lib(ctx, d, pr, fresh)
        return download(d)
    finally:
        if own:
            ctx.close()


def run_checker(bd, st, pr, teq_out=None):
    o = {n: st[n].copy(order="F") for n in st}
    cnt = R.held_suarez_tend(bd, st["pt"].shape[2], pr, o, teq_out=teq_out)
    return o, cnt


def compute(bd, a):
    return bd.view(a, "A", bd.is_, bd.ie, bd.js, bd.je)


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
        assert np.array_equal(got[n].view(np.uint64), st[n].view(np.uint64)), f"{n}: an input was written"
    for n in ("u_dt", "v_dt"):
        assert np.array_equal(got[n].view(np.uint64), ref[n].view(np.uint64)), \
            f"{n}: not bit-identical, max diff {np.max(np.abs(got[n] - ref[n])):.3e}"
    out = {}
    for bs, m in branch_masks(bd, km, pr, st).items():
        if not m.any():
            continue
        a, b = got["t_dt"][m], ref["t_dt"][m]
        assert np.all(np.isfinite(a)), f"t_dt ({bs}): non-finite values"
        if BOUND[bs] == 0.0:
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"t_dt ({bs}): not bit-identical, max diff {np.max(np.abs(a - b)):.3e}"
            out[bs] = 0.0
        else:
            out[bs] = P.assert_close(f"t_dt ({bs})", a, b, BOUND[bs])
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
        assert np.array_equal(got[n].view(np.uint64), ref[n].view(np.uint64)), f"{name}: {n} of the restatement is not the reference's"
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
        assert np.array_equal(got2["t_dt"].view(np.uint64), got["t_dt"].view(np.uint64)), "t_dt with fresh"
        for n in ("u_dt", "v_dt"):
            assert np.array_equal(compute(bd, got2[n]).view(np.uint64), compute(bd, got[n]).view(np.uint64)), f"{n} with fresh"
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
    assert np.array_equal(got["t_dt"].view(np.uint64), zeroed["t_dt"].view(np.uint64)), "t_dt: fresh differs from zero-then-call"
    assert np.any(np.signbit(zeroed["t_dt"])) and np.any(zeroed["t_dt"] != 0.0)
    for n in ("u_dt", "v_dt"):
        a, b = compute(bd, got[n]), compute(bd, zeroed[n])
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{n}: fresh differs from zero-then-call"
        assert np.any(b != 0.0) and np.any(b == 0.0), f"{n}: the case has no cell with / without friction"
        halo = np.ones(got[n].shape, dtype=bool)
        compute(bd, halo)[...] = False
        assert np.array_equal(got[n][halo].view(np.uint64), pat[n][halo].view(np.uint64)), f"{n}: fresh wrote the halo"
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
        assert np.array_equal(a[~m].view(np.uint64), b[~m].view(np.uint64)), f"{n}: written where no friction acts"
        assert np.all(a[m] != b[m]), f"{n}: unchanged where the friction acts"


# ---- age_of_air --------------------------------------------------------------------------------------------------------------------
def run_age(lib, bd, st, c, ctx=None):
    own = ctx is None
    if own:
        ctx = Context(P.make_grid(bd, False), c["km"], lib=lib)
    try:
        pe, q = ctx.from_host(st["pe"]), ctx.from_host(st["q"])
        ctx.age_of_air(c["km"], c["time"], pe, q)
        assert np.array_equal(pe.download().view(np.uint64), st["pe"].view(np.uint64)), "pe was written"
        return q.download()
    finally:
        if own:
            ctx.close()


def check_age_against_golden(lib, name):
    c = HI.AGE_CASES[name]
    bd, st = HI.age_inputs(name)
    g = golden("age")
    assert str(g[f"{name}|sha"]) == HI.checksum(st), name
    ref = st["q"].copy(order="F")
    compute(bd, ref)[...] = g[f"{name}|out|q"]
    chk = st["q"].copy(order="F")
    R.age_of_air(bd, c["km"], c["time"], st["pe"], chk)
    assert np.array_equal(chk.view(np.uint64), ref.view(np.uint64)), f"{name}: the restatement is not the reference's"
    if lib is not None:
        got = run_age(lib, bd, st, c)
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), f"{name}: q is not the reference's (the halo included)"


def check_age_against_checker(lib, shape, time):
    nx, ny, km = shape
    bd, s = HI.state(nx, ny, km, 2101 + km)
    st = dict(pe=s["pe"], q=np.asfortranarray(np.random.default_rng(2102).uniform(-1.0, 1.0, bd.shape("A", km))))
    ref = st["q"].copy(order="F")
    R.age_of_air(bd, km, time, st["pe"], ref)
    got = run_age(lib, bd, st, dict(km=km, time=time))
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    pr, bd, st = generic_case((12, 9, 12), "strat_zurita", seed=2201)
    ctx = Context(P.make_grid(bd, False), 12, lib=lib)
    try:
        d = upload(ctx, st)

        def refused(match, p=pr, drop=()):
            try:
                call_lib(ctx, dict(d, **{n: None for n in drop}), p)
            except Fv3Error as e:
                assert match in str(e), (match, str(e))
            else:
                raise AssertionError(f"fv3_held_suarez_tend took a call that must be refused ({match})")

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
        for bad in (dict(pe=None), dict(q=None)):
            try:
                ctx.age_of_air(12, 1.0, bad.get("pe", d["pe"]), bad.get("q", d["pt"]))
            except Fv3Error as e:
                assert "null" in str(e)
            else:
                raise AssertionError("fv3_age_of_air took a null field")
        try:
            ctx.age_of_air(0, 1.0, d["pe"], d["pt"])
        except Fv3Error as e:
            assert "km" in str(e)
        else:
            raise AssertionError("fv3_age_of_air took km = 0")
        got = download(d)
        for n in DEVICE:
            assert np.array_equal(got[n].view(np.uint64), st[n].view(np.uint64)), f"{n}: a refused call wrote"
        # npz < 1 cannot be reached: fv3_create refuses such a domain.  NOT refused: pkz left out with zurita
        call_lib(ctx, dict(d, pkz=None), pr)
    finally:
        ctx.close()


# ---- six faces as one group ------------------------------------------------------------------------------------------------------
def check_six_faces(lib, set_name, npx=13, npz=12):
    """the six faces as one fv3_group: the bits of six single launches, and ONE merged launch"""
    import cubed_common as CC
    from gfdl_atmos_cubed_sphere_amd.cubed_dyn import MultiContext
    cs, gs = CC.sphere(npx)
    n = npx - 1
    sts = []
    for t in range(6):
        pr, bd, st = generic_case((n, n, npz), set_name, seed=2301 + t)
        sts.append(st)
    alone = [run_lib(lib, bd, st, pr, fresh=bool(t % 2)) for t, st in enumerate(sts)]
    for fresh in (False, True):
        mctx = MultiContext([Context(g, npz, lib=lib) for g in gs], group=True)
        try:
            assert mctx.group is not None
            for c, st in zip(mctx.ctxs, sts):
                c.upload_lat(st["lat"])
            d = {name: mctx.from_host([st[name] for st in sts]) for name in DEVICE}
            mctx.flush()
            mctx.group.stats()
            call_lib(mctx, d, pr, fresh)
            mctx.flush()
            merged, single = mctx.group.stats()
            assert merged == 1 and single == 0, f"held_suarez_tend of six faces: {merged} merged launches, {single} single ones"
            for name in DEVICE:
                got = d[name].download()
                for t in range(6):
                    if bool(t % 2) == fresh:
                        assert np.array_equal(got[t].view(np.uint64), alone[t][name].view(np.uint64)), f"face {t + 1} {name}"
        finally:
            mctx.close()


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
        assert np.array_equal(ud["q_dt"].download().view(np.uint64), q_dt.view(np.uint64)), "q_dt was written"
        age = np.asfortranarray(np.random.default_rng(2404).uniform(-1.0, 1.0, bd.shape("A", km)))
        ref_age = age.copy(order="F")
        R.age_of_air(bd, km, 86400.0, st["pe"], ref_age)
        got_age = run_age(lib, bd, dict(pe=st["pe"], q=age), dict(km=km, time=86400.0), ctx=ctx)
        assert np.array_equal(got_age.view(np.uint64), ref_age.view(np.uint64)), "age_of_air"
    finally:
        ctx.close()
    for n in DEVICE:
        assert np.array_equal(again[n].view(np.uint64), first[n].view(np.uint64)), f"{n}: a call after fv3_fv_update_phys differs from a fresh context"
    return max(worst.values())


# ---- the Python host: FvDynamics.held_suarez -----------------------------------------------------------------------------------------
def check_host(lib, where, set_name="strat", age_tracer=7, time_total=3600.0):
    """FvDynamics.held_suarez on the state a step of parity_negadj.run_tile / run_sphere leaves (24 x 16 x 10 on the doubly periodic
    tile, C12 L8, moist, nq = 7, nonhydrostatic) against restatement-then-fv_update_phys: the restatement of Held_Suarez_Tend on
    zeroed tendencies, the restatement of the column routine of fv_update_phys, a real exchange of u_dt, v_dt and the restatement
    of update_dwinds_phys; the age tracer against age_of_air's restatement on the pe fv_update_phys leaves"""
    import gfdl_atmos_cubed_sphere_amd.fv_dynamics as M
    import parity_negadj as NA
    import parity_remap as PR
    import parity_subgrid as PS
    import parity_update_phys as UP
    import ref_fv_sg as SG
    import ref_update_phys as RU
    import update_phys_inputs as UI
    from gfdl_atmos_cubed_sphere_amd.layout import periodic_fill
    orig, kept = M.FvDynamics, {}
    fields = ("u", "v", "w", "delp", "pt", "ua", "va", "q", "delz", "pe", "peln", "pk", "ps", "pkz")
    strat, zurita = HI.SETS[set_name]

    class HsFvDynamics(orig):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            if where == "sphere":      # the tests' gridstructs are the oracle's: what update_dwinds_phys reads comes from there as well
                import cubed_common as CC
                cs, _ = CC.sphere(self.ctx.grid.npx)
                for t, c in enumerate(self.ctx.ctxs):
                    c.upload_dwinds(PS.oracle_dwinds_geom(cs, t))

        def step_from_temperature(self, bdt):
            super().step_from_temperature(bdt)
            d = self.dc.d
            dl = lambda n: NA._faces(d[n].download())      # noqa: E731
            before = {n: [a.copy(order="F") for a in dl(n)] for n in fields}
            self.held_suarez(bdt, strat=strat, zurita=zurita, age_tracer=age_tracer, time_total=time_total)
            kept.update(before=before, bdt=bdt, consts=dict(self.neg_adj_consts, kappa=self.fl.akap), ptop=self.fl.ptop, radius=self.radius,
                        after={n: dl(n) for n in fields + ("u_srf", "v_srf", "t_dt")}, ak=self.ak, bk=self.bk,
                        lats=[np.asarray(c.grid.m["agrid"])[..., 1] for c in (self.ctx.ctxs if hasattr(self.ctx, "ctxs") else [self.ctx])])

    M.FvDynamics = HsFvDynamics
    try:
        base = (NA.run_tile if where == "tile" else NA.run_sphere)(lib)
    finally:
        M.FvDynamics = orig
    bd = base["bd"]
    before, after = kept["before"], kept["after"]
    nf = len(before["pt"])
    npz = before["pt"][0].shape[2]
    sp = {n: PR.MOIST6[n] for n in UI.SPECIES if n != "sphum"}
    sp["sphum"] = 1
    nq = before["q"][0].shape[3]
    upr = dict(dt=kept["bdt"], ptop=kept["ptop"], hydrostatic=False, phys_hydrostatic=True, gfs_phys=False, nq=nq, ncnst=nq, nwat=PR.MOIST6["nwat"],
               species=sp, adjust_mass=np.ones(nq, dtype=np.int32), has_qdt=False, tau_h2o=0.0, ak=kept["ak"], bk=kept["bk"])
    hpr = dict(pdt=kept["bdt"], strat=strat, zurita=zurita, rd_zur=1.0 / 25.0, radius=kept["radius"], pi=HI.PI)
    r = (bd.is_, bd.ie, bd.js, bd.je)
    ref = []
    for t in range(nf):
        s = {n: before[n][t].copy(order="F") for n in fields}
        s.update(t_dt=np.zeros((bd.nx, bd.ny, npz), order="F"), u_dt=bd.zeros("A", npz), v_dt=bd.zeros("A", npz),
                 lat=np.asfortranarray(bd.view(kept["lats"][t], "A", *r)))
        cnt = R.held_suarez_tend(bd, npz, hpr, s)
        assert cnt["friction"] > 0 and cnt["no_friction"] > 0, cnt
        P.assert_close(f"face {t + 1} t_dt", after["t_dt"][t], s["t_dt"], max(BOUND.values()) or 10.0 * np.finfo(float).eps)
        s.update(q_dt=np.zeros((bd.nx, bd.ny, npz, nq), order="F"), qdiag=np.zeros(bd.shape("A", npz) + (0,), order="F"),
                 u_srf=np.zeros((bd.nx, bd.ny), order="F"), v_srf=np.zeros((bd.nx, bd.ny), order="F"))
        RU.fv_update_phys(bd, npz, upr, s, consts=kept["consts"])
        ref.append(s)
    if where == "tile":
        for n in ("u_dt", "v_dt"):
            periodic_fill(bd, ref[0][n], "A")
        geoms = [None]
    else:
        import cubed_common as CC
        cs, _ = CC.sphere(base["gs"][0].npx)
        CC.exchange(cs, ref, ("u_dt", "v_dt"), "A")
        geoms = [PS.oracle_dwinds_geom(cs, t) for t in range(6)]
    worst = 0.0
    for t in range(nf):
        g = base["g"] if where == "tile" else base["gs"][t]
        SG.update_dwinds_phys(bd, g.npx, g.npy, g.grid_type, kept["bdt"], ref[t]["u_dt"], ref[t]["v_dt"], ref[t]["u"], ref[t]["v"], geoms[t])
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
            assert np.array_equal(after[n][t].view(np.uint64), before[n][t].view(np.uint64)), f"{n}: the forcing has no such tendency"
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
        d = fv.dc.d
        for n in ("u", "v", "w", "delp", "pt", "ua", "va", "q", "ps", "pe", "peln", "pk", "pkz"):
            if n in d:
                d[n].upload(st[n])
            else:
                d[n] = ctx.from_host(st[n])
        ctx.upload_lat(st["lat"])
        fv.held_suarez(c["pdt"], strat=c["strat"], zurita=c["zurita"], rd_zur=c["rd_zur"])
        got = {n: d[n].download() for n in HI.CHAIN_OUT + ("delp", "q")}
    finally:
        ctx.close()

    def rng(n, a):
        if n == "u":
            return bd.view(a, "U", bd.is_, bd.ie, bd.js, bd.je + 1)
        if n == "v":
            return bd.view(a, "V", bd.is_, bd.ie + 1, bd.js, bd.je)
        if n == "pe":
            return a[1:-1, :, 1:-1]
        return compute(bd, a) if n in ("pt", "ua", "va", "ps") else a
    for n in HI.CHAIN_OUT:
        a, b = rng(n, got[n]), g[f"chain|out|{n}"]
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
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"chain: {n} is not the reference's, max diff {np.max(np.abs(a - b)):.3e}"
    for n in ("delp", "q"):      # the reference's q_dt is zero there: the air mass and the tracers keep their bits
        assert np.array_equal(got[n].view(np.uint64), st[n].view(np.uint64)), n
