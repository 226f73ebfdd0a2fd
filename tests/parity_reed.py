"""Check bodies of the Reed-Jablonowski simple physics and the terminator chemistry -- fv3_reed_sim_phys, fv3_grid_upload_reed,
fv3_terminator_advance, fv3_grid_upload_terminator (driver/solo/fv_phys.F90:551-602, :2332-2894) and FvDynamics.reed_sim_phys -- shared
by tests/test_reed_hostemu.py (CPU) and tests/test_reed_gpu.py, and by the contract tests of both: the library against the outputs of
the reference's compiled Fortran (tests/golden/reed/*.npz), against the numpy restatement tests/ref_reed.py, and properties that need
no restatement.

Bounds.  The two host-formed planes and the terminator's k1 are bit-identical with the reference's compiler.  Every tendency of
reed_sim_physics passes through a log (za) and usually an exp or a power, so none is expected to be bit-identical with the compiled
reference, and none is claimed to be -- except where the routine adds nothing (u_dt, v_dt with reed_cond_only), which is.  The bound
is measured on the REFERENCE side alone: `python tests/golden/make_reed_golden.py --measure` perturbs every log, exp and power of the
restatement by one unit in the last place (the power: 1 + |y ln x| units), seeded signs, 8 seeds, every recorded case, and takes per
output field and flag set the worst relative RMS change -- MEASURED below, what one last bit of the reference's own libm is worth.
The tests assert TEN times that: the project's margin, which here covers a systematic one-sided last-bit error adding up linearly
over at most 32 levels of the solve where random signs add up as the root.  A figure measured as zero is asserted bit-identical.
The library's actual differences (CPU harness against the compiled reference), printed by --measure beside them:
LIBRARY below."""
from __future__ import annotations

import functools

import numpy as np

import parity_common as P
import parity_phys as H
import reed_inputs as RI
import ref_reed as R
from gfdl_atmos_cubed_sphere_amd.lib import Context
from parity_phys import compute, same_bits  # noqa: F401

DEVICE = RI.DEVICE
TEND = ("u_dt", "v_dt", "t_dt", "q_dt")
# (flag set, field) -> relative RMS, perturbed restatement against the restatement, worst of 8 seeds x the recorded cases
MEASURED = {("alt", "q_dt"): 8.347e-14, ("alt", "rain"): 1.626e-15, ("alt", "t_dt"): 2.467e-13, ("alt", "u_dt"): 9.842e-14, ("alt", "v_dt"): 1.035e-13,
            ("cond", "q_dt"): 1.004e-13, ("cond", "rain"): 1.540e-15, ("cond", "t_dt"): 2.363e-13, ("cond", "u_dt"): 1.145e-13, ("cond", "v_dt"): 1.035e-13,
            ("condonly", "q_dt"): 1.394e-15, ("condonly", "rain"): 1.414e-15, ("condonly", "t_dt"): 1.391e-15, ("condonly", "u_dt"): 0.0,
            ("condonly", "v_dt"): 0.0,
            ("nocond", "q_dt"): 1.350e-13, ("nocond", "t_dt"): 2.093e-12, ("nocond", "u_dt"): 1.052e-13, ("nocond", "v_dt"): 1.014e-13}
# the same keys -> the library of the CPU harness against the compiled reference, worst recorded case (not a bound: for the reader)
LIBRARY = {("alt", "q_dt"): 2.345e-14, ("alt", "rain"): 6.016e-16, ("alt", "t_dt"): 6.435e-14, ("alt", "u_dt"): 2.376e-14, ("alt", "v_dt"): 1.903e-14,
           ("cond", "q_dt"): 2.068e-14, ("cond", "rain"): 5.434e-16, ("cond", "t_dt"): 6.241e-14, ("cond", "u_dt"): 2.700e-14, ("cond", "v_dt"): 2.202e-14,
           ("condonly", "q_dt"): 4.766e-16, ("condonly", "rain"): 4.671e-16, ("condonly", "t_dt"): 4.826e-16, ("condonly", "u_dt"): 0.0,
           ("condonly", "v_dt"): 0.0,
           ("nocond", "q_dt"): 2.817e-14, ("nocond", "t_dt"): 5.324e-13, ("nocond", "u_dt"): 2.147e-14, ("nocond", "v_dt"): 3.048e-14}
# Cl, Cl2 of the terminator, the same two measurements
TERM_MEASURED = {"cl": 1.097e-17, "cl2": 2.007e-17}
TERM_LIBRARY = {"cl": 4.908e-18, "cl2": 2.775e-18}


def bound(fam, n):
    return 10.0 * MEASURED[(fam, n)]


def family(c):
    return c["flags"] if "flags" in c else next(f for f, v in RI.FLAGS.items() if v == (c["do_reed_cond"], c["reed_cond_only"], c["reed_alt_mxg"]))


def fields_of(c):
    return TEND + (("rain",) if c["do_reed_cond"] else ())


golden = functools.partial(H.golden, "reed/", slashes=True)


def call_lib(ctx, d, pr, fresh=False):
    ctx.reed_sim_phys(pr["pdt"], d["delp"], d["pt"], d["ua"], d["va"], d["q"], d["pe"], d["peln"], d["phis"], d["delz"], d["u_dt"], d["v_dt"],
                      d["t_dt"], d["q_dt"], d["rain"], hydrostatic=pr["hydrostatic"], reed_test=pr["reed_test"], do_reed_cond=pr["do_reed_cond"],
                      reed_cond_only=pr["reed_cond_only"], reed_alt_mxg=pr["reed_alt_mxg"], fresh=fresh, consts=pr["consts"])


def upload(ctx, st):
    return H.upload(ctx, st, DEVICE)


def download(d):
    return H.download(d, DEVICE)


def run_lib(lib, bd, st, pr, fresh=False, ctx=None):
    """fv3_reed_sim_phys on a copy of the state -> {field: whole array}"""
    with H.own_or_borrowed(lib, bd, st["pt"].shape[2], ctx) as ctx:
        ctx.grid_upload_reed(pr["reed_test"], st["lat"], consts=pr["consts"])
        d = upload(ctx, st)
        call_lib(ctx, d, pr, fresh)
        return download(d)


def run_checker(bd, st, pr, M=None):
    o = {n: st[n].copy(order="F") for n in st}
    cnt = R.reed_wrapper(bd, st["pt"].shape[2], pr, o, M=M)
    return o, cnt


def lib_planes(lib, lat, test, consts=None):
    bd = RI.Bounds(1, lat.shape[0], 1, lat.shape[1])
    with H.own_or_borrowed(lib, bd, 1) as ctx:
        ctx.grid_upload_reed(test, lat, consts=consts or RI.CONSTS)
        return ctx.grid_download_reed()


def lib_k1(lib, bd, agrid):
    with H.own_or_borrowed(lib, bd, 1) as ctx:
        ctx.grid_upload_terminator(agrid, RI.PI)
        return ctx.grid_download_terminator()


def compare(bd, st, got, ref, c, what=""):
    """every input unchanged, the halo of u_dt, v_dt unchanged, each output field at its bound -> {field: relative RMS}"""
    fam = family(c)
    for n in RI.IN:
        assert same_bits(got[n], st[n]), f"{what}{n}: an input was written"
    for n in ("u_dt", "v_dt"):
        halo = H.halo_mask(bd, got[n].shape)
        assert same_bits(got[n][halo], st[n][halo]), f"{what}{n}: the halo was written"
    if not c["do_reed_cond"]:
        assert same_bits(got["rain"], st["rain"]), f"{what}rain: written without do_reed_cond"
    out = {}
    for n in fields_of(c):
        a, b = (compute(bd, got[n]), compute(bd, ref[n])) if n in ("u_dt", "v_dt") else (got[n], ref[n])
        if bound(fam, n) != 0.0 and not b.any():      # only here: a reference field that is all zero (no relative figure) must come back zero
            assert np.all(np.isfinite(a)) and not a.any(), f"{what}{n}: the reference is zero"
            out[n] = 0.0
        else:
            out[n] = H.assert_bounded(f"{what}{n} ({fam})", a, b, bound(fam, n))
    return out


# ---- the recorded outputs of the reference's compiled Fortran ----------------------------------------------------------------------
def golden_case(name):
    """-> (case, bd, inputs, the reference's outputs as whole arrays)"""
    c = RI.CASES[name]
    bd, st = RI.case_inputs(name)
    g = golden(c["group"])
    assert str(g[f"{name}|sha"]) == RI.checksum(st), f"{name}: the inputs formed from the seed are not those the golden was recorded with"
    ref = {n: st[n].copy(order="F") for n in DEVICE}
    for n in ("t_dt", "q_dt", "rain"):
        ref[n][...] = g[f"{name}|out|{n}"]
    for n in ("u_dt", "v_dt"):
        compute(bd, ref[n])[...] = g[f"{name}|out|{n}"]
    return c, bd, st, ref


def assert_conditions(c, cnt, km):
    assert cnt["q_neg"] > 0, cnt
    if c["do_reed_cond"]:
        assert cnt["sat"] > 0 and cnt["unsat"] > 0 and cnt["qsat_edge"] == 0, cnt
    if not c["reed_cond_only"]:
        assert cnt["wind_lt_v20"] > 0 and cnt["wind_ge_v20"] > 0, cnt
        if km >= 2:
            assert (cnt["z_above"] > 0 and cnt["z_below"] > 0) if c["reed_alt_mxg"] else (cnt["p_above"] > 0 and cnt["p_below"] > 0), cnt


def check_checker_against_golden(name):
    """the restatement against the compiled reference, at the library's bounds; it also holds what DESIGN says of the branches: the
    recorded cases take every branch, and no cell lies within 4 ulp of saturation"""
    c, bd, st, ref = golden_case(name)
    got, cnt = run_checker(bd, st, RI.params_of(c))
    assert_conditions(c, cnt, c["km"])
    compare(bd, st, {**got, **{n: st[n] for n in RI.IN}}, ref, c, what=f"{name} restatement ")
    return cnt


def check_lib_against_golden(lib, name):
    """the library against the recorded outputs with nothing in between -> {field: relative RMS}"""
    import memory_contract as MC
    c, bd, st, ref = golden_case(name)
    pr = RI.params_of(c)
    got = run_lib(lib, bd, st, pr)
    out = compare(bd, st, got, ref, c, what=f"{name} ")
    print(name, {n: float(v) for n, v in out.items()})
    if c["zero"]:      # the pair of fresh: the same outputs without reading the four, and nothing of a prefilled pattern left
        st2 = dict(st, **{n: MC.pattern_array(st[n].shape) for n in TEND})
        got2 = run_lib(lib, bd, st2, pr, fresh=True)
        for n in TEND:
            a, b = (compute(bd, got2[n]), compute(bd, got[n])) if n in ("u_dt", "v_dt") else (got2[n], got[n])
            assert same_bits(a, b), f"{name}: {n} with fresh differs from zero-then-call"
            assert np.all(np.abs(a) < 1.0e29), f"{name}: {n}: the pattern survives on the compute domain"
        if c["do_reed_cond"]:
            assert same_bits(got2["rain"], got["rain"]), f"{name}: rain with fresh"
    return out


def check_planes(lib):
    """the host-formed planes against the same expressions from the reference's compiler, bit for bit, on every recorded latitude"""
    g = golden("planes")
    lat = RI.latitude()
    assert same_bits(g["lat"], lat)
    assert 0.5 * RI.PI - lat.max() <= 1.0e-12 and 0.5 * RI.PI + lat.min() <= 1.0e-12
    for test in (0, 1):
        ts, sf = lib_planes(lib, lat, test)
        for n, a in (("tsurf", ts), ("sstf", sf)):
            b = g[f"t{test}|{n}"]
            assert same_bits(a, b), \
                f"reed_test {test} {n}: not the compiler's, max relative difference {np.max(np.abs(a - b) / np.abs(b)):.3e}"
    for name in RI.TERM_CASES:
        bd, st = RI.term_inputs(name)
        a, b = lib_k1(lib, bd, st["agrid"]), g[f"{name}|k1"]
        assert same_bits(a, b), f"{name} k1: not the compiler's, max difference {np.max(np.abs(a - b)):.3e}"


# ---- fresh, properties -------------------------------------------------------------------------------------------------------------
def generic_case(shape, flags, hydrostatic=True, reed_test=0, seed=6101, zero=False, pdt=225.0):
    nx, ny, km = shape
    cnd, only, alt = RI.FLAGS[flags]
    c = dict(flags=flags, km=km, hydrostatic=hydrostatic, reed_test=reed_test, do_reed_cond=cnd, reed_cond_only=only, reed_alt_mxg=alt, pdt=pdt,
             zero=zero)
    bd, st = RI.state(nx, ny, km, seed + km, zero_tendencies=zero, lat_seed=seed + 1)
    return c, bd, st


def check_against_checker(lib, shape, flags, hydrostatic=True, reed_test=1):
    """a shape with more than one block of 256 columns and a tail block, against the restatement"""
    c, bd, st = generic_case(shape, flags, hydrostatic, reed_test)
    pr = RI.params_of(c)
    ref, cnt = run_checker(bd, st, pr)
    assert_conditions(c, cnt, shape[2])
    return compare(bd, st, run_lib(lib, bd, st, pr), ref, c)


def check_fresh(lib, shape, flags, reed_test=0):
    """fresh is bit-identical, the sign of zero included, with zero-then-call, and writes every cell"""
    import memory_contract as MC
    c, bd, st = generic_case(shape, flags, hydrostatic=False, reed_test=reed_test, seed=6201, zero=True)
    pr = RI.params_of(c)
    zeroed = run_lib(lib, bd, st, pr)
    pat = {n: MC.pattern_array(st[n].shape) for n in TEND}
    got = run_lib(lib, bd, dict(st, **pat), pr, fresh=True)
    for n in TEND:
        a, b = (compute(bd, got[n]), compute(bd, zeroed[n])) if n in ("u_dt", "v_dt") else (got[n], zeroed[n])
        assert same_bits(a, b), f"{n}: fresh differs from zero-then-call"
        assert np.all(np.abs(a) < 1.0e29), f"{n}: the pattern survives on the compute domain"
    for n in ("u_dt", "v_dt"):
        halo = H.halo_mask(bd, got[n].shape)
        assert same_bits(got[n][halo], pat[n][halo]), f"{n}: fresh wrote the halo"
    assert same_bits(got["rain"], zeroed["rain"])


def check_test2_and_rain(lib, shape):
    """reed_test = 2 leaves the tendencies' bits alone (with fresh: zeros) and, with do_reed_cond, writes rain = 0; with do_reed_cond
    off rain keeps its bits whatever the test"""
    import memory_contract as MC
    for flags in ("cond", "nocond"):
        c, bd, st = generic_case(shape, flags, reed_test=2, seed=6301)
        pr = RI.params_of(c)
        got = run_lib(lib, bd, st, pr)
        for n in TEND + RI.IN:
            assert same_bits(got[n], st[n]), f"{n}: written with reed_test = 2"
        st2 = dict(st, **{n: MC.pattern_array(st[n].shape) for n in TEND})
        got2 = run_lib(lib, bd, st2, pr, fresh=True)
        for n in TEND:
            a = compute(bd, got2[n]) if n in ("u_dt", "v_dt") else got2[n]
            assert not a.any() and not np.signbit(a).any(), f"{n}: not +0 with reed_test = 2 and fresh"
        for g in (got, got2):
            if c["do_reed_cond"]:
                assert not g["rain"].any()
            else:
                assert same_bits(g["rain"], st["rain"]), "rain: written without do_reed_cond"
    c, bd, st = generic_case(shape, "nocond", reed_test=0, seed=6302)
    got = run_lib(lib, bd, st, RI.params_of(c))
    assert same_bits(got["rain"], st["rain"]), "rain: written without do_reed_cond"
    assert not np.array_equal(got["t_dt"], st["t_dt"])


# ---- the terminator ----------------------------------------------------------------------------------------------------------------
def run_term(lib, bd, st, c, ctx=None):
    with H.own_or_borrowed(lib, bd, c["km"], ctx) as ctx:
        ctx.grid_upload_terminator(st["agrid"], RI.PI)
        cl, cl2 = ctx.from_host(st["cl"]), ctx.from_host(st["cl2"])
        ctx.terminator_advance(c["km"], c["pdt"], cl, cl2, term_fill_negative=c["fill"])
        return dict(cl=cl.download(), cl2=cl2.download())


def term_compare(what, got, ref):
    for n in ("cl", "cl2"):
        H.assert_bounded(f"{what} {n}", got[n], ref[n], 10.0 * TERM_MEASURED[n])


def check_term_against_golden(lib, name):
    """the restatement (lib None) or the library against the compiled reference: the whole planes, halo included"""
    c = RI.TERM_CASES[name]
    bd, st = RI.term_inputs(name)
    g = golden("terminator")
    assert str(g[f"{name}|sha"]) == RI.checksum(st), name
    ref = dict(cl=g[f"{name}|out|cl"], cl2=g[f"{name}|out|cl2"])
    if lib is None:
        got = {n: st[n].copy(order="F") for n in ("cl", "cl2")}
        night = R.terminator_advance(c["pdt"], c["fill"], R.term_k1(st["agrid"], RI.PI), got["cl"], got["cl2"])
        assert night > 0 and (st["cl"] < 0.0).any() and (st["cl2"] < 0.0).any()
    else:
        got = run_term(lib, bd, st, c)
    term_compare(name, got, ref)


def check_term_conserves(lib, shape, fill):
    """Cl + 2 Cl2 per cell.  The routine forms Cl' = Cl + f pdt and Cl2' = Cl2 - f 0.5 pdt with ONE f; (f 0.5) pdt and f pdt are
    each one rounding (the halving is exact), so Cl' + 2 Cl2' differs from Cl + 2 Cl2 by the rounding of f pdt (twice: once in each
    product, eps/2 |f pdt| each), of the two sums Cl', Cl2' (eps/2 |Cl'|, 2 x eps/2 |Cl2'|) and of the two sums the check itself
    forms (eps/2 |Cly| each): |d Cly| <= eps (|f pdt| + 0.5 |Cl'| + |Cl2'| + |Cly|), with |f pdt| = |Cl' - Cl| up to its own rounding.  The
    repair of term_fill_negative conserves Cly in the same way: dq is formed once, Cl + dq and Cl2 - dq 0.5 round once each, which
    adds eps (0.5 |Cl + dq| + |Cl2 - dq/2|) <= eps (|Cl| + 2 |Cl2| + |dq| ...); taken together as the bound below with a factor 2."""
    nx, ny, km = shape
    bd, st = RI.term_state(nx, ny, km, 6401 + km)
    got = run_term(lib, bd, st, dict(km=km, pdt=450.0, fill=fill))
    eps = np.finfo(float).eps
    before, after = st["cl"] + 2.0 * st["cl2"], got["cl"] + 2.0 * got["cl2"]
    mag = np.abs(got["cl"] - st["cl"]) + np.abs(got["cl"]) + np.abs(st["cl"]) + 2.0 * (np.abs(got["cl2"]) + np.abs(st["cl2"])) + np.abs(before)
    print("terminator conservation", shape, fill, "max |d Cly| / bound", float(np.max(np.abs(after - before) / (2.0 * eps * mag))))
    assert np.all(np.abs(after - before) <= 2.0 * eps * mag)
    assert not np.array_equal(got["cl"], st["cl"])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    c, bd, st = generic_case((12, 9, 12), "cond", hydrostatic=False, seed=6501)
    pr = RI.params_of(c)
    ctx = Context(P.make_grid(bd, False), 12, lib=lib)
    try:
        d = upload(ctx, st)
        refused = H.refusals(functools.partial(call_lib, ctx), d, pr)

        ctx.reed_ready = 0                       # (the wrapper would upload the gridstruct's on first use)
        refused("no Reed table")
        refused("reed_test", call=lambda: ctx.grid_upload_reed(3, st["lat"]))
        ctx.grid_upload_reed(1, st["lat"])
        refused("uploaded for reed_test = 1")
        ctx.grid_upload_reed(0, st["lat"])
        for n in ("delp", "pt", "ua", "va", "q", "pe", "peln", "phis", "u_dt", "v_dt", "t_dt", "q_dt", "rain"):
            refused("null", drop=(n,))
        refused("delz", drop=("delz",))
        refused("pdt", dict(pr, pdt=0.0))
        refused("pdt", dict(pr, pdt=-225.0))
        refused("reed_test", dict(pr, reed_test=3))
        refused("reed_test", dict(pr, reed_test=-1))
        cl = ctx.from_host(np.zeros(bd.shape("A", 12), order="F"))
        cl2 = ctx.from_host(np.zeros(bd.shape("A", 12), order="F"))
        ctx.terminator_ready = True
        refused("no k1 plane", call=lambda: ctx.terminator_advance(12, 225.0, cl, cl2))
        ctx.grid_upload_terminator(st["agrid"])
        refused("null", call=lambda: ctx.terminator_advance(12, 225.0, None, cl2))
        refused("null", call=lambda: ctx.terminator_advance(12, 225.0, cl, None))
        refused("same plane", call=lambda: ctx.terminator_advance(12, 225.0, cl, cl))
        refused("km", call=lambda: ctx.terminator_advance(0, 225.0, cl, cl2))
        refused("pdt", call=lambda: ctx.terminator_advance(12, 0.0, cl, cl2))
        H.assert_nothing_written(d, st, DEVICE)
        assert not cl.download().any() and not cl2.download().any()
        # npz < 1 cannot be reached: fv3_create refuses such a domain.  NOT refused: delz left out when hydrostatic
        call_lib(ctx, dict(d, delz=None), dict(pr, hydrostatic=True))
    finally:
        ctx.close()


# ---- six faces as one group ------------------------------------------------------------------------------------------------------
def check_six_faces(lib, flags, npx=13, npz=12):
    """the six C12 faces as one fv3_group: the bits of six single launches, and ONE merged launch; the terminator likewise"""
    import cubed_common as CC
    cs, gs = CC.sphere(npx)
    n = npx - 1
    sts, tsts = [], []
    for t in range(6):
        c, bd, st = generic_case((n, n, npz), flags, hydrostatic=bool(t % 2), reed_test=1, seed=6601 + t)
        sts.append(st)
        tsts.append(RI.term_state(n, n, npz, 6651 + t)[1])
    pr = RI.params_of(dict(c, hydrostatic=False))
    alone = [run_lib(lib, bd, st, pr, fresh=bool(t % 2)) for t, st in enumerate(sts)]
    talone = [run_term(lib, bd, st, dict(km=npz, pdt=225.0, fill=True)) for st in tsts]
    def prepare(mctx):
        for cx, st, tst in zip(mctx.ctxs, sts, tsts):
            cx.grid_upload_reed(1, st["lat"], consts=pr["consts"])
            cx.grid_upload_terminator(tst["agrid"], RI.PI)

    def terminator(mctx):
        cl, cl2 = (mctx.from_host([st[name] for st in tsts]) for name in ("cl", "cl2"))
        H.merged_once(mctx, "terminator_advance", lambda: mctx.terminator_advance(npz, 225.0, cl, cl2, term_fill_negative=True))
        for name, a in (("cl", cl), ("cl2", cl2)):
            got = a.download()
            for t in range(6):
                assert same_bits(got[t], talone[t][name]), f"face {t + 1} {name}"
    for fresh in (False, True):      # fresh is one flag of the group's call: the faces run alone with it are compared
        H.six_faces(lib, gs, npz, sts, DEVICE, lambda mctx, d: call_lib(mctx, d, pr, fresh), alone, prepare, "reed_sim_phys",
                    faces=[t for t in range(6) if bool(t % 2) == fresh], then=None if fresh else terminator)


# ---- the memory contract -----------------------------------------------------------------------------------------------------------
def check_contract(lib, shape, flags):
    """meant to run under memory_contract.run_case (every device array between guard bands, FV3_MI355X_POISON=1, so the six coefficient
    planes of the solve start every call as the pattern): the layouts between their bands; with fresh the outputs prefilled with
    the pattern; inputs and halos bit-unchanged; a call made after an fv3_fv_update_phys and a terminator call in the same context
    gives the bits of a fresh context"""
    import parity_update_phys as UP
    c, bd, st = generic_case(shape, flags, hydrostatic=False, reed_test=1, seed=6701)
    km = shape[2]
    pr = RI.params_of(c)
    ref, cnt = run_checker(bd, st, pr)
    first = run_lib(lib, bd, st, pr)
    worst = compare(bd, st, first, ref, c)
    check_fresh(lib, shape, flags, reed_test=1)
    ctx = Context(P.make_grid(bd, False), km, lib=lib)
    try:
        upr, _, ust = UP.generic_case(shape, True, True, 6, seed=6703)
        ud = UP.upload(ctx, ust)
        UP.call_lib(ctx, ud, upr)
        tbd, tst = RI.term_state(shape[0], shape[1], km, 6704)
        tref = {n: tst[n].copy(order="F") for n in ("cl", "cl2")}
        R.terminator_advance(225.0, True, R.term_k1(tst["agrid"], RI.PI), tref["cl"], tref["cl2"])
        term_compare("terminator", run_term(lib, tbd, tst, dict(km=km, pdt=225.0, fill=True), ctx=ctx), tref)
        again = run_lib(lib, bd, st, pr, ctx=ctx)
        other = run_lib(lib, bd, st, dict(pr, reed_alt_mxg=not pr["reed_alt_mxg"]), ctx=ctx)      # another instantiation in between
        assert np.array_equal(other["t_dt"], first["t_dt"]) == (km == 1 or pr["reed_cond_only"])      # (no interface, no solve: the same bits)
        third = run_lib(lib, bd, st, pr, ctx=ctx)
    finally:
        ctx.close()
    H.same_as_fresh_context(DEVICE, first, again, "fv3_fv_update_phys")
    H.same_as_fresh_context(DEVICE, first, third, "another branch set")
    return max(worst.values())


# ---- the Python host: FvDynamics.reed_sim_phys -------------------------------------------------------------------------------------
def check_host(lib, where, flags="cond", reed_test=1):
    """FvDynamics.reed_sim_phys on the state a step of parity_negadj.run_tile / run_sphere leaves (24 x 16 x 10 on the doubly periodic
    tile, C12 L8, moist, nq = 7, nonhydrostatic) against restatement-then-fv_update_phys, in the reference's order: the restatement of
    the column loop on zeroed tendencies, the restatement of the terminator on the last two tracers, the restatement of the column
    routine of fv_update_phys with that q_dt, a real exchange of u_dt, v_dt and the restatement of update_dwinds_phys"""
    import parity_update_phys as UP
    fields = ("u", "v", "w", "delp", "pt", "ua", "va", "q", "delz", "pe", "peln", "pk", "ps", "pkz", "phis")
    cnd, only, alt = RI.FLAGS[flags]

    def call_method(fv, bdt):
        for c in (fv.ctx.ctxs if hasattr(fv.ctx, "ctxs") else [fv.ctx]):
            c.grid_upload_reed(reed_test, consts=dict(fv.neg_adj_consts, radius=fv.radius))
        fv.reed_sim_phys(bdt, reed_test=reed_test, do_reed_cond=cnd, reed_cond_only=only, reed_alt_mxg=alt, terminator=(fv.nq - 1, fv.nq),
                         term_fill_negative=True)

    base, kept = H.host_step(lib, where, fields, ("u_srf", "v_srf", "t_dt", "q_dt", "rain"), call_method)
    bd = base["bd"]
    before, after = kept["before"], kept["after"]
    nf = len(before["pt"])
    npz = before["pt"][0].shape[2]
    nq = before["q"][0].shape[3]
    upr = H.update_phys_params(kept, nq)
    k = dict(RI.CONSTS, **{n: v for n, v in kept["consts"].items() if n in RI.CONSTS}, radius=kept["radius"])
    rpr = dict(pdt=kept["bdt"], hydrostatic=kept["hyd"], reed_test=reed_test, do_reed_cond=cnd, reed_cond_only=only, reed_alt_mxg=alt, consts=k)
    r = (bd.is_, bd.ie, bd.js, bd.je)
    tol = 10.0 * max(v for (f, _), v in MEASURED.items() if f == flags)
    ref = []
    for t in range(nf):
        s = {n: before[n][t].copy(order="F") for n in fields}
        q4 = s["q"]
        s.update(t_dt=np.zeros((bd.nx, bd.ny, npz), order="F"), u_dt=bd.zeros("A", npz), v_dt=bd.zeros("A", npz), q_dt=np.zeros((bd.nx, bd.ny, npz), order="F"),
                 rain=np.zeros((bd.nx, bd.ny), order="F"), lat=np.asfortranarray(bd.view(kept["agrids"][t][..., 1], "A", *r)), q=np.asfortranarray(q4[..., 0]))
        R.reed_wrapper(bd, npz, rpr, s)
        for n in ("t_dt", "q_dt") + (("rain",) if cnd else ()):
            assert s[n].any(), n
            P.assert_close(f"face {t + 1} {n}", after[n][t][..., 0] if n == "q_dt" else after[n][t], s[n], tol)
        assert not after["q_dt"][t][..., 1:].any(), "q_dt: a plane other than sphum was written"
        cl, cl2 = (np.asfortranarray(q4[..., m]) for m in (nq - 2, nq - 1))
        R.terminator_advance(kept["bdt"], True, R.term_k1(kept["agrids"][t], k["pi"]), cl, cl2)
        q4[..., nq - 2], q4[..., nq - 1] = cl, cl2
        qd4 = np.zeros((bd.nx, bd.ny, npz, nq), order="F")
        qd4[..., 0] = s["q_dt"]
        s.update(q=q4, q_dt=qd4)
        ref.append(s)
    H.update_phys_reference(where, base, kept, ref, upr)
    worst = 0.0
    for t in range(nf):
        rows = [("u", "U", (bd.is_, bd.ie, bd.js, bd.je + 1)), ("v", "V", (bd.is_, bd.ie + 1, bd.js, bd.je)), ("pt", "A", r), ("ua", "A", r),
                ("va", "A", r), ("q", "A", r), ("delp", "A", r)]
        for n, kind, rg in rows:
            a, b = bd.view(after[n][t], kind, *rg), bd.view(ref[t][n], kind, *rg)
            assert np.any(b != bd.view(before[n][t], kind, *rg)), n
            worst = max(worst, P.assert_close(f"face {t + 1} {n}", a, b, P.TOL))
        for m in (nq - 2, nq - 1):      # the terminator ran before fv_update_phys: the two tracers changed beyond the mass adjustment
            assert np.any(compute(bd, after["q"][t][..., m]) != compute(bd, before["q"][t][..., m]))
        P.assert_close(f"face {t + 1} pe", after["pe"][t][1:-1, :, 1:-1], ref[t]["pe"][1:-1, :, 1:-1], P.TOL)
        for n in ("peln", "pk"):
            P.assert_close(f"face {t + 1} {n}", after[n][t], ref[t][n], UP.BOUND[n])
    return worst


def check_chain(lib):
    """the chained golden -- the reference's column loop with reed_sim_physics inside it, followed by its whole fv_update_phys with
    moist_phys true and q_dt present -- through FvDynamics.reed_sim_phys on the doubly periodic tile: the recorded state is laid into
    the resident fields of a hydrostatic FvDynamics (the constants of the recipe's constants_mod), one call, and the fields the
    reference wrote are compared on the ranges it wrote.  It holds the order inside the method.  The four tendencies and rain at the
    bounds of their flag set; what fv_update_phys forms from them inherits their last bits: P.TOL, and peln, pk, pkz at
    fv_update_phys' own bounds where those are wider."""
    import held_suarez_inputs as HI
    import parity_update_phys as UP
    from gfdl_atmos_cubed_sphere_amd.dyn_core import DynFlags
    from gfdl_atmos_cubed_sphere_amd.fv_dynamics import FvDynamics
    c = RI.CHAIN
    bd, st = RI.chain_inputs()
    g = golden("chain")
    assert str(g["chain|sha"]) == RI.checksum(st), "chain: the inputs formed from the seed are not those the golden was recorded with"
    km, nq = c["km"], c["nq"]
    ak, bk = HI.eta_levels(km)
    fl = DynFlags(hydrostatic=True, ptop=c["ptop"], akap=2.0 / 7.0, grav=9.80, rdgas=287.04, cp_air=287.04 / (2.0 / 7.0))
    ctx = Context(P.make_grid(bd, False), km, lib=lib)
    try:
        fv = FvDynamics(ctx, fl, ak, bk, nq=nq, radius=RI.CONSTS["radius"], moist=dict(nwat=1, sphum=1), moist_phys=True)
        d = H.lay_state(fv, ctx, st, ("u", "v", "w", "delp", "pt", "ua", "va", "q", "ps", "pe", "peln", "pk", "pkz", "phis", "rain"))
        ctx.grid_upload_reed(c["reed_test"], st["lat"], consts=RI.CONSTS)
        fv.reed_sim_phys(c["pdt"], reed_test=c["reed_test"], do_reed_cond=c["do_reed_cond"], reed_cond_only=c["reed_cond_only"],
                         reed_alt_mxg=c["reed_alt_mxg"], consts=RI.CONSTS)
        got = {n: d[n].download() for n in RI.CHAIN_OUT}
    finally:
        ctx.close()
    fam = family(c)
    for n in RI.CHAIN_OUT:
        a, b = H.written_range(bd, n, got[n], ("pt", "ua", "va", "ps", "delp", "q")), g[f"chain|out|{n}"]
        if n in ("t_dt", "q_dt", "rain"):
            a1, b1 = (a[..., 0], b[..., 0]) if n == "q_dt" else (a, b)
            P.assert_close(f"chain {n}", a1, b1, bound(fam, n))
            if n == "q_dt":
                assert not a[..., 1:].any() and not b[..., 1:].any()
        elif n in ("u_dt", "v_dt"):
            P.assert_close(f"chain {n}", a, b, bound(fam, n))
        else:
            P.assert_close(f"chain {n}", a, b, max(P.TOL, UP.BOUND.get(n, 0.0)))
