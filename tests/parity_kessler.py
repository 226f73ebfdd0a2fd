"""Check bodies of the Kessler warm-rain microphysics -- fv3_k_warm_rain, fv3_qs_wat_init (driver/solo/fv_phys.F90:1992-2291,
driver/solo/qs_tables.F90) and FvDynamics.k_warm_rain -- shared by tests/test_kessler_hostemu.py (CPU) and tests/test_kessler_gpu.py,
and by the contract tests of both: the library against the outputs of the reference's compiled Fortran
(tests/golden/kessler/*.npz), against the numpy restatement tests/ref_kessler.py, and properties that need no restatement.

Bounds.  table_w and des_w are bit-identical with the reference's compiler.  ua, va, w, u_dt, v_dt are bit-identical where the
routine adds nothing to them (K_sedi_transport off; w without do_K_sedi_w) -- u_dt, v_dt as the reference leaves them, incoming
value + 0.  pe is bit-identical with the running sum of the library's own delp.  Every other field passes through a log, an exp or
a power and none is claimed bit-identical.  The bound is measured on the REFERENCE side alone: `python
tests/golden/make_kessler_golden.py --measure` perturbs every log, exp, power and sqrt of the restatement by one unit in the last
place (the power: 1 + |y ln x| units), seeded signs, 8 seeds, every recorded case, and takes per output field and flag set the
worst relative RMS change -- MEASURED below.  The tests assert TEN times that: one order covers the amplification through
K_cycle cycles and the downward recurrences, which the perturbation measures but does not bound.  A figure measured as zero is
asserted bit-identical.  The library's actual differences (CPU harness against the compiled reference), printed by --measure
beside them: LIBRARY below.  The library is not used to set its own bound."""
from __future__ import annotations

import functools

import numpy as np

import kessler_inputs as KI
import parity_common as P
import parity_phys as H
import ref_kessler as R
from gfdl_atmos_cubed_sphere_amd.lib import Context
from parity_phys import compute, same_bits as same  # noqa: F401
DEVICE = KI.STATE
FIELDS = ("pt", "delp", "q_sphum", "q_liq", "q_rain", "rain", "ps", "peln", "pk", "ua", "va", "w", "u_dt", "v_dt")
WINDS = ("ua", "va", "w", "u_dt", "v_dt")
# (flag set, field) -> relative RMS, perturbed restatement against the restatement, worst of 8 seeds x the recorded cases
MEASURED = {("heat", "delp"): 4.108e-17, ("heat", "peln"): 1.688e-16, ("heat", "pk"): 5.948e-16, ("heat", "ps"): 3.948e-17,
            ("heat", "pt"): 4.515e-16, ("heat", "q_liq"): 2.458e-14, ("heat", "q_rain"): 1.809e-14, ("heat", "q_sphum"): 3.740e-15,
            ("heat", "rain"): 5.829e-14, ("heat", "u_dt"): 0.0, ("heat", "ua"): 0.0, ("heat", "v_dt"): 0.0, ("heat", "va"): 0.0,
            ("heat", "w"): 0.0, ("none", "delp"): 4.902e-17, ("none", "peln"): 1.687e-16, ("none", "pk"): 6.129e-16,
            ("none", "ps"): 3.954e-17, ("none", "pt"): 5.387e-16, ("none", "q_liq"): 2.451e-14, ("none", "q_rain"): 2.144e-14,
            ("none", "q_sphum"): 4.452e-15, ("none", "rain"): 7.092e-14, ("none", "u_dt"): 0.0, ("none", "ua"): 0.0, ("none", "v_dt"): 0.0,
            ("none", "va"): 0.0, ("none", "w"): 0.0, ("tr", "delp"): 6.166e-17, ("tr", "peln"): 1.686e-16, ("tr", "pk"): 5.923e-16,
            ("tr", "ps"): 4.274e-17, ("tr", "pt"): 3.357e-16, ("tr", "q_liq"): 1.973e-14, ("tr", "q_rain"): 1.778e-14,
            ("tr", "q_sphum"): 3.148e-15, ("tr", "rain"): 5.641e-14, ("tr", "u_dt"): 1.170e-14, ("tr", "ua"): 3.465e-17,
            ("tr", "v_dt"): 1.074e-14, ("tr", "va"): 3.552e-17, ("tr", "w"): 0.0, ("trw", "delp"): 3.880e-17, ("trw", "peln"): 1.691e-16,
            ("trw", "pk"): 6.246e-16, ("trw", "ps"): 4.253e-17, ("trw", "pt"): 3.329e-16, ("trw", "q_liq"): 2.138e-14,
            ("trw", "q_rain"): 1.000e-14, ("trw", "q_sphum"): 2.804e-15, ("trw", "rain"): 5.498e-14, ("trw", "u_dt"): 1.483e-14,
            ("trw", "ua"): 3.566e-17, ("trw", "v_dt"): 1.070e-14, ("trw", "va"): 3.487e-17, ("trw", "w"): 9.559e-17,
            ("trwh", "delp"): 4.805e-17, ("trwh", "peln"): 1.686e-16, ("trwh", "pk"): 5.945e-16, ("trwh", "ps"): 4.269e-17,
            ("trwh", "pt"): 3.291e-16, ("trwh", "q_liq"): 1.472e-14, ("trwh", "q_rain"): 1.118e-14, ("trwh", "q_sphum"): 3.142e-15,
            ("trwh", "rain"): 5.426e-14, ("trwh", "u_dt"): 9.706e-15, ("trwh", "ua"): 6.167e-17, ("trwh", "v_dt"): 1.265e-14,
            ("trwh", "va"): 3.631e-17, ("trwh", "w"): 1.054e-16}
# the same keys -> the library of the CPU harness against the compiled reference, worst recorded case (not a bound: for the reader)
LIBRARY = {("heat", "delp"): 7.741e-18, ("heat", "peln"): 3.372e-17, ("heat", "pk"): 1.415e-16, ("heat", "ps"): 0.0,
           ("heat", "pt"): 3.904e-17, ("heat", "q_liq"): 1.072e-15, ("heat", "q_rain"): 3.080e-16, ("heat", "q_sphum"): 1.808e-16,
           ("heat", "rain"): 8.878e-15, ("heat", "u_dt"): 0.0, ("heat", "ua"): 0.0, ("heat", "v_dt"): 0.0, ("heat", "va"): 0.0,
           ("heat", "w"): 0.0, ("none", "delp"): 9.603e-18, ("none", "peln"): 2.340e-17, ("none", "pk"): 9.986e-17, ("none", "ps"): 0.0,
           ("none", "pt"): 1.618e-17, ("none", "q_liq"): 3.719e-16, ("none", "q_rain"): 9.512e-16, ("none", "q_sphum"): 3.553e-17,
           ("none", "rain"): 2.354e-14, ("none", "u_dt"): 0.0, ("none", "ua"): 0.0, ("none", "v_dt"): 0.0, ("none", "va"): 0.0,
           ("none", "w"): 0.0, ("tr", "delp"): 2.400e-18, ("tr", "peln"): 2.551e-17, ("tr", "pk"): 1.266e-16, ("tr", "ps"): 0.0,
           ("tr", "pt"): 3.609e-18, ("tr", "q_liq"): 1.427e-16, ("tr", "q_rain"): 2.732e-16, ("tr", "q_sphum"): 3.032e-17,
           ("tr", "rain"): 1.289e-14, ("tr", "u_dt"): 4.404e-15, ("tr", "ua"): 1.062e-17, ("tr", "v_dt"): 2.405e-15,
           ("tr", "va"): 1.290e-17, ("tr", "w"): 0.0, ("trw", "delp"): 9.647e-18, ("trw", "peln"): 2.919e-17, ("trw", "pk"): 1.017e-16,
           ("trw", "ps"): 0.0, ("trw", "pt"): 1.611e-17, ("trw", "q_liq"): 1.161e-16, ("trw", "q_rain"): 1.901e-16,
           ("trw", "q_sphum"): 2.009e-17, ("trw", "rain"): 2.378e-14, ("trw", "u_dt"): 2.418e-15, ("trw", "ua"): 9.902e-18,
           ("trw", "v_dt"): 2.411e-15, ("trw", "va"): 1.466e-17, ("trw", "w"): 3.291e-17, ("trwh", "delp"): 6.813e-18,
           ("trwh", "peln"): 2.919e-17, ("trwh", "pk"): 1.313e-16, ("trwh", "ps"): 0.0, ("trwh", "pt"): 3.610e-17,
           ("trwh", "q_liq"): 8.537e-16, ("trwh", "q_rain"): 4.472e-16, ("trwh", "q_sphum"): 1.401e-16, ("trwh", "rain"): 6.904e-15,
           ("trwh", "u_dt"): 1.650e-15, ("trwh", "ua"): 1.107e-17, ("trwh", "v_dt"): 2.130e-15, ("trwh", "va"): 1.311e-17,
           ("trwh", "w"): 3.611e-17}


def bound(fam, n):
    return 10.0 * MEASURED[(fam, n)]


def stored(c):
    """the fields the recorder keeps of a case: the winds only where the routine adds to them"""
    tr, sw, _ = KI.FLAGS[c["flags"]]
    return tuple(n for n in FIELDS if n not in WINDS or (tr and (n != "w" or sw)))


def parts_of(c):
    return ("",) if c["km"] <= 12 else ("_a", "_b", "_c")


golden = functools.partial(H.golden, "kessler/", slashes=True)


def golden_of(c):
    g = {}
    for s in parts_of(c):
        g.update(golden(c["group"] + s))
    return g


def call_lib(ctx, d, pr):
    ctx.k_warm_rain(pr["pdt"], d["ua"], d["va"], d["w"], d["u_dt"], d["v_dt"], d["q"], d["pt"], d["delp"], d["delz"], d["pe"], d["peln"], d["pk"],
                    d["ps"], d["rain"], pr["nq"], sphum=pr["sphum"], liq_wat=pr["liq_wat"], rainwat=pr["rainwat"], K_cycle=pr["K_cycle"],
                    K_sedi_transport=pr["K_sedi_transport"], do_K_sedi_w=pr["do_K_sedi_w"], do_K_sedi_heat=pr["do_K_sedi_heat"],
                    hydrostatic=pr["hydrostatic"], moist_kappa=pr["moist_kappa"], consts=pr["consts"])


def upload(ctx, st):
    return H.upload(ctx, st, DEVICE)


def download(d):
    return H.download(d, DEVICE)


def run_lib(lib, bd, st, pr, ctx=None):
    """fv3_k_warm_rain on a copy of the state -> {field: whole array}"""
    with H.own_or_borrowed(lib, bd, st["pt"].shape[2], ctx) as ctx:
        ctx.qs_wat_init(pr["consts"])
        d = upload(ctx, st)
        call_lib(ctx, d, pr)
        return download(d)


def run_checker(bd, st, pr, M=None):
    o = {n: st[n].copy(order="F") for n in DEVICE}
    cnt = R.k_warm_rain(bd, st["pt"].shape[2], pr, o, M=M)
    return o, cnt


def views(bd, pr, o):
    """{field of FIELDS: the range the routine writes}"""
    q = compute(bd, o["q"])
    v = {n: compute(bd, o[n]) for n in ("pt", "delp", "ps", "ua", "va", "w", "u_dt", "v_dt")}
    v.update(q_sphum=q[..., pr["sphum"] - 1], q_liq=q[..., pr["liq_wat"] - 1], q_rain=q[..., pr["rainwat"] - 1], rain=o["rain"],
             peln=o["peln"][:, 1:, :], pk=o["pk"][:, :, 1:])
    return v


def assert_untouched(bd, st, got, pr, what=""):
    """halos, the other tracers, level 1 of pe, peln, pk, the ring of pe and delz keep their bits; pe is the running sum of delp"""
    halo = H.halo_mask(bd, st["pt"].shape)
    for n in ("pt", "delp", "ua", "va", "w", "u_dt", "v_dt"):
        assert same(got[n][halo], st[n][halo]), f"{what}{n}: the halo was written"
    h2 = H.halo_mask(bd, st["ps"].shape)
    assert same(got["ps"][h2], st["ps"][h2]), f"{what}ps: the halo was written"
    for iq in range(st["q"].shape[3]):
        if iq + 1 in (pr["sphum"], pr["liq_wat"], pr["rainwat"]):
            assert same(got["q"][..., iq][halo], st["q"][..., iq][halo]), f"{what}q({iq + 1}): the halo was written"
        else:
            assert same(got["q"][..., iq], st["q"][..., iq]), f"{what}q({iq + 1}): a tracer the routine does not read was written"
    assert same(got["delz"], st["delz"]), f"{what}delz was written"
    assert same(got["peln"][:, 0, :], st["peln"][:, 0, :]) and same(got["pk"][:, :, 0], st["pk"][:, :, 0]), f"{what}level 1 of peln / pk was written"
    ring = np.ones(st["pe"].shape, dtype=bool)
    ring[1:-1, 1:, 1:-1] = False
    assert same(got["pe"][ring], st["pe"][ring]), f"{what}pe: the ring or level 1 was written"
    pe = got["pe"][1:-1, 0, 1:-1].copy()
    dp = compute(bd, got["delp"])
    for k in range(dp.shape[2]):
        pe = pe + dp[:, :, k]
        assert same(got["pe"][1:-1, k + 1, 1:-1], pe), f"{what}pe({k + 2}) is not the running sum of the library's delp"
    assert same(compute(bd, got["ps"]), pe), f"{what}ps is not pe(km+1)"


def compare(bd, st, got, ref, c, pr, what=""):
    """what the routine may not touch is untouched, each output field at its bound -> {field: relative RMS}"""
    fam = c["flags"]
    assert_untouched(bd, st, got, pr, what)
    a_, b_ = views(bd, pr, got), views(bd, pr, ref)
    out = {}
    for n in FIELDS:
        out[n] = float(H.assert_bounded(f"{what}{n} ({fam})", a_[n], b_[n], bound(fam, n)))
    return out


# ---- the recorded outputs of the reference's compiled Fortran ----------------------------------------------------------------------
def golden_case(name):
    """-> (case, bd, inputs, parameters, the reference's outputs as whole arrays)"""
    c = KI.CASES[name]
    bd, st = KI.case_inputs(name)
    pr = KI.params_of(c)
    g = golden_of(c)
    assert str(g[f"{name}|sha"]) == KI.checksum(st), f"{name}: the inputs formed from the seed are not those the golden was recorded with"
    ref = {n: st[n].copy(order="F") for n in DEVICE}
    v = views(bd, pr, ref)
    for n in stored(c):
        v[n][...] = g[f"{name}|out|{n}"]
    for n in ("u_dt", "v_dt"):      # where nothing is added the reference leaves u_dt + 0.
        if n not in stored(c):
            v[n][...] = v[n] + 0.0
    pe = ref["pe"]
    dp = compute(bd, ref["delp"])
    for k in range(c["km"]):
        pe[1:-1, k + 1, 1:-1] = pe[1:-1, k, 1:-1] + dp[:, :, k]
    return c, bd, st, pr, ref


def check_checker_against_golden(name):
    """the restatement against the compiled reference, at the library's bounds -> the branch counts"""
    c, bd, st, pr, ref = golden_case(name)
    got, cnt = run_checker(bd, st, pr)
    compare(bd, st, got, ref, c, pr, what=f"{name} restatement ")
    return cnt


def check_lib_against_golden(lib, name):
    """the library against the recorded outputs with nothing in between -> {field: relative RMS}"""
    c, bd, st, pr, ref = golden_case(name)
    got = run_lib(lib, bd, st, pr)
    rms = lambda n: float(P.rel_rms(views(bd, pr, got)[n], views(bd, pr, ref)[n]))      # noqa: E731
    print(name, {n: rms(n) for n in FIELDS})
    return compare(bd, st, got, ref, c, pr, what=f"{name} ")


def lib_table(lib, consts=None):
    bd = KI.Bounds(1, 4, 1, 4)
    with H.own_or_borrowed(lib, bd, 1) as ctx:
        ctx.qs_wat_init(consts or KI.CONSTS)
        return ctx.qs_wat_download()


def check_table(lib):
    """table_w and des_w against the reference's compiled qs_tables.F90, bit for bit"""
    g = golden("table")
    tw, dw = lib_table(lib)
    for n, a in (("table_w", tw), ("des_w", dw)):
        b = g[n]
        assert a.shape == b.shape == (R.QS_LENGTH,)
        assert same(a, b), \
            f"{n}: not the compiler's, max relative difference {np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)):.3e}"


# ---- shapes with several blocks, against the restatement ---------------------------------------------------------------------------
def generic_case(shape, flags, hydrostatic=False, moist_kappa=False, K_cycle=1, pdt=30.0, seed=8101, tracers=(1, 2, 3), nq=KI.NQ):
    nx, ny, km = shape
    c = dict(flags=flags, km=km, hydrostatic=hydrostatic, moist_kappa=moist_kappa, K_cycle=K_cycle, pdt=pdt, tracers=tracers, nq=nq)
    bd, st = KI.state(nx, ny, km, seed + km, hydrostatic=hydrostatic, nq=nq, tracers=tracers)
    return c, bd, st


def check_against_checker(lib, shape, flags, hydrostatic=False, moist_kappa=False, K_cycle=1):
    """a shape with more than one block of 256 columns and a tail block, against the restatement"""
    c, bd, st = generic_case(shape, flags, hydrostatic, moist_kappa, K_cycle)
    pr = KI.params_of(c)
    ref, cnt = run_checker(bd, st, pr)
    return compare(bd, st, run_lib(lib, bd, st, pr), ref, c, pr)


def check_conservation(lib, shape, flags, K_cycle=3, moist_kappa=True):
    """drym of every level is bit-unchanged by construction (:2065 forms it, :2168 adds the water back to it): the dry mass the
    library's outputs imply, delp (1 - q1 - q2 - q3), against the restatement's drym, at the bound of delp (the subtraction of the
    three products rounds).  Total water of the column plus rain * grav: the routine moves water between the three species and
    down the column, and what leaves the bottom is rain -- but the clamps of :2073-2079 put water in (their differences are
    added at :2164-2166, not taken out) and max(0., m1) drops a negative flux, so the budget does not close on its own in the
    reference either; the check is the library's budget against the restatement's, at the wider of the measured bounds of delp
    and rain."""
    c, bd, st = generic_case(shape, flags, hydrostatic=False, moist_kappa=moist_kappa, K_cycle=K_cycle, seed=8201)
    pr = KI.params_of(c)
    ref, _ = run_checker(bd, st, pr)
    got = run_lib(lib, bd, st, pr)
    g, r = views(bd, pr, got), views(bd, pr, ref)
    dry = lambda v: v["delp"] * (1.0 - (v["q_sphum"] + v["q_liq"] + v["q_rain"]))      # noqa: E731
    tol = bound(c["flags"], "delp")
    e = P.rel_rms(dry(g), ref["drym"])
    print("dry mass against the restatement's drym", float(e), "the restatement's own", float(P.rel_rms(dry(r), ref["drym"])))
    assert e <= max(tol, 4.0 * np.finfo(float).eps)
    water = lambda v: np.sum(v["delp"] * (v["q_sphum"] + v["q_liq"] + v["q_rain"]), axis=2) + v["rain"] * pr["consts"]["grav"]      # noqa: E731
    e = P.rel_rms(water(g), water(r))
    print("column water + rain * grav against the restatement's", float(e))
    assert e <= max(tol, bound(c["flags"], "rain"))
    return float(e)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    c, bd, st = generic_case((12, 9, 12), "trwh", hydrostatic=False, seed=8501)
    pr = KI.params_of(c)
    ctx = Context(P.make_grid(bd, False), 12, lib=lib)
    ready = lambda k: tuple(float(dict(KI.CONSTS, **k)[n]) for n in ("rdgas", "rvgas", "cp_air", "cp_vapor", "hlv", "c_liq", "grav", "kappa"))      # noqa: E731
    try:
        d = upload(ctx, st)
        refused = H.refusals(functools.partial(call_lib, ctx), d, pr)

        ctx.qs_wat_ready = ready({})                 # (the wrapper would form the table on first use)
        refused("no qs_wat table")
        refused("no table", call=ctx.qs_wat_download)
        ctx.qs_wat_init(KI.CONSTS)
        other = dict(KI.CONSTS, hlv=2.4e6)
        ctx.qs_wat_ready = ready(other)
        refused("other constants", dict(pr, consts=other))
        ctx.qs_wat_ready = ready({})
        for n in ("ua", "va", "u_dt", "v_dt", "q", "pt", "delp", "pe", "peln", "pk", "ps", "rain"):
            refused("null", drop=(n,))
        refused("delz", drop=("delz",))
        refused("delz", dict(pr, hydrostatic=True), drop=("delz",))                      # do_K_sedi_heat reads it either way
        refused("delz", dict(pr, do_K_sedi_heat=False), drop=("delz",))                  # not hydrostatic
        refused("null w", drop=("w",))
        refused("pdt", dict(pr, pdt=0.0))
        refused("pdt", dict(pr, pdt=-30.0))
        refused("K_cycle", dict(pr, K_cycle=-1))
        refused("1..nq", dict(pr, sphum=0))
        refused("1..nq", dict(pr, rainwat=pr["nq"] + 1))
        refused("not distinct", dict(pr, liq_wat=pr["sphum"]))
        refused("not distinct", dict(pr, rainwat=pr["liq_wat"]))
        refused("grav", dict(pr, consts=dict(KI.CONSTS, grav=0.0)), call=lambda: ctx.qs_wat_init(dict(KI.CONSTS, grav=0.0)))
        H.assert_nothing_written(d, st, DEVICE)
        # npz < 1 cannot be reached: fv3_create refuses such a domain.  NOT refused: w left out without do_K_sedi_w, and delz left
        # out when hydrostatic without do_K_sedi_heat -- and then w keeps its bits
        call_lib(ctx, dict(d, w=None, delz=None), dict(pr, hydrostatic=True, do_K_sedi_w=False, do_K_sedi_heat=False))
        assert same(d["w"].download(), st["w"])
    finally:
        ctx.close()


# ---- six faces as one group ------------------------------------------------------------------------------------------------------
def check_six_faces(lib, flags, K_cycle=2, npx=13, npz=12):
    """the six C12 faces as one fv3_group: the bits of six single launches, and ONE merged launch"""
    import cubed_common as CC
    cs, gs = CC.sphere(npx)
    n = npx - 1
    sts = []
    for t in range(6):
        c, bd, st = generic_case((n, n, npz), flags, hydrostatic=False, moist_kappa=True, K_cycle=K_cycle, seed=8601 + t)
        sts.append(st)
    pr = KI.params_of(c)
    alone = [run_lib(lib, bd, st, pr) for st in sts]
    def prepare(mctx):
        for cx in mctx.ctxs:
            cx.qs_wat_init(pr["consts"])
    H.six_faces(lib, gs, npz, sts, DEVICE, lambda mctx, d: call_lib(mctx, d, pr), alone, prepare, "k_warm_rain")


# ---- the memory contract -----------------------------------------------------------------------------------------------------------
def check_contract(lib, shape, flags, K_cycle=3):
    """meant to run under memory_contract.run_case (every device array between guard bands, FV3_MI355X_POISON=1, so the twelve planes
    that hold the state between cycles start every call as the pattern): the layouts between their bands; rain prefilled with the
    pattern and written in every cell; halos and the other tracer planes bit-unchanged; a call made after an fv3_fv_update_phys,
    a call with K_cycle = 1 (no work plane) and a call of another instantiation in the same context gives a fresh context's bits"""
    import memory_contract as MC
    import parity_update_phys as UP
    c, bd, st = generic_case(shape, flags, hydrostatic=False, moist_kappa=True, K_cycle=K_cycle, seed=8701)
    st = dict(st, rain=MC.pattern_array(st["rain"].shape))
    km = shape[2]
    pr = KI.params_of(c)
    ref, cnt = run_checker(bd, st, pr)
    first = run_lib(lib, bd, st, pr)
    worst = compare(bd, st, first, ref, c, pr)
    assert np.all(np.abs(first["rain"]) < 1.0e29), "rain: the pattern survives"
    for n in DEVICE:      # nothing of the poisoned work planes reaches an output
        assert np.all(np.isfinite(first[n])) and np.all(np.abs(first[n]) < 1.0e29), f"{n}: the pattern of a work plane reached it"
    ctx = Context(P.make_grid(bd, False), km, lib=lib)
    try:
        upr, _, ust = UP.generic_case(shape, True, True, 6, seed=8703)
        ud = UP.upload(ctx, ust)
        UP.call_lib(ctx, ud, upr)
        again = run_lib(lib, bd, st, pr, ctx=ctx)
        one = run_lib(lib, bd, st, dict(pr, K_cycle=1), ctx=ctx)
        other = run_lib(lib, bd, st, dict(pr, moist_kappa=False, K_sedi_transport=not pr["K_sedi_transport"], do_K_sedi_w=False), ctx=ctx)
        assert not np.array_equal(one["pt"], first["pt"]) and not np.array_equal(other["pt"], first["pt"])
        third = run_lib(lib, bd, st, pr, ctx=ctx)
    finally:
        ctx.close()
    H.same_as_fresh_context(DEVICE, first, again, "fv3_fv_update_phys")
    H.same_as_fresh_context(DEVICE, first, third, "another instantiation")
    return max(worst[n] / bound(c["flags"], n) for n in worst if bound(c["flags"], n) > 0.0)


# ---- the Python host: FvDynamics.k_warm_rain ---------------------------------------------------------------------------------------
def check_host(lib, where, flags="trw", K_cycle=2):
    """FvDynamics.k_warm_rain on the state a step of parity_negadj.run_tile / run_sphere leaves (24 x 16 x 10 on the doubly periodic
    tile, C12 L8, moist, nq = 7, nonhydrostatic) against restatement-then-fv_update_phys, in the reference's order: the restatement
    of K_warm_rain on zeroed u_dt, v_dt, and with K_sedi_transport the restatement of the column routine of fv_update_phys with
    zero t_dt, q_dt, a real exchange of u_dt, v_dt and the restatement of update_dwinds_phys"""
    import parity_update_phys as UP
    fields = ("u", "v", "w", "delp", "pt", "ua", "va", "q", "delz", "pe", "peln", "pk", "ps", "pkz", "phis")
    tr, sw, sh = KI.FLAGS[flags]
    base, kept = H.host_step(lib, where, fields, ("u_dt", "v_dt", "rain"),
                             lambda fv, bdt: fv.k_warm_rain(bdt, K_cycle=K_cycle, K_sedi_transport=tr, do_K_sedi_w=sw, do_K_sedi_heat=sh))
    bd = base["bd"]
    before, after = kept["before"], kept["after"]
    nf = len(before["pt"])
    npz = before["pt"][0].shape[2]
    nq = before["q"][0].shape[3]
    upr = H.update_phys_params(kept, nq)
    sp = upr["species"]
    k = dict(KI.CONSTS, **{n: v for n, v in kept["consts"].items() if n in KI.CONSTS})
    kpr = dict(pdt=kept["bdt"], K_cycle=K_cycle, K_sedi_transport=tr, do_K_sedi_w=sw, do_K_sedi_heat=sh, hydrostatic=kept["hyd"], moist_kappa=kept["mk"],
               nq=nq, sphum=1, liq_wat=sp["liq_wat"], rainwat=sp["rainwat"], consts=k)
    r = (bd.is_, bd.ie, bd.js, bd.je)
    ref = []
    for t in range(nf):
        s = {n: before[n][t].copy(order="F") for n in fields}
        s.update(u_dt=bd.zeros("A", npz), v_dt=bd.zeros("A", npz), rain=np.zeros((bd.nx, bd.ny), order="F"))
        R.k_warm_rain(bd, npz, kpr, s)
        assert s["rain"].any(), "no rain: the state is too dry a test"
        assert P.rel_rms(after["rain"][t], s["rain"]) <= bound(flags, "rain"), f"face {t + 1} rain"
        ref.append(s)
    if tr:      # only K_sedi_transport leaves u_dt, v_dt for fv_update_phys (with zero t_dt, q_dt)
        H.update_phys_reference(where, base, kept, ref, upr)
    worst = 0.0
    tol = {"pt": bound(flags, "pt"), "delp": bound(flags, "delp"), "q": max(bound(flags, n) for n in ("q_sphum", "q_liq", "q_rain")),
           "ua": max(P.TOL, bound(flags, "ua")), "va": max(P.TOL, bound(flags, "va")), "w": max(P.TOL, bound(flags, "w")),
           "u": max(P.TOL, bound(flags, "ua")), "v": max(P.TOL, bound(flags, "va"))}
    for t in range(nf):
        rows = [("pt", "A", r), ("ua", "A", r), ("va", "A", r), ("delp", "A", r), ("w", "A", r)]
        if tr:
            rows += [("u", "U", (bd.is_, bd.ie, bd.js, bd.je + 1)), ("v", "V", (bd.is_, bd.ie + 1, bd.js, bd.je))]
        for n, kind, rg in rows:
            a, b = bd.view(after[n][t], kind, *rg), bd.view(ref[t][n], kind, *rg)
            if n in ("pt", "delp") or (tr and (n != "w" or sw)):
                assert np.any(b != bd.view(before[n][t], kind, *rg)), n
            e = P.rel_rms(a, b)
            assert e <= tol[n], f"face {t + 1} {n}: rel-rms {e:.3e} > {tol[n]:.1e}"
            worst = max(worst, e / tol[n])
        for m, name in ((0, "q_sphum"), (sp["liq_wat"] - 1, "q_liq"), (sp["rainwat"] - 1, "q_rain")):
            a, b = compute(bd, after["q"][t][..., m]), compute(bd, ref[t]["q"][..., m])
            e = P.rel_rms(a, b)
            assert e <= bound(flags, name), f"face {t + 1} {name}: rel-rms {e:.3e} > {bound(flags, name):.1e}"
        P.assert_close(f"face {t + 1} pe", after["pe"][t][1:-1, :, 1:-1], ref[t]["pe"][1:-1, :, 1:-1], max(P.TOL, bound(flags, "delp")))
        for n in ("peln", "pk"):
            P.assert_close(f"face {t + 1} {n}", after[n][t], ref[t][n], max(UP.BOUND[n], bound(flags, n)))
    return worst


def check_chain(lib):
    """the chained golden -- the reference's K_warm_rain with K_sedi_transport, followed by its whole fv_update_phys with moist_phys
    true and zero t_dt, q_dt -- through FvDynamics.k_warm_rain on the doubly periodic tile: the recorded state is laid into the
    resident fields of a nonhydrostatic FvDynamics (the constants of the recipe's constants_mod), one call, and the fields the
    reference wrote are compared on the ranges it wrote.  It holds the order inside the method.  Each field at the bound of its
    flag set; what fv_update_phys forms from them inherits their last bits: P.TOL where that is wider, and peln, pk, pkz at
    fv_update_phys' own bounds where those are wider."""
    import held_suarez_inputs as HI
    import parity_update_phys as UP
    from gfdl_atmos_cubed_sphere_amd.dyn_core import DynFlags
    from gfdl_atmos_cubed_sphere_amd.fv_dynamics import FvDynamics
    c = KI.CHAIN
    tr, sw, sh = KI.FLAGS[c["flags"]]
    bd, st = KI.chain_inputs()
    g = dict(golden("chain"), **golden("chain_b"))
    assert str(g["chain|sha"]) == KI.checksum(st), "chain: the inputs formed from the seed are not those the golden was recorded with"
    km, nq = c["km"], c["nq"]
    ak, bk = HI.eta_levels(km)
    fl = DynFlags(hydrostatic=c["hydrostatic"], ptop=c["ptop"], akap=KI.KAPPA, grav=9.80, rdgas=287.04, cp_air=287.04 / KI.KAPPA,
                  moist_kappa=c["moist_kappa"])
    ctx = Context(P.make_grid(bd, False), km, lib=lib)
    try:
        fv = FvDynamics(ctx, fl, ak, bk, nq=nq, moist=dict(nwat=4, sphum=1, liq_wat=2, rainwat=3, ice_wat=4), moist_phys=True)
        d = H.lay_state(fv, ctx, st, ("u", "v", "w", "delp", "pt", "ua", "va", "q", "ps", "pe", "peln", "pk", "pkz", "phis", "rain", "delz", "u_dt", "v_dt"))
        fv.k_warm_rain(c["pdt"], K_cycle=c["K_cycle"], K_sedi_transport=tr, do_K_sedi_w=sw, do_K_sedi_heat=sh, consts=KI.CONSTS)
        got = {n: d[n].download() for n in KI.CHAIN_OUT}
    finally:
        ctx.close()
    on_compute = ("pt", "ua", "va", "w", "ps", "delp", "q", "u_dt", "v_dt")
    fam = c["flags"]
    qb = max(bound(fam, n) for n in ("q_sphum", "q_liq", "q_rain"))
    tol = dict(pt=bound(fam, "pt"), delp=bound(fam, "delp"), q=qb, rain=bound(fam, "rain"), ps=bound(fam, "ps"), pe=bound(fam, "delp"),
               peln=max(bound(fam, "peln"), UP.BOUND["peln"]), pk=max(bound(fam, "pk"), UP.BOUND["pk"]), pkz=max(bound(fam, "pk"), UP.BOUND["pkz"]),
               ua=bound(fam, "ua"), va=bound(fam, "va"), w=bound(fam, "w"), u=bound(fam, "ua"), v=bound(fam, "va"), u_dt=bound(fam, "u_dt"),
               v_dt=bound(fam, "v_dt"), delz=0.0)      # (delz: fv_update_phys rescales it by pt_new / pt, :512-520)
    out = {}
    for n in KI.CHAIN_OUT:
        a, b = H.written_range(bd, n, got[n], on_compute), g[f"chain|out|{n}"]
        out[n] = float(P.assert_close(f"chain {n}", a, b, max(P.TOL, tol[n])))
    print("chain", out)
    return out
