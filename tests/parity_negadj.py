"""Check bodies of fv3_neg_adj3 (fv_sg.F90:968-1370), shared by tests/test_fv_dynamics_tail_hostemu.py (CPU) and
tests/test_fv_dynamics_tail_gpu.py: the library against the numpy restatement tests/ref_neg_adj3.py, and properties that need no
restatement.  The inputs are a positive moist state with negatives planted by construction, cell by cell, so that the restatement
takes every branch it counts; that is asserted before anything is compared."""
from __future__ import annotations

import numpy as np

import parity_common as P
import parity_phys as H
import ref_neg_adj3 as R
from gfdl_atmos_cubed_sphere_amd.layout import Bounds
from gfdl_atmos_cubed_sphere_amd.lib import Context

SPECIES = ("qv", "ql", "qr", "qi", "qs", "qg")     # tracer order sphum, liq_wat, rainwat, ice_wat, snowwat, graupel (+ cld_amt)
FIELDS = ("pt",) + SPECIES + ("qa",)
SHAPES = ((40, 19, 12), (130, 100, 5))


def positive_state(nx, ny, npz, seed):
    """a moist state without any negative water: every species > 0, so neither the pointwise phase nor a column phase acts"""
    bd = Bounds(1, nx, 1, ny)
    rng = np.random.default_rng(seed)
    shp = bd.shape("A", npz)
    u = lambda lo, hi: np.asfortranarray(rng.uniform(lo, hi, shp))
    st = dict(pt=u(200.0, 300.0), delp=u(500.0, 1500.0), qv=u(1.0e-3, 1.0e-2), qa=u(0.05, 1.0))
    for n in SPECIES[1:]:
        st[n] = u(1.0e-6, 1.0e-4)
    st["delz"] = np.asfortranarray(-rng.uniform(100.0, 500.0, (nx, ny, npz)))
    pe = np.cumsum(np.concatenate([np.full((nx, ny, 1), 300.0), bd.view(st["delp"], "A", 1, nx, 1, ny)], axis=2), axis=2)
    st["peln"] = np.asfortranarray(np.log(pe).transpose(0, 2, 1))     # (is:ie, npz+1, js:je)
    return bd, st


# the pointwise cases: what one cell is set to ({field: value}; the other fields keep their positive values)
POINTWISE_CASES = (
    dict(qi=-1.0e-5, qs=5.0e-5),                                               # ice pair, qi negative
    dict(qs=-1.0e-5, qi=5.0e-5),                                               # ice pair, qs negative
    dict(qi=-3.0e-5, qs=1.0e-5, qg=1.0e-4),                                    # the pair's deficit goes to graupel, which can pay
    dict(qg=-1.0e-5, qs=5.0e-5),                                               # graupel from snow
    dict(qg=-6.0e-5, qs=2.0e-5, qi=8.0e-5),                                    # ... then ice
    dict(qg=-1.0e-4, qs=1.0e-5, qi=1.0e-5, qr=5.0e-4),                         # ... then rain
    dict(qg=-1.0e-4, qs=1.0e-5, qi=1.0e-5, qr=2.0e-5, ql=5.0e-4),              # ... then cloud water
    dict(qg=-1.0e-4, qs=1.0e-5, qi=1.0e-5, qr=1.0e-5, ql=1.0e-5),              # ... then vapor
    dict(qr=-1.0e-5, ql=5.0e-5),                                               # liquid pair, qr negative
    dict(ql=-1.0e-5, qr=5.0e-5),                                               # liquid pair, ql negative
    dict(ql=1.0e-5, qr=-5.0e-5, qg=1.0e-4),                                    # negative rain paid by graupel
    dict(ql=1.0e-5, qr=-5.0e-4, qg=1.0e-5, qi=1.0e-4, qs=1.0e-4),              # ... by graupel, ice + snow, vapor
    dict(ql=-5.0e-5, qr=1.0e-5, qg=0.0, qi=1.0e-4, qs=1.0e-4),                 # :1133: qr came in >= 0, so ice is NOT asked; vapor pays
    dict(ql=1.0e-5, qr=-5.0e-4, qg=0.0, qi=3.0e-4, qs=1.0e-4),                 # ice pays more than the snow there is (dq1 < dq)
)
# cells the pointwise phase cannot repair (no donor in the cell): they are left to the column phases
LEFT_FOR_FILLQ = (
    dict(qg=-1.0e-4, qs=1.0e-5, qi=1.0e-5, qr=1.0e-5, ql=1.0e-5, qv=1.0e-6),   # vapor's 0.999 qv is not enough: qg stays negative
    dict(ql=1.0e-5, qr=-5.0e-4, qg=1.0e-5, qi=1.0e-5, qs=1.0e-5, qv=1.0e-7),   # qr stays negative
)


def planted_state(nx, ny, npz, seed, column_cases=True, per_case=6):
    """positive_state with negatives planted: every case in `per_case` columns of its own (a column holds one case, so the cases do not
    disturb each other).  column_cases = False: only cells that the pointwise phase repairs completely."""
    bd, st = positive_state(nx, ny, npz, seed)
    rng = np.random.default_rng(seed + 1000)
    cols = rng.permutation(nx * ny)
    taken = [0]

    def columns(n=per_case):
        c = cols[taken[0]:taken[0] + n]
        taken[0] += n
        assert len(c) == n, "the shape is too small for the planted cases"
        return [(int(x) % nx + bd.ng, int(x) // nx + bd.ng) for x in c]

    def put(i, j, k, case):
        for n, val in case.items():
            st[n][i, j, k] = val

    for case in POINTWISE_CASES:
        for i, j in columns():
            put(i, j, int(rng.integers(0, npz)), case)
    if not column_cases:
        return bd, st
    kb = npz - 1
    for case in LEFT_FOR_FILLQ:                              # fillq acting: the rest of the column is positive and pays
        for i, j in columns():
            put(i, j, int(rng.integers(0, npz)), case)
    for name in ("qg", "qr"):                                # fillq's early return: nothing positive in the column, one negative cell
        for i, j in columns(3):
            st[name][i, j, :] = 0.0
            k = int(rng.integers(0, npz))
            put(i, j, k, dict(qv=0.0, ql=0.0, qr=0.0, qi=0.0, qs=0.0, qg=0.0))
            st[name][i, j, k] = -1.0e-5
    for i, j in columns():                                   # vapor: top layer
        st["qv"][i, j, 0] = -1.0e-4
    for i, j in columns():                                   # interior with a donor above that pays all
        st["qv"][i, j, int(rng.integers(1, kb))] = -1.0e-4
    for i, j in columns():                                   # interior, more than the donor has: the rest cascades down to the bottom layer,
        st["qv"][i, j, 1] = -0.5                             # which borrows upward, nearest donor first
    for i, j in columns():                                   # interior without a donor above
        k = int(rng.integers(1, kb))
        st["qv"][i, j, k - 1] = 0.0
        st["qv"][i, j, k] = -1.0e-4
    for i, j in columns():                                   # bottom layer with donors above
        st["qv"][i, j, kb] = -1.0e-4
    for i, j in columns(3):                                  # bottom layer, no donor in the column
        st["qv"][i, j, :] = 0.0
        st["qv"][i, j, kb] = -1.0e-4
    for i, j in columns():                                   # cloud fraction: interior
        st["qa"][i, j, int(rng.integers(0, kb))] = -0.2
    for i, j in columns():                                   # bottom, the layer above pays all
        st["qa"][i, j, kb - 1], st["qa"][i, j, kb] = 0.9, -0.1
    for i, j in columns():                                   # bottom, the layer above pays what it has, the rest is clipped
        st["qa"][i, j, kb - 1], st["qa"][i, j, kb] = 0.1, -5.0
    for i, j in columns():                                   # bottom, no donor
        st["qa"][i, j, kb - 1], st["qa"][i, j, kb] = 0.0, -0.1
    return bd, st


def column_only_state(nx, ny, npz, seed, per_case=8):
    """negatives the pointwise phase leaves exactly as they are (no donor in the cell), in columns whose positive mass can pay: what
    the vertical fills are given is then the input itself"""
    bd, st = positive_state(nx, ny, npz, seed)
    rng = np.random.default_rng(seed + 2000)
    cols = rng.permutation(nx * ny)
    n = 0
    for name in ("qg", "qr", "qv"):
        for x in cols[n:n + per_case]:
            i, j, k = int(x) % nx + bd.ng, int(x) // nx + bd.ng, int(rng.integers(0, npz))
            if name != "qv":
                for s in SPECIES:
                    st[s][i, j, k] = 0.0
            st[name][i, j, k] = -1.0e-5
        n += per_case
    return bd, st


def reference(bd, st, hydrostatic, with_qa, **kw):
    ref = {n: st[n].copy(order="F") for n in FIELDS}
    cnt = R.neg_adj3(bd, hydrostatic, st["delp"], ref["pt"], *(ref[n] for n in SPECIES), qa=ref["qa"] if with_qa else None, **kw)
    return ref, cnt


def tracer_array(st, with_qa):
    return np.asfortranarray(np.stack([st[n] for n in SPECIES + (("qa",) if with_qa else ())], axis=3))


def run_lib(lib, bd, st, hydrostatic, with_qa, ctx=None, grid=None):
    """fv3_neg_adj3 on a copy of the state -> {field: array with halos}"""
    with H.own_or_borrowed(lib, bd, st["pt"].shape[2], ctx, grid) as ctx:
        d_pt, d_dp, d_q = ctx.from_host(st["pt"]), ctx.from_host(st["delp"]), ctx.from_host(tracer_array(st, with_qa))
        d_dz = None if hydrostatic else ctx.from_host(st["delz"])
        d_pl = ctx.from_host(st["peln"]) if hydrostatic else None
        ctx.neg_adj3(hydrostatic, d_pl, d_dz, d_dp, d_pt, d_q, qa=7 if with_qa else 0, consts=R.CONSTS)
        q = d_q.download()
        got = dict(pt=d_pt.download(), qa=q[:, :, :, 6] if with_qa else st["qa"].copy(order="F"))
        for n, s in enumerate(SPECIES):
            got[s] = q[:, :, :, n]
        assert np.array_equal(d_dp.download(), st["delp"])
        return got


def assert_every_branch(cnt, with_qa):
    missing = [b for b in R.BRANCHES if cnt[b] == 0 and (with_qa or not b.startswith("qa_"))]
    assert not missing, f"the planted state does not reach {missing}"


def compare(bd, st, got, ref):
    """every field at parity_common.TOL; cells the restatement left as they were are what they were; the halo is untouched"""
    r = (bd.is_, bd.ie, bd.js, bd.je)
    worst = 0.0
    for n in FIELDS:
        g, f, s = bd.view(got[n], "A", *r), bd.view(ref[n], "A", *r), bd.view(st[n], "A", *r)
        worst = max(worst, P.assert_close(n, g, f, P.TOL))
        same = f == s
        assert np.array_equal(g[same], s[same]), f"{n}: a cell the reference leaves unchanged came back different"
        halo = H.halo_mask(bd, st[n].shape)
        assert np.array_equal(got[n][halo], st[n][halo]), f"{n}: the halo was written"
    return worst


def check_against_restatement(lib, shape, hydrostatic, with_qa):
    nx, ny, npz = shape
    bd, st = planted_state(nx, ny, npz, seed=41 if hydrostatic else 43)
    ref, cnt = reference(bd, st, hydrostatic, with_qa)
    assert_every_branch(cnt, with_qa)
    assert any(np.any(ref[n] != st[n]) for n in ("pt",) + SPECIES)
    return compare(bd, st, run_lib(lib, bd, st, hydrostatic, with_qa), ref)


def check_noop(lib, shape, hydrostatic, with_qa):
    nx, ny, npz = shape
    bd, st = positive_state(nx, ny, npz, seed=47)
    got = run_lib(lib, bd, st, hydrostatic, with_qa)
    for n in FIELDS:
        assert np.array_equal(got[n], st[n]), n
    assert np.array_equal(got["pt"].view(np.int64), st["pt"].view(np.int64))


def check_properties(lib, shape, hydrostatic):
    nx, ny, npz = shape
    r = (1, nx, 1, ny)
    # (a) a state whose negatives the pointwise phase repairs completely: the column phases have nothing to do, and per cell the
    # water total is what it was, to the rounding of six numbers of its size
    bd, st = planted_state(nx, ny, npz, seed=53, column_cases=False)
    got = run_lib(lib, bd, st, hydrostatic, True)
    v = lambda a: bd.view(a, "A", *r)
    t0, t1 = sum(v(st[n]) for n in SPECIES), sum(v(got[n]) for n in SPECIES)
    assert any(np.any(got[n] != st[n]) for n in SPECIES) and np.any(got["pt"] != st["pt"])
    scale = sum(np.abs(v(st[n])) for n in SPECIES)
    assert np.all(np.abs(t1 - t0) <= 16 * np.finfo(float).eps * scale), np.max(np.abs(t1 - t0) / scale)
    for n in SPECIES[1:]:
        assert v(got[n]).min() >= 0.0, n
    # (b) negatives only the vertical fills can repair, in columns that can pay: each of qg, qr, qv keeps its column mass, and no
    # negative value is left
    bd, st = column_only_state(nx, ny, npz, seed=59)
    got = run_lib(lib, bd, st, hydrostatic, True)
    dp = v(st["delp"])
    for n in ("qg", "qr", "qv"):
        m0, m1 = (v(st[n]) * dp).sum(axis=2), (v(got[n]) * dp).sum(axis=2)
        assert np.any(v(got[n]) != v(st[n])), n
        mass = (np.abs(v(st[n])) * dp).sum(axis=2)
        assert np.all(np.abs(m1 - m0) <= 4 * npz * np.finfo(float).eps * mass), (n, np.max(np.abs(m1 - m0) / mass))
        pos, neg = (np.maximum(v(st[n]), 0.0) * dp).sum(axis=2), (np.maximum(-v(st[n]), 0.0) * dp).sum(axis=2)
        assert np.all(pos > 2.0 * neg)                       # the builder's columns can pay ...
        assert v(got[n]).min() >= -1.0e-20, (n, v(got[n]).min())   # ... so nothing negative is left (a fill ends within rounding of 0)
    for n in ("pt", "ql", "qi", "qs"):
        assert np.array_equal(got[n], st[n]), n
    # (c) the cloud fraction of the bottom layer is never negative
    bd, st = planted_state(nx, ny, npz, seed=61)
    got = run_lib(lib, bd, st, hydrostatic, True)
    assert v(st["qa"])[:, :, -1].min() < 0.0 and v(got["qa"])[:, :, -1].min() >= 0.0


def check_refusals(lib):
    bd, st = positive_state(12, 9, 4, seed=3)
    ctx = Context(P.make_grid(bd, False), 4, lib=lib)
    try:
        d_pt, d_dp, d_q = ctx.from_host(st["pt"]), ctx.from_host(st["delp"]), ctx.from_host(tracer_array(st, False))
        refused = H.refusals()
        refused("delz", call=lambda: ctx.neg_adj3(False, None, None, d_dp, d_pt, d_q))      # a NULL delz when nonhydrostatic,
        refused("peln", call=lambda: ctx.neg_adj3(True, None, None, d_dp, d_pt, d_q))       # a NULL peln when hydrostatic
        assert np.array_equal(d_q.download(), tracer_array(st, False))
    finally:
        ctx.close()


def check_six_faces(lib, npx=13, npz=6, hydrostatic=False):
    """the six faces as one fv3_group (cubed_dyn.MultiContext): the same fields as face by face, and ONE launch for the six"""
    import cubed_common as CC
    cs, gs = CC.sphere(npx)
    n = npx - 1
    sts = [planted_state(n, n, npz, seed=70 + t, per_case=3) for t in range(6)]
    bd = gs[0].bd
    alone = [run_lib(lib, bd, st, hydrostatic, True, grid=gs[t]) for t, (_, st) in enumerate(sts)]
    for t, (_, st) in enumerate(sts):
        ref, cnt = reference(bd, st, hydrostatic, True)
        compare(bd, st, alone[t], ref)
    # this package hands its tracers as one array: the states and the single runs in that form, the inputs as they went
    names = ("pt", "delp", "q", "peln" if hydrostatic else "delz")
    packed = [dict(st, q=tracer_array(st, True)) for _, st in sts]
    alone = [dict(p, pt=a["pt"], q=tracer_array(a, True)) for p, a in zip(packed, alone)]
    H.six_faces(lib, gs, npz, packed, names, label="neg_adj3", alone=alone,
                call=lambda mctx, d: mctx.neg_adj3(hydrostatic, d.get("peln"), d.get("delz"), d["delp"], d["pt"], d["q"], qa=7, consts=R.CONSTS))


# ---- the hosts: FvDynamics with the switches of the tail of fv_dynamics ------------------------------------------------------------
TILE_FIELDS = (("u", "U"), ("v", "V"), ("w", "A"), ("delp", "A"), ("pt", "A"), ("omga", "A"), ("ua", "A"), ("va", "A"))


def plant_tracer_negatives(q, seed=91, share=0.04):
    """negative patches in the six water species of a tracer array (any number of faces' worth): after a step some are still there"""
    rng = np.random.default_rng(seed)
    for iq in range(1, 6):
        m = rng.uniform(0.0, 1.0, q.shape[:3]) < share
        q[..., iq][m] = -0.5 * q[..., iq][m] - 1.0e-6
    m = rng.uniform(0.0, 1.0, q.shape[:3]) < 0.25 * share
    q[..., 0][m] = -0.2 * q[..., 0][m]
    m = rng.uniform(0.0, 1.0, q.shape[:3]) < 0.25 * share       # cells without any donor: every condensate negative, hardly any vapor
    for iq in range(1, 6):
        q[..., iq][m] = -np.abs(q[..., iq][m])
    q[..., 0][m] = 1.0e-4 * np.abs(q[..., 0][m])
    return q


def run_tile(lib, nq=7, nx=24, ny=16, npz=10, k_split=2, n_split=2, bdt=8.0, negatives=False, spy=None, **opts):
    """one fv_dynamics call of the Python host on the doubly periodic tile, the moist nonhydrostatic state of
    parity_dyn.check_fv_cycle_moist -> {field: host array}, 'omga_halo' = omga after a halo update, 'q'"""
    import parity_dyn as D
    import parity_nh as N
    import parity_remap as PR
    from gfdl_atmos_cubed_sphere_amd.dyn_core import DynFlags
    from gfdl_atmos_cubed_sphere_amd.fv_dynamics import FvDynamics
    from gfdl_atmos_cubed_sphere_amd.layout import periodic_fill
    from gfdl_atmos_cubed_sphere_amd.lib import GRAV, KAPPA, RDGAS
    bd = Bounds(1, nx, 1, ny)
    g = P.make_grid(bd, False)
    st, dp0 = D.make_state(bd, npz)
    ng = bd.ng
    c = (slice(ng, ng + nx), slice(ng, ng + ny))
    rng = np.random.default_rng(8)
    q = np.asfortranarray(rng.uniform(0.0, 1.0, bd.shape("A", npz) + (7,)))
    q[..., 0] *= 0.02
    q[..., 1:6] *= 0.002
    if negatives:
        plant_tracer_negatives(q)
    q = np.asfortranarray(q[..., :nq])
    for iq in range(nq):
        for k in range(npz):
            periodic_fill(bd, q[:, :, k, iq], "A")
    th = st["pt"]
    T = th.copy(order="F")
    T[c] = th[c] * np.exp(KAPPA / (1.0 - KAPPA) * np.log((-RDGAS / GRAV) * st["delp"][c] * th[c] / st["delz"]))
    sig = np.linspace(0.0, 1.0, npz + 1) ** 1.5
    ak, bk = N.PTOP * (1.0 - sig), sig.copy()
    fl = DynFlags(n_split=n_split, ptop=N.PTOP, use_cond=True, moist_kappa=True)
    ctx = Context(g, npz, lib=lib)
    try:
        fv = FvDynamics(ctx, fl, ak, bk, nq=nq, k_split=k_split, adiabatic=False, moist=dict(PR.MOIST6, sphum=1), c2l_ord=2, **opts)
        fv.dc.set_state(st["u"], st["v"], st["w"], st["delp"], T, st["delz"], st["phis"])
        fv.set_tracers(q)
        if spy is not None:
            spy(fv, g, ak, bk)
        fv.step_from_temperature(bdt)
        d = fv.dc.d
        out = {n: d[n].download() for n, _ in TILE_FIELDS}
        out["q"], out["delz"] = d["q"].download(), d["delz"].download()
        fv.dc.halo.update([(d["omga"], "A")])
        out["omga_halo"] = d["omga"].download()
        out.update(bd=bd, g=g, q_in=q, fv=fv)
        return out
    finally:
        ctx.close()


def run_sphere(lib, npx=13, npz=8, k_split=1, n_split=2, bdt=900.0, nq=7, negatives=False, **opts):
    """the same on the six faces of C12 from the Jablonowski-Williamson state (parity_cubed.check_jw_step_moist's run)"""
    import cubed_common as CC
    import parity_cubed as PC
    import parity_remap as PR
    from gfdl_atmos_cubed_sphere_amd import lib as L
    from gfdl_atmos_cubed_sphere_amd.cubed_dyn import CubeHaloAdapter, MultiContext
    from gfdl_atmos_cubed_sphere_amd.dyn_core import DynFlags
    from gfdl_atmos_cubed_sphere_amd.fv_dynamics import FvDynamics
    cs, gs = CC.sphere(npx)
    sig = np.linspace(0.0, 1.0, npz + 1) ** 1.5
    ak, bk = 300.0 * (1.0 - sig), sig.copy()
    st = cs.jablonowski_williamson(ak, bk, hydrostatic=False, rdgas=L.RDGAS, grav=L.GRAV)
    CC.exchange(cs, st, ("phis",), "A")
    fl = DynFlags(n_split=n_split, hydrostatic=False, d_ext=0.0, ptop=float(ak[0]), use_cond=True, moist_kappa=True)
    q0 = PC.tracer_fields(cs, npz, 7)
    for t, q in enumerate(q0):
        q[..., 0] *= 0.01
        for iq in range(1, 6):
            q[..., iq] *= 0.001 / (1.0 + iq)
        if negatives:
            plant_tracer_negatives(q, seed=91 + t)
    if negatives:
        CC.exchange(cs, [dict(q=q) for q in q0], ("q",), "A")
    q0 = [np.asfortranarray(q[..., :nq]) for q in q0]
    mctx = MultiContext([Context(g, npz, lib=lib) for g in gs])
    try:
        fv = FvDynamics(mctx, fl, ak, bk, nq=nq, k_split=k_split, adiabatic=False, moist=dict(PR.MOIST6, sphum=1), c2l_ord=2,
                        halo=CubeHaloAdapter(mctx, npx, topo=CC.product_topo(npx)), **opts)
        fv.dc.set_state([s["u"] for s in st], [s["v"] for s in st], [s["w"] for s in st], [s["delp"] for s in st],
                        [s["pt"] for s in st], [s["delz"] for s in st], [s["phis"] for s in st])
        fv.set_tracers(q0)
        fv.step_from_temperature(bdt)
        d = fv.dc.d
        out = {n: d[n].download() for n, _ in TILE_FIELDS}
        out["q"], out["delz"] = d["q"].download(), d["delz"].download()
        fv.dc.halo.update([(d["omga"], "A")])
        out["omga_halo"] = d["omga"].download()
        out.update(bd=gs[0].bd, gs=gs, fv=fv)
        return out
    finally:
        mctx.close()


def _faces(x):
    return x if isinstance(x, list) else [x]


def assert_same_fields(a, b, names, what):
    for n in names:
        for t, (x, y) in enumerate(zip(_faces(a[n]), _faces(b[n]))):
            assert np.array_equal(x, y), f"{what}: {n} (face {t + 1}) differs"


def check_nf_omega(lib, base, run, nf):
    """omga of a run with nf_omega = nf is the oracle's del2_cubed (the checker that exists, min(3, nf) passes) of the halo-updated
    omga of the run without the filter (`base`); nothing else moves"""
    import oracle_lib as O
    got = run(lib, nf_omega=nf)
    bd = base["bd"]
    r = (bd.is_, bd.ie, bd.js, bd.je)
    gs = base["gs"] if "gs" in base else [base["g"]]
    worst = 0.0
    for t, (g, om0, om) in enumerate(zip(gs, _faces(base["omga_halo"]), _faces(got["omga"]))):
        ref = om0.copy(order="F")
        O.del2_cubed(g, ref.shape[2], 0.18 * g.da_min, nf, ref)
        assert P.rel_rms(bd.view(ref, "A", *r), bd.view(om0, "A", *r)) > 1e-6, "the filter moves nothing: omga is too smooth a test"
        worst = max(worst, P.assert_close(f"face {t + 1} omga", bd.view(om, "A", *r), bd.view(ref, "A", *r), P.TOL))
    assert_same_fields(base, got, [n for n, _ in TILE_FIELDS if n != "omga"] + ["q", "delz"], f"nf_omega = {nf}")
    return worst


def check_cld_amt_rules(lib):
    """dnats = 1, cld_amt = 7 of nq = 7 on the tile (fv_dynamics.F90:200-201, :264, :569-572)"""
    import oracle_lib as O
    import parity_remap as PR
    six = run_tile(lib, nq=6)
    snap = {}

    def spy(fv, g, ak, bk):
        ctx, orig = fv.ctx, fv.ctx.lagrangian_to_eulerian

        def l2e(par, *a):
            d = fv.dc.d
            if not snap:                                     # the state the first remap is handed, and what it is told
                snap.update(par=dict(par), g=g, ak=ak, bk=bk, f={n: d[n].download() for n in (
                    "ps", "pe", "delp", "pkz", "pk", "u", "v", "w", "delz", "pt", "q", "peln", "omga", "ws", "q_con", "cappa")})
            orig(par, *a)
            if "after" not in snap:
                snap["after"] = d["q"].download()
        ctx.lagrangian_to_eulerian = l2e

    # dnrts = 0: the 7th tracer is not advected but remapped, with kord 9 whatever kord_tr is
    got = run_tile(lib, nq=7, dnats=1, dnrts=0, cld_amt=7, spy=spy)
    bd = got["bd"]
    r = (bd.is_, bd.ie, bd.js, bd.je)
    assert snap["par"]["nq"] == 7 and list(snap["par"]["kord_tr"]) == [8] * 6 + [9]
    assert np.array_equal(snap["f"]["q"][..., 6], got["q_in"][..., 6]), "tracer_2d moved the tracer that is not advected"
    ref = {k: v.copy(order="F") for k, v in snap["f"].items()}
    opar = dict(snap["par"], **dict(PR.MOIST6, moist_kappa=1, use_cond=1), sphum=1)
    O.lagrangian_to_eulerian(snap["g"], bd_npz(ref), opar, ref, snap["ak"], snap["bk"])
    a, b = bd.view(snap["after"][..., 6], "A", *r), bd.view(ref["q"][..., 6], "A", *r)
    assert np.array_equal(a, b), f"cld_amt after the remap is not the oracle's kord 9 remap of it: {np.max(np.abs(a - b)):.3e}"
    eight = {k: v.copy(order="F") for k, v in snap["f"].items()}
    O.lagrangian_to_eulerian(snap["g"], bd_npz(eight), dict(opar, kord_tr=[8] * 7), eight, snap["ak"], snap["bk"])
    assert not np.array_equal(bd.view(eight["q"][..., 6], "A", *r), b), "kord 8 and 9 agree on this tracer: the test shows nothing"
    for iq in range(6):
        assert np.array_equal(bd.view(got["q"][..., iq], "A", *r), bd.view(six["q"][..., iq], "A", *r)), f"tracer {iq + 1} != the nq = 6 run"
    assert_same_fields(six, got, [n for n, _ in TILE_FIELDS] + ["delz"], "nq = 7 with a passive 7th tracer")
    # dnrts = -1 (= dnats, fv_control.F90:567) and dnrts = 1: the 7th tracer is neither advected nor remapped
    for dnrts in (-1, 1):
        got = run_tile(lib, nq=7, dnats=1, dnrts=dnrts, cld_amt=7)
        assert np.array_equal(got["q"][..., 6], got["q_in"][..., 6]), f"dnrts = {dnrts}: the 7th tracer moved"
        for iq in range(6):
            assert np.array_equal(bd.view(got["q"][..., iq], "A", *r), bd.view(six["q"][..., iq], "A", *r)), (dnrts, iq)


def bd_npz(f):
    return f["delp"].shape[2]


def check_step_with_neg_adj(lib, run, with_qa=True):
    """a whole step with neg_adj = True on a moist state with planted negatives = the step without it, then the restatement"""
    opts = dict(cld_amt=7, dnats=1) if with_qa else {}
    base = run(lib, negatives=True, **opts)
    got = run(lib, negatives=True, neg_adj=True, check_negative=True, **opts)
    bd = base["bd"]
    r = (bd.is_, bd.ie, bd.js, bd.je)
    total = {b: 0 for b in R.BRANCHES}
    worst = 0.0
    for t, (pt, q, dp) in enumerate(zip(_faces(base["pt"]), _faces(base["q"]), _faces(base["delp"]))):
        ref = dict(pt=pt.copy(order="F"), **{s: np.asfortranarray(q[..., k]) for k, s in enumerate(SPECIES + ("qa",))})
        cnt = R.neg_adj3(bd, False, dp, ref["pt"], *(ref[s] for s in SPECIES), qa=ref["qa"] if with_qa else None,
                         consts=got["fv"].neg_adj_consts)
        for b in cnt:
            total[b] += cnt[b]
        gq = _faces(got["q"])[t]
        worst = max(worst, P.assert_close(f"face {t + 1} pt", bd.view(_faces(got["pt"])[t], "A", *r), bd.view(ref["pt"], "A", *r), P.TOL))
        for k, s in enumerate(SPECIES + ("qa",)):
            worst = max(worst, P.assert_close(f"face {t + 1} {s}", bd.view(gq[..., k], "A", *r), bd.view(ref[s], "A", *r), P.TOL))
    acted = [b for b in total if total[b] > 0]
    assert len(acted) >= 8 and total["fillq_g_acting"] + total["fillq_r_acting"] > 0 and total["qv_int_donor"] > 0, total
    assert_same_fields(base, got, ["u", "v", "w", "delp", "omga", "delz"], "neg_adj")
    rep = got["fv"].negative_report
    assert any(w == "before" for w, _, _ in rep), rep          # the planted state is below prt_negative's thresholds before the repair
    return worst


def check_host_refusals(lib):
    """neg_adj without nwat == 6; dnats, dnrts, cld_amt outside 0..nq"""
    import pytest
    import parity_nh as N
    import parity_remap as PR
    from gfdl_atmos_cubed_sphere_amd.dyn_core import DynFlags
    from gfdl_atmos_cubed_sphere_amd.fv_dynamics import FvDynamics
    bd = Bounds(1, 12, 1, 9)
    npz = 4
    sig = np.linspace(0.0, 1.0, npz + 1) ** 1.5
    ak, bk = N.PTOP * (1.0 - sig), sig.copy()
    ctx = Context(P.make_grid(bd, False), npz, lib=lib)
    try:
        make = lambda **kw: FvDynamics(ctx, DynFlags(n_split=1, ptop=N.PTOP), ak, bk, **kw)
        with pytest.raises(ValueError, match="nwat"):
            make(nq=7, neg_adj=True)
        with pytest.raises(ValueError, match="nwat"):
            make(nq=7, neg_adj=True, moist=dict(PR.MOIST6, nwat=3))
        for bad in (dict(dnats=8), dict(dnats=-1), dict(dnrts=9), dict(cld_amt=8), dict(nf_omega=-1)):
            with pytest.raises(ValueError):
                make(nq=7, moist=dict(PR.MOIST6), **bad)
        make(nq=7, moist=dict(PR.MOIST6), neg_adj=True, dnats=1, cld_amt=7, nf_omega=1)      # the SHiELD-style set is taken
    finally:
        ctx.close()


# ---- the Fortran hosts: the reference-signature fv_dynamics (fv3_dyn_core_mod over fv3_host_mod / fv3_sphere_mod) -----------------------
TAIL_OPTS = dict(neg_adj=True, nf_omega=1, dnats=1, cld_amt=7)
TAIL_ENV = dict(FV3_REFSIG_NEG_ADJ="1", FV3_REFSIG_NF_OMEGA="1", FV3_REFSIG_DNATS="1")


def check_fortran_tail(lib, workdir, where):
    """tests/fortran_host.py's comparisons of the reference-signature fv_dynamics with the Python host (check_fortran_fv_dynamics on the
    tile, check_refsig_sphere on the six faces: bit-identical u, v, w, delp, pt, delz, q, ua, q_con), nq = 7 and moist, with the tail
    switched on on both sides: the three environment switches for the Fortran driver, the same options for the Python host.  Those
    helpers build their Python host themselves, so this is a thin variant AROUND them: while they run, the FvDynamics they import takes
    TAIL_OPTS, plants negatives into the tracer array it is handed (in place -- the array the helper then writes into the driver's
    input file) and keeps what omga and the check_negative report were.  omga, which the drivers append to their output when
    FV3_REFSIG_NF_OMEGA is set, is compared here."""
    import os

    import fortran_host as FH
    import gfdl_atmos_cubed_sphere_amd.fv_dynamics as M
    orig, kept = M.FvDynamics, {}

    class TailFvDynamics(orig):
        def __init__(self, *a, **kw):
            super().__init__(*a, **dict(kw, check_negative=True, **TAIL_OPTS))

        def set_tracers(self, q):
            for t, x in enumerate(q if isinstance(q, list) else [q]):
                plant_tracer_negatives(x, seed=91 + t)
            super().set_tracers(q)

        def step_from_temperature(self, bdt):
            super().step_from_temperature(bdt)
            kept.update(omga=self.dc.d["omga"].download(), report=list(self.negative_report), bd=self.ctx.bd)

    M.FvDynamics = TailFvDynamics
    os.environ.update(TAIL_ENV)
    try:
        if where == "tile":
            assert "fv3_solo_refsig: done" in FH.check_fortran_fv_dynamics(lib, workdir, nq=7, moist=True)
        else:
            assert FH.check_refsig_sphere(lib, workdir, npx=13, npz=12, n_split=2, k_split=2, bdt=900.0, nq=7, thermo=True) == 0.0
    finally:
        M.FvDynamics = orig
        for k in TAIL_ENV:
            os.environ.pop(k, None)
    assert any(w == "before" for w, _, _ in kept["report"]), "neg_adj3 had nothing to repair in this run"
    bd = kept["bd"]
    r = (bd.is_, bd.ie, bd.js, bd.je)
    faces = _faces(kept["omga"])
    n3 = int(np.prod(faces[0].shape))
    fn = os.path.join(str(workdir), "out_fd.bin" if where == "tile" else "rs_out.bin.0")
    tail = np.fromfile(fn, dtype=np.float64)[-n3 * len(faces):]
    for t, om in enumerate(faces):
        got = tail[t * n3:(t + 1) * n3].reshape(om.shape, order="F")
        assert np.array_equal(bd.view(got, "A", *r), bd.view(om, "A", *r)), f"omga of face {t + 1}: the Fortran host and the Python host differ"
