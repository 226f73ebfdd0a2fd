"""Parity checks shared by the GPU tests (product library, -m gpu) and the host-emulation
logic tests (tests/hostemu, CPU).  Each check runs the oracle and a library exporting the fv3_*
C ABI on identical seeded inputs and compares on the index ranges where the reference defines
the output.

Tolerance (BASELINE.json north_star): relative RMS difference of every prognostic/output field
< 1e-12 in fp64.  With FMA contraction off the kernels reproduce the oracle bit for bit, so the
checks below use a much tighter bound (1e-14 relative to the field's RMS) and report the worst
value; anything larger is an indexing or logic error, not round-off."""
from __future__ import annotations

import numpy as np

import oracle_lib as O
from fields import smooth_state
from gfdl_atmos_cubed_sphere_amd.grid import doubly_periodic, perturbed
from gfdl_atmos_cubed_sphere_amd.layout import Bounds, periodic_fill
from gfdl_atmos_cubed_sphere_amd.lib import Context
from memory_contract import host_out, out_array
from test_oracle_properties import _courant, default_levels

TOL = 1e-14


def rel_rms(a, b):
    d = np.sqrt(np.mean((a - b) ** 2))
    s = np.sqrt(np.mean(b ** 2))
    return d / s if s > 0 else d


def make_grid(bd, perturb):
    g = doubly_periodic(bd, bd.ie - bd.is_ + 2, bd.je - bd.js + 2)
    if perturb == "ortho":  # varying lengths / areas, exact angle terms (Grid::geom == 1)
        return perturbed(g, ortho=True)
    return perturbed(g) if perturb else g


def assert_close(name, got, ref, tol=TOL):
    assert np.all(np.isfinite(got)), f"{name}: non-finite values"
    e = rel_rms(got, ref)
    assert e <= tol, f"{name}: rel-rms {e:.3e} > {tol:.1e} (max abs diff {np.max(np.abs(got - ref)):.3e})"
    return e


# ------------------------------------------------------------------------------------------------
def check_fv_tp_2d(lib, hord, nx=40, ny=19, nk=3, perturb=True, mode="plain", nord=-1, damp_c=0.0, seed=5, out_fill=0.0):
    """out_fill: what the arrays the header calls `out` hold before the call (memory_contract.py); fx, fy are compared whole"""
    bd = Bounds(1, nx, 1, ny)
    g = make_grid(bd, perturb)
    rng = np.random.default_rng(seed)
    q = bd.zeros("A", nk)
    arrs = {n: bd.zeros(k, nk) for n, k in (("crx", "CX"), ("xfx", "CX"), ("cry", "CY"), ("yfx", "CY"),
                                             ("ra_x", "RX"), ("ra_y", "RY"), ("mfx", "FX"), ("mfy", "FY"),
                                             ("mass", "A"))}
    for k in range(nk):
        q[:, :, k] = 1.0 + rng.uniform(0, 1, bd.shape("A")) + (k == 1) * 5.0 * (rng.uniform(0, 1, bd.shape("A")) > 0.7)
        periodic_fill(bd, q[:, :, k], "A")
        c = _courant(bd, g, rng)
        for n, a in zip(("crx", "cry", "xfx", "yfx", "ra_x", "ra_y"), c):
            arrs[n][:, :, k] = a
        arrs["mfx"][:, :, k] = rng.uniform(-1, 1, bd.shape("FX")) * 1e5
        arrs["mfy"][:, :, k] = rng.uniform(-1, 1, bd.shape("FY")) * 1e5
        arrs["mass"][:, :, k] = 500.0 + 50 * rng.uniform(0, 1, bd.shape("A"))
        periodic_fill(bd, arrs["mass"][:, :, k], "A")
    use_mf = mode in ("mass_flux", "mass_flux_damp")
    use_mass = mode == "mass_flux_damp"
    # oracle
    fx_ref, fy_ref = bd.zeros("FX", nk), bd.zeros("FY", nk)
    for k in range(nk):
        sl = lambda n: np.asfortranarray(arrs[n][:, :, k])
        fx, fy = O.fv_tp_2d(g, np.asfortranarray(q[:, :, k]), sl("crx"), sl("cry"), hord, sl("xfx"), sl("yfx"),
                            sl("ra_x"), sl("ra_y"), sl("mfx") if use_mf else None, sl("mfy") if use_mf else None,
                            sl("mass") if use_mass else None, nord, damp_c)
        fx_ref[:, :, k], fy_ref[:, :, k] = fx, fy
    # library
    ctx = Context(g, nk, lib=lib)
    try:
        d = {n: ctx.from_host(a) for n, a in arrs.items()}
        dq = ctx.from_host(q)
        dfx, dfy = out_array(ctx, "FX", nk, out_fill), out_array(ctx, "FY", nk, out_fill)
        ctx.fv_tp_2d(dq, d["crx"], d["cry"], hord, dfx, dfy, d["xfx"], d["yfx"], d["ra_x"], d["ra_y"],
                     d["mfx"] if use_mf else None, d["mfy"] if use_mf else None, d["mass"] if use_mass else None,
                     nord, damp_c, nk=nk)
        e1 = assert_close("fx", dfx.download(), fx_ref)
        e2 = assert_close("fy", dfy.download(), fy_ref)
    finally:
        ctx.close()
    return max(e1, e2)


# ------------------------------------------------------------------------------------------------
from gfdl_atmos_cubed_sphere_amd.synthetic import CSW_OUT, DSW_PAR  # noqa: E402


def csw_valid_ranges(bd):
    i0, i1, j0, j1 = bd.is_, bd.ie, bd.js, bd.je
    return {"delpc": (i0 - 1, i1 + 1, j0 - 1, j1 + 1), "ptc": (i0 - 1, i1 + 1, j0 - 1, j1 + 1),
            "wc": (i0 - 1, i1 + 1, j0 - 1, j1 + 1), "uc": (i0 - 1, i1 + 2, j0 - 1, j1 + 1),
            "vc": (i0 - 1, i1 + 1, j0 - 1, j1 + 2), "ua": (i0 - 1, i1 + 1, j0 - 1, j1 + 1),
            "va": (i0 - 1, i1 + 1, j0 - 1, j1 + 1), "ut": (i0 - 1, i1 + 2, j0 - 1, j1 + 1),
            "vt": (i0 - 1, i1 + 1, j0 - 1, j1 + 2), "divg_d": (i0 - 1, i1 + 2, j0 - 1, j1 + 2)}


def run_c_sw_oracle(g, bd, npz, st, dt2, hydrostatic, nord=1):
    f = {k: v.copy(order="F") for k, v in st.items()}
    for n, kind in CSW_OUT:
        f[n] = bd.zeros(kind, npz)
    O.c_sw_3d(g, npz, f, nord=nord, dt2=dt2, hydrostatic=hydrostatic)
    return f


def run_c_sw_lib(ctx, bd, npz, st, dt2, hydrostatic, nord=1, out_fill=0.0):
    d = {k: ctx.from_host(v) for k, v in st.items()}
    for n, kind in CSW_OUT:
        d[n] = out_array(ctx, kind, npz, out_fill)
    ctx.c_sw(d["delpc"], d["delp"], d["ptc"], d["pt"], d["u"], d["v"], d.get("w"), d["uc"], d["vc"], d["ua"],
             d["va"], None if hydrostatic else d["wc"], d["ut"], d["vt"], d["divg_d"], nord, dt2, hydrostatic)
    return d


def degenerate_state(bd, npz, hydrostatic, kind):
    """states that sit on the branch points of the limiters: "rest" = no wind, constant scalars (every Courant number
    and slope exactly 0, the flat / tie branches); "tophat" = piecewise-constant fields with jumps (extrema detection,
    Huynh constraints active nearly everywhere); "checker" = 2-cell oscillations (every cell a local extremum)"""
    from gfdl_atmos_cubed_sphere_amd.layout import periodic_fill
    st = smooth_state(bd, npz, hydrostatic=hydrostatic, noise=0.0)
    for n, a in st.items():
        stag = {"u": "U", "v": "V"}.get(n, "A")
        i = np.arange(a.shape[0])[:, None, None]
        j = np.arange(a.shape[1])[None, :, None]
        base = {"u": 8.0, "v": -5.0, "delp": 900.0, "pt": 300.0, "w": 0.3}[n]
        if kind == "rest":
            a[...] = 0.0 if n in ("u", "v", "w") else base
        elif kind == "tophat":
            a[...] = base * (1.0 + 0.25 * (((i // 5) + (j // 4)) % 2))
        elif kind == "checker":
            a[...] = base * (1.0 + 0.1 * ((i + j) % 2))
        elif kind == "westward":            # every wind reversed: the upwind side is the OTHER neighbour everywhere
            if n in ("u", "v", "w"):
                a[...] = -smooth_state(bd, npz, hydrostatic=hydrostatic)[n]
            else:
                a[...] = smooth_state(bd, npz, hydrostatic=hydrostatic)[n]
        elif kind == "swirl":               # winds of both signs, sign changes every few cells in x and in y
            full = smooth_state(bd, npz, hydrostatic=hydrostatic)[n]
            if n in ("u", "v"):
                ph = 0.0 if n == "u" else 1.3
                a[...] = 9.0 * np.sin(2 * np.pi * (i / 7.3 + j / 5.1) + ph) + (full - np.mean(full)) * 0.3
            else:
                a[...] = full
        for k in range(npz):
            periodic_fill(bd, a[:, :, k], stag, fill_edge=True)
    return st


def check_c_sw(lib, nx=40, ny=19, npz=3, hydrostatic=False, perturb=True, dt=6.0, state=None, out_fill=0.0, nord=1):
    """nord = 0: the header says divg_d is not written -- it comes back bit for bit as it went in"""
    bd = Bounds(1, nx, 1, ny)
    g = make_grid(bd, perturb)
    st = degenerate_state(bd, npz, hydrostatic, state) if state else smooth_state(bd, npz, hydrostatic=hydrostatic)
    ref = run_c_sw_oracle(g, bd, npz, st, 0.5 * dt, hydrostatic, nord=nord)
    ctx = Context(g, npz, lib=lib)
    worst = 0.0
    try:
        d = run_c_sw_lib(ctx, bd, npz, st, 0.5 * dt, hydrostatic, nord=nord, out_fill=out_fill)
        rng_ = csw_valid_ranges(bd)
        for n, kind in CSW_OUT:
            if hydrostatic and n == "wc":
                continue
            got = d[n].download()
            if n == "divg_d" and nord == 0:
                assert np.array_equal(got, host_out(got.shape, out_fill)), "c_sw, nord = 0: divg_d was written"
                continue
            r = rng_[n]
            worst = max(worst, assert_close(n, bd.view(got, kind, *r), bd.view(ref[n], kind, *r)))
    finally:
        ctx.close()
    return worst


# ------------------------------------------------------------------------------------------------


def check_d_sw(lib, nx=40, ny=19, npz=4, hydrostatic=False, perturb=True, par_over=None, lev_over=None,
               flags=None, use_cond=False, phases=False, state=None, out_fill=0.0, poison_inputs=()):
    """c_sw (oracle) -> periodic halo of uc, vc, divg_d -> d_sw by oracle and by the library.
    out_fill: what the `out` arrays hold before the call (memory_contract.py); crx, cry, xfx, yfx are compared whole, so the oracle's
    hold the same.  poison_inputs: inputs the header says this configuration does not read ("ua", "va", "divg_d"): the library gets
    them filled with the pattern, the oracle the real ones."""
    bd = Bounds(1, nx, 1, ny)
    g = make_grid(bd, perturb)
    for k, v in (flags or {}).items():
        setattr(g, k, v)
    par = dict(DSW_PAR)
    par.update(par_over or {})
    par["hydrostatic"], par["use_cond"] = int(hydrostatic), int(use_cond)
    dt = par["dt"]
    st = degenerate_state(bd, npz, hydrostatic, state) if state else smooth_state(bd, npz, hydrostatic=hydrostatic)
    f = run_c_sw_oracle(g, bd, npz, st, 0.5 * dt, hydrostatic)
    for n, kind in (("uc", "V"), ("vc", "U"), ("divg_d", "B")):
        for k in range(npz):
            periodic_fill(bd, f[n][:, :, k], kind, fill_edge=True)
    rng = np.random.default_rng(99)
    if use_cond:
        f["q_con"] = np.asfortranarray(0.01 * rng.uniform(0, 1, bd.shape("A", npz)))
        for k in range(npz):
            periodic_fill(bd, f["q_con"][:, :, k], "A")
    for n, kind in (("mfx", "FX"), ("mfy", "FY"), ("cx", "CX"), ("cy", "CY")):
        f[n] = np.asfortranarray(rng.uniform(-1, 1, bd.shape(kind, npz)))  # non-zero: accumulation is checked
    for n, kind in (("crx", "CX"), ("cry", "CY"), ("xfx", "CX"), ("yfx", "CY")):
        f[n] = host_out(bd.shape(kind, npz), out_fill)
    for n, kind in (("heat_source", "CC"), ("diss_est", "CC")):      # (the oracle accumulates into these)
        f[n] = bd.zeros(kind, npz)
    lev = default_levels(npz, **(lev_over or {}))
    inp = {k: v.copy(order="F") for k, v in f.items()}

    # ---- oracle (in place, reference semantics) ----
    opar = dict(par)
    opar.update(nord=1, nord_v=1, nord_w=1, nord_t=1, d2_bg=0.0, damp_v=0.0, damp_w=0.0, damp_t=0.0, d_con=0.0)
    O.d_sw_3d(g, npz, opar, lev, f)

    # ---- library ----
    ctx = Context(g, npz, lib=lib)
    worst = {}
    try:
        ctx.dsw_levels(lev)
        d = {k: ctx.from_host(v) for k, v in inp.items() if k not in ("heat_source", "diss_est")}
        for n in poison_inputs:
            d[n].upload(host_out(d[n].shape, "pattern"))
        out = {n: out_array(ctx, kind, npz, out_fill) for n, kind in (("delp_out", "A"), ("pt_out", "A"), ("u_out", "U"),
                                                                      ("v_out", "V"), ("w_out", "A"), ("q_con_out", "A"),
                                                                      ("heat_s", "CC"), ("diss_e", "CC"), ("delpc_o", "A"))}
        args = (par, out["delpc_o"], d["delp"], d["pt"], d["u"], d["v"], d.get("w"), d["uc"], d["vc"], d["ua"],
                d["va"], d["divg_d"], d["mfx"], d["mfy"], d["cx"], d["cy"], d["crx"], d["cry"], d["xfx"], d["yfx"],
                d.get("q_con"), out["delp_out"], out["pt_out"], out["u_out"], out["v_out"],
                None if hydrostatic else out["w_out"], out["q_con_out"] if use_cond else None, out["heat_s"],
                out["diss_e"])
        if phases:   # the halo-overlap form: interior strips / segments first, then the rest
            if phases == "poison":
                # the exchange of uc, vc is in flight during 'interior' (dyn_core.F90:565-578): their halos hold junk until
                # 'rest'.  The interior launch must not read them (ragged last strips / segments are the trap).
                ng, keep = bd.ng, {}
                for n in ("uc", "vc"):
                    h = inp[n].copy(order="F")
                    core = h[ng:ng + nx + (n == "uc"), ng:ng + ny + (n == "vc"), :].copy()
                    h[...] = 1.0e30
                    h[ng:ng + nx + (n == "uc"), ng:ng + ny + (n == "vc"), :] = core
                    d[n].upload(h)
            ctx.d_sw(*args, phase="interior")
            if phases == "poison":
                for n in ("uc", "vc"):
                    d[n].upload(inp[n])
            ctx.d_sw(*args, phase="rest")
        else:
            ctx.d_sw(*args)
        i0, i1, j0, j1 = bd.is_, bd.ie, bd.js, bd.je
        cmp = [("crx", d["crx"], "CX", None), ("cry", d["cry"], "CY", None), ("xfx", d["xfx"], "CX", None),
               ("yfx", d["yfx"], "CY", None), ("cx", d["cx"], "CX", None), ("cy", d["cy"], "CY", None),
               ("mfx", d["mfx"], "FX", None), ("mfy", d["mfy"], "FY", None),
               ("delp", out["delp_out"], "A", (i0, i1, j0, j1)), ("pt", out["pt_out"], "A", (i0, i1, j0, j1)),
               ("u", out["u_out"], "U", (i0, i1, j0, j1 + 1)), ("v", out["v_out"], "V", (i0, i1 + 1, j0, j1)),
               ("heat_source", out["heat_s"], "CC", None), ("diss_est", out["diss_e"], "CC", None),
               ("delpc", out["delpc_o"], "A", (i0, i1 + 1, j0, j1 + 1))]
        if not hydrostatic:
            cmp.append(("w", out["w_out"], "A", (i0, i1, j0, j1)))
        if use_cond:
            cmp.append(("q_con", out["q_con_out"], "A", (i0, i1, j0, j1)))
        for name, dev, kind, r in cmp:
            got, ref = dev.download(), f[name]
            if r is not None:
                got, ref = bd.view(got, kind, *r), bd.view(ref, kind, *r)
            if not np.any(ref) and not np.any(got):
                worst[name] = 0.0
                continue
            worst[name] = assert_close(name, got, ref)
    finally:
        ctx.close()
    return worst


# ------------------------------------------------------------------------------------------------
def check_halo_periodic(lib, nx=21, ny=10, nk=3):
    bd = Bounds(1, nx, 1, ny)
    g = make_grid(bd, False)
    rng = np.random.default_rng(4)
    ctx = Context(g, nk, lib=lib)
    try:
        for kind in ("A", "U", "V", "B"):
            a = np.asfortranarray(rng.uniform(-1, 1, bd.shape(kind, nk)))
            ref = a.copy(order="F")
            for k in range(nk):
                periodic_fill(bd, ref[:, :, k], kind)
            dev = ctx.from_host(a)
            ctx.halo_fill_periodic(dev, kind)
            got = dev.download()
            assert np.array_equal(got, ref), kind
    finally:
        ctx.close()


def check_halo_packed(lib, nx=20, ny=12, nk=3):
    """pack -> (self messages) -> unpack on one rank == the periodic fill"""
    from gfdl_atmos_cubed_sphere_amd.halo import HaloExchanger
    bd = Bounds(1, nx, 1, ny)
    g = make_grid(bd, False)
    ctx = Context(g, nk, lib=lib)
    try:
        halo = HaloExchanger(ctx, 1, 1, 0, 1, packed_single=True)
        rng = np.random.default_rng(4)
        fields, exps = [], []
        for kind in ("A", "U", "V", "B"):
            a = np.asfortranarray(rng.uniform(-1, 1, bd.shape(kind, nk)))
            e = a.copy(order="F")
            for k in range(nk):
                periodic_fill(bd, e[:, :, k], kind)
            fields.append((ctx.from_host(a), kind))
            exps.append(e)
        halo.update(fields)
        for (f, kind), e in zip(fields, exps):
            np.testing.assert_array_equal(f.download(), e, err_msg=kind)
    finally:
        ctx.close()


def check_sponge_levels_march(lib, nx=130, ny=64, npz=4, hydrostatic=False, flags=None, par_over=None):
    """Cartesian doubly periodic gridstruct, the reference's default level coefficients (levels 1, 2 = sponge: nord_k = 0, nord_w = 0,
    damp_w = d2_divg, dyn_core.F90:703-724): d_sw against the oracle, AND no level left to the LDS-tile kernels -- the sponge levels run in
    the branch-free marching kernels (dsw_fused.h run_bf) when the metrics are uniform."""
    worst = check_d_sw(lib, nx=nx, ny=ny, npz=npz, perturb=False, hydrostatic=hydrostatic, flags=flags, par_over=par_over)
    bd = Bounds(1, nx, 1, ny)
    g = make_grid(bd, False)
    for k, v in (flags or {}).items():
        setattr(g, k, v)
    par = dict(DSW_PAR)
    par.update(par_over or {})
    par["hydrostatic"], par["use_cond"] = int(hydrostatic), 0
    st = smooth_state(bd, npz, hydrostatic=hydrostatic)
    ctx = Context(g, npz, lib=lib)
    try:
        ctx.dsw_levels(default_levels(npz))
        d = {k: ctx.from_host(v) for k, v in st.items()}
        for n, kind in (("uc", "V"), ("vc", "U"), ("ua", "A"), ("va", "A"), ("divg_d", "B"), ("mfx", "FX"), ("mfy", "FY"), ("cx", "CX"), ("cy", "CY"),
                        ("crx", "CX"), ("cry", "CY"), ("xfx", "CX"), ("yfx", "CY"), ("delp_out", "A"), ("pt_out", "A"), ("u_out", "U"),
                        ("v_out", "V"), ("w_out", "A"), ("heat_s", "CC"), ("diss_e", "CC"), ("delpc", "A")):
            d[n] = ctx.zeros(kind, npz)
        ctx.profile(True)
        ctx.d_sw(par, d["delpc"], d["delp"], d["pt"], d["u"], d["v"], d.get("w"), d["uc"], d["vc"], d["ua"], d["va"], d["divg_d"], d["mfx"],
                 d["mfy"], d["cx"], d["cy"], d["crx"], d["cry"], d["xfx"], d["yfx"], None, d["delp_out"], d["pt_out"], d["u_out"], d["v_out"],
                 None if hydrostatic else d["w_out"], None, d["heat_s"], d["diss_e"])
        rep = ctx.profile_report()
        ctx.profile(False)
    finally:
        ctx.close()
    assert "d_sw_fused" in rep and "d_sw_mom_fused" in rep, rep
    return worst, rep


def check_registry_forget(lib):
    """the host-address registry in lazy mode (include/fv3_mi355x.h): a put of a current entry is skipped; an array that was freed and
    allocated again at the same address must leave the registry (fv3_registry_forget) or the device keeps the old values"""
    import ctypes as C
    bd = Bounds(1, 8, 1, 8)
    ctx = Context(doubly_periodic(bd, 9, 9, dx_const=1.0, dy_const=1.0), 2, lib=lib)
    try:
        dll, h = lib.dll, ctx.h
        host = np.arange(64, dtype=np.float64)
        dev = ctx.from_host(np.zeros(64))
        hp = host.ctypes.data_as(C.c_void_p)
        nb = C.c_size_t(host.nbytes)
        lib.check(dll.fv3_registry_mode(h, C.c_int(1)), "mode")
        lib.check(dll.fv3_registry_put(h, dev.p, hp, nb), "put")
        assert np.array_equal(dev.download().ravel(), host)
        host[:] = -host                                            # "a new array at the old address"
        lib.check(dll.fv3_registry_put(h, dev.p, hp, nb), "put")   # lazy: the entry says the mirror is current -> skipped
        assert np.array_equal(dev.download().ravel(), -host)
        lib.check(dll.fv3_registry_forget(h, hp, C.c_int(1)), "forget")
        lib.check(dll.fv3_registry_put(h, dev.p, hp, nb), "put")   # no entry: copied
        assert np.array_equal(dev.download().ravel(), host)
        # discard = 0 brings a deferred result to the host before the entry goes
        dev.upload(np.full(64, 7.0))
        lib.check(dll.fv3_registry_get(h, hp, dev.p, nb), "get")   # lazy: deferred
        assert not np.array_equal(host, np.full(64, 7.0))
        lib.check(dll.fv3_registry_forget(h, None, C.c_int(0)), "forget")
        assert np.array_equal(host, np.full(64, 7.0))
        st = (C.c_longlong * 4)()
        lib.check(dll.fv3_registry_stats(h, st), "stats")
        assert list(st) == [2, 1, 1, 1], list(st)
        lib.check(dll.fv3_registry_mode(h, C.c_int(0)), "mode")
    finally:
        ctx.close()


def check_golden_ppm_lines(lib, iord, which):
    """every reference-held vector of the 1-D PPM operator (tests/golden/ppm1d_golden.npz) of scheme iord straight through fv3_ppm_line:
    which = 0 the tile kernels' operator, 1 / 2 the marching kernels' along the lanes / through the register window.  No oracle."""
    import json
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppm1d_golden.npz"))
    meta = [m for m in json.loads(str(z["meta"])) if m["iord"] == iord]
    assert len(meta) == (36 if iord >= 8 else 24)
    bd = Bounds(1, 8, 1, 8)
    ctx = Context(doubly_periodic(bd, 9, 9, dx_const=1.0, dy_const=1.0), 2, lib=lib)
    worst = 0.0
    try:
        for m in meta:
            ql, c, want = z[m["key"] + "_q"], z[m["key"] + "_c"], z[m["key"] + "_flux"]
            n = ql.size
            h = np.concatenate([ql[-3:], ql, ql[:3]])
            dflux = ctx.from_host(np.zeros(n + 1))
            ctx.ppm_line(iord, which, ctx.from_host(h), ctx.from_host(np.ascontiguousarray(c)), dflux, n)
            got = dflux.download().ravel()
            worst = max(worst, np.max(np.abs(got - want)) / max(1e-300, np.max(np.abs(want))))
    finally:
        ctx.close()
    assert worst < 5e-15, (iord, which, worst)        # observed: 0.0
    return worst


def check_golden_ppm_through_fv_tp_2d(lib, iord, direction="x"):
    """The reference-held vectors of the 1-D PPM operator (tests/golden/ppm1d_golden.npz: (q, c) -> face values, produced by executing
    the reference's own docs/examples/tp_core.ipynb) THROUGH THE LIBRARY's fv_tp_2d -- no oracle in between.  Every vector of the scheme is
    one level: a field that is uniform across the sweep direction on a unit Cartesian doubly periodic grid (area = 1), the other
    direction's Courant numbers and area fluxes zero, this direction's area flux one.  Then the inner transverse update is the
    identity (q * 1 + 0 - 0) / 1, inner and outer sweep see the same line (inner order == outer order for hord 5, -5, 6, 8:
    tp_core.F90:136-141), 0.5 * (f + f) * 1 is f, and the flux that comes back IS the face value of xppm / yppm (tp_core.F90:324-1152)."""
    import json
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppm1d_golden.npz"))
    meta = [m for m in json.loads(str(z["meta"])) if m["iord"] == iord]
    assert len(meta) == (36 if iord >= 8 else 24)
    nl = z[meta[0]["key"] + "_q"].size            # cells along the sweep
    nt, nk = 12, len(meta)                        # cells across it; one level per vector
    nx, ny = (nl, nt) if direction == "x" else (nt, nl)
    bd = Bounds(1, nx, 1, ny)
    g = doubly_periodic(bd, nx + 1, ny + 1, dx_const=1.0, dy_const=1.0)
    assert np.all(g.area == 1.0)
    q = bd.zeros("A", nk)
    crx, cry, xfx, yfx = bd.zeros("CX", nk), bd.zeros("CY", nk), bd.zeros("CX", nk), bd.zeros("CY", nk)
    want = np.zeros((nl + 1, nk))
    ng = bd.ng
    for k, m in enumerate(meta):
        ql, c, want[:, k] = z[m["key"] + "_q"], z[m["key"] + "_c"], z[m["key"] + "_flux"]
        line = np.concatenate([ql[-ng:], ql, ql[:ng]])          # the periodic halo
        if direction == "x":
            q[:, :, k] = line[:, None]
            crx[:, :, k] = c[:, None]
            xfx[:, :, k] = 1.0
        else:
            q[:, :, k] = line[None, :]
            cry[:, :, k] = c[None, :]
            yfx[:, :, k] = 1.0
    ctx = Context(g, nk, lib=lib)
    try:
        dfx, dfy = ctx.zeros("FX", nk), ctx.zeros("FY", nk)
        ctx.fv_tp_2d(ctx.from_host(q), ctx.from_host(crx), ctx.from_host(cry), iord, dfx, dfy, ctx.from_host(xfx), ctx.from_host(yfx), nk=nk)
        fx, fy = dfx.download(), dfy.download()
    finally:
        ctx.close()
    got = fx if direction == "x" else fy               # (nl + 1, nt, nk) / (nt, nl + 1, nk)
    other = fy if direction == "x" else fx
    assert np.all(other == 0.0)                        # zero area flux across the sweep
    worst = 0.0
    for k in range(nk):
        for t in range(nt):
            f = got[:, t, k] if direction == "x" else got[t, :, k]
            worst = max(worst, np.max(np.abs(f - want[:, k])) / max(1e-300, np.max(np.abs(want[:, k]))))
    assert worst < 5e-15, (iord, direction, worst)     # observed: 0.0 -- the notebook's face values bit for bit
    return worst
