"""The memory contract of the kernels (tests/test_memory_contract_*.py): helpers that make four kinds of error visible which a parity
check in a fresh context, on zeroed outputs, compared on the valid range only, cannot see.

  * a work array read before it is written      -> FV3_MI355X_POISON=1 (the library poisons its work arrays at every compute entry)
  * a pure output that depends on what it held  -> out_fill="pattern" (the check functions create `out` arrays holding the pattern)
  * a small overrun of an array                 -> guarded() (a band of the pattern on either side of every DeviceArray) and the
                                                   library's own guard bands around its work arrays under the switch
  * an input read where the header says it is not, an in-place array written outside its range
                                                -> the input filled with the pattern; unchanged_outside()

The pattern is the library's (csrc/fv3_api.hip poison_value): element i holds (i odd ? -1 : +1) * 1e30 * (1 + i mod 7) -- finite (the
kernels are built with -fno-honor-nans and their min / max drop a NaN), sign-alternating and not constant (a stencil difference
does not cancel it).  conftest.py does not load this module: the two test files import it."""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from gfdl_atmos_cubed_sphere_amd import lib as L

G = 1024   # doubles per guard band: 8 KB, the array keeps the allocator's 256-byte alignment


def pattern(n: int) -> np.ndarray:
    i = np.arange(int(n), dtype=np.int64)
    return np.where(i & 1, -1.0e30, 1.0e30) * (1 + i % 7).astype(np.float64)


def pattern_array(shape) -> np.ndarray:
    """a Fortran-ordered array of the shape whose memory holds the pattern"""
    shape = tuple(int(s) for s in shape)
    return np.asfortranarray(pattern(int(np.prod(shape))).reshape(shape, order="F"))


def host_out(shape, out_fill=0.0) -> np.ndarray:
    """the initial value of a pure output on the host: zeros (the checks' default) or the pattern"""
    if isinstance(out_fill, str):
        assert out_fill == "pattern", out_fill
        return pattern_array(shape)
    return np.full(tuple(shape), float(out_fill), order="F")


def out_array(ctx, kind, nk=None, out_fill=0.0):
    """a device array for an argument the header calls `out`: ctx.zeros(...) as before, or, with out_fill="pattern", an array that
    holds the pattern -- a kernel that adds into it, or skips a cell the reference writes, then differs from the oracle"""
    if isinstance(out_fill, str):
        return ctx.from_host(host_out(ctx.bd.shape(kind, nk), out_fill))
    a = ctx.zeros(kind, nk)
    if out_fill != 0.0:
        a.upload(host_out(a.shape, out_fill))
    return a


def unchanged_outside(name, before, after, kind, range, bd=None):
    """bit equality of an in-place array outside the index range the header gives for what the routine writes.
    kind: the stagger ("A", "U", ...) with range = (i0, i1, j0, j1) in the reference's indices and bd the Bounds; kind None:
    range is a tuple of slices into the array itself (arrays with a layout of their own, e.g. pe(is-1:ie+1, km+1, js-1:je+1))."""
    before, after = np.asarray(before), np.asarray(after)
    assert before.shape == after.shape, (name, before.shape, after.shape)
    mask = np.ones(before.shape, dtype=bool)
    if kind is None:
        mask[tuple(range)] = False
    else:
        bd.view(mask, kind, *range)[...] = False
    same = before.view(np.uint64) == after.view(np.uint64) if before.dtype == np.float64 else before == after
    bad = mask & ~same
    if np.any(bad):
        idx = np.argwhere(bad)
        raise AssertionError(f"{name}: {len(idx)} elements changed outside the written range {range} of kind {kind}; first at array "
                             f"index {tuple(int(v) for v in idx[0])}: {before[tuple(idx[0])]!r} -> {after[tuple(idx[0])]!r}")


class GuardError(AssertionError):
    pass


@contextlib.contextmanager
def guarded(monkeypatch):
    """For the duration of a test every lib.DeviceArray lies between two bands of G doubles of the pattern (one fv3_malloc); free()
    downloads both bands, frees, and raises GuardError with the array's shape and the damaged offsets.  Context.close() frees every
    array and destroys the context before the first such error is raised again."""
    vp = C.c_void_p
    bands = np.ascontiguousarray(pattern(G))

    def init(self, ctx, shape):
        self.ctx = ctx
        self.shape = tuple(int(s) for s in shape)
        self.nbytes = int(np.prod(self.shape)) * 8
        base = vp()
        ctx.lib.check(ctx.lib.dll.fv3_malloc(C.byref(base), C.c_size_t(self.nbytes + 2 * G * 8)), "fv3_malloc")
        self._base = base.value
        self.ptr = self._base + G * 8
        for at in (self._base, self.ptr + self.nbytes):
            ctx.lib.check(ctx.lib.dll.fv3_memcpy_h2d(ctx.h, vp(at), bands.ctypes.data_as(vp), C.c_size_t(G * 8)), "fv3_memcpy_h2d")
        ctx.sync()
        ctx._buffers.append(self)

    def free(self):
        if not self.ptr:
            return
        ctx, got = self.ctx, np.empty(2 * G)
        rc = 0
        for n, at in enumerate((self._base, self.ptr + self.nbytes)):
            rc = rc or ctx.lib.dll.fv3_memcpy_d2h(ctx.h, got[n * G:].ctypes.data_as(vp), vp(at), C.c_size_t(G * 8))
        rc = rc or ctx.lib.dll.fv3_sync(ctx.h)
        what = ctx.lib.dll.fv3_last_error().decode() if rc else ""
        ctx.lib.dll.fv3_free(vp(self._base))      # freeing comes first
        self.ptr = None
        if rc:
            raise L.Fv3Error(f"guard bands of a {self.shape} array: {what}")
        bad = np.flatnonzero(got.view(np.uint64) != np.concatenate([bands, bands]).view(np.uint64))
        if bad.size:
            n = self.nbytes // 8
            offs = [int(b) - G if b < G else n + int(b) - G for b in bad]
            raise GuardError(f"array of shape {self.shape} ({n} doubles): {len(offs)} guard elements damaged, at offsets "
                             f"{offs[:8]}{' ...' if len(offs) > 8 else ''} (negative: before the array; >= {n}: past its end)")

    def close(self):
        first = None
        for b in self._buffers:
            try:
                b.free()
            except (AssertionError, L.Fv3Error) as e:
                first = first or e
        self._buffers.clear()
        if self.h:
            rc = self.lib.dll.fv3_destroy(self.h)
            self.h = None
            if first is None:
                self.lib.check(rc, "fv3_destroy")
        if first is not None:
            raise first

    with monkeypatch.context() as m:     # (restores the classes on the way out, and nothing else the test has patched)
        m.setattr(L.DeviceArray, "__init__", init)
        m.setattr(L.DeviceArray, "free", free)
        m.setattr(L.Context, "close", close)
        yield


# ---- stale work arrays: a call after another kind of call in ONE context against the same call in a fresh context -------------------
def _download(d):
    return {n: a.download() for n, a in d.items()}


def _dsw_case(bd, g, npz, lev_over, par_over=None):
    """the inputs of parity_common.check_d_sw (nonhydrostatic) and a runner ctx -> {output: array}"""
    import parity_common as P
    from fields import smooth_state
    from gfdl_atmos_cubed_sphere_amd.layout import periodic_fill
    from test_oracle_properties import default_levels
    par = dict(P.DSW_PAR)
    par.update(par_over or {})
    par["hydrostatic"], par["use_cond"] = 0, 0
    f = P.run_c_sw_oracle(g, bd, npz, smooth_state(bd, npz, hydrostatic=False), 0.5 * par["dt"], False)
    for n, kind in (("uc", "V"), ("vc", "U"), ("divg_d", "B")):
        for k in range(npz):
            periodic_fill(bd, f[n][:, :, k], kind, fill_edge=True)
    rng = np.random.default_rng(99)
    for n, kind in (("mfx", "FX"), ("mfy", "FY"), ("cx", "CX"), ("cy", "CY")):
        f[n] = np.asfortranarray(rng.uniform(-1, 1, bd.shape(kind, npz)))
    lev = default_levels(npz, **lev_over)

    def run(ctx):
        ctx.dsw_levels(lev)
        d = {k: ctx.from_host(v) for k, v in f.items()}
        for n, kind in (("crx", "CX"), ("cry", "CY"), ("xfx", "CX"), ("yfx", "CY"), ("delp_out", "A"), ("pt_out", "A"), ("u_out", "U"),
                        ("v_out", "V"), ("w_out", "A"), ("heat_s", "CC"), ("diss_e", "CC"), ("delpc_o", "A")):
            d[n] = out_array(ctx, kind, npz, "pattern")
        ctx.d_sw(par, d["delpc_o"], d["delp"], d["pt"], d["u"], d["v"], d["w"], d["uc"], d["vc"], d["ua"], d["va"], d["divg_d"], d["mfx"],
                 d["mfy"], d["cx"], d["cy"], d["crx"], d["cry"], d["xfx"], d["yfx"], None, d["delp_out"], d["pt_out"], d["u_out"],
                 d["v_out"], d["w_out"], None, d["heat_s"], d["diss_e"])
        return _download({n: d[n] for n in ("mfx", "mfy", "cx", "cy", "crx", "cry", "xfx", "yfx", "delp_out", "pt_out", "u_out", "v_out",
                                            "w_out", "heat_s", "diss_e", "delpc_o")})
    return run


def _tp_case(bd, g, nk, hord, nord, damp_c):
    import parity_common as P
    from gfdl_atmos_cubed_sphere_amd.layout import periodic_fill
    rng = np.random.default_rng(5)
    a = {n: bd.zeros(k, nk) for n, k in (("q", "A"), ("crx", "CX"), ("xfx", "CX"), ("cry", "CY"), ("yfx", "CY"), ("ra_x", "RX"),
                                         ("ra_y", "RY"), ("mfx", "FX"), ("mfy", "FY"), ("mass", "A"))}
    for k in range(nk):
        a["q"][:, :, k] = 1.0 + rng.uniform(0, 1, bd.shape("A"))
        a["mass"][:, :, k] = 500.0 + 50 * rng.uniform(0, 1, bd.shape("A"))
        for n in ("q", "mass"):
            periodic_fill(bd, a[n][:, :, k], "A")
        for n, v in zip(("crx", "cry", "xfx", "yfx", "ra_x", "ra_y"), P._courant(bd, g, rng)):
            a[n][:, :, k] = v
        a["mfx"][:, :, k] = rng.uniform(-1, 1, bd.shape("FX")) * 1e5
        a["mfy"][:, :, k] = rng.uniform(-1, 1, bd.shape("FY")) * 1e5
    damp = nord >= 0

    def run(ctx):
        d = {n: ctx.from_host(v) for n, v in a.items()}
        fx, fy = out_array(ctx, "FX", nk, "pattern"), out_array(ctx, "FY", nk, "pattern")
        ctx.fv_tp_2d(d["q"], d["crx"], d["cry"], hord, fx, fy, d["xfx"], d["yfx"], d["ra_x"], d["ra_y"], d["mfx"] if damp else None,
                     d["mfy"] if damp else None, d["mass"] if damp else None, nord, damp_c, nk=nk)
        return _download(dict(fx=fx, fy=fy))
    return run


def _riem3_case(bd, km):
    from gfdl_atmos_cubed_sphere_amd.lib import nh_consts
    from gfdl_atmos_cubed_sphere_amd.synthetic import PTOP, nh_state
    s = nh_state(bd, km)
    ws = np.asfortranarray(0.1 * np.random.default_rng(4).uniform(-1, 1, bd.shape("CC")))

    def run(ctx):
        ctx.set_condensate(None, None)
        ctx.set_fast_tau_w(None)
        d = dict(w=ctx.from_host(s["w"]), zh=ctx.from_host(s["zh"]))
        for n, shape in (("delz", bd.shape("CC", km)), ("ppe", bd.shape("A", km + 1)), ("pk3", bd.shape("A", km + 1)),
                         ("pk", bd.shape("CC", km + 1)), ("pe", (bd.nx + 2, km + 1, bd.ny + 2)), ("peln", (bd.nx, km + 1, bd.ny))):
            d[n] = ctx.from_host(host_out(shape, "pattern"))
        ctx.riem_solver3(6.0, nh_consts(PTOP), ctx.from_host(s["zs"]), d["w"], d["delz"], ctx.from_host(s["pt"]), ctx.from_host(s["delp"]),
                         d["zh"], d["pe"], d["ppe"], d["pk3"], d["pk"], d["peln"], ctx.from_host(ws), False, True, False)
        return _download(d)
    return run


def _tracer_case(bd, g, npz, nq, hord=8):
    from gfdl_atmos_cubed_sphere_amd.halo import HaloExchanger
    from gfdl_atmos_cubed_sphere_amd.tracer2d import tracer_2d
    from test_oracle_properties import run_pair
    before, after = run_pair(bd, npz, g, True, dt=8.0)
    q = np.asfortranarray(np.random.default_rng(17).uniform(0, 1, bd.shape("A", npz) + (nq,)))
    a = dict(q=q, dp1=before["delp"], mfx=after["mfx"] * 3.0, mfy=after["mfy"] * 3.0, cx=after["cx"] * 9.0, cy=after["cy"] * 9.0)   # sub-cycled

    def run(ctx):
        halo = HaloExchanger(ctx, 1, 1, 0, 1)
        d = {n: ctx.from_host(np.asfortranarray(v)) for n, v in a.items()}
        d["q_nxt"], d["dp1_nxt"] = ctx.from_host(host_out(q.shape, "pattern")), out_array(ctx, "A", npz, "pattern")
        d["xfx"], d["yfx"] = out_array(ctx, "CX", npz, "pattern"), out_array(ctx, "CY", npz, "pattern")
        assert np.all(np.abs(ctx.tracer_2d_prep(0, d["cx"], d["cy"], d["xfx"], d["yfx"])) < 1.0e3), "cmax"   # (never a poisoned loop count)
        qf, dpf, nsplt = tracer_2d(ctx, halo, d["q"], d["q_nxt"], d["dp1"], d["dp1_nxt"], d["mfx"], d["mfy"], d["cx"], d["cy"], d["xfx"],
                                   d["yfx"], nq, hord, 0, 1, 0.0)
        assert nsplt > 1
        r = (bd.is_, bd.ie, bd.js, bd.je)
        out = _download({n: d[n] for n in ("mfx", "mfy", "cx", "cy", "xfx", "yfx")})
        out.update(q=bd.view(qf.download(), "A", *r).copy(), dp1=bd.view(dpf.download(), "A", *r).copy())
        return out
    return run


def check_stale_work_arrays(lib, nx=59, ny=49, npz=3):
    """In ONE context: d_sw with the damping / heating level set, then d_sw with nord = 0 on every level and d_con = 0; fv_tp_2d with
    nord = 2, then plain; riem_solver3, then tracer_2d.  The second result of each pair equals, bit for bit, the same call made in a
    fresh context: nothing a routine leaves in the work arrays it shares with the others reaches the next one.  (Under
    FV3_MI355X_POISON the leftovers are the pattern; without the switch, the first call's own.)"""
    import parity_common as P
    from gfdl_atmos_cubed_sphere_amd.layout import Bounds
    from gfdl_atmos_cubed_sphere_amd.lib import Context
    bd = Bounds(1, nx, 1, ny)
    g = P.make_grid(bd, True)
    pairs = [("d_sw", _dsw_case(bd, g, npz, dict(nord=2, do_vort_damp=True, vtdm4=0.06, d_con=1.0, d2_bg=0.0075), dict(dddmp=0.2, kgb=1e-3)),
              _dsw_case(bd, g, npz, dict(nord=0, d_con=0.0))),
             ("fv_tp_2d", _tp_case(bd, g, npz, 10, 2, 0.06), _tp_case(bd, g, npz, 10, -1, 0.0)),
             ("riem_solver3 -> tracer_2d", _riem3_case(bd, npz), _tracer_case(bd, g, npz, 2))]
    shared = []
    ctx = Context(g, npz, lib=lib)
    try:
        ctx.set_dp_ref(np.linspace(500.0, 1500.0, npz))
        for _, first, second in pairs:
            first(ctx)
            shared.append(second(ctx))
    finally:
        ctx.close()
    for (name, _, second), got in zip(pairs, shared):
        ctx = Context(g, npz, lib=lib)
        try:
            ctx.set_dp_ref(np.linspace(500.0, 1500.0, npz))
            fresh = second(ctx)
        finally:
            ctx.close()
        for n in fresh:
            assert np.array_equal(got[n], fresh[n]), f"{name}: {n} after another call in the same context differs from a fresh context's"


# ---- the cases of tests/test_memory_contract_hostemu.py and tests/test_memory_contract_gpu.py ------------------------------------------
# Shapes: the smallest at which each kernel form still has its edge -- 58-column strips and 48-row segments plus one more (59 x 49), a
# width that is no multiple of 64 (33, 61, 31), widths below a tile (7 x 5, 6 x 5), km on either side of the levels-per-lane switches
# (3, 17, 127; 79 / 80 in the remap), a cube face whose frames overlap (npx = 13) and one with an interior (npx = 25, faces 1 and 4).
PAT = dict(out_fill="pattern")
DAMP = dict(par_over=dict(dddmp=0.2, kgb=1e-3), lev_over=dict(nord=2, do_vort_damp=True, vtdm4=0.06, d_con=1.0, d2_bg=0.0075))
NORD3 = dict(lev_over=dict(nord=3, do_vort_damp=True, vtdm4=0.03, d_con=0.5), flags=dict(prevent_diss_cooling=False, do_diss_est=True))
CUBED_DAMP = dict(flags=dict(nord=2, do_vort_damp=True, vtdm4=0.06, d_con=1.0))
FORMS = {"unfused_march": {"FV3_MI355X_FUSED": "0"}, "tile": {"FV3_MI355X_MARCH": "0"}}      # refpin_common.KERNEL_FORMS, minus the default


def cases():
    """[(id, env, run(lib))]: env = the switches the context is created under, beside FV3_MI355X_POISON=1"""
    import parity_common as P
    import parity_cubed as CU
    import parity_dyn as D
    import parity_negadj as NA
    import parity_nh as N
    import parity_remap as R
    import parity_tracer as T
    out = []

    def add(name, run, env=None):
        out.append((name, env or {}, run))

    for hord in (10, 8, 5, -5):
        for nx, ny, nk in ((33, 9, 2), (59, 49, 2), (7, 5, 1)):
            add(f"fv_tp_2d-hord{hord}-{nx}x{ny}x{nk}-plain", lambda lib, a=(hord, nx, ny, nk): P.check_fv_tp_2d(lib, *a, **PAT))
            add(f"fv_tp_2d-hord{hord}-{nx}x{ny}x{nk}-mass_flux_damp",
                lambda lib, a=(hord, nx, ny, nk): P.check_fv_tp_2d(lib, *a, mode="mass_flux_damp", nord=2, damp_c=0.06, **PAT))
    for nx, ny, npz in ((61, 13, 1), (28, 4, 2), (59, 49, 2)):
        for hyd in (False, True):
            for perturb in ((True, False, "ortho") if nx == 59 else (True,)):
                add(f"c_sw-{nx}x{ny}x{npz}-{'hydro' if hyd else 'nh'}-perturb_{perturb}",
                    lambda lib, a=(nx, ny, npz, hyd, perturb): P.check_c_sw(lib, *a, **PAT))
    dsw_sets = (("default", {}), ("damping", DAMP), ("nord3", NORD3), ("use_cond", dict(use_cond=True)), ("phases", dict(phases=True)),
                ("sponge_cartesian", dict(perturb=False)))
    for nx, ny, npz in ((59, 49, 3), (33, 9, 2), (6, 5, 3)):
        for hyd in (False, True):
            for sname, kw in dsw_sets:
                add(f"d_sw-{nx}x{ny}x{npz}-{'hydro' if hyd else 'nh'}-{sname}",
                    lambda lib, a=(nx, ny, npz, hyd), kw=kw: P.check_d_sw(lib, *a, **kw, **PAT))
    for form, env in FORMS.items():
        for sname, kw in dsw_sets[:2]:
            add(f"d_sw-59x49x3-nh-{sname}-{form}", lambda lib, kw=kw: P.check_d_sw(lib, 59, 49, 3, **kw, **PAT), env)
    add("d_sw-130x100x3-interior_then_rest", lambda lib: P.check_d_sw(lib, 130, 100, 3, phases=True, **PAT))      # 3 x 3 strips / segments
    add("update_dz_c-24x13x6", lambda lib: N.check_update_dz_c(lib, 24, 13, 6, **PAT))
    add("update_dz_d-24x13x6", lambda lib: N.check_update_dz_d(lib, 24, 13, 6, **PAT))
    for nx, ny, km in ((33, 9, 3), (59, 49, 3)):
        add(f"update_dz_c-{nx}x{ny}x{km}", lambda lib, a=(nx, ny, km): N.check_update_dz_c(lib, *a, **PAT))
        add(f"update_dz_d-{nx}x{ny}x{km}-nord2_vort_damp",
            lambda lib, a=(nx, ny, km): N.check_update_dz_d(lib, *a, lev_over=dict(nord=2, do_vort_damp=True, vtdm4=0.06), **PAT))
    for nx, ny, km in ((24, 13, 8), (33, 9, 3), (31, 15, 17), (17, 3, 127)):
        for lds in (True, False):
            for a_imp in (1.0, 0.75):
                add(f"riem_solver_c-{nx}x{ny}x{km}-lds{int(lds)}-a_imp{a_imp}",
                    lambda lib, a=(nx, ny, km), kw=dict(lds=lds, a_imp=a_imp): N.check_riem_solver_c(lib, *a, **kw, **PAT))
                add(f"riem_solver3-{nx}x{ny}x{km}-lds{int(lds)}-a_imp{a_imp}",
                    lambda lib, a=(nx, ny, km), kw=dict(lds=lds, a_imp=a_imp): N.check_riem_solver3(lib, *a, **kw, **PAT))
    add("riem_solver_c-24x13x8-moist", lambda lib: N.check_riem_solver_c(lib, 24, 13, 8, use_cond=True, moist_kappa=True, **PAT))
    add("riem_solver3-24x13x8-moist", lambda lib: N.check_riem_solver3(lib, 24, 13, 8, use_cond=True, moist_kappa=True, **PAT))
    add("riem_solver3-24x13x8-not_last_call", lambda lib: N.check_riem_solver3(lib, 24, 13, 8, last_call=False, **PAT))
    for nx, ny, km in ((33, 9, 3), (31, 15, 17)):
        for hyd in (False, True):
            add(f"p_grad_c-{nx}x{ny}x{km}-{'hydro' if hyd else 'nh'}", lambda lib, a=(nx, ny, km, hyd): N.check_p_grad_c(lib, *a, **PAT))
        for fused in (True, False):
            add(f"nh_p_grad-{nx}x{ny}x{km}-fused{int(fused)}", lambda lib, a=(nx, ny, km), f=fused: N.check_nh_p_grad(lib, *a, fused=f, **PAT))
    for name, kw in (("km20", dict()), ("km79", dict(km=79, nx=17, ny=3)), ("km80", dict(km=80, nx=17, ny=3)), ("nq7", dict(nq=7)),
                     ("slab", dict(lds=False)), ("fill", dict(fill=True)), ("last_step_diabatic", dict(last_step=True, adiabatic=False))):
        add(f"remap-{name}", lambda lib, kw=kw: R.check_remap(lib, **dict(dict(km=20, nx=33, ny=9), **kw), **PAT))
    for nt in (1, 3):
        env = {"FV3_MI355X_TRACER_NT": str(nt)}
        add(f"tracer_2d-33x9x7-nq7-big_courant-nt{nt}", lambda lib: T.check_tracer_2d(lib, 33, 9, 7, nq=7, big_courant=True, **PAT), env)
        add(f"tracer_2d-59x49x3-nq2-nt{nt}", lambda lib: T.check_tracer_2d(lib, 59, 49, 3, nq=2, **PAT), env)
    add("fill2d", lambda lib: T.check_fill2d(lib, **PAT))
    add("mix_dp-nh", lambda lib: N.check_mix_dp(lib, **PAT))
    add("mix_dp-hydro", lambda lib: N.check_mix_dp(lib, hydrostatic=True, **PAT))
    add("ray_fast", lambda lib: N.check_ray_fast(lib, **PAT))
    add("neg_adj3", lambda lib: NA.check_against_restatement(lib, NA.SHAPES[0], False, True))      # (its compare() holds the halo)
    # ---- cubed sphere
    for npx, faces in ((13, range(6)), (25, (0, 3))):
        for hyd in (False, True):
            add(f"cubed-c_sw-npx{npx}-{'hydro' if hyd else 'nh'}", lambda lib, a=(npx, hyd, faces): CU.check_c_sw(lib, npx=a[0], hydrostatic=a[1], faces=a[2], **PAT))
        for hord in (10, 5):
            add(f"cubed-fv_tp_2d-npx{npx}-hord{hord}-plain", lambda lib, a=(hord, npx, faces): CU.check_fv_tp_2d(lib, a[0], npx=a[1], faces=a[2], **PAT))
            add(f"cubed-fv_tp_2d-npx{npx}-hord{hord}-nord2",
                lambda lib, a=(hord, npx, faces): CU.check_fv_tp_2d(lib, a[0], npx=a[1], faces=a[2], mass_flux=True, nord=2, damp_c=0.06, **PAT))
        for sname, kw in (("default", {}), ("damping", CUBED_DAMP), ("nh", dict(hydrostatic=False)), ("use_cond", dict(use_cond=True))):
            add(f"cubed-d_sw-npx{npx}-{sname}", lambda lib, a=(npx, faces), kw=kw: CU.check_d_sw(lib, npx=a[0], faces=a[1], **kw, **PAT))
        add(f"cubed-tracer_2d-npx{npx}", lambda lib, n=npx: CU.check_tracer_2d(lib, npx=n, **PAT))
        add(f"cubed-del2_cubed-npx{npx}", lambda lib, a=(npx, faces): CU.check_del2_cubed(lib, npx=a[0], faces=a[1]))
    # ---- sequences: stale work arrays would show (every work array is poisoned between any two compute entries)
    add("seq-substeps-n_split2", lambda lib: D.check_substeps(lib, n_split=2))
    add("seq-substeps_hydrostatic", lambda lib: D.check_substeps_hydrostatic(lib))
    add("seq-fv_step-nq2", lambda lib: D.check_fv_step(lib, nq=2))
    add("seq-fv_step-inline_q", lambda lib: D.check_fv_step(lib, flags=dict(inline_q=True)))
    add("seq-cubed-substeps_nh", lambda lib: CU.check_substeps_nh(lib, npx=13, npz=5))
    add("seq-cubed-substeps_hydrostatic", lambda lib: CU.check_substeps_hydrostatic(lib, npx=13))
    add("seq-cubed-jw_step-nh-nq2", lambda lib: CU.check_jw_step(lib, npx=13, npz=8, nq=2, hydrostatic=False))
    add("seq-stale_work_arrays", lambda lib: check_stale_work_arrays(lib))
    # ---- inputs the header says are not read: filled with the pattern, unchanged parity
    for form, env in (("default", {}), ("tile", FORMS["tile"])):      # (the LDS-tile kernels hold the nord_k = 0 branch that reads ua, va)
        for nx, ny in ((59, 49), (33, 9)):
            add(f"unread-d_sw-ua_va-no_level_with_nord_k0-{nx}x{ny}-{form}",      # (npz = 1: dyn_core's level rules leave nord_k = nord)
                lambda lib, a=(nx, ny): P.check_d_sw(lib, a[0], a[1], 1, poison_inputs=("ua", "va"), **PAT), env)
            add(f"unread-d_sw-divg_d-every_level_nord_k0-{nx}x{ny}-{form}",
                lambda lib, a=(nx, ny): P.check_d_sw(lib, a[0], a[1], 3, lev_over=dict(nord=0), poison_inputs=("divg_d",), **PAT), env)
            add(f"unread-c_sw-divg_d-nord0-{nx}x{ny}-{form}", lambda lib, a=(nx, ny): P.check_c_sw(lib, a[0], a[1], 2, nord=0, **PAT), env)
    return out


def run_case(lib, monkeypatch, env, run):
    """one case under the whole contract: the switch on before the context is made, every DeviceArray guarded"""
    monkeypatch.setenv("FV3_MI355X_POISON", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with guarded(monkeypatch):
        return run(lib)


# ---- the detectors themselves -----------------------------------------------------------------------------------------------------
def check_guard_detects_overrun(lib, monkeypatch):
    """one double written through fv3_memcpy_h2d just past the end of an array -- inside the test's own allocation, its guard band --
    makes free() raise, with the offset"""
    import pytest
    import parity_common as P
    from gfdl_atmos_cubed_sphere_amd.layout import Bounds
    bd = Bounds(1, 8, 1, 8)
    with guarded(monkeypatch):
        ctx = L.Context(P.make_grid(bd, False), 2, lib=lib)
        a = ctx.zeros("A", 2)
        n = a.nbytes // 8
        one = np.array([1.0])
        ctx.lib.check(ctx.lib.dll.fv3_memcpy_h2d(ctx.h, C.c_void_p(a.ptr + a.nbytes), one.ctypes.data_as(C.c_void_p), C.c_size_t(8)), "h2d")
        ctx.sync()
        with pytest.raises(GuardError, match=rf"at offsets \[{n}\]"):
            ctx.close()
        assert ctx.h is None and a.ptr is None        # freed and destroyed all the same
        ctx = L.Context(P.make_grid(bd, False), 2, lib=lib)      # ... and an array nobody overran is silent
        ctx.zeros("A", 2)
        ctx.close()


def check_switch_off_makes_no_fill(lib, monkeypatch):
    """a context created without the switch launches no fill kernel; with it, the work arrays of a d_sw call are filled"""
    import parity_common as P
    seen = {}
    orig_close = L.Context.close

    def close(self):
        seen.update(self.profile_report())
        orig_close(self)

    for on in (False, True):
        seen.clear()
        with monkeypatch.context() as m:
            m.delenv("FV3_MI355X_POISON", raising=False)
            if on:
                m.setenv("FV3_MI355X_POISON", "1")
            orig_init = L.Context.__init__
            m.setattr(L.Context, "__init__", lambda self, *a, **k: (orig_init(self, *a, **k), self.profile(True))[0])
            m.setattr(L.Context, "close", close)
            P.check_d_sw(lib, 59, 49, 3)                         # marching kernels: the mass-flux work arrays
        assert "d_sw_fused" in seen, seen
        assert ("poison_fill" in seen) == on, seen
