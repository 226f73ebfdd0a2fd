"""What the check bodies of the column-physics packages share (parity_negadj, parity_subgrid, parity_update_phys, parity_held_suarez,
parity_diag, parity_reed, parity_kessler): bit comparison, the compute-domain view and its halo mask, the checksum and the loader of
the recorded cases, a context that is the caller's or the run's own, the bounded comparison, the refusal checker, the six-faces-as-
one-group check, the same-bits-as-a-fresh-context check, the FvDynamics step that records the state around one host method with the
restatement of the fv_update_phys sequence behind it, and the `emu` / `lib` fixtures.  What a package does that the others do not
-- its bounds and where they were measured, its masks, its branch assertions -- stays in the package."""
from __future__ import annotations

import contextlib
import functools
import hashlib
import os
import subprocess

import numpy as np
import pytest

import parity_common as P
from gfdl_atmos_cubed_sphere_amd.lib import Context, Fv3Error, Fv3Lib

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- small helpers -----------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """the same doubles bit for bit: the sign of zero and the payload of a NaN count"""
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def compute(bd, a):
    """the compute domain of an A-grid array with halo"""
    return bd.view(a, "A", bd.is_, bd.ie, bd.js, bd.je)


def halo_mask(bd, shape):
    """True on the halo of an A-grid array of this shape"""
    m = np.ones(shape, dtype=bool)
    compute(bd, m)[...] = False
    return m


def checksum(st, with_shape=False):
    """of the inputs a golden was recorded with (with_shape: fv_diag's, which hashes each array's shape as well)"""
    h = hashlib.sha256()
    for n in sorted(st):
        a = np.ascontiguousarray(st[n])
        h.update(n.encode())
        if with_shape:
            h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def golden(prefix, group, slashes=False):
    """tests/golden/<prefix><group>.npz (slashes: the recorder wrote '/' in a key as '%')"""
    g = np.load(os.path.join(HERE, "golden", f"{prefix}{group}.npz"))
    return {(k.replace("%", "/") if slashes else k): v for k, v in g.items()}


# ---- context and runs --------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def own_or_borrowed(lib, bd, km, ctx=None, grid=None):
    """the caller's context, left open; or one of this run's own on the doubly periodic tile (or on `grid`), closed at the end"""
    if ctx is not None:
        yield ctx
        return
    ctx = Context(grid if grid is not None else P.make_grid(bd, False), km, lib=lib)
    try:
        yield ctx
    finally:
        ctx.close()


def upload(ctx, st, names):
    return {n: ctx.from_host(st[n]) for n in names}


def download(d, names):
    return {n: d[n].download() for n in names}


# ---- comparison and refusals -------------------------------------------------------------------------------------------------------
def assert_bounded(what, a, b, bound):
    """finite; bit-identical where the bound is 0.0, relative RMS <= bound elsewhere -> the figure"""
    assert np.all(np.isfinite(a)), f"{what}: non-finite values"
    if bound == 0.0:
        assert same_bits(a, b), f"{what}: not bit-identical, max diff {np.max(np.abs(a - b)):.3e}"
        return 0.0
    return P.assert_close(what, a, b, bound)


def refusals(call_lib=None, d=None, pr=None):
    """-> refused(match, p=pr, drop=(), call=None, **over): call_lib(d with the dropped fields None, p, **over), or the given call(),
    must raise Fv3Error with `match` in its text"""
    def refused(match, p=pr, drop=(), call=None, **over):
        try:
            if call is not None:
                call()
            else:
                call_lib(dict(d, **{n: None for n in drop}), p, **over)
        except Fv3Error as e:
            assert match in str(e), (match, str(e))
        else:
            raise AssertionError(f"a call that must be refused was taken ({match})")
    return refused


def assert_nothing_written(d, st, names):
    for n in names:
        if st[n].size:
            assert same_bits(d[n].download(), st[n]), f"{n}: a refused call wrote"


# ---- whole checks ------------------------------------------------------------------------------------------------------------------
def merged_once(mctx, label, call, merged=1):
    """the call on a flushed group is ONE merged launch (or `merged` of them) and no single one"""
    mctx.flush()
    mctx.group.stats()
    call()
    mctx.flush()
    got, single = mctx.group.stats()
    assert got == merged and single == 0, f"{label} of six faces: {got} merged launches, {single} single ones"


def six_faces(lib, gs, npz, sts, names, call, alone, prepare=None, label="", faces=range(6), host=lambda a: a, then=None):
    """the six faces as one fv3_group: call(mctx, d) is one merged launch, and every field of `names` on every face of `faces` has
    the bits of the single-context run alone[t].  prepare(mctx) uploads the package's tables; then(mctx) runs before the close"""
    from gfdl_atmos_cubed_sphere_amd.cubed_dyn import MultiContext
    mctx = MultiContext([Context(g, npz, lib=lib) for g in gs], group=True)
    try:
        assert mctx.group is not None
        if prepare:
            prepare(mctx)
        d = {n: mctx.from_host([host(st[n]) for st in sts]) for n in names}
        merged_once(mctx, label, lambda: call(mctx, d))
        for n in names:
            got = d[n].download()
            for t in faces:
                assert same_bits(got[t], alone[t][n]), f"face {t + 1} {n}"
        if then:
            then(mctx)
    finally:
        mctx.close()


def same_as_fresh_context(names, fresh, again, after):
    """a call made after another kind of call in the same context gives the bits of a fresh context"""
    for n in names:
        assert same_bits(again[n], fresh[n]), f"{n}: a call after {after} differs from a fresh context"


def host_step(lib, where, fields, extra_after, call_method):
    """parity_negadj.run_tile / run_sphere with an FvDynamics that, after step_from_temperature, records `fields` per face, makes
    call_method(self, bdt) and records `fields + extra_after` again -> (the run, kept); kept also holds what the reference of the
    step needs (bdt, consts, ptop, radius, ak, bk, hyd, mk, agrids per face) and whatever dict call_method returns.  On the sphere
    the oracle's geometry of update_dwinds_phys is uploaded: the tests' gridstructs are the oracle's"""
    import cubed_common as CC
    import gfdl_atmos_cubed_sphere_amd.fv_dynamics as M
    import parity_negadj as NA
    import parity_subgrid as PS
    orig, kept = M.FvDynamics, {}

    class RecordingFvDynamics(orig):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            if where == "sphere":
                cs, _ = CC.sphere(self.ctx.grid.npx)
                for t, c in enumerate(self.ctx.ctxs):
                    c.upload_dwinds(PS.oracle_dwinds_geom(cs, t))

        def step_from_temperature(self, bdt):
            super().step_from_temperature(bdt)
            dl = lambda n: NA._faces(self.dc.d[n].download())      # noqa: E731
            before = {n: [a.copy(order="F") for a in dl(n)] for n in fields}
            extra = call_method(self, bdt) or {}
            ctxs = self.ctx.ctxs if hasattr(self.ctx, "ctxs") else [self.ctx]
            kept.update(before=before, after={n: dl(n) for n in fields + extra_after}, bdt=bdt, consts=dict(self.neg_adj_consts, kappa=self.fl.akap),
                        ptop=self.fl.ptop, radius=self.radius, ak=self.ak, bk=self.bk, hyd=self.fl.hydrostatic, mk=bool(self.fl.moist_kappa),
                        agrids=[np.asarray(c.grid.m["agrid"]) for c in ctxs], **extra)

    M.FvDynamics = RecordingFvDynamics
    try:
        base = (NA.run_tile if where == "tile" else NA.run_sphere)(lib)
    finally:
        M.FvDynamics = orig
    return base, kept


def update_phys_params(kept, nq, **over):
    """the parameters of the restatement of fv_update_phys for the moist state of parity_negadj's runs (nwat = 6, sphum first)"""
    import parity_remap as PR
    import update_phys_inputs as UI
    sp = {n: PR.MOIST6[n] for n in UI.SPECIES if n != "sphum"}
    sp["sphum"] = 1
    pr = dict(dt=kept["bdt"], ptop=kept["ptop"], hydrostatic=kept["hyd"], phys_hydrostatic=True, gfs_phys=False, nq=nq, ncnst=nq, nwat=PR.MOIST6["nwat"],
              species=sp, adjust_mass=np.ones(nq, dtype=np.int32), has_qdt=True, tau_h2o=0.0, ak=kept["ak"], bk=kept["bk"])
    return dict(pr, **over)


def update_phys_reference(where, base, kept, ref, upr):
    """on the per-face states `ref`, in place: the restatement of the column routine of fv_update_phys (a tendency or output the state
    lacks is zero), the real exchange of u_dt, v_dt as two scalars, the restatement of update_dwinds_phys"""
    import cubed_common as CC
    import parity_subgrid as PS
    import ref_fv_sg as SG
    import ref_update_phys as RU
    from gfdl_atmos_cubed_sphere_amd.layout import periodic_fill
    bd = base["bd"]
    npz, nq = ref[0]["pt"].shape[2], ref[0]["q"].shape[3]
    for s in ref:
        for n, shape in (("t_dt", (bd.nx, bd.ny, npz)), ("q_dt", (bd.nx, bd.ny, npz, nq)), ("qdiag", bd.shape("A", npz) + (0,)),
                         ("pkz", (bd.nx, bd.ny, npz)), ("u_srf", (bd.nx, bd.ny)), ("v_srf", (bd.nx, bd.ny))):
            if n not in s:
                s[n] = np.zeros(shape, order="F")
        RU.fv_update_phys(bd, npz, upr, s, consts=kept["consts"])
    if where == "tile":
        for n in ("u_dt", "v_dt"):
            periodic_fill(bd, ref[0][n], "A")
        geoms = [None]
    else:
        cs, _ = CC.sphere(base["gs"][0].npx)
        CC.exchange(cs, ref, ("u_dt", "v_dt"), "A")
        geoms = [PS.oracle_dwinds_geom(cs, t) for t in range(6)]
    for t, s in enumerate(ref):
        g = base["g"] if where == "tile" else base["gs"][t]
        SG.update_dwinds_phys(bd, g.npx, g.npy, g.grid_type, kept["bdt"], s["u_dt"], s["v_dt"], s["u"], s["v"], geoms[t])


def lay_state(fv, ctx, st, names):
    """a recorded state into the resident fields of an FvDynamics"""
    d = fv.dc.d
    for n in names:
        if n in d:
            d[n].upload(st[n])
        else:
            d[n] = ctx.from_host(st[n])
    return d


def written_range(bd, n, a, on_compute):
    """the range a chained golden keeps of a field: the D-grid winds on their own points, pe without its ring, the fields of
    `on_compute` on the compute domain, every other whole"""
    if n == "u":
        return bd.view(a, "U", bd.is_, bd.ie, bd.js, bd.je + 1)
    if n == "v":
        return bd.view(a, "V", bd.is_, bd.ie + 1, bd.js, bd.je)
    if n == "pe":
        return a[1:-1, :, 1:-1]
    return compute(bd, a) if n in on_compute else a


# ---- the libraries under test ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "hostemu"), "-s"])
    return Fv3Lib(os.path.join(HERE, "hostemu", "libfv3_hostemu.so"))


@pytest.fixture(scope="module")
def lib():
    from gfdl_atmos_cubed_sphere_amd import lib as L
    return L.load()
