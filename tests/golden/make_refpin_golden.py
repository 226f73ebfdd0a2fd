"""Golden fixtures from the REFERENCE's own compiled Fortran: small cases, inputs and reference outputs, recorded through
tests/ref_lib.py (oracle/_ref/libfv3ref.so, `make -C oracle ref` where the reference tree and amdflang are present):

    python tests/golden/make_refpin_golden.py

-> tests/golden/refpin_grid_<grid>.npz (the gridstructs the cases run on) and tests/golden/refpin_<routine>.npz (per case: the
inputs "<input set>|in|<name>" and the reference's outputs "<case>|out|<name>").  Data only.  What a case is -- routine,
grid, parameters -- is the table CASES below; tests/test_reference_pin*.py replay it through the oracle, the host emulation
and the GPU library, so nothing there depends on the reference library being present.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle_lib as O  # noqa: E402
import refpin_common as RC  # noqa: E402

F = np.asfortranarray
ROUTINES = ("fv_tp_2d", "c_sw", "d_sw", "d_sw_face", "a2b_ord4", "update_dz", "riem", "remap")
GRID_NAMES = ("dp", "face", "west")
NPZ = 2
KM_NH = 6        # levels of the column-solver cases


# ---- grids and input sets: built from the seeded generators when recording, read back from the files when replaying ----------
def build_grid(name):
    if name == "dp":
        return RC.periodic_grid(8, 6, True)
    if name == "face":
        return RC.tile_state("face", NPZ, npx=13)[0]
    return RC.tile_state(name, NPZ)[0]


def _state(grid, hydrostatic=False):
    if grid == "dp":
        return RC.smooth_state(build_grid("dp").bd, NPZ, hydrostatic=hydrostatic)
    return RC.tile_state(grid, NPZ, hydrostatic=hydrostatic, npx=13 if grid == "face" else 25)[1]


def build_inputs(inset):
    kind, grid = inset.split("@")
    g = build_grid(grid)
    if kind == "tp":
        return RC.tp_inputs(g, q=None if grid == "dp" else _state(grid)["delp"][:, :, 0])
    if kind in ("state", "state_hydro"):
        return _state(grid, kind == "state_hydro")
    if kind in ("dsw", "dsw_hydro", "dsw_cond"):
        case = {"dsw": "defaults", "dsw_hydro": "defaults", "dsw_cond": "use_cond_low_order"}[kind]
        f = RC.dsw_inputs(g, _state(grid, kind == "dsw_hydro"), NPZ, kind == "dsw_hydro", case)[3]
        return {k: v for k, v in f.items() if k not in ("crx", "cry", "xfx", "yfx", "heat_source", "diss_est", "delpc", "ptc")}
    if kind == "nh":
        km = KM_NH
        s = RC.nh_inputs(g, km)
        arr, _ = RC.dz_d_inputs(g, km)
        _, f = RC.run_c_sw(O, g, RC.smooth_state(g.bd, km), km, 3.0, False)
        s.update({k: arr[k] for k in ("crx", "cry", "xfx", "yfx")}, ut=f["ut"], vt=f["vt"], dp0=np.asarray(s["dp0"]))
        return s
    raise KeyError(inset)


def _dsw_full(g, f):
    """the d_sw work arrays the input set leaves out (all zeros on entry)"""
    bd, npz = g.bd, f["delp"].shape[2]
    f = dict(f)
    for n, kind in (("crx", "CX"), ("cry", "CY"), ("xfx", "CX"), ("yfx", "CY"), ("heat_source", "CC"), ("diss_est", "CC"),
                    ("delpc", "A"), ("ptc", "A")):
        f[n] = bd.zeros(kind, npz)
    return f


def _dsw_case(case, hydrostatic):
    """(par, lev) of a DSW_CASES entry, as refpin_common.dsw_inputs forms them"""
    from gfdl_atmos_cubed_sphere_amd.synthetic import DSW_PAR
    kw = RC.DSW_CASES[case]
    lev_over = dict(kw.get("lev_over") or {})
    par = dict(DSW_PAR)
    par.update(kw.get("par_over") or {})
    par["hydrostatic"], par["use_cond"] = int(hydrostatic), int(bool(kw.get("use_cond")))
    par.update(nord=1, nord_v=1, nord_w=1, nord_t=1, d2_bg=0.0, damp_v=0.0, damp_w=0.0, damp_t=0.0, d_con=0.0)
    return par, RC.default_levels(NPZ, **lev_over), kw.get("flags") or {}


# ---- the case table --------------------------------------------------------------------------------------------------------
# name -> (bound key, input set, run(M, g, inp) for a backend with oracle_lib's signatures, run(lib, g, inp) through the C ABI or None)
def _cases():
    c = {}
    for grid, modes in (("dp", ("plain", "mass_flux", "damp1", "damp2")), ("face", ("plain", "damp2"))):
        for hord in RC.ALL_HORD:
            for mode in modes:
                c[f"fv_tp_2d/{grid}/hord{hord}/{mode}"] = (
                    "fv_tp_2d", f"tp@{grid}", lambda M, g, i, h=hord, m=mode: RC.run_fv_tp_2d(M, g, i, h, m),
                    lambda lib, g, i, h=hord, m=mode: RC.lib_fv_tp_2d(lib, g, i, h, m))
    for grid in ("dp", "face"):
        for hyd in (False, True):
            c[f"c_sw/{grid}/hyd{int(hyd)}"] = (
                "c_sw", f"{'state_hydro' if hyd else 'state'}@{grid}", lambda M, g, i, h=hyd: RC.run_c_sw(M, g, i, NPZ, 3.0, h)[0],
                lambda lib, g, i, h=hyd: RC.lib_c_sw(lib, g, i, NPZ, 3.0, h))

    def dsw(case, hyd):
        def run(M, g, i):
            par, lev, flags = _dsw_case(case, hyd)
            for k, v in flags.items():
                setattr(g, k, v)
            return RC.run_d_sw(M, g, par, lev, _dsw_full(g, i), NPZ)

        def lib_run(lib, g, i):
            par, lev, flags = _dsw_case(case, hyd)
            for k, v in flags.items():
                setattr(g, k, v)
            return RC.lib_d_sw(lib, g, par, lev, _dsw_full(g, i), NPZ)
        return run, lib_run
    for case in ("defaults", "nord0", "nord2_vort_dcon", "nord3_diss_est", "hord5", "hord_lin", "lim_fac"):
        c[f"d_sw/dp/{case}"] = ("d_sw", "dsw@dp") + dsw(case, False)
    c["d_sw/dp/use_cond_low_order"] = ("d_sw", "dsw_cond@dp") + dsw("use_cond_low_order", False)
    c["d_sw_face/face/nord0"] = ("d_sw", "dsw@face") + dsw("nord0", False)
    for k, n in ((0, "delp"), (1, "pt")):
        for grid in ("dp", "west"):
            for rep in (False, True):
                c[f"a2b_ord4/{grid}/{n}/replace{int(rep)}"] = (
                    "a2b_ord4", f"state@{grid}", lambda M, g, i, k=k, n=n, r=rep: RC.run_a2b_ord4(M, g, F(i[n][:, :, k]), r), None)
    c["update_dz/dp/c"] = ("update_dz_c", "nh@dp", lambda M, g, i: RC.run_update_dz_c(M, g, i, KM_NH, i["ut"], i["vt"]),
                           lambda lib, g, i: RC.lib_update_dz_c(lib, g, i, KM_NH, i["ut"], i["vt"]))
    for hord in (10, 5, 6, 8):
        def run(M, g, i, h=hord):
            arr, _ = RC.dz_d_inputs(g, KM_NH)
            return RC.run_update_dz_d(M, g, i, KM_NH, dict(arr, **{k: i[k] for k in ("crx", "cry", "xfx", "yfx")}), h)

        def lib_run(lib, g, i, h=hord):
            arr, lev = RC.dz_d_inputs(g, KM_NH)
            return RC.lib_update_dz_d(lib, g, i, KM_NH, dict(arr, **{k: i[k] for k in ("crx", "cry", "xfx", "yfx")}), lev, h)
        c[f"update_dz/dp/d_hord{hord}"] = ("update_dz_d", "nh@dp", run, lib_run)
    for uc, mk in ((False, False), (True, False), (True, True)):
        kw = dict(use_cond=uc, moist_kappa=mk)
        c[f"riem/dp/c/cond{int(uc)}{int(mk)}"] = ("riem_solver_c", "nh@dp", lambda M, g, i, kw=kw: RC.run_riem_solver_c(M, g, i, KM_NH, **kw),
                                                lambda lib, g, i, kw=kw: RC.lib_riem_solver_c(lib, g, i, KM_NH, **kw))
        for ulp, lc in ((False, True), (True, False)):
            kw3 = dict(kw, use_logp=ulp, last_call=lc)
            c[f"riem/dp/3/cond{int(uc)}{int(mk)}/logp{int(ulp)}/last{int(lc)}"] = (
                "riem_solver3", "nh@dp", lambda M, g, i, kw=kw3: RC.run_riem_solver3(M, g, i, KM_NH, **kw),
                lambda lib, g, i, kw=kw3: RC.lib_riem_solver3(lib, g, i, KM_NH, **kw))
    return c


CASES = _cases()


def routine_of(name):
    return name.split("/")[0]


# ---- remap and fillz: columns, no grid -----------------------------------------------------------------------------------------
def remap_table():
    """(key, which, iv, kord, km, seed) of every recorded column"""
    out = []
    for which in RC.REMAP_OPS:
        for iv in {0: (1,), 1: (-2, -1, 1), 2: (0,), 3: (0,)}[which]:
            for kord in RC.KORDS:
                out.append((f"remap/{RC.REMAP_OPS[which]}/iv{iv}/kord{kord}", which, iv, kord, 12 if kord % 2 else 33, 1 + kord % 2))
    return out


def remap_args(iv, km, seed):
    pe1, pe2, q = RC.remap_columns(km, seed)
    return pe1, pe2, (q - 280.0 if iv == 0 else q), 1.5, (184.0 if iv == 1 else 0.0)


def make_remap(M):
    d = {}
    for km, seed in ((12, 2), (33, 1)):
        pe1, pe2, q = RC.remap_columns(km, seed)
        d[f"col{km}|in|pe1"], d[f"col{km}|in|pe2"], d[f"col{km}|in|q"] = pe1, pe2, q
    for key, which, iv, kord, km, seed in remap_table():
        pe1, pe2, q, qs, qmin = remap_args(iv, km, seed)
        d[f"{key}|out|q2"] = M.remap_column(which, pe1, pe2, q, qs, iv, kord, qmin)
    q, dp = RC.fillz_inputs(5, 12, 3)
    d["fillz|in|q"], d["fillz|in|dp"] = q, dp
    out = q.copy(order="F")
    M.fillz(out, dp)
    d["remap/fillz|out|q"] = out
    return d


def replay_remap(d):
    """(name, key, got, want) with the ORACLE on the recorded columns (the map routines have no entry point of their own in the
    library: replay() hands this no other runner)"""
    import ref_lib as R
    for key, which, iv, kord, km, seed in remap_table():
        pe1, pe2, q0 = d[f"col{km}|in|pe1"], d[f"col{km}|in|pe2"], d[f"col{km}|in|q"]
        q = q0 - 280.0 if iv == 0 else q0
        yield key, "remap", dict(q2=O.remap_column(which, pe1, pe2, q, 1.5, iv, kord, 184.0 if iv == 1 else 0.0)), dict(q2=d[f"{key}|out|q2"])
    a = F(d["fillz|in|q"].copy())
    R.oracle_fillz(a, F(d["fillz|in|dp"]))
    yield "remap/fillz", "fillz", dict(q=a), dict(q=d["remap/fillz|out|q"])


# ---- record / replay ---------------------------------------------------------------------------------------------------------
def _path(name):
    return os.path.join(HERE, f"refpin_{name}.npz")


def make_grid_file(name):
    return {k: np.asarray(v) for k, v in RC.grid_to_arrays(build_grid(name)).items()}


def make(routine):
    """the arrays of refpin_<routine>.npz, recorded through the reference library"""
    import ref_lib as R
    if routine.startswith("grid_"):
        return make_grid_file(routine[5:])
    if routine == "remap":
        return make_remap(R)
    d = {}
    for name, (key, inset, run, _) in CASES.items():
        if routine_of(name) != routine:
            continue
        inp = build_inputs(inset)
        for k, v in inp.items():
            d.setdefault(f"{inset}|in|{k}", np.asarray(v))
        g = build_grid(inset.split("@")[1])
        for k, v in run(R, g, {k: (F(v) if np.ndim(v) > 1 else v) for k, v in inp.items()}).items():
            d[f"{name}|out|{k}"] = np.asarray(v)
    return d


def load_grid(name):
    return RC.grid_from_arrays(dict(np.load(_path("grid_" + name))))


def oracle_runner():
    run = lambda case, g, inp: case[2](O, g, inp)  # noqa: E731
    run.is_oracle = True
    return run


def lib_runner(lib):
    return lambda case, g, inp: case[3](lib, g, inp) if case[3] is not None else None


def replay(routine, runner):
    """(name, bound key, got, want) for every recorded case of a routine; runner(case, g, inputs) -> outputs (None: not a form
    of that backend).  Grids and inputs come from the files only."""
    d = dict(np.load(_path(routine)))
    if routine == "remap":
        assert getattr(runner, "is_oracle", False), "the recorded columns of the map routines replay through the oracle only"
        yield from replay_remap(d)
        return
    for name, case in CASES.items():
        if routine_of(name) != routine:
            continue
        inset = case[1]
        g = load_grid(inset.split("@")[1])
        pre = f"{inset}|in|"
        inp = {k[len(pre):]: (F(v) if v.ndim > 1 else v) for k, v in d.items() if k.startswith(pre)}
        got = runner(case, g, inp)
        if got is None:
            continue
        pre = f"{name}|out|"
        yield name, case[0], got, {k[len(pre):]: v for k, v in d.items() if k.startswith(pre)}


def main():
    for name in tuple("grid_" + n for n in GRID_NAMES) + ROUTINES:
        d = make(name)
        np.savez_compressed(_path(name), **d)
        print(f"{os.path.basename(_path(name))}: {len(d)} arrays, {os.path.getsize(_path(name))} bytes")
        assert os.path.getsize(_path(name)) <= 213341, "larger than the largest golden committed before (ppm1d_golden.npz)"


if __name__ == "__main__":
    main()
