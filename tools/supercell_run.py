"""BASELINE config 4's initial condition as a simulation on one GPU: the doubly periodic supercell sounding with its warm bubble
(test_case 17), nonhydrostatic, water vapour carried as tracer 1 with its virtual effect.  Without --kessler there is no
microphysics in this path, so what develops is the buoyant thermal of the bubble, not the storm.  With --kessler every step is
FvDynamics.supercell_step: the Kessler warm-rain microphysics (K_warm_rain, driver/solo/fv_phys.F90:466-499) behind the dynamics, with
liq_wat, rainwat and the reference's fake ice as tracers 2 .. 4 (nwat = 4).  Every `--every` s: max w, max |u|, the global air mass,
the vapour mass and, with --kessler, the extrema of liq_wat and rainwat, the total water mass and the rain accumulated at the ground."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=256)
    ap.add_argument("--npz", type=int, default=64)
    ap.add_argument("--dx", type=float, default=500.0)
    ap.add_argument("--minutes", type=float, default=20.0)
    ap.add_argument("--dt-atmos", type=float, default=6.0)
    ap.add_argument("--n-split", type=int, default=8)   # c_s dt / dx = 0.5 at dx = 500 m (1.0 goes unstable within 20 steps)
    ap.add_argument("--every", type=float, default=120.0)
    ap.add_argument("--flags", type=str, default="", help="JSON of DynFlags overrides")
    ap.add_argument("--kessler", action="store_true", help="run K_warm_rain behind every step")
    ap.add_argument("--K-cycle", type=int, default=0)
    ap.add_argument("--K-sedi-transport", action="store_true")
    ap.add_argument("--K-sedi-w", action="store_true")
    ap.add_argument("--K-sedi-heat", action="store_true")
    ap.add_argument("--out", default=None, help="also write the result to this file")
    a = ap.parse_args()
    from gfdl_atmos_cubed_sphere_amd import lib as L
    from gfdl_atmos_cubed_sphere_amd.dyn_core import DynFlags
    from gfdl_atmos_cubed_sphere_amd.fv_dynamics import FvDynamics
    from gfdl_atmos_cubed_sphere_amd.grid import doubly_periodic
    from gfdl_atmos_cubed_sphere_amd.layout import Bounds, periodic_fill
    from gfdl_atmos_cubed_sphere_amd.test_cases import supercell
    nx, npz = a.nx, a.npz
    bd = Bounds(1, nx, 1, nx)
    g = doubly_periodic(bd, nx + 1, nx + 1, dx_const=a.dx, dy_const=a.dx)
    sig = np.linspace(0.0, 1.0, npz + 1) ** 1.2
    ptop = 5000.0                                           # ~20 km lid
    ak, bk = ptop * (1.0 - sig), sig.copy()
    st = supercell(bd, npz, ak, bk, a.dx, a.dx, dt_amp=2.0, dt_rad=10.0e3)
    q = st.pop("q")
    for n, kind in (("u", "U"), ("v", "V"), ("w", "A"), ("delp", "A"), ("pt", "A")):
        for k in range(npz):
            periodic_fill(bd, st[n][:, :, k], kind)
    for k in range(npz):
        periodic_fill(bd, q[:, :, k, 0], "A")
    fl = DynFlags(n_split=a.n_split, ptop=ptop, **(json.loads(a.flags) if a.flags else {}))
    ctx = L.Context(g, npz)
    if a.kessler:                                           # sphum, liq_wat, rainwat, the fake ice: the last three start empty
        q = np.asfortranarray(np.concatenate([q[..., :1], np.zeros(q.shape[:3] + (3,))], axis=3))
        fv = FvDynamics(ctx, fl, ak, bk, nq=4, k_split=1, adiabatic=False, c2l_ord=2, moist=dict(nwat=4, sphum=1, liq_wat=2, rainwat=3, ice_wat=4),
                        moist_phys=True)
    else:
        fv = FvDynamics(ctx, fl, ak, bk, nq=1, k_split=1, adiabatic=False, c2l_ord=2)
    fv.dc.set_state(st["u"], st["v"], st["w"], st["delp"], st["pt"], st["delz"], st["phis"])
    fv.set_tracers(q)
    ng = bd.ng
    c = (slice(ng, ng + nx), slice(ng, ng + nx))
    t_env = st["pt"][ng, ng, :].copy()                      # the sounding away from the bubble

    rain_acc = np.zeros((nx, nx))                           # kg/m2 = mm, summed over the steps

    def diag(t):
        d = fv.dc.d
        w, dp, T, qq, u = d["w"].download(), d["delp"].download(), d["pt"].download(), d["q"].download(), d["u"].download()
        r = {"t_s": t, "w_max": float(w[c].max()), "w_min": float(w[c].min()), "u_max": float(np.abs(u[ng:ng + nx, ng:ng + nx + 1]).max()),
             "dT_max": float((T[c] - t_env[None, None, :]).max()), "mass": float(dp[c].sum()), "vapour_mass": float((dp[c] * qq[c][..., 0]).sum()),
             "finite": bool(np.isfinite(w[c]).all())}
        if a.kessler:
            r.update(liq_wat_max=float(qq[c][..., 1].max()), liq_wat_min=float(qq[c][..., 1].min()), rainwat_max=float(qq[c][..., 2].max()),
                     rainwat_min=float(qq[c][..., 2].min()), rainwat_bottom_max=float(qq[c][:, :, -1, 2].max()),
                     water_mass=float((dp[c] * qq[c][..., :3].sum(axis=3)).sum()), rain_acc_max_mm=float(rain_acc.max()),
                     rain_acc_mean_mm=float(rain_acc.mean()), rain_cells=int(np.count_nonzero(rain_acc > 0.0)))
        return r
    out = [diag(0.0)]
    nsteps = int(round(a.minutes * 60.0 / a.dt_atmos))
    every = max(1, int(round(a.every / a.dt_atmos)))
    t0 = time.perf_counter()
    for n in range(1, nsteps + 1):
        if a.kessler:
            fv.supercell_step(a.dt_atmos, K_cycle=a.K_cycle, K_sedi_transport=a.K_sedi_transport, do_K_sedi_w=a.K_sedi_w,
                              do_K_sedi_heat=a.K_sedi_heat)
            rain_acc += fv.dc.d["rain"].download()
        else:
            fv.step_from_temperature(a.dt_atmos)
        if n % every == 0:
            out.append(diag(n * a.dt_atmos))
            if not out[-1]["finite"]:
                break
    ctx.sync()
    wall = time.perf_counter() - t0
    m0, v0 = out[0]["mass"], out[0]["vapour_mass"]
    phys = (f"Kessler warm rain (K_cycle {a.K_cycle}, transport {a.K_sedi_transport}, w {a.K_sedi_w}, heat {a.K_sedi_heat})" if a.kessler
            else "dry dynamics + vapour tracer")
    res = {"config": f"doubly periodic {nx} x {nx} x {npz}, dx = {a.dx} m, supercell IC (test_case 17), nonhydrostatic, {phys}, "
                     f"dt_atmos {a.dt_atmos} s x n_split {a.n_split}", "minutes": a.minutes, "steps": nsteps, "wall_s": wall,
           "mass_drift_rel": abs(out[-1]["mass"] - m0) / m0, "vapour_mass_drift_rel": abs(out[-1]["vapour_mass"] - v0) / v0,
           "w_max_overall": max(s["w_max"] for s in out), "build_id": L.build_id(), "series": out}
    if a.kessler:                                           # what fell out is rain * dA / (dA/grav) in the units of the masses above: Pa
        res.update(rain_reaches_ground=bool(rain_acc.max() > 0.0), rain_acc_max_mm=float(rain_acc.max()),
                   water_budget_rel=abs(out[-1]["water_mass"] + fl.grav * float(rain_acc.sum()) - out[0]["water_mass"]) / out[0]["water_mass"])
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
