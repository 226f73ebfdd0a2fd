#!/usr/bin/env python3
"""What the Held-Suarez forcing costs, timed with device events in one process.

Tile legs, one 384 x 384 x 127 doubly periodic tile with a seeded latitude field and the columns of the tests' recipe
(tests/held_suarez_inputs.py: interfaces spaced geometrically from 1 Pa, so with strat every column has all three branches):
fv3_held_suarez_tend alone in the standard form and with strat, each with and without fresh; then the whole held_suarez step --
the kernel with fresh, fv3_fv_update_phys without q_dt, the halo update of u_dt, v_dt and fv3_update_dwinds_phys.
Sphere legs, the six C96 L79 faces of the Jablonowski-Williamson state as one fv3_group: the kernel alone (strat, fresh), the whole
FvDynamics.held_suarez, FvDynamics.forced_step, and the share of the second in the third.

Algorithmic bytes per cell, computed from what a branch has to read and write once (8 B each):
  without fresh: read delp, peln, pt, t_dt; write t_dt                                    = 5; troposphere standard form + pkz = 6;
                 where the friction acts + ua, va, u_dt, v_dt read and u_dt, v_dt written  = 12 (the 96 B of the full set)
  with fresh:    t_dt, u_dt, v_dt are not read and all three are written everywhere        = 6 / 7 / 9
The script weighs the cases with the share of cells in each branch, counted on the host from the same inputs.  The share of the HBM
roofline is these bytes over the kernel time over 8 TB/s.  Compare only within one run of this script.

usage: held_suarez_bench.py [--nx 384] [--npz 127] [--steps 10] [--warmup 3] [--no-sphere] [--out FILE.json]
       (default FILE: profiles/held_suarez_bench_<build_id>.json)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=384)
    ap.add_argument("--npz", type=int, default=127)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-sphere", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import held_suarez_inputs as HI
    from gfdl_atmos_cubed_sphere_amd import lib as L
    from gfdl_atmos_cubed_sphere_amd.grid import doubly_periodic

    def timed(fn, before=None):
        for _ in range(a.warmup):
            if before:
                before()
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.steps):
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        return dict(ms_median=ms[len(ms) // 2], ms_min=ms[0], ms_max=ms[-1])

    rows = {}
    # ---- the tile
    nx, km = a.nx, a.npz
    bd, st = HI.state(nx, nx, km, 7)
    g = doubly_periodic(bd, nx + 1, nx + 1, dx_const=26000.0, dy_const=26000.0)
    ctx = L.Context(g, km, stream=torch.cuda.current_stream().cuda_stream)
    ctx.upload_lat(st["lat"])
    d = {n: ctx.from_host(st[n]) for n in HI.DEVICE}
    cells = nx * nx * km
    ng = bd.ng
    pl = st["delp"][ng:ng + nx, ng:ng + nx] / np.transpose(st["peln"][:, 1:, :] - st["peln"][:, :-1, :], (0, 2, 1))
    sig = pl / st["pe"][1:-1, km, 1:-1][:, :, None]
    for name, strat in (("standard", False), ("strat", True)):
        upper = (pl <= 1.0e4) if strat else np.zeros(pl.shape, dtype=bool)
        fr = ~upper & (sig > 0.7)
        share = dict(strat_meso=float(upper.mean()), troposphere=float((~upper & ~fr).mean()), friction=float(fr.mean()))
        for fresh in (False, True):
            per = (6, 7, 9) if fresh else (5, 6, 12)
            bpc = 8.0 * (per[0] * share["strat_meso"] + per[1] * share["troposphere"] + per[2] * share["friction"])
            r = timed(lambda: ctx.held_suarez_tend(225.0, d["delp"], d["peln"], d["pe"], d["pkz"], d["pt"], d["ua"], d["va"], d["u_dt"], d["v_dt"],
                                                   d["t_dt"], strat=strat, fresh=fresh))
            r.update(bytes_per_cell=bpc, bytes=bpc * cells, share_of_cells=share, finite=bool(np.isfinite(d["t_dt"].download()).all()))
            rows[f"tile_kernel_{name}_{'fresh' if fresh else 'incoming'}"] = r
    up = {n: ctx.zeros(k, km) for n, k in (("u", "U"), ("v", "V"))}
    up.update(ps=ctx.zeros("A"), u_srf=ctx.zeros("CC"), v_srf=ctx.zeros("CC"),
              pk=ctx.from_host(np.asfortranarray(np.exp(HI.KAPPA * np.transpose(st["peln"], (0, 2, 1))))))
    keep = ctx.from_host(st["pt"])

    def hs_step():
        ctx.held_suarez_tend(225.0, d["delp"], d["peln"], d["pe"], d["pkz"], d["pt"], d["ua"], d["va"], d["u_dt"], d["v_dt"], d["t_dt"], fresh=True)
        ctx.fv_update_phys(225.0, 1.0, True, 0, 0, 0, {}, d["u_dt"], d["v_dt"], d["t_dt"], None, d["delp"], d["pt"], None, None, d["ua"], d["va"],
                           None, None, up["ps"], d["pe"], d["peln"], up["pk"], d["pkz"], up["u_srf"], up["v_srf"])
        ctx.halo_periodic_group([(d["u_dt"], "A"), (d["v_dt"], "A")])
        ctx.update_dwinds_phys(225.0, d["u_dt"], d["v_dt"], up["u"], up["v"])
    rows["tile_held_suarez_step"] = timed(hs_step, lambda: d["pt"].copy_from(keep))
    ctx.close()
    # ---- the sphere: C96 L79, hydrostatic, as tools/jw_long_run.py sets it up
    if not a.no_sphere:
        from gfdl_atmos_cubed_sphere_amd.cubed_dyn import CubeHaloAdapter, MultiContext
        from gfdl_atmos_cubed_sphere_amd.cubed_sphere import CubedSphere
        from gfdl_atmos_cubed_sphere_amd.dyn_core import DynFlags
        from gfdl_atmos_cubed_sphere_amd.fv_dynamics import FvDynamics
        from gfdl_atmos_cubed_sphere_amd.test_cases import jablonowski_williamson, set_eta
        npx, npz = 97, 79
        cs = CubedSphere(npx)
        gs = [cs.gridstruct(t) for t in range(6)]
        sbd = gs[0].bd
        ak, bk, _, _ = set_eta(npz)
        s6 = jablonowski_williamson(cs, ak, bk, hydrostatic=True)
        cs.topo.update("A", [s_["phis"] for s_ in s6])
        fl = DynFlags(n_split=6, hydrostatic=True, ptop=float(ak[0]), d_ext=0.0)
        mctx = MultiContext([L.Context(g_, npz, stream=torch.cuda.current_stream().cuda_stream) for g_ in gs])
        fv = FvDynamics(mctx, fl, ak, bk, nq=0, k_split=2, halo=CubeHaloAdapter(mctx, npx, topo=cs.topo))
        zero = np.zeros_like(s6[0]["delp"])
        fv.dc.set_state([s_["u"] for s_ in s6], [s_["v"] for s_ in s6], [zero for _ in s6], [s_["delp"] for s_ in s6],
                        [s_["pt"] for s_ in s6], [sbd.zeros("CC", npz) for _ in s6], [s_["phis"] for s_ in s6])
        pkz = []
        for s_ in s6:      # p_var: the hydrostatic T -> theta_v conversion of fv_dynamics divides by the resident pkz
            pe = ak[0] + np.concatenate([np.zeros(s_["delp"].shape[:2] + (1,)), np.cumsum(s_["delp"], axis=2)], axis=2)[sbd.ng:sbd.ng + 96, sbd.ng:sbd.ng + 96]
            pln = np.log(pe)
            pkz.append(np.asfortranarray((pe[:, :, 1:] ** fl.akap - pe[:, :, :-1] ** fl.akap) / (fl.akap * (pln[:, :, 1:] - pln[:, :, :-1]))))
        fv.dc.d["pkz"].upload(pkz)
        fv.forced_step(1800.0)
        dd = fv.dc.d
        scells = 6 * 96 * 96 * npz
        r = timed(lambda: (mctx.held_suarez_tend(1800.0, dd["delp"], dd["peln"], dd["pe"], dd["pkz"], dd["pt"], dd["ua"], dd["va"], dd["u_dt"],
                                                 dd["v_dt"], dd["t_dt"], fresh=True), mctx.flush()))
        r.update(cells=scells)
        rows["sphere_kernel_strat_fresh"] = r
        rows["sphere_held_suarez_step"] = timed(lambda: (fv.held_suarez(1800.0), mctx.flush()))
        rows["sphere_forced_step"] = timed(lambda: (fv.forced_step(1800.0), mctx.flush()))
        rows["sphere_held_suarez_share_of_forced_step"] = rows["sphere_held_suarez_step"]["ms_median"] / rows["sphere_forced_step"]["ms_median"]
        finite = bool(all(np.isfinite(x).all() for x in dd["pt"].download()))
        rows["sphere_finite"] = finite
        mctx.close()
    for r in rows.values():
        if isinstance(r, dict) and "bytes" in r:
            r["bytes_per_s"] = r["bytes"] / (r["ms_median"] * 1.0e-3)
            r["of_8TBps"] = r["bytes_per_s"] / PEAK
    res = dict(build_id=L.build_id(), nx=nx, npz=km, steps=a.steps, device=torch.cuda.get_device_name(0), rows=rows)
    out = a.out or os.path.join(ROOT, "profiles", f"held_suarez_bench_{L.build_id()}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
