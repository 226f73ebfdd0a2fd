#!/usr/bin/env python3
"""What the Reed-Jablonowski simple physics costs, timed with device events in one process.

Tile legs, one 384 x 384 x 127 doubly periodic tile with a seeded latitude field and the columns of the tests' recipe
(tests/reed_inputs.py): fv3_reed_sim_phys alone per branch set -- (do_reed_cond, reed_cond_only, reed_alt_mxg) of the four flag sets,
the height form both hydrostatic and not --, each with fresh and with incoming tendencies; fv3_terminator_advance alone.
Sphere legs, the six C96 L79 faces of the Jablonowski-Williamson state with the moisture of the moist baroclinic wave as one fv3_group:
the kernel alone (fresh), the whole FvDynamics.reed_sim_phys, FvDynamics.moist_forced_step, and the share of the second in the third.

Bytes per cell the kernel actually ISSUES (8 B each; peln and pe once per level and walk, the neighbouring level from the cache):
  the sweep up:   delp, pt, q, peln, pe, ua, va read = 7; CE, CEm, CFu, CFv, CFt, CFq written to the work planes = 6;
                  the height form reads pt, q of the level again for zint when hydrostatic = +2, delz when not = +1
  the sweep down: delp, pt, q, peln, ua, va read = 6; the six work planes read = 6; u_dt, v_dt, t_dt, q_dt written = 4;
                  without fresh the four are read as well = +4
  => 29 per cell with fresh (232 B), of which 12 are the work planes' round trip; reed_cond_only is the sweep down alone without the
     winds and the work planes: 4 read, 4 written (+4 without fresh).
The share of the HBM roofline is these bytes over the kernel time over 8 TB/s.  Compare only within one run of this script.

usage: reed_bench.py [--nx 384] [--npz 127] [--steps 10] [--warmup 3] [--no-sphere] [--out FILE.json]
       (default FILE: profiles/reed_bench_<build_id>.json)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8.0e12


def words_per_cell(flags, hydrostatic, fresh):
    """(all, of which work planes) 8-byte words per cell the kernel issues"""
    cnd, only, alt = flags
    if only:
        return 8 + (0 if fresh else 4), 0
    return 29 + ((2 if hydrostatic else 1) if alt else 0) + (0 if fresh else 4), 12


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
    import reed_inputs as RI
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
    bd, st = RI.state(nx, nx, km, 7)
    g = doubly_periodic(bd, nx + 1, nx + 1, dx_const=26000.0, dy_const=26000.0)
    ctx = L.Context(g, km, stream=torch.cuda.current_stream().cuda_stream)
    ctx.grid_upload_reed(1, st["lat"], consts=RI.CONSTS)
    d = {n: ctx.from_host(st[n]) for n in RI.DEVICE}
    cells = nx * nx * km
    for name, flags in RI.FLAGS.items():
        for hyd in ((True, False) if flags[2] else (True,)):
            for fresh in (True, False):
                w, wk = words_per_cell(flags, hyd, fresh)
                r = timed(lambda: ctx.reed_sim_phys(225.0, d["delp"], d["pt"], d["ua"], d["va"], d["q"], d["pe"], d["peln"], d["phis"], d["delz"],
                                                    d["u_dt"], d["v_dt"], d["t_dt"], d["q_dt"], d["rain"], hydrostatic=hyd, reed_test=1,
                                                    do_reed_cond=flags[0], reed_cond_only=flags[1], reed_alt_mxg=flags[2], fresh=fresh, consts=RI.CONSTS))
                r.update(bytes_per_cell=8.0 * w, work_plane_bytes_per_cell=8.0 * wk, bytes=8.0 * w * cells,
                         finite=bool(all(np.isfinite(d[n].download()).all() for n in ("t_dt", "q_dt", "rain"))))
                rows[f"tile_kernel_{name}{'' if hyd else '_nh'}_{'fresh' if fresh else 'incoming'}"] = r
    tbd, tst = RI.term_state(nx, nx, km, 8)
    ctx.grid_upload_terminator(tst["agrid"], RI.PI)
    cl, cl2 = ctx.from_host(tst["cl"]), ctx.from_host(tst["cl2"])
    r = timed(lambda: ctx.terminator_advance(km, 225.0, cl, cl2, term_fill_negative=True))
    tcells = int(np.prod(bd.shape("A", km)))
    r.update(bytes_per_cell=8.0 * 4 + 8.0 / km, bytes=(8.0 * 4 + 8.0 / km) * tcells, finite=bool(np.isfinite(cl.download()).all()))
    rows["tile_terminator_advance"] = r
    ctx.close()
    # ---- the sphere: C96 L79, hydrostatic, as tools/jw_long_run.py --reed sets it up
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
        fv = FvDynamics(mctx, fl, ak, bk, nq=1, k_split=2, halo=CubeHaloAdapter(mctx, npx, topo=cs.topo), moist=dict(nwat=1, sphum=1), moist_phys=True)
        eta = (0.5 * (ak[1:] + ak[:-1]) / 1.0e5 + 0.5 * (bk[1:] + bk[:-1]))[None, None, :]
        fv.set_tracers([np.asfortranarray((0.021 * np.exp(-(cs.grids[t]["agrid"][..., 1:2] / (2.0 * np.pi / 9.0)) ** 4)
                                           * np.exp(-((eta - 1.0) * 1.0e5 / 34000.0) ** 2))[..., None]) for t in range(6)])
        zero = np.zeros_like(s6[0]["delp"])
        fv.dc.set_state([s_["u"] for s_ in s6], [s_["v"] for s_ in s6], [zero for _ in s6], [s_["delp"] for s_ in s6],
                        [s_["pt"] for s_ in s6], [sbd.zeros("CC", npz) for _ in s6], [s_["phis"] for s_ in s6])
        pkz = []
        for s_ in s6:      # p_var: the hydrostatic T -> theta_v conversion of fv_dynamics divides by the resident pkz
            pe = ak[0] + np.concatenate([np.zeros(s_["delp"].shape[:2] + (1,)), np.cumsum(s_["delp"], axis=2)], axis=2)[sbd.ng:sbd.ng + 96, sbd.ng:sbd.ng + 96]
            pln = np.log(pe)
            pkz.append(np.asfortranarray((pe[:, :, 1:] ** fl.akap - pe[:, :, :-1] ** fl.akap) / (fl.akap * (pln[:, :, 1:] - pln[:, :, :-1]))))
        fv.dc.d["pkz"].upload(pkz)
        fv.moist_forced_step(1800.0, reed_test=1)
        dd = fv.dc.d
        scells = 6 * 96 * 96 * npz
        from gfdl_atmos_cubed_sphere_amd.fv_dynamics import _TracerView

        def kernel():
            for t, c in enumerate(mctx.ctxs):
                c.reed_sim_phys(1800.0, dd["delp"][t], dd["pt"][t], dd["ua"][t], dd["va"][t], _TracerView(dd["q"][t], 0), dd["pe"][t], dd["peln"][t],
                                dd["phis"][t], None, dd["u_dt"][t], dd["v_dt"][t], dd["t_dt"][t], _TracerView(dd["q_dt"][t], 0), dd["rain"][t],
                                reed_test=1, fresh=True)
            mctx.flush()
        r = timed(kernel)
        r.update(cells=scells, bytes_per_cell=8.0 * 29, bytes=8.0 * 29 * scells)
        rows["sphere_kernel_cond_fresh"] = r
        rows["sphere_reed_sim_phys_step"] = timed(lambda: (fv.reed_sim_phys(1800.0, reed_test=1), mctx.flush()))
        rows["sphere_moist_forced_step"] = timed(lambda: (fv.moist_forced_step(1800.0, reed_test=1), mctx.flush()))
        rows["sphere_reed_share_of_moist_forced_step"] = rows["sphere_reed_sim_phys_step"]["ms_median"] / rows["sphere_moist_forced_step"]["ms_median"]
        rows["sphere_finite"] = bool(all(np.isfinite(x).all() for x in dd["pt"].download()))
        mctx.close()
    for r in rows.values():
        if isinstance(r, dict) and "bytes" in r:
            r["bytes_per_s"] = r["bytes"] / (r["ms_median"] * 1.0e-3)
            r["of_8TBps"] = r["bytes_per_s"] / PEAK
    res = dict(build_id=L.build_id(), nx=nx, npz=km, steps=a.steps, device=torch.cuda.get_device_name(0), rows=rows)
    out = a.out or os.path.join(ROOT, "profiles", f"reed_bench_{L.build_id()}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
