#!/usr/bin/env python3
"""What fv_subgrid_z costs: fv3_fv_subgrid_z and fv3_update_dwinds_phys on one 384 x 384 x 127 doubly periodic tile, nonhydrostatic,
nwat = 6, nq = 7 mixed tracers, timed with device events.  The columns are those of the tests' recipe (sigma = linspace(0, 1, km+1)^1.5,
theta = 290 (1e5 / pm)^0.05 + 3 K N(0, 1), winds 10 m/s N(0, 1), w 0.5 N(0, 1), qv <= 1.5e-2 (pm / 1e5)^3, condensates <= 2e-4, dt = 225,
fv_sg_adj = 600), so the share of layer pairs that mix is the one the tests see; the state is restored from device copies before every
call, because the routine mixes what it is timed on.

Rows: the column kernel at full depth (k_bot_full = npz) and at k_bot_full = 30, the wind update, and for scale the vertical remap
(every kernel under the reference's `Remapping` timer) of one model step of FvDynamics on a tile of the same size with the same
number of tracers, in the same process.  Algorithmic bytes per cell of the column kernel, levels 1..kbot: read delp, pkz, delz, peln
(+1/km) and T, u, v, w, nq tracers; write T, u, v, w, nq tracers, u_dt, v_dt = (8 + 2 nq + 6) x 8 = 224 for nq = 7.  What the kernel
moves beyond that is its work array: (7 + nq) fields written once and read and written once per sweep and read once at the end, 8 x
(7 + nq) x 8 = 896 bytes per cell more, plus the tracers of a mixing pair a second time.  The wind update: u_dt, v_dt read, u, v read
and written = 48.  Compare only within one run of this script.

usage: subgrid_bench.py [--nx 384] [--npz 127] [--steps 10] [--warmup 3] [--out FILE.json]
       (default FILE: profiles/subgrid_bench_<build_id>.json)"""
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
    ap.add_argument("--kbot", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from gfdl_atmos_cubed_sphere_amd import lib as L
    from gfdl_atmos_cubed_sphere_amd import synthetic as N
    from gfdl_atmos_cubed_sphere_amd.dyn_core import DynFlags
    from gfdl_atmos_cubed_sphere_amd.fv_dynamics import FvDynamics
    from gfdl_atmos_cubed_sphere_amd.grid import doubly_periodic
    from gfdl_atmos_cubed_sphere_amd.layout import Bounds
    nx, km, nq = a.nx, a.npz, 7
    bd = Bounds(1, nx, 1, nx)
    ng = bd.ng
    g = doubly_periodic(bd, nx + 1, nx + 1, dx_const=26000.0, dy_const=26000.0)
    ctx = L.Context(g, km, stream=torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(7)
    rdgas, rvgas, grav, kappa, ptop = L.RDGAS, 461.50, L.GRAV, L.KAPPA, 300.0
    sig = np.linspace(0.0, 1.0, km + 1) ** 1.5
    ps = rng.uniform(9.5e4, 1.02e5, (nx + 2, nx + 2))
    pe = np.asfortranarray(np.transpose(ptop * (1.0 - sig)[None, None, :] + sig[None, None, :] * ps[:, :, None], (0, 2, 1)))
    pec = np.transpose(pe[1:-1, :, 1:-1], (0, 2, 1))
    pl = np.log(pec)
    dpc, dl = np.diff(pec, axis=2), np.diff(pl, axis=2)
    pm = dpc / dl
    pkz = np.diff(np.exp(kappa * pl), axis=2) / (kappa * dl)
    T = (290.0 * (1.0e5 / pm) ** 0.05 + 3.0 * rng.standard_normal((nx, nx, km))) * pkz * (1.0e5 ** -kappa)
    q = rng.uniform(0.0, 1.0, (nx, nx, km, nq))
    q[..., 0] *= 1.5e-2 * (pm / 1.0e5) ** 3
    q[..., 1:6] *= 2.0e-4
    delz = -rdgas * T * (1.0 + (rvgas / rdgas - 1.0) * q[..., 0]) * dl / grav

    def halo(c, fill=0.0):
        x = np.full(bd.shape("A", km) + c.shape[3:], fill, order="F")
        x[ng:ng + nx, ng:ng + nx] = c
        return x
    host = dict(delp=halo(dpc, 1.0e3), ta=halo(T), qa=halo(q), ua=halo(10.0 * rng.standard_normal((nx, nx, km))),
                va=halo(10.0 * rng.standard_normal((nx, nx, km))), w=halo(0.5 * rng.standard_normal((nx, nx, km))),
                peln=np.asfortranarray(np.transpose(pl, (0, 2, 1))), pkz=np.asfortranarray(pkz), delz=np.asfortranarray(delz))
    d = {n: ctx.from_host(x) for n, x in host.items()}
    keep = {n: ctx.from_host(host[n]) for n in ("ta", "qa", "ua", "va", "w")}
    d["u_dt"], d["v_dt"] = ctx.zeros("A", km), ctx.zeros("A", km)
    d["u"], d["v"] = ctx.zeros("U", km), ctx.zeros("V", km)
    species = dict(sphum=1, liq_wat=2, rainwat=3, ice_wat=4, snowwat=5, graupel=6)

    def restore():
        for n, x in keep.items():
            d[n].copy_from(x)

    def timed(fn, restore=None):
        for _ in range(a.warmup):
            if restore:
                restore()
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.steps):
            if restore:
                restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        return dict(ms_median=ms[len(ms) // 2], ms_min=ms[0], ms_max=ms[-1])

    def sg(kbf):
        return lambda: ctx.fv_subgrid_z(False, nq, 6, species, kbf, 600, 0, 225.0, ptop, d["delp"], None, d["peln"], d["pkz"], d["ta"], d["qa"],
                                        d["ua"], d["va"], d["w"], d["delz"], d["u_dt"], d["v_dt"])
    rows = {}
    cols = nx * nx
    for name, kbf in ((f"fv_subgrid_z_kbot{a.kbot}", min(a.kbot, km)), ("fv_subgrid_z_full_depth", km)):      # (the smaller work array first)
        r = timed(sg(kbf), restore)
        ua = d["ua"].download()[ng:ng + nx, ng:ng + nx, :kbf]
        r.update(kbot=kbf, bytes=(8 + 2 * nq + 6) * 8 * cols * kbf, work_array_bytes=(7 + nq) * 8 * cols * kbf,
                 share_of_u_cells_changed=float((ua != host["ua"][ng:ng + nx, ng:ng + nx, :kbf]).mean()), finite=bool(np.isfinite(ua).all()))
        rows[name] = r
    r = timed(lambda: ctx.update_dwinds_phys(225.0, d["u_dt"], d["v_dt"], d["u"], d["v"]))
    r.update(bytes=6 * 8 * cols * km)
    rows["update_dwinds_phys"] = r
    for r in rows.values():
        r["bytes_per_s"] = r["bytes"] / (r["ms_median"] * 1.0e-3)
        r["of_8TBps"] = r["bytes_per_s"] / PEAK
    for x in list(d.values()) + list(keep.values()):
        x.free()
    # for scale: the vertical remap of one model step on the same tile with the same number of tracers
    st, _ = N.balanced_nh_state(bd, km)
    ak, bk = N.PTOP * (1.0 - sig), sig.copy()
    fv = FvDynamics(ctx, DynFlags(n_split=5, ptop=N.PTOP), ak, bk, nq=nq, k_split=2)
    fv.dc.set_state(st["u"], st["v"], st["w"], st["delp"], st["pt"], st["delz"], st["phis"])
    fv.set_tracers(np.asfortranarray(np.random.default_rng(1).uniform(0, 1, bd.shape("A", km) + (nq,))))
    fv.step(225.0)
    ctx.sync()
    ctx.profile(True)
    fv.step(225.0)
    rep = ctx.profile_report()
    ctx.profile(False)
    remap = {k: v for k, v in rep.items() if k.startswith("remap")}
    calls = 2                                                # k_split
    rows["lagrangian_to_eulerian"] = dict(ms_per_call=sum(v[1] for v in remap.values()) / calls, kernels={k: list(v) for k, v in remap.items()})
    res = dict(build_id=L.build_id(), nx=nx, npz=km, nq=nq, steps=a.steps, device=torch.cuda.get_device_name(0), rows=rows)
    out = a.out or os.path.join(ROOT, "profiles", f"subgrid_bench_{L.build_id()}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
