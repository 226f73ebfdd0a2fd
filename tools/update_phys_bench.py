#!/usr/bin/env python3
"""What fv_update_phys costs: fv3_fv_update_phys on one 384 x 384 x 127 doubly periodic tile with nq = 7 tracers, timed with device
events.  The columns are those of the tests' recipe (tests/update_phys_inputs.py: sigma = linspace(0, 1, km+1)^1.5, T = 210 .. 300 K,
qv <= 1.5e-2 (pm / 1e5)^3, condensates <= 2e-4, dt = 225, q_dt changing a species by up to 5 %); delp, pt, q and delz are restored from
device copies before every call, because the routine updates what it is timed on.

Legs: hydrostatic (nwat 6, moist_cp, pkz rebuilt), nonhydrostatic nwat 6 (moist_cv and the tmax limiter), and the nonhydrostatic
call with q_dt absent; for scale the halo update of u_dt, v_dt and fv3_update_dwinds_phys, the rest of the sequence.
Algorithmic bytes per cell, computed from the shape -- what the routine has to read and write once:
  hydrostatic:     read delp, pt, t_dt, ua, va, u_dt, v_dt, nq of q, nq of q_dt; write delp, pt, ua, va, nq of q, pe, peln, pk, pkz
                   = (15 + 3 nq) x 8 = 288 for nq = 7;
  nonhydrostatic:  the same with delz read and written and the old pe read in the place of pkz = (17 + 3 nq) x 8 = 304;
  q_dt absent:     read delp, pt, t_dt, ua, va, u_dt, v_dt, delz, pe, the six species; write pt, ua, va, delz, pe, peln, pk = 22 x 8 = 176.
The share of the HBM roofline is these bytes over the kernel time over 8 TB/s.  Compare only within one run of this script.  The
kernel's own time, without the launch, comes from `rocprofv3 --kernel-trace --stats -- python tools/update_phys_bench.py --steps 3`
in a run of its own.

usage: update_phys_bench.py [--nx 384] [--npz 127] [--steps 10] [--warmup 3] [--out FILE.json]
       (default FILE: profiles/update_phys_bench_<build_id>.json)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8.0e12


def bytes_per_cell(hydrostatic, has_qdt, nq, nwat_species=6):
    if not has_qdt:
        return (7 + (0 if hydrostatic else 2) + nwat_species + 3 + 4) * 8      # (the fourth written: pkz when hydrostatic, else delz)
    return ((15 if hydrostatic else 17) + 3 * nq) * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=384)
    ap.add_argument("--npz", type=int, default=127)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from gfdl_atmos_cubed_sphere_amd import lib as L
    from gfdl_atmos_cubed_sphere_amd.grid import doubly_periodic
    from gfdl_atmos_cubed_sphere_amd.layout import Bounds
    nx, km, nq = a.nx, a.npz, 7
    bd = Bounds(1, nx, 1, nx)
    ng = bd.ng
    g = doubly_periodic(bd, nx + 1, nx + 1, dx_const=26000.0, dy_const=26000.0)
    ctx = L.Context(g, km, stream=torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(7)
    rdgas, rvgas, grav, kappa, ptop, dt = L.RDGAS, 461.50, L.GRAV, L.KAPPA, 300.0, 225.0
    sig = np.linspace(0.0, 1.0, km + 1) ** 1.5
    ps = rng.uniform(9.5e4, 1.02e5, (nx + 2, nx + 2))
    pe = np.asfortranarray(np.transpose(ptop * (1.0 - sig)[None, None, :] + sig[None, None, :] * ps[:, :, None], (0, 2, 1)))
    pec = np.transpose(pe[1:-1, :, 1:-1], (0, 2, 1))
    pl = np.log(pec)
    dpc, dl = np.diff(pec, axis=2), np.diff(pl, axis=2)
    pm = dpc / dl
    T = 210.0 + 90.0 * (pm / 1.0e5) + 3.0 * rng.standard_normal((nx, nx, km))
    q = rng.uniform(0.0, 1.0, (nx, nx, km, nq))
    q[..., 0] *= 1.5e-2 * (pm / 1.0e5) ** 3
    q[..., 1:6] *= 2.0e-4
    delz = -rdgas * T * (1.0 + (rvgas / rdgas - 1.0) * q[..., 0]) * dl / grav

    def halo(c, fill=0.0):
        x = np.full(bd.shape("A", km) + c.shape[3:], fill, order="F")
        x[ng:ng + nx, ng:ng + nx] = c
        return x
    f32 = lambda s, shape: np.asfortranarray(s * rng.standard_normal(shape))      # noqa: E731
    host = dict(delp=halo(dpc, 1.0e3), pt=halo(T), q=halo(q), ua=halo(f32(10.0, (nx, nx, km))), va=halo(f32(10.0, (nx, nx, km))),
                w=halo(f32(0.5, (nx, nx, km))), delz=np.asfortranarray(delz), t_dt=f32(2.0e-3, (nx, nx, km)),
                q_dt=np.asfortranarray(q * rng.uniform(-0.05, 0.05, q.shape) / dt), u_dt=f32(1.0e-3, bd.shape("A", km)),
                v_dt=f32(1.0e-3, bd.shape("A", km)), pe=pe, peln=np.asfortranarray(np.transpose(pl, (0, 2, 1))),
                pk=np.asfortranarray(np.exp(kappa * pl)))
    del q, T, delz, pm, dpc, dl, pec, pl
    d = {n: ctx.from_host(x) for n, x in host.items()}
    keep = {n: ctx.from_host(host[n]) for n in ("delp", "pt", "q", "delz")}
    d["pkz"] = ctx.zeros("CC", km)
    d["ps"], d["u_srf"], d["v_srf"] = ctx.zeros("A"), ctx.zeros("CC"), ctx.zeros("CC")
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

    def up(hyd, has_qdt):
        return lambda: ctx.fv_update_phys(dt, ptop, hyd, nq, nq, 6, species, d["u_dt"], d["v_dt"], d["t_dt"], d["q_dt"] if has_qdt else None,
                                          d["delp"], d["pt"], d["q"], None, d["ua"], d["va"], None if hyd else d["w"], None if hyd else d["delz"],
                                          d["ps"], d["pe"], d["peln"], d["pk"], d["pkz"] if hyd else None, d["u_srf"], d["v_srf"],
                                          phys_hydrostatic=False)
    rows = {}
    cells = nx * nx * km
    for name, hyd, has_qdt in (("hydrostatic_nwat6", True, True), ("nonhydrostatic_nwat6", False, True), ("nonhydrostatic_no_q_dt", False, False)):
        r = timed(up(hyd, has_qdt), restore)
        pt = d["pt"].download()[ng:ng + nx, ng:ng + nx]
        r.update(bytes_per_cell=bytes_per_cell(hyd, has_qdt, nq), bytes=bytes_per_cell(hyd, has_qdt, nq) * cells, finite=bool(np.isfinite(pt).all()),
                 share_of_cells_limited=float((pt == 330.0).mean()))
        rows[name] = r
    r = timed(lambda: ctx.halo_periodic_group([(d["u_dt"], "A"), (d["v_dt"], "A")]))
    rows["halo_u_dt_v_dt"] = r
    r = timed(lambda: ctx.update_dwinds_phys(dt, d["u_dt"], d["v_dt"], d["u"], d["v"]))
    r.update(bytes=6 * 8 * cells)
    rows["update_dwinds_phys"] = r
    for r in rows.values():
        if "bytes" in r:
            r["bytes_per_s"] = r["bytes"] / (r["ms_median"] * 1.0e-3)
            r["of_8TBps"] = r["bytes_per_s"] / PEAK
    res = dict(build_id=L.build_id(), nx=nx, npz=km, nq=nq, steps=a.steps, device=torch.cuda.get_device_name(0), rows=rows)
    out = a.out or os.path.join(ROOT, "profiles", f"update_phys_bench_{L.build_id()}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
