#!/usr/bin/env python3
"""What the Kessler warm-rain microphysics costs, timed with device events in one process.

Tile legs, one 384 x 384 x 127 doubly periodic tile with the columns of the tests' recipe (tests/kessler_inputs.py): fv3_k_warm_rain
alone for K_cycle 1, 2, 8, both moist_kappa forms, the flag sets (none) and (transport, w, heat), nonhydrostatic.  The state is
uploaded again before every timed call (the routine changes it in place), outside the timed interval.
Step legs, the supercell case (test_case 17) on the same 384 x 384 x 127 tile -- the block one GPU holds of BASELINE config 4's
domain --: FvDynamics.k_warm_rain alone, FvDynamics.supercell_step, and the share of the first in the second.

8-byte words per cell the kernel ISSUES (the level above comes from registers, the bottom level's entry state once per column):
  K_cycle = 1:  read delp, pt, the three tracers, delz (peln when hydrostatic), ua, va, u_dt, v_dt = 10; written pt, delp, the three
                tracers, u_dt, v_dt, pe, peln, pk = 10; K_sedi_transport writes ua, va = +2; do_K_sedi_w reads and writes w = +2;
                do_K_sedi_heat reads delz, which is in the cache when not hydrostatic
  K_cycle > 1:  the first cycle reads the 6 inputs (+ ua, va, w with the transports) and writes the planes t1, q1, q2, q3, drym, dz, qa,
                qb, qc = 9 (+ u1, v1, w1); a middle cycle reads the 9 planes and delp = 10 (+ 3; + delz with the heat transport) and
                writes t1, q1, q2, q3 = 4 (+ 3); the last cycle reads the same and ua, va, u_dt, v_dt = +4 and writes the 10 (+ 3)
                outputs.  So the sweeps re-read the state from HBM once per cycle: 14 (+ 6, + 1) words per cell and extra cycle.
The share of the HBM roofline is these bytes over the kernel time over 8 TB/s.  Compare only within one run of this script.

usage: kessler_bench.py [--nx 384] [--npz 127] [--steps 10] [--warmup 3] [--no-step] [--out FILE.json]
       (default FILE: profiles/kessler_bench_<build_id>.json)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8.0e12


def words_per_cell(K, tr, sw, sh, hydrostatic=False):
    """(all, of which work planes) 8-byte words per cell the kernel issues"""
    x = (2 if tr else 0) + (1 if sw else 0)              # u1, v1, w1
    heat = 1 if (sh and hydrostatic) else 0              # delz beside peln
    if K == 1:
        return 10 + (1 if sw else 0) + heat + 10 + x, 0
    first = 6 + x + heat + 9 + x
    mid = 10 + x + (1 if sh else 0) + 4 + x
    last = 10 + x + (1 if sh else 0) + 4 + 10 + x
    planes = (9 + x) + (K - 2) * (9 + x + 4 + x) + (9 + x)
    return first + (K - 2) * mid + last, planes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=384)
    ap.add_argument("--npz", type=int, default=127)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import kessler_inputs as KI
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
    bd, st = KI.state(nx, nx, km, 7, hydrostatic=False)
    g = doubly_periodic(bd, nx + 1, nx + 1, dx_const=500.0, dy_const=500.0)
    ctx = L.Context(g, km, stream=torch.cuda.current_stream().cuda_stream)
    ctx.qs_wat_init(KI.CONSTS)
    d = {n: ctx.from_host(st[n]) for n in KI.STATE}
    keep = {n: ctx.from_host(st[n]) for n in KI.STATE}       # the routine changes the state in place: every call starts from this copy
    cells = nx * nx * km

    def restore():
        for n in KI.STATE:
            d[n].copy_from(keep[n])
    for name in ("none", "trwh"):
        tr, sw, sh = KI.FLAGS[name]
        for mk in (False, True):
            for K in (1, 2, 8):
                w, wk = words_per_cell(K, tr, sw, sh)
                r = timed(lambda: ctx.k_warm_rain(240.0, d["ua"], d["va"], d["w"], d["u_dt"], d["v_dt"], d["q"], d["pt"], d["delp"], d["delz"],
                                                  d["pe"], d["peln"], d["pk"], d["ps"], d["rain"], KI.NQ, K_cycle=K, K_sedi_transport=tr,
                                                  do_K_sedi_w=sw, do_K_sedi_heat=sh, hydrostatic=False, moist_kappa=mk, consts=KI.CONSTS),
                          before=restore)
                r.update(bytes_per_cell=8.0 * w, work_plane_bytes_per_cell=8.0 * wk, bytes=8.0 * w * cells,
                         finite=bool(all(np.isfinite(d[n].download()).all() for n in ("pt", "q", "rain", "pk"))))
                rows[f"tile_kernel_{name}_{'mk' if mk else 'dry'}_K{K}"] = r
    ctx.close()
    # ---- the supercell step on the same tile, as tools/supercell_run.py --kessler sets it up
    if not a.no_step:
        from gfdl_atmos_cubed_sphere_amd.dyn_core import DynFlags
        from gfdl_atmos_cubed_sphere_amd.fv_dynamics import FvDynamics
        from gfdl_atmos_cubed_sphere_amd.layout import periodic_fill
        from gfdl_atmos_cubed_sphere_amd.test_cases import supercell
        sig = np.linspace(0.0, 1.0, km + 1) ** 1.2
        ptop = 5000.0
        ak, bk = ptop * (1.0 - sig), sig.copy()
        s = supercell(bd, km, ak, bk, 500.0, 500.0, dt_amp=2.0, dt_rad=10.0e3)
        q = s.pop("q")
        for n, kind in (("u", "U"), ("v", "V"), ("w", "A"), ("delp", "A"), ("pt", "A")):
            for k in range(km):
                periodic_fill(bd, s[n][:, :, k], kind)
        for k in range(km):
            periodic_fill(bd, q[:, :, k, 0], "A")
        q = np.asfortranarray(np.concatenate([q[..., :1], np.zeros(q.shape[:3] + (3,))], axis=3))
        ctx = L.Context(g, km, stream=torch.cuda.current_stream().cuda_stream)
        fv = FvDynamics(ctx, DynFlags(n_split=8, ptop=ptop), ak, bk, nq=4, k_split=1, adiabatic=False, c2l_ord=2,
                        moist=dict(nwat=4, sphum=1, liq_wat=2, rainwat=3, ice_wat=4), moist_phys=True)
        fv.dc.set_state(s["u"], s["v"], s["w"], s["delp"], s["pt"], s["delz"], s["phis"])
        fv.set_tracers(q)
        dt = 6.0
        fv.supercell_step(dt)
        rows["step_k_warm_rain_K1"] = timed(lambda: fv.k_warm_rain(dt))
        rows["step_supercell_step_K1"] = timed(lambda: fv.supercell_step(dt))
        rows["step_kessler_share_of_supercell_step"] = rows["step_k_warm_rain_K1"]["ms_median"] / rows["step_supercell_step_K1"]["ms_median"]
        rows["step_finite"] = bool(np.isfinite(fv.dc.d["pt"].download()).all())
        ctx.close()
    for r in rows.values():
        if isinstance(r, dict) and "bytes" in r:
            r["bytes_per_s"] = r["bytes"] / (r["ms_median"] * 1.0e-3)
            r["of_8TBps"] = r["bytes_per_s"] / PEAK
    res = dict(build_id=L.build_id(), nx=nx, npz=km, steps=a.steps, device=torch.cuda.get_device_name(0), rows=rows)
    out = a.out or os.path.join(ROOT, "profiles", f"kessler_bench_{L.build_id()}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
