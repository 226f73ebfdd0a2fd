#!/usr/bin/env python3
"""What the transport schemes cost: the 384 x 384 x 127 doubly periodic c_sw -> halo -> d_sw pair (bench.py's setup) timed with
device events for several (hord_mt, hord_vt, hord_tm, hord_dp) sets.

One child process per setting (the library reads its switches once per process), each under its own time limit; the chain stops
at the first child that does not exit with 0.  The yardstick is (5, 5, 5, -5) under FV3_MI355X_FUSED=0: an order set the library
always had, on exactly the per-field marching kernels the orders outside the fused kernels' instantiation set run on.  Compare
only within one run of this script.

usage: hord_bench.py [--nx 384] [--npz 127] [--steps 20] [--warmup 5] [--timeout 240] [--out FILE.json]
       hord_bench.py --child MT VT TM DP [--nx ...]       (one setting, one JSON line)"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (hord_mt, hord_vt, hord_tm, hord_dp), lim_fac, environment
SETTINGS = [((5, 5, 5, -5), 1.0, {"FV3_MI355X_FUSED": "0"}),
            ((6, 6, 6, -6), 1.0, {}), ((1, 1, 1, -1), 2.0, {}), ((2, 2, 2, 2), 1.0, {}), ((3, 3, 3, -3), 1.0, {}),
            ((10, 9, 12, 7), 1.0, {}), ((5, 5, 5, -5), 1.0, {}), ((10, 10, 10, 10), 1.0, {})]


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    from gfdl_atmos_cubed_sphere_amd import lib as L
    from gfdl_atmos_cubed_sphere_amd import synthetic as P
    from gfdl_atmos_cubed_sphere_amd.dyn_core import DynFlags, level_coefficients
    from gfdl_atmos_cubed_sphere_amd.grid import doubly_periodic
    from gfdl_atmos_cubed_sphere_amd.halo import HaloExchanger
    from gfdl_atmos_cubed_sphere_amd.layout import Bounds
    nx, npz = a.nx, a.npz
    bd = Bounds(1, nx, 1, nx)
    g = doubly_periodic(bd, nx + 1, nx + 1, dx_const=26000.0, dy_const=26000.0)
    g.lim_fac = a.lim_fac
    ctx = L.Context(g, npz, stream=torch.cuda.current_stream().cuda_stream)
    halo = HaloExchanger(ctx, 1, 1, 0, 1)
    d = {k: ctx.from_host(v) for k, v in P.smooth_state(bd, npz, noise=0.05).items()}
    for n, kind in P.CSW_OUT:
        d[n] = ctx.zeros(kind, npz)
    for n, kind in (("mfx", "FX"), ("mfy", "FY"), ("cx", "CX"), ("cy", "CY"), ("crx", "CX"), ("cry", "CY"), ("xfx", "CX"), ("yfx", "CY"),
                    ("delp_out", "A"), ("pt_out", "A"), ("u_out", "U"), ("v_out", "V"), ("w_out", "A")):
        d[n] = ctx.zeros(kind, npz)
    ctx.dsw_levels(level_coefficients(npz, DynFlags()))
    dt = 22.5
    mt, vt, tm, dp = a.child
    par = dict(P.DSW_PAR)
    par.update(dt=dt, hydrostatic=0, use_cond=0, hord_mt=mt, hord_vt=vt, hord_tm=tm, hord_dp=dp)

    def pair():
        ctx.c_sw(d["delpc"], d["delp"], d["ptc"], d["pt"], d["u"], d["v"], d["w"], d["uc"], d["vc"], d["ua"], d["va"], d["wc"], d["ut"],
                 d["vt"], d["divg_d"], 1, 0.5 * dt, False)
        halo.update([(d["uc"], "V"), (d["vc"], "U"), (d["divg_d"], "B")])
        ctx.d_sw(par, None, d["delp"], d["pt"], d["u"], d["v"], d["w"], d["uc"], d["vc"], d["ua"], d["va"], d["divg_d"], d["mfx"], d["mfy"],
                 d["cx"], d["cy"], d["crx"], d["cry"], d["xfx"], d["yfx"], None, d["delp_out"], d["pt_out"], d["u_out"], d["v_out"],
                 d["w_out"], None, None, None)
    for _ in range(a.warmup):
        pair()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pair()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    import numpy as np
    finite = bool(np.isfinite(d["delp_out"].download()).all() and np.isfinite(d["u_out"].download()).all())
    print(json.dumps({"hord": [mt, vt, tm, dp], "lim_fac": a.lim_fac, "fused_env": os.environ.get("FV3_MI355X_FUSED", ""),
                      "pair_ms_median": ms[len(ms) // 2], "pair_ms_min": ms[0], "pair_ms_max": ms[-1], "steps": a.steps, "finite": finite}))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=384)
    ap.add_argument("--npz", type=int, default=127)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--lim-fac", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, nargs=4, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for s, lim, env in SETTINGS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child"] + [str(x) for x in s] + \
              ["--nx", str(a.nx), "--npz", str(a.npz), "--steps", str(a.steps), "--warmup", str(a.warmup), "--lim-fac", str(lim)]
        r = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout, r.stderr, file=sys.stderr)
            sys.exit(f"hord_bench: {s} {env} ended with status {r.returncode}: nothing more is started")
        rows.append(json.loads(r.stdout.strip().split("\n")[-1]))
        print(json.dumps(rows[-1]), flush=True)
    base = rows[0]["pair_ms_median"]
    for r in rows:
        r["vs_yardstick"] = r["pair_ms_median"] / base
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    print(json.dumps({"yardstick_ms": base, "ratios": {("%d,%d,%d,%d" % tuple(r["hord"])) + ("@FUSED=0" if r["fused_env"] else ""): round(r["vs_yardstick"], 3)
                                                       for r in rows}}))


if __name__ == "__main__":
    main()
