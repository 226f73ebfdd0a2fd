"""bench.py --gpus N without a GPU (FV3_BENCH_DRYRUN=1): the driver's own launch line for N = 2, 4, 8 (px x py blocks of a doubly periodic
domain, halo messages between the ranks) and N = 6 (one cubed-sphere face per rank, cube-edge messages through the library's exchange, whole
Jablonowski-Williamson steps), with the host logic harness in place of the HIP library and gloo in place of RCCL -- so that the first
SCALE run on hardware cannot die on plumbing: rank layout, communicators, barriers, the MAX over ranks, ONE JSON line from rank 0."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [2, 4, 6, 8])
def test_bench_gpus_n_dry_run(n, tmp_path):
    if not os.path.exists(os.path.join(ROOT, "tests", "hostemu", "libfv3_hostemu.so")):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "hostemu")], check=True, capture_output=True, timeout=1800)
    env = dict(os.environ, FV3_BENCH_DRYRUN="1", OMP_NUM_THREADS="1")
    env.pop("FV3_MI355X_SO", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(29600 + n), os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "2", "--warmup", "1",
           "--nx", "16", "--npz", "6", "--strong-domain", "32", "--strong-steps", "1", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]                       # the contract: ONE JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == n and out["steps"] == 2 and out["warmup"] == 1 and out["finite"] is True
    assert out["metric"] == "c_sw+d_sw cell-updates/s" and out["scaling"] == "weak" and "dry_run" in out
    cells = 16 * 16 * 6
    assert abs(out["value"] - n * cells * 2 / (out["ms_per_step"] * 2e-3)) <= 1e-6 * out["value"]   # whole-job units over the MAX-over-ranks time
    if n == 6:
        assert out["config"]["layout"] == "6 faces x 1x1" and out["sphere_six_gpus"].get("finite") is True, out["sphere_six_gpus"]
    else:
        assert out["config"]["halo"] == "RCCL send/recv" and out["config"]["layout"] in ("2x1", "1x2", "2x2", "4x2", "2x4")
        # BASELINE config 4 beside the headline: ONE 32 x 32 domain split over the same layout (16 x 32, 16 x 16, 8 x 16 blocks)
        ss = out["strong_scaling"]
        assert ss and "error" not in ss, ss
        px, py = (int(x) for x in out["config"]["layout"].split("x"))
        assert ss["scaling"] == "strong" and ss["finite"] is True and f"{32 // px}x{32 // py} per GPU" in ss["workload"]
        assert abs(ss["value"] - 32 * 32 * 6 / (ss["ms_per_step"] * 1e-3)) <= 1e-6 * ss["value"]   # the DOMAIN's cells, whatever N


@pytest.mark.parametrize("n", [2, 4, 8])
def test_bench_strong_scaling_domain_dry_run(n, tmp_path):
    """--domain D: `value` is the strong-scaling number of ONE D x D domain (BASELINE config 4's decomposition), the block shrinks with N"""
    env = dict(os.environ, FV3_BENCH_DRYRUN="1", OMP_NUM_THREADS="1")
    env.pop("FV3_MI355X_SO", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(29700 + n), os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "1",
           "--domain", "32", "--npz", "6"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == n and out["scaling"] == "strong" and out["finite"] is True and out["strong_scaling"] is None
    px, py = (int(x) for x in out["config"]["layout"].split("x"))
    assert f"split {px}x{py}: {32 // px}x{32 // py} per GPU" in out["config"]["workload"]
    assert abs(out["value"] - 32 * 32 * 6 / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]


def test_bench_plain_run_and_dump_outputs_dry_run(tmp_path):
    """a plain run (no --full) times the headline pair alone; --dump-outputs DIR writes what its last timed step computed, the same
    arrays on every run with the same arguments"""
    if not os.path.exists(os.path.join(ROOT, "tests", "hostemu", "libfv3_hostemu.so")):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "hostemu")], check=True, capture_output=True, timeout=1800)
    env = dict(os.environ, FV3_BENCH_DRYRUN="1", OMP_NUM_THREADS="1")
    env.pop("FV3_MI355X_SO", None)
    dumps = []
    for run in range(2):
        dump = tmp_path / f"dump{run}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--nx", "16", "--npz", "6",
               "--dump-outputs", str(dump)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, env=env, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, r.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["steps"] == 3 and out["warmup"] == 1 and out["finite"] is True and out["n_gpus"] == 1
        assert out["metric"] == "c_sw+d_sw cell-updates/s" and out["unit"] == "cell-updates/s" and out["dtype"] == "f64"
        assert abs(out["value"] - 16 * 16 * 6 * 3 / (out["ms_per_step"] * 3e-3)) <= 1e-6 * out["value"]
        for leg in ("roofline", "general_metrics", "strong_scaling", "model_step", "cubed_sphere", "cpu_baseline"):
            assert out[leg] is None, leg
        files = sorted(dump.glob("*.npy"))
        assert {f.stem for f in files} == {"delpc", "ptc", "wc", "uc", "vc", "ua", "va", "ut", "vt", "divg_d", "mfx", "mfy", "cx", "cy",
                                           "crx", "cry", "xfx", "yfx", "delp_out", "pt_out", "u_out", "v_out", "w_out"}
        assert sum(f.stat().st_size for f in files) <= 64 << 20
        arrays = {f.stem: np.load(f) for f in files}
        stagger = {"uc": (1, 0), "vc": (0, 1), "divg_d": (1, 1), "mfx": (1, 0), "mfy": (0, 1), "cx": (1, 0), "cy": (0, 1), "crx": (1, 0),
                   "cry": (0, 1), "xfx": (1, 0), "yfx": (0, 1), "u_out": (0, 1), "v_out": (1, 0)}    # the compute domain's points
        for name, v in arrays.items():
            di, dj = stagger.get(name, (0, 0))
            assert v.dtype == np.float64 and v.shape == (16 + di, 16 + dj, 6) and np.isfinite(v).all(), name
        assert np.any(arrays["u_out"] != 0.0) and np.any(arrays["mfx"] != 0.0)
        dumps.append(arrays)
    for name, v in dumps[0].items():
        assert np.array_equal(v, dumps[1][name]), name


def test_dump_outputs_samples_fixed_points_of_a_large_compute_domain(tmp_path):
    """a compute domain larger than DUMP_POINTS is written as the values at DUMP_POINTS seeded points, the same on every call"""
    sys.path.insert(0, ROOT)
    import bench

    class Field:
        def __init__(self, a):
            self.a = a

        def download(self):
            return self.a
    ng, nx, ny, nk = 3, 70, 60, 40
    a = np.asfortranarray(np.random.default_rng(5).standard_normal((nx + 2 * ng + 1, ny + 2 * ng, nk)))
    assert nx * ny * nk > bench.DUMP_POINTS
    from gfdl_atmos_cubed_sphere_amd.layout import Bounds
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"f": (Field(a), "V")}, Bounds(1, nx, 1, ny, ng))
    x, y = np.load(tmp_path / "x" / "f.npy"), np.load(tmp_path / "y" / "f.npy")
    assert x.dtype == np.float64 and x.shape == (bench.DUMP_POINTS,) and np.array_equal(x, y)
    box = a[ng:ng + nx + 1, ng:ng + ny, :].ravel(order="F")     # kind V: is..ie+1, js..je
    assert np.isin(x, box).all() and len(np.unique(x)) == bench.DUMP_POINTS
