"""The V(1,1) step of 3-D Poisson 256^3 on the SA hierarchy tests/midsize.py builds (level sizes of C3) with TWO BUILDS of libpyamg_amd.so, for
changes that have no switch to turn (a kernel rewritten in place): the stand-in for bench.py's before / after where bench.py's reference-built
hierarchy is not at hand.  Not product code.

    python tools/step_ab_builds.py 256x256x256 OUTDIR before=PATH/libpyamg_amd.so after=PATH/libpyamg_amd.so [runs=5] [limit=120]
    python tools/step_ab_builds.py 256x256x256 OUTDIR only=PATH/libpyamg_amd.so [steps=10] [warmup=2]       (one build in this process: for a profiler)

The hierarchy is built ONCE, in a process that never touches the device; every run is a child forked from it that loads one of the libraries,
uploads the hierarchy, runs 5 warm-up cycles and 20 timed replayed steps (b = rand, x0 = 0: 25 cycles in all) and leaves the iterate and the last
residual norm behind.  Runs alternate between the builds; each has its own time limit, and the first run that fails, faults or runs out of time
ends the session -- nothing is started on the device after it.  The iterates of all runs are compared with np.array_equal."""
import hashlib
import json
import multiprocessing as mp
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import midsize as M                                   # noqa: E402


def one_run(lib, spec, b, x0, warmup, steps, out):
    """in a process of its own (or the profiled one): returns nothing, writes `out`.json and `out`.npy"""
    from pyamg_amd import _capi as capi
    capi.LIB_PATH = Path(lib)
    from pyamg_amd import DeviceMultilevelSolver
    n = b.size
    t = time.time()
    d = DeviceMultilevelSolver(spec)
    up = time.time() - t
    xd, bd = capi.DeviceArray(n, np.float64), capi.DeviceArray(n, np.float64)
    xd.upload(x0); bd.upload(b)
    d.load_device(xd, bd)
    d.iterate_device(warmup)                          # plans' first use, capture
    t = time.time()
    r = d.iterate_device(steps)                       # returns after the residual norms came back: synchronised
    ms = (time.time() - t) * 1e3 / steps
    d.store_device(xd)
    x = xd.download()
    flow = [bool(A.flow_error()) for A in d.A]
    np.save(str(out) + ".npy", x)
    Path(str(out) + ".json").write_text(json.dumps({"library": str(lib), "version": capi.version(), "upload_s": up, "ms_per_step": ms,
                                                    "residual_norm": float(r[-1]), "residual_norm_hex": float(r[-1]).hex(),
                                                    "x_sha256": hashlib.sha256(x.tobytes()).hexdigest(), "flow_error": flow}))
    d.free()
    if any(flow):
        raise SystemExit(3)


def main():
    grid, outdir = sys.argv[1], Path(sys.argv[2])
    kw = dict(a.split("=", 1) for a in sys.argv[3:])
    outdir.mkdir(parents=True, exist_ok=True)
    tmp = Path(kw.get("tmp", outdir))
    tmp.mkdir(parents=True, exist_ok=True)
    t0 = time.time()
    spec = M.hierarchy(f"poisson:{grid}", ("gs", "symmetric"))
    sizes = [L.A.shape[0] for L in spec.levels]
    print(f"hierarchy {sizes} built in {time.time() - t0:.1f} s", flush=True)
    b, x0 = np.random.RandomState(0).rand(sizes[0]), np.zeros(sizes[0])
    if "only" in kw:
        one_run(kw["only"], spec, b, x0, int(kw.get("warmup", 2)), int(kw.get("steps", 10)), tmp / "only")
        print(json.loads((tmp / "only.json").read_text()), flush=True)
        return 0
    builds = {k: kw[k] for k in ("before", "after")}
    runs, limit = int(kw.get("runs", 5)), float(kw.get("limit", 120))
    res = {"grid": grid, "levels": sizes, "warmup": 5, "steps": 20, "builds": {k: {"library": v, "runs": []} for k, v in builds.items()}}
    ctx = mp.get_context("fork")
    ref = None
    for i in range(runs):
        for tag, lib in builds.items():
            out = tmp / f"{tag}_{i}"
            p = ctx.Process(target=one_run, args=(lib, spec, b, x0, 5, 20, out))
            p.start()
            p.join(limit)
            if p.is_alive():
                p.kill(); p.join()
                print(f"{tag} run {i}: no result within {limit:.0f} s; the session ends here", flush=True)
                return 124
            if p.exitcode != 0:
                print(f"{tag} run {i}: exit code {p.exitcode}; the session ends here", flush=True)
                return 1
            r = json.loads(Path(str(out) + ".json").read_text())
            x = np.load(str(out) + ".npy")
            Path(str(out) + ".npy").unlink()
            if ref is None:
                ref = (x, r["residual_norm_hex"], f"{tag} run {i}")
            r["x_equals_first_run"] = bool(np.array_equal(x, ref[0]))
            r["residual_norm_equals_first_run"] = r["residual_norm_hex"] == ref[1]
            res["builds"][tag]["runs"].append(r)
            print(f"{tag} run {i}: {r['ms_per_step']:.4f} ms per step, upload {r['upload_s']:.1f} s, residual norm {r['residual_norm']:.12g}, "
                  f"x == x of {ref[2]}: {r['x_equals_first_run']}, residual norm equal: {r['residual_norm_equals_first_run']}", flush=True)
            (outdir / f"step_ab_builds_{grid}.json").write_text(json.dumps(res, indent=1))
    for tag, v in res["builds"].items():
        a = np.array([r["ms_per_step"] for r in v["runs"]])
        v["median"], v["min"], v["max"], v["range"] = float(np.median(a)), float(a.min()), float(a.max()), float(a.max() - a.min())
    bf, af = res["builds"]["before"], res["builds"]["after"]
    wider = max(bf["range"], af["range"])
    res["rule"] = {"ranges_do_not_overlap": bool(af["max"] < bf["min"] or bf["max"] < af["min"]), "median_gain_ms": bf["median"] - af["median"],
                   "gain_over_wider_range": (bf["median"] - af["median"]) / wider if wider > 0 else None}
    res["same_results"] = all(r["x_equals_first_run"] and r["residual_norm_equals_first_run"] for v in res["builds"].values() for r in v["runs"])
    (outdir / f"step_ab_builds_{grid}.json").write_text(json.dumps(res, indent=1))
    print(json.dumps({k: {q: v[q] for q in ("median", "min", "max", "range")} for k, v in res["builds"].items()}), res["rule"], "same results:", res["same_results"], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
