"""The V(1,1) step of 3-D Poisson 256^3 on the SA hierarchy tests/midsize.py builds (level sizes of C3), dense tail off (every launch the parent's)
against automatic, in one process: alternating runs of 20 replayed steps; iterate and residual norm after 25 cycles; a row-limit scan by forced mode.
Not product code.

    python tools/step_ab_dense_tail.py [256x256x256] [output directory]
"""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import midsize as M                                   # noqa: E402
from pyamg_amd import DeviceMultilevelSolver          # noqa: E402
from pyamg_amd import _capi as capi                   # noqa: E402

grid = sys.argv[1] if len(sys.argv) > 1 else "256x256x256"
out = Path(sys.argv[2] if len(sys.argv) > 2 else ".") / f"step_ab_{grid}.json"
t0 = time.time()
spec = M.hierarchy(f"poisson:{grid}", ("gs", "symmetric"))
sizes = [L.A.shape[0] for L in spec.levels]
print(f"hierarchy {sizes} built in {time.time() - t0:.1f} s", flush=True)
n = sizes[0]
rng = np.random.RandomState(0)
b, x0 = rng.rand(n), np.zeros(n)
res = {"grid": grid, "levels": sizes, "variants": {}}


def make(tag, tail):
    t = time.time()
    d = DeviceMultilevelSolver(spec, dense_tail=tail)
    up = time.time() - t
    xd, bd = capi.DeviceArray(n, np.float64), capi.DeviceArray(n, np.float64)
    xd.upload(x0); bd.upload(b)
    d.load_device(xd, bd)
    t = time.time()
    d.iterate_device(5)                               # warm-up: tabulation, capture
    first = time.time() - t
    print(f"{tag}: upload {up:.2f} s, first five cycles {first:.3f} s, {d.stats()['dense_tail']}", flush=True)
    res["variants"][tag] = {"upload_s": up, "first_five_cycles_s": first, "runs_ms_per_step": []}
    return d, xd, bd


def run(tag, d, steps=20):
    t = time.time()
    d.iterate_device(steps)                           # returns after the residual norms came back: synchronised
    ms = (time.time() - t) * 1e3 / steps
    res["variants"][tag]["runs_ms_per_step"].append(ms)
    print(f"{tag}: {ms:.4f} ms per step", flush=True)


off = make("off", False)
auto = make("auto", None)
for _ in range(5):
    run("off", off[0])
    run("auto", auto[0])
# 25 cycles done in both (5 + 20) after the first run; compare fresh solves of 25 cycles
cmp = {}
for tag, (d, xd, bd) in (("off", off), ("auto", auto)):
    xd.upload(x0)
    d.load_device(xd, bd)
    r = d.iterate_device(25)
    d.store_device(xd)
    cmp[tag] = (xd.download(), float(r[-1]))
dx = float(np.max(np.abs(cmp["auto"][0] - cmp["off"][0])) / np.max(np.abs(cmp["off"][0])))
res["after_25_cycles"] = {"max_dx_over_max_x": dx, "residual_norm_off": cmp["off"][1], "residual_norm_auto": cmp["auto"][1],
                          "relative_difference": abs(cmp["auto"][1] - cmp["off"][1]) / cmp["off"][1]}
print("after 25 cycles:", res["after_25_cycles"], flush=True)
res["dense_tail_auto"] = auto[0].stats()["dense_tail"]
for tag, v in res["variants"].items():
    a = np.array(v["runs_ms_per_step"])
    v["median"], v["range"] = float(np.median(a)), float(a.max() - a.min())
out.write_text(json.dumps(res, indent=1))
auto[0].free()
# the row-limit scan: forced mode at 256 / 512 / 1024 / 2048 rows against off, three alternating runs each
scan = {}
for lim in (256, 1024):          # (on these level sizes 512, 1024 and 2048 pick the same level)
    tag = f"force{lim}"
    d = make(tag, dict(mode=2, max_rows=lim))
    for _ in range(3):
        run("off", off[0])
        run(tag, d[0])
    scan[lim] = {"dense_tail": d[0].stats()["dense_tail"], "runs": res["variants"][tag]["runs_ms_per_step"]}
    d[0].free()
    res["scan"] = scan
    out.write_text(json.dumps(res, indent=1))
print("done", flush=True)
