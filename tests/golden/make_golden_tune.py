#!/usr/bin/env python3
"""Generate tests/golden/tune_table.npz: what pamg_matrix_tune answered and dropped at commit 8f4a1d7, the last one whose
pamg_matrix_tune was a switch over key numbers.  The recording itself is tests/tune_cases.py, which calls the C ABI by number.

Run on an MI355X, at the commit whose behaviour is to be recorded (to the path given, default the fixture itself):
    python tests/golden/make_golden_tune.py [out.npz]

Data only, a few kilobytes:

  keys / values                      the grid of the acceptance recording (tune_cases.KEYS / VALUES)
  accept.rc / accept.window          [keys, values] return code / pamg_matrix_info[4] after the call; one fresh operator per key
  refuse.values / refuse.rc          [keys] on an operator held by a solver
  effect.<scene>.actions             [n, 2] (key, value): every live key set to the value it has, then (39, 1)
  effect.<scene>.rc / .before / .after     [n] / [n, 132] / [n, 132]: return code and tune_cases.observe() around the call
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

import tune_cases as tc  # noqa: E402

OUT = HERE / "tune_table.npz"


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else OUT
    d = {"keys": np.array(tc.KEYS, dtype=np.int32), "values": np.array(tc.VALUES, dtype=np.int32)}
    d["accept.rc"], d["accept.window"] = tc.accept()
    d["refuse.values"], d["refuse.rc"] = tc.refuse(d["accept.rc"])
    print("accepted values per key:", {k: int(n) for k, n in zip(tc.KEYS, (d["accept.rc"] == 0).sum(axis=1)) if n})
    print("refusals:", dict(zip(tc.KEYS, d["refuse.rc"].tolist())))
    for scene in tc.SCENES:
        acts, rc, before, after = tc.effect(scene)
        d[f"effect.{scene}.actions"], d[f"effect.{scene}.rc"], d[f"effect.{scene}.before"], d[f"effect.{scene}.after"] = acts, rc, before, after
        assert (before == before[0]).all(), f"{scene}: the observables before the call differ from operator to operator"
        print(f"[{scene}] before: {before[0].tolist()}")
        for (key, v), r, a in zip(acts, rc, after):
            ch = np.flatnonzero(a != before[0])
            print(f"[{scene}] key {key} = {v}: rc {r}, changed {dict(zip(ch.tolist(), a[ch].tolist()))}")
    np.savez_compressed(out, **d)
    print(f"wrote {out} ({out.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
