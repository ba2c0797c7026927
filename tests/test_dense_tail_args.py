"""DeviceMultilevelSolver(dense_tail=...): what of the rule lives in Python -- the argument's forms, the environment's override for tools that build
their own solvers, and the names of the library's decline codes (include/pyamg_amd.h: pamg_solver_dense_tail_info)."""
import re
from pathlib import Path

import pytest

from pyamg_amd.multilevel import DENSE_TAIL_HARD_MAX_ROWS, DENSE_TAIL_REASONS, dense_tail_args

ROOT = Path(__file__).resolve().parent.parent


def test_argument_forms(monkeypatch):
    monkeypatch.delenv("PAMG_DENSE_TAIL", raising=False)
    assert dense_tail_args(None) == (0, 0)
    assert dense_tail_args(False) == (1, 0)
    assert dense_tail_args({}) == (2, 0)
    assert dense_tail_args(dict(max_rows=219)) == (2, 219)
    assert dense_tail_args(dict(mode=0, max_rows=2048)) == (0, 2048)
    assert dense_tail_args(dict(mode=1)) == (1, 0)
    assert dense_tail_args(dict(mode=2, max_rows=DENSE_TAIL_HARD_MAX_ROWS)) == (2, DENSE_TAIL_HARD_MAX_ROWS)
    for bad in (dict(mode=3), dict(mode=-1), dict(max_rows=-1), dict(max_rows=DENSE_TAIL_HARD_MAX_ROWS + 1), dict(rows=5), "on", 2):
        with pytest.raises(ValueError):
            dense_tail_args(bad)


def test_environment_decides_only_where_the_caller_does_not(monkeypatch):
    monkeypatch.setenv("PAMG_DENSE_TAIL", "0")
    assert dense_tail_args(None) == (1, 0)
    assert dense_tail_args(dict(mode=2, max_rows=34)) == (2, 34) and dense_tail_args(False) == (1, 0)
    monkeypatch.setenv("PAMG_DENSE_TAIL", "auto:2048")
    assert dense_tail_args(None) == (0, 2048)
    monkeypatch.setenv("PAMG_DENSE_TAIL", "force:256")
    assert dense_tail_args(None) == (2, 256)
    monkeypatch.setenv("PAMG_DENSE_TAIL", "auto")
    assert dense_tail_args(None) == (0, 0)
    for bad in ("1", "on", "auto:", "auto:x", "force:99999"):
        monkeypatch.setenv("PAMG_DENSE_TAIL", bad)
        if bad == "auto:":
            assert dense_tail_args(None) == (0, 0)
            continue
        with pytest.raises(ValueError):
            dense_tail_args(None)


def test_reason_names_follow_the_library():
    """the solver's enum (csrc/pamg_solver.hip) has as many codes as Python has names, and the hard row limit is the library's"""
    src = (ROOT / "pyamg_amd" / "csrc" / "pamg_solver.hip").read_text()
    names = re.search(r"enum \{ (TAIL_OFF = 1[^}]*)\};", src).group(1).split(",")
    assert len(names) + 1 == len(DENSE_TAIL_REASONS) and DENSE_TAIL_REASONS[0] is None
    common = (ROOT / "pyamg_amd" / "csrc" / "pamg_common.h").read_text()
    assert int(re.search(r"DENSE_TAIL_HARD_MAX_ROWS = (\d+);", common).group(1)) == DENSE_TAIL_HARD_MAX_ROWS
