"""CPU-side checks (no GPU) of the grids tests/test_gpu_jacobi_twins.py runs: flow_states.RUNS_TABLE names the mapping of every grid
as jit.choose / jit.geometry give it and covers every strip width that takes the Jacobi cell runs; each grid's default plugin says it
has the runs and its twin built with -DBCN_JACOBI_RUNS=0 says it has not (the shared objects load without a device)."""
import ctypes

import pytest

import flow_states as FS


def _mapping(nx, ny):
    from beacon_amd import jit
    m = jit.choose(nx, ny, False, 0)
    return m["rows"], m["nw"], m["R"], jit.geometry(1, nx, ny, m["R"], m["gf"], False)["rl"]


def test_runs_table_covers_every_strip_width_that_takes_the_runs():
    from beacon_amd import jit
    assert [(nx, ny, False, 0) for nx, ny, _, _ in FS.RUNS_TABLE] == jit.RUNS_GRIDS
    for nx, ny, R, RL in FS.RUNS_TABLE:
        assert _mapping(nx, ny) == (1, 8, R, RL), (nx, ny)
        assert (nx, ny, False, 0) not in jit.BUILTIN_GRIDS and (nx, ny, False, 0) not in jit.TEST_GRIDS
    # the rule of csrc/bcn_jacobi_cells.h (jacobi_runs_fit), restated: the interior R - 4 is one short run, or at least two runs of four
    assert {R for _, _, R, _ in FS.RUNS_TABLE} == {R for R in range(7, 27) if R - 4 <= 3 or R - 4 >= 8} == {7} | set(range(12, 27))
    last = {RL for _, _, _, RL in FS.RUNS_TABLE}
    assert {3, 8, 9, 10, 11} <= last, "the R == 3 body and every last-strip body of a width the rule excludes as R"
    assert sum(ny == 64 for _, ny, _, _ in FS.RUNS_TABLE) >= 3
    # the ends of the excluded band
    assert [_mapping(nx, ny)[2] for nx, ny, _, _ in jit.RUNS_EXCLUDED_GRIDS] == [8, 11]
    assert jit.RUNS_TWIN_DEFS == {"BCN_JACOBI_RUNS": 0} and all((g, {"BCN_JACOBI_RUNS": 0}) in jit.EXTRA_BUILDS for g in jit.RUNS_GRIDS)


def _cell_runs(grid, defs, monkeypatch):
    from beacon_amd import jit
    monkeypatch.delenv("BEACON_JIT_DEFS", raising=False)
    monkeypatch.setenv("BEACON_NO_BUILD", "1")               # prebuilt means prebuilt
    path = jit.build_plugin(*grid, extra_defs=defs)
    assert path is not None, (grid, defs)
    return ctypes.CDLL(path).bcn_jit_cell_runs()


def test_default_plugins_have_the_runs_and_their_twins_do_not(monkeypatch):
    from beacon_amd import jit
    names = set()
    for g in jit.RUNS_GRIDS:
        assert _cell_runs(g, None, monkeypatch) == 1, g
        assert _cell_runs(g, dict(jit.RUNS_TWIN_DEFS), monkeypatch) == 0, g
        names |= {jit.build_plugin(*g), jit.build_plugin(*g, extra_defs=dict(jit.RUNS_TWIN_DEFS))}
    assert len(names) == 2 * len(jit.RUNS_GRIDS)             # two shared objects per grid


def test_the_excluded_band_has_no_runs_at_either_end(monkeypatch):
    from beacon_amd import jit
    for g in jit.RUNS_EXCLUDED_GRIDS:
        assert _cell_runs(g, None, monkeypatch) == 0, g
