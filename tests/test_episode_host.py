"""CPU-side checks of the auto-reset / episode statistics feature (VecEnv.step_autoreset, track_episodes, EpisodeStats): the three
C entry points, the op table, the torch op's schema, the Python surface, and the bookkeeping kernel's build for gfx950."""
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT

NEW = ("bcn_episode_bytes", "bcn_episode_layout", "bcn_episode_track")


def test_entry_points_are_declared_bound_and_exported_and_refuse_null_handles():
    from beacon_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "beacon_hip.h")).read()
    declared = set(re.findall(r"BCN_API\s+[\w\s\*]+?\b(bcn_\w+)\s*\(", hdr))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.SIGNATURES)
    assert int(re.search(r"#define BCN_API_VERSION (\d+)", hdr).group(1)) == 4 and _lib.API_VERSION == 4
    if build.hipcc() is None and not os.path.exists(build.LIB):
        pytest.skip("no hipcc and no prebuilt library")
    L = _lib.load()
    for name in NEW:
        assert hasattr(L, name)
    assert L.bcn_api_version() == 4
    assert L.bcn_episode_bytes(None) == 0 and b"bcn_episode_bytes: null handle" in L.bcn_last_error()
    segs = (_lib.SnapshotSeg * 16)()
    assert L.bcn_episode_layout(None, segs, 16) == 0 and b"null handle" in L.bcn_last_error()
    assert L.bcn_episode_track(None, None, None, None, None) == 1 and b"bcn_episode_track" in L.bcn_last_error()


def test_op_tables():
    from beacon_amd import vec
    assert vec._EPISODE_OPS == ("episode_track",)
    assert vec._OPS == ("rayleigh_reset", "rayleigh_step", "mixing_reset", "mixing_step", "burgers_reset", "burgers_step",
                        "shkadov_reset", "shkadov_step", "sloshing_reset", "sloshing_step")
    assert vec._ODE_OPS == ("lorenz_reset", "lorenz_step", "vortex_reset", "vortex_step")
    assert vec._STATE_OPS == ("snapshot_save", "snapshot_load")


def test_torch_extension_defines_and_registers_the_episode_op():
    from beacon_amd import build, torch_ext, vec
    src = open(os.path.join(ROOT, "beacon_amd", "csrc", "torch", "beacon_torch.cpp")).read()
    assert src.count('m.def("episode_track(') == 1 and src.count('m.impl("episode_track"') == 2            # CUDA and Meta
    if (shutil.which("g++") is None and torch_ext.stale()) or (build.hipcc() is None and not os.path.exists(build.LIB)):
        pytest.skip("no compiler and no prebuilt extension")
    path = torch_ext.build_ext()
    assert path and os.path.exists(path) and not torch_ext.stale()
    ops = torch_ext.load()
    table = vec._op_table()
    assert ops is not None and table is not None and set(vec._EPISODE_OPS) <= set(table)
    assert str(ops.episode_track.default._schema) == ("beacon::episode_track(int handle, Tensor out_buf, Tensor(a!) ep_buf, "
                                                      "Tensor? mask) -> ()")
    ops.episode_track(0, torch.zeros(16, dtype=torch.uint8, device="meta"), torch.zeros(16, dtype=torch.uint8, device="meta"), None)
    with pytest.raises((NotImplementedError, RuntimeError)):                # CUDA key only: CPU tensors find no kernel
        ops.episode_track(0, torch.zeros(16, dtype=torch.uint8), torch.zeros(16, dtype=torch.uint8), None)


def test_python_surface_exists():
    import beacon_amd
    from beacon_amd import vec
    assert beacon_amd.EpisodeStats is vec.EpisodeStats
    for m in ("step_autoreset", "track_episodes"):
        assert callable(getattr(vec.VecEnv, m))
    assert isinstance(vec.VecEnv.episodes, property)
    assert list(inspect.signature(vec.VecEnv.step_autoreset).parameters) == ["self", "actions", "noise", "mask"]
    cap = inspect.signature(vec.VecEnv.capture).parameters
    assert list(cap) == ["self", "actions", "noise", "n_steps", "keep_steps", "autoreset"] and cap["autoreset"].default is False
    assert vec.EpisodeStats.NAMES == ("ret", "len", "last_ret", "last_len", "count", "sum_ret", "sum_len", "finished", "final_obs")
    for m in ("clear", "totals", "state_dict", "load_state_dict", "view"):
        assert callable(getattr(vec.EpisodeStats, m))


def test_bookkeeping_kernel_compiles_for_gfx950_without_scratch_or_atomics(tmp_path):
    """csrc/episode.hip with the library's own flags: exactly one kernel, no private segment, the observation copy loads and
    stores 16 bytes per lane, every store is a vector store to global memory, and there is no atomic instruction."""
    from beacon_amd import build
    cc = build.hipcc()
    if cc is None:
        pytest.skip("no hipcc")
    src = os.path.join(build.CSRC, "episode.hip")
    assert src in build.sources()
    asm = str(tmp_path / "episode.s")
    subprocess.check_call(build.compile_cmd(src, asm, mode=("--cuda-device-only", "-S")))
    text = open(asm).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    assert len(kernels) == 1 and "episode_track_k" in kernels[0], kernels
    assert re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text) == ["0"]
    assert text.count("global_load_dwordx4") >= 1 and text.count("global_store_dwordx4") >= 1
    stores = set(re.findall(r"^\s*((?:global|flat|scratch|buffer|ds|s)_\w*store\w*)", text, flags=re.M))
    assert stores and all(s.startswith("global_store_") for s in stores), stores
    assert not re.findall(r"^\s*\w*atomic\w*", text, flags=re.M)
    assert not re.findall(r"^\s*ds_(?:read|write)\w*", text, flags=re.M)                                  # no LDS hand-offs
