"""CPU-side checks of the per-jet rewards of shkadov (VecShkadov.set_jet_rewards / rwd_jets / jet_episodes / obs_jets,
bcn_shkadov_jet_rewards): the three C entry points in the header, the binding and the built library, the op table, the torch op's
schema, the Python surface, and the kernel's build for gfx950."""
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT

NEW = ("bcn_shkadov_jets_bytes", "bcn_shkadov_jets_layout", "bcn_shkadov_jet_rewards")


def test_entry_points_are_declared_bound_and_exported_and_refuse_null_handles():
    import ctypes as C
    from beacon_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "beacon_hip.h")).read()
    assert re.search(r"BCN_API size_t bcn_shkadov_jets_bytes\(bcn_env_t h\);", hdr)
    assert re.search(r"BCN_API int bcn_shkadov_jets_layout\(bcn_env_t h, bcn_snapshot_seg\* segs, int max_segs\);", hdr)
    assert re.search(r"BCN_API int bcn_shkadov_jet_rewards\(bcn_env_t h, const void\* out_buf_dev, void\* jets_buf_dev, int with_stats, "
                     r"void\* stream\);", hdr)
    assert "shkadov.py:469-481" in hdr and "shkadov.py:376-481" in hdr                      # the reference lines they replace
    assert int(re.search(r"#define BCN_API_VERSION (\d+)", hdr).group(1)) == 4 and _lib.API_VERSION == 4     # no buffer changed size
    vp = C.c_void_p
    assert _lib.SIGNATURES["bcn_shkadov_jets_bytes"] == (C.c_size_t, [vp])
    assert _lib.SIGNATURES["bcn_shkadov_jets_layout"] == (C.c_int, [vp, C.POINTER(_lib.SnapshotSeg), C.c_int])
    assert _lib.SIGNATURES["bcn_shkadov_jet_rewards"] == (C.c_int, [vp, vp, vp, C.c_int, vp])
    if build.hipcc() is None and not os.path.exists(build.LIB):
        pytest.skip("no hipcc and no prebuilt library")
    L = _lib.load()
    for name in NEW:
        assert hasattr(L, name)
    assert L.bcn_api_version() == 4
    assert L.bcn_shkadov_jet_rewards(None, None, None, 1, None) == 1 and b"bcn_shkadov_jet_rewards" in L.bcn_last_error()
    assert L.bcn_shkadov_jets_bytes(None) == 0 and b"bcn_shkadov_jets_bytes: null handle" in L.bcn_last_error()
    segs = (_lib.SnapshotSeg * 8)()
    assert L.bcn_shkadov_jets_layout(None, segs, 8) == 0 and b"null handle" in L.bcn_last_error()


def test_op_tables():
    from beacon_amd import vec
    assert vec._JET_OPS == ("shkadov_jet_rewards",)
    assert vec._OPS == ("rayleigh_reset", "rayleigh_step", "mixing_reset", "mixing_step", "burgers_reset", "burgers_step",
                        "shkadov_reset", "shkadov_step", "sloshing_reset", "sloshing_step")
    assert vec._ODE_OPS == ("lorenz_reset", "lorenz_step", "vortex_reset", "vortex_step")
    assert vec._STATE_OPS == ("snapshot_save", "snapshot_load")
    assert vec._EPISODE_OPS == ("episode_track",)
    assert vec._WARM_OPS == ("shkadov_reset_random",)
    assert vec._ALL_OPS == vec._OPS + vec._ODE_OPS + vec._STATE_OPS + vec._EPISODE_OPS + vec._WARM_OPS + vec._JET_OPS


def test_torch_extension_defines_and_registers_the_jets_op():
    from beacon_amd import build, torch_ext, vec
    src = open(os.path.join(ROOT, "beacon_amd", "csrc", "torch", "beacon_torch.cpp")).read()
    assert src.count('m.def("shkadov_jet_rewards(') == 1 and src.count('m.impl("shkadov_jet_rewards"') == 2     # CUDA and Meta
    if (shutil.which("g++") is None and torch_ext.stale()) or (build.hipcc() is None and not os.path.exists(build.LIB)):
        pytest.skip("no compiler and no prebuilt extension")
    path = torch_ext.build_ext()
    assert path and os.path.exists(path) and not torch_ext.stale()
    ops = torch_ext.load()
    table = vec._op_table()
    assert ops is not None and table is not None and set(vec._JET_OPS) <= set(table)
    assert str(ops.shkadov_jet_rewards.default._schema) == ("beacon::shkadov_jet_rewards(int handle, Tensor out_buf, "
                                                            "Tensor(a!) jets_buf, int with_stats) -> ()")
    ops.shkadov_jet_rewards(0, torch.zeros(16, dtype=torch.uint8, device="meta"), torch.zeros(16, dtype=torch.uint8, device="meta"), 1)
    with pytest.raises((NotImplementedError, RuntimeError)):                # CUDA key only: CPU tensors find no kernel
        ops.shkadov_jet_rewards(0, torch.zeros(16, dtype=torch.uint8), torch.zeros(16, dtype=torch.uint8), 1)


def test_python_surface_exists_on_shkadov_alone_and_is_off_by_default():
    import inspect
    import beacon_amd
    from beacon_amd import vec
    assert beacon_amd.JetStats is vec.JetStats
    S = vec.VecShkadov
    assert callable(S.set_jet_rewards)
    sig = inspect.signature(S.set_jet_rewards).parameters
    assert list(sig) == ["self", "on", "stats"] and sig["on"].default is True and sig["stats"].default is True
    for p in ("rwd_jets", "jet_episodes", "obs_jets"):
        assert isinstance(getattr(S, p), property)
    assert vec.JetStats.NAMES == ("rwd_jets", "ret", "last_ret", "sum_ret")
    for m in ("clear", "state_dict", "load_state_dict", "view"):
        assert callable(getattr(vec.JetStats, m))
    for cls in (vec.VecEnv, vec.VecRayleigh, vec.VecMixing, vec.VecBurgers, vec.VecSloshing, vec.VecLorenz, vec.VecVortex):
        for name in ("set_jet_rewards", "rwd_jets", "jet_episodes", "obs_jets"):
            assert not hasattr(cls, name), (cls.__name__, name)
    doc = S.set_jet_rewards.__doc__
    assert "Snapshot" in doc and "snapshot_signature" in doc                # bookkeeping: said so where the user reads it
    # off by default: an object without a handle (no GPU here) refuses to hand out rewards, and says how to get them
    env = S.__new__(S)
    assert env._jets_on is False and env._jets is None
    for name in ("rwd_jets", "jet_episodes"):
        with pytest.raises((AttributeError, ValueError), match="set_jet_rewards"):
            getattr(env, name)
    assert vec.VecEnv._after_step(env) is None                              # the other envs launch nothing behind a step


def test_jets_kernel_compiles_for_gfx950_without_scratch_or_lds(tmp_path):
    """csrc/shkadov_jets.hip with the library's own flags: exactly the float and the double instantiation of shkadov_jets_k, each
    without a private segment and without LDS, no barrier and no atomic instruction."""
    from beacon_amd import build
    cc = build.hipcc()
    if cc is None:
        pytest.skip("no hipcc")
    src = os.path.join(build.CSRC, "shkadov_jets.hip")
    assert src in build.sources()
    asm = str(tmp_path / "shkadov_jets.s")
    subprocess.check_call(build.compile_cmd(src, asm, mode=("--cuda-device-only", "-S")))
    text = open(asm).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    assert len(kernels) == 2 and all("shkadov_jets_k" in k for k in kernels), kernels
    assert sorted(re.search(r"shkadov_jets_kI(\w)E", k).group(1) for k in kernels) == ["d", "f"]        # <double>, <float>
    assert re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text) == ["0", "0"]
    assert re.findall(r"\.group_segment_fixed_size:\s*(\d+)", text) == ["0", "0"]
    assert not re.findall(r"^\s*\w*atomic\w*", text, flags=re.M)
    assert not re.findall(r"^\s*s_barrier", text, flags=re.M)
