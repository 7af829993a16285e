"""CPU-side checks of shkadov's device-side random-start reset (VecShkadov.set_random_init / bcn_shkadov_reset_random): the entry
point in the header, the binding, the built library and the torch schema; the two new translation units built for gfx950 with the
warm kernels in them; the op tuples that other tests pin; the argument checks that need no device."""
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT

NAME = "bcn_shkadov_reset_random"
UNITS = ("shkadov_warm_f32.hip", "shkadov_warm_f64.hip")


def test_header_declares_the_entry_point_and_the_api_version_stays_4():
    from beacon_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "beacon_hip.h")).read()
    declared = set(re.findall(r"BCN_API\s+[\w\s\*]+?\b(bcn_\w+)\s*\(", hdr))
    assert NAME in declared
    flat = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"bcn_shkadov_reset_random\(bcn_env_t h, const void\* init_fields_dev, const int32_t\* n_steps_dev\s*,\s*"
                     r"int rand_steps, int32_t\* n_out_dev\s*, void\* obs_dev, void\* stream\)", flat)
    assert int(re.search(r"#define BCN_API_VERSION (\d+)", hdr).group(1)) == 4 and _lib.API_VERSION == 4   # no buffer changed size
    assert "without its rand_init loop" not in hdr                          # the old comment of bcn_shkadov_reset is gone


def test_binding_and_library_have_it_and_it_checks_handle_and_arguments():
    import ctypes as C
    from beacon_amd import _lib, build
    assert NAME in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == 7 and args[3] is C.c_int
    if build.hipcc() is None and not os.path.exists(build.LIB):
        pytest.skip("no hipcc and no prebuilt library")
    L = _lib.load()
    assert hasattr(L, NAME) and L.bcn_api_version() == 4
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True)
    if out.returncode == 0:
        assert NAME in set(line.split()[-1] for line in out.stdout.splitlines() if line.strip())
    # a null handle is refused, not dereferenced
    assert L.bcn_shkadov_reset_random(None, None, None, 400, None, None, None) == 1
    assert b"BCN_SHKADOV" in L.bcn_last_error()


def test_op_tuples():
    from beacon_amd import vec
    assert vec._WARM_OPS == ("shkadov_reset_random",)
    assert vec._OPS == ("rayleigh_reset", "rayleigh_step", "mixing_reset", "mixing_step", "burgers_reset", "burgers_step",
                        "shkadov_reset", "shkadov_step", "sloshing_reset", "sloshing_step") and len(vec._OPS) == 10
    assert vec._ODE_OPS == ("lorenz_reset", "lorenz_step", "vortex_reset", "vortex_step")
    assert vec._STATE_OPS == ("snapshot_save", "snapshot_load")
    assert vec._EPISODE_OPS == ("episode_track",)


def test_torch_extension_defines_and_registers_the_op():
    from beacon_amd import build, torch_ext, vec
    src = open(os.path.join(ROOT, "beacon_amd", "csrc", "torch", "beacon_torch.cpp")).read()
    assert src.count('m.def("shkadov_reset_random(') == 1 and src.count('m.impl("shkadov_reset_random"') == 2   # CUDA and Meta
    if (shutil.which("g++") is None and torch_ext.stale()) or (build.hipcc() is None and not os.path.exists(build.LIB)):
        pytest.skip("no compiler and no prebuilt extension")
    path = torch_ext.build_ext()
    assert path and os.path.exists(path) and not torch_ext.stale()
    ops = torch_ext.load()
    table = vec._op_table()
    assert ops is not None and table is not None and set(vec._WARM_OPS) <= set(table)
    assert str(ops.shkadov_reset_random.default._schema) == (
        "beacon::shkadov_reset_random(int handle, Tensor? init_fields, Tensor? n_steps, int rand_steps, Tensor(a!)? n_out, "
        "Tensor(b!) obs) -> ()")
    ops.shkadov_reset_random(0, None, None, 400, torch.zeros(4, dtype=torch.int32, device="meta"), torch.zeros(8, device="meta"))
    with pytest.raises((NotImplementedError, RuntimeError)):                # CUDA key only: CPU tensors find no kernel
        ops.shkadov_reset_random(0, None, None, 400, None, torch.zeros(8))


def test_python_surface_and_its_argument_checks():
    """set_random_init exists on VecShkadov only, refuses a bad rand_steps before anything is launched (checked on an object
    without a handle: there is nothing it could launch on), and reset_random keeps its signature."""
    from beacon_amd import vec
    assert callable(vec.VecShkadov.set_random_init) and callable(vec.VecShkadov.reset_random_device)
    assert list(inspect.signature(vec.VecShkadov.set_random_init).parameters) == ["self", "rand_steps"]
    assert inspect.signature(vec.VecShkadov.set_random_init).parameters["rand_steps"].default == 400
    assert list(inspect.signature(vec.VecShkadov.reset_random).parameters) == ["self", "rand_steps", "n_steps"]
    assert "set_random_init" in vec.VecShkadov.reset_random.__doc__
    for cls in (vec.VecEnv, vec.VecBurgers, vec.VecSloshing, vec.VecRayleigh, vec.VecMixing, vec.VecLorenz, vec.VecVortex):
        assert not hasattr(cls, "set_random_init"), cls
    env = vec.VecShkadov.__new__(vec.VecShkadov)                           # no handle, no device
    for bad in (-1, 65536, 2.5, "400", True):
        with pytest.raises(ValueError):
            env.set_random_init(bad)
    assert env.set_random_init(400) is env and env.rand_steps == 400
    assert env.set_random_init(0).rand_steps == 0 and env.set_random_init(65535).rand_steps == 65535
    assert env.set_random_init(None).rand_steps is None
    with pytest.raises(ValueError):
        env.reset_random_device()                                            # switch off: refused before any launch


def _kernels(text):
    return re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)


@pytest.mark.parametrize("unit", UNITS)
def test_the_new_units_compile_for_gfx950_and_hold_only_warm_kernels(unit, tmp_path):
    """hipcc --offload-arch=gfx950 --cuda-device-only -S with the library's own flags: every kernel of the unit is a
    shkadov_warm_k instantiation -- all twenty (K, NT) shapes of one precision, the shapes shkadov_step_k comes in -- and the
    float64 unit is built with the flag of env1d_f64.hip (no FMA contraction)."""
    from beacon_amd import build
    cc = build.hipcc()
    if cc is None:
        pytest.skip("no hipcc")
    src = os.path.join(build.CSRC, unit)
    assert src in build.sources()
    assert build.FILE_FLAGS.get("shkadov_warm_f64.hip") == build.FILE_FLAGS["env1d_f64.hip"] == ["-ffp-contract=off"]
    assert "shkadov_warm_f32.hip" not in build.FILE_FLAGS and "env1d_f32.hip" not in build.FILE_FLAGS
    asm = str(tmp_path / (unit + ".s"))
    subprocess.check_call(build.compile_cmd(src, asm, mode=("--cuda-device-only", "-S")))
    text = open(asm).read()
    kernels = _kernels(text)
    real = "f" if unit.endswith("f32.hip") else "d"
    want = set("shkadov_warm_kI%sLi%dELi%dEE" % (real, k, nt) for k in (1, 2, 4, 8) for nt in (64, 128, 256, 512, 1024))
    assert len(kernels) == 20 and all("shkadov_warm_k" in k for k in kernels), kernels
    assert set(re.search(r"shkadov_warm_kI\wLi\d+ELi\d+EE", k).group(0) for k in kernels) == want


def test_the_step_body_is_one_text_shared_by_both_kernels():
    csrc = os.path.join(ROOT, "beacon_amd", "csrc")
    impl = open(os.path.join(csrc, "env1d_impl.inc")).read()
    assert impl.count('#include "shkadov_action.inc"') == 2                  # shkadov_step_k and shkadov_warm_k
    assert re.search(r"template <typename real, int K, int NT>\s*__global__ __launch_bounds__\(NT\) void shkadov_step_k\(Env1DArgs<real> A\)", impl)
    assert "#ifdef BCN_ENV1D_WARM" in impl
    for unit in ("env1d_f32.hip", "env1d_f64.hip"):
        assert "BCN_ENV1D_WARM" not in open(os.path.join(csrc, unit)).read()
    for unit in UNITS:
        text = open(os.path.join(csrc, unit)).read()
        assert "#define BCN_ENV1D_WARM 1" in text and '#include "env1d_impl.inc"' in text
