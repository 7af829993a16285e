"""CPU-side checks of the per-replica physical parameters (VecEnv.set_params / bcn_set_params): the C ABI's four entry points in
the header, the binding and the built library; the PARAMS table of every class; the derived constants against the expressions
of the reference's constructors; and the gfx950 code of the 1D and ODE kernels, which must not have gained a private segment."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT

NEW = ("bcn_n_params", "bcn_param_name", "bcn_set_params", "bcn_get_params")

# the issue's table: env -> the reference's constructor arguments, in the order of the C ABI's value rows
TABLE = {"VecLorenz": ("sigma", "rho", "beta"), "VecVortex": ("re", "weight"), "VecBurgers": ("u_target", "amp"),
         "VecShkadov": ("delta",), "VecSloshing": ("amp", "alpha", "g"), "VecRayleigh": ("ra",), "VecMixing": ("re", "pe")}
# include/beacon_hip.h: BCN_RAYLEIGH .. BCN_VORTEX
KIND = {"VecRayleigh": 0, "VecMixing": 1, "VecBurgers": 2, "VecShkadov": 3, "VecSloshing": 4, "VecLorenz": 5, "VecVortex": 6}


def _lib_or_skip():
    from beacon_amd import _lib, build
    if build.hipcc() is None and not os.path.exists(build.LIB):
        pytest.skip("no hipcc and no prebuilt library")
    return _lib.load()


def test_header_binding_and_library_have_the_four_entry_points():
    from beacon_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "beacon_hip.h")).read()
    declared = set(re.findall(r"BCN_API\s+[\w\s\*]+?\b(bcn_\w+)\s*\(", hdr))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.SIGNATURES)
    assert re.search(r"bcn_set_params\(bcn_env_t h, const double\* values_host, void\* stream\)", hdr)
    assert re.search(r"bcn_get_params\(bcn_env_t h, double\* values_host\)", hdr)
    assert int(re.search(r"#define BCN_API_VERSION (\d+)", hdr).group(1)) == 4 and _lib.API_VERSION == 4     # no buffer changed size
    L = _lib_or_skip()
    for name in NEW:
        assert hasattr(L, name)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True)
    if out.returncode == 0:
        exported = set(line.split()[-1] for line in out.stdout.splitlines() if line.strip())
        assert set(NEW) <= exported
    # null handles are refused, not dereferenced
    assert L.bcn_n_params(None) == 0 and L.bcn_param_name(None, 0) == b""
    assert L.bcn_set_params(None, None, None) == 1 and L.bcn_get_params(None, None) == 1
    assert b"bcn_set_params" in L.bcn_last_error() or b"bcn_get_params" in L.bcn_last_error()


def test_params_of_every_class_equal_the_table():
    import beacon_amd
    from beacon_amd import vec
    assert vec.VecEnv.PARAMS == ()
    for cls, names in TABLE.items():
        assert getattr(vec, cls).PARAMS == names, cls
        assert getattr(beacon_amd, cls) is getattr(vec, cls)
    for m in ("set_params", "clear_params"):
        assert callable(getattr(vec.VecEnv, m))
    assert isinstance(vec.VecEnv.params, property)
    assert issubclass(vec.ParamsWarning, Warning)
    # what must be > 0: every divisor / argument of a root among them
    assert set(vec._POSITIVE_PARAMS) == {"ra", "re", "pe", "delta", "g"}


def _derive(L, kind, params, aux=(0.0, 0.0)):
    p = (C.c_double * 3)(*params)
    a = (C.c_double * 2)(*aux)
    d = (C.c_double * 3)()
    n = L.bcn_derive_params_host(kind, p, a, d)
    assert n > 0
    return [d[k] for k in range(n)]


def test_derived_constants_are_those_of_the_constructors():
    """The inline functions *_create and bcn_set_params share (csrc/params.h), called through the host-only bcn_derive_params_host,
    against the expressions of the reference's constructors evaluated here in double, for the default configuration of every env
    and for the parameter sets of the GPU tests: equal bit for bit."""
    from beacon_amd import vec
    L = _lib_or_skip()
    pr = 0.71
    for ra in (1.0e4, 8.0e3, 5.0e4, 2.0e5):                                     # rayleigh.py: sqrt(pr/ra), 1/sqrt(pr*ra)
        assert _derive(L, 0, [ra], [pr, 0.0]) == [math.sqrt(pr / ra), 1.0 / math.sqrt(pr * ra)]
    m = vec.VecMixing._derive(vec.VecMixing.__new__(vec.VecMixing))            # defaults: re 100, pe 1e4, u_max = re nu / L
    assert _derive(L, 1, [m.re, m.pe], [m.re, m.u_max]) == [1.0 / m.re, 1.0 / m.pe, m.u_max]
    for re_, pe in ((50.0, 1.0e3), (200.0, 1.0e5), (400.0, 2.0e3)):
        assert _derive(L, 1, [re_, pe], [m.re, m.u_max]) == [1.0 / re_, 1.0 / pe, re_ * m.nu / m.L]
    assert _derive(L, 2, [0.5, 10.0]) == [0.5, 10.0]                            # burgers: u_target, amp as they are
    for delta in (0.1, 0.05, 0.08, 0.15, 0.2):                                  # shkadov: 1 / (5 delta)
        assert _derive(L, 3, [delta]) == [1.0 / (5.0 * delta)]
    assert _derive(L, 4, [5.0, 0.0005, 9.81]) == [5.0, 0.0005, 9.81]            # sloshing: amp, alpha, g
    assert _derive(L, 5, [10.0, 28.0, 8.0 / 3.0]) == [10.0, 28.0, 8.0 / 3.0]    # lorenz
    for re_ in (50.0, 47.0, 80.0, 120.0):                                       # vortex.py: 1/re_crit - 1/re
        assert _derive(L, 6, [re_, 50.0], [46.6, 0.0]) == [1.0 / 46.6 - 1.0 / re_, 50.0]
    assert L.bcn_derive_params_host(99, (C.c_double * 3)(), (C.c_double * 2)(), (C.c_double * 3)()) == -1
    # and *_create calls the same functions: no second copy of an expression in capi.hip
    src = open(os.path.join(ROOT, "beacon_amd", "csrc", "capi.hip")).read()
    for fn in ("bcn_rayleigh_kmom", "bcn_rayleigh_ksc", "bcn_mixing_kmom", "bcn_mixing_ksc", "bcn_mixing_u_max", "bcn_shkadov_delta_p",
               "bcn_vortex_ire"):
        assert src.count(fn + "(") == 1, fn
    assert "sqrt(c->pr" not in src and "1.0 / c->re" not in src and "5.0 * c->delta" not in src


def test_ns2d_args_and_the_fast_kernels_sources_are_untouched_by_the_table():
    """NS2DArgs is the kernel argument block of the register-saturated kernels: the table must not be a member of it (nor of
    anything ns2d.h declares); it is an argument of the generic kernel of its own."""
    csrc = os.path.join(ROOT, "beacon_amd", "csrc")
    assert "prm" not in open(os.path.join(csrc, "ns2d.h")).read()
    gen = open(os.path.join(csrc, "ns2d_generic.hip")).read()
    assert re.search(r"void ns2d_generic_step\(NS2DArgs<real> A, const real\* __restrict__ prm\)", gen)
    for f in ("ns2d_fast.hip", "ns2d_fast_f64.hip", "ns2d_fast2.hip", os.path.join("jit", "ns2d_jit.hip")):
        assert "params.h" not in open(os.path.join(csrc, f)).read()


def _kernel_meta(text):
    """{kernel symbol: private segment bytes} from the metadata of a device assembly file"""
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1))
    return out


@pytest.mark.parametrize("unit", ["env1d_f32.hip", "env1d_f64.hip", "ode_f32.hip", "ode_f64.hip"])
def test_no_1d_or_ode_kernel_gained_a_private_segment(unit, tmp_path):
    """hipcc --offload-arch=gfx950 --cuda-device-only -S of the unit with the library's own flags, against the per-kernel list of
    the commit before the feature (tests/golden/params_parent_private_segments.json): the same kernels, and none that had no
    private segment has one now (the overwritten copy of the argument block stays in scalar registers).  The 1D units keep their
    number of vector loads from global memory: the table is read by scalar loads."""
    from beacon_amd import build
    cc = build.hipcc()
    if cc is None:
        pytest.skip("no hipcc")
    parent = json.load(open(os.path.join(GOLD, "params_parent_private_segments.json")))[unit]
    src = os.path.join(build.CSRC, unit)
    asm = str(tmp_path / (unit + ".s"))
    subprocess.check_call(build.compile_cmd(src, asm, mode=("--cuda-device-only", "-S")))
    text = open(asm).read()
    now = _kernel_meta(text)
    assert set(now) == set(parent), set(now) ^ set(parent)
    grew = {k: (parent[k], now[k]) for k in parent if parent[k] == 0 and now[k] != 0}
    assert not grew, grew
    assert all(now[k] <= parent[k] for k in parent), {k: (parent[k], now[k]) for k in parent if now[k] > parent[k]}
    # the parameter loads: scalar in the one-workgroup-per-replica kernels (s_load_*), one column per lane in the ODE kernels
    body = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith(";"))
    if unit.startswith("env1d"):
        start = {"env1d_f32.hip": 1320, "env1d_f64.hip": 1245}[unit]            # vector loads of the unit before the feature
        assert len(re.findall(r"^\s+global_load_", body, flags=re.M)) == start
    stores = set(re.findall(r"^\s*((?:global|flat|scratch|buffer|s)_\w*store\w*)", body, flags=re.M))
    assert all(not s.startswith("s_") for s in stores), stores                  # nothing is stored through the scalar unit


def test_byte_model_of_the_ode_benchmark_counts_the_parameter_columns():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_envs", os.path.join(ROOT, "scripts", "bench_envs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for esz in (4, 8):
        assert mod.ode_bytes_per_replica_step("lorenz", esz, params=True) - mod.ode_bytes_per_replica_step("lorenz", esz) == 3 * esz
        assert mod.ode_bytes_per_replica_step("vortex", esz, params=True) - mod.ode_bytes_per_replica_step("vortex", esz) == 2 * esz
    assert mod.ode_bytes_per_replica_step("lorenz", 4) == 94 and mod.ode_bytes_per_replica_step("lorenz", 4, params=True) == 106
