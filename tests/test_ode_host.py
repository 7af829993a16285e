"""CPU-side checks of the batched ODE envs (VecLorenz, VecVortex): their derived parameters and spaces equal the host ports',
the header declares and the binding binds their six entry points, the built library exports them, the torch extension
registers their four ops, and without a GPU their constructors raise like every other env's."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

NEW = ("bcn_lorenz_create", "bcn_lorenz_reset", "bcn_lorenz_step", "bcn_vortex_create", "bcn_vortex_reset", "bcn_vortex_step")


def _derived(cls, **kw):
    c = cls.__new__(cls)
    return c._derive(**kw)._make_spaces()


def test_vec_ode_envs_derive_what_the_host_classes_do():
    import beacon_amd
    for cls, host, kw in ((beacon_amd.VecLorenz, beacon_amd.lorenz, {}), (beacon_amd.VecLorenz, beacon_amd.lorenz, dict(rho=20.0)),
                          (beacon_amd.VecVortex, beacon_amd.vortex, {}), (beacon_amd.VecVortex, beacon_amd.vortex, dict(re=60.0))):
        v, h = _derived(cls, **kw), host(**kw)
        for k in ("dt", "ndt_act", "n_act", "n_obs"):
            assert getattr(v, k) == getattr(h, k), (cls.__name__, k)
        assert type(v.action_space) is type(h.action_space)
        assert v.observation_space.shape == h.observation_space.shape
        assert np.array_equal(v.observation_space.high, h.observation_space.high)
        assert np.array_equal(v.observation_space.low, h.observation_space.low)
    lz = _derived(beacon_amd.VecLorenz)
    assert (lz.ndt_act, lz.n_act, lz.n_obs) == (1, 500, 6) and lz.action_space.n == 3 and beacon_amd.VecLorenz.action_is_int
    vx = _derived(beacon_amd.VecVortex)
    assert (vx.ndt_act, vx.n_act, vx.n_obs) == (5, 800, 8) and vx.action_space.shape == (2,)
    assert not beacon_amd.VecVortex.action_is_int
    h = beacon_amd.vortex()
    for k in ("lmbda_re", "lmbda_cx", "mu_re", "mu_cx", "alpha_re", "alpha_cx", "beta", "re", "re_crit", "omega_s", "omega_f",
              "gamma", "mass", "weight", "mod_min", "mod_max", "phase_min", "phase_max"):
        assert getattr(vx, k) == getattr(h, k), k
    assert beacon_amd.VEC_ENVS["lorenz-v0"] is beacon_amd.VecLorenz and beacon_amd.VEC_ENVS["vortex-v0"] is beacon_amd.VecVortex


def test_ode_entry_points_declared_bound_and_exported():
    from beacon_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "beacon_hip.h")).read()
    declared = set(re.findall(r"BCN_API\s+[\w\s\*]+?\b(bcn_\w+)\s*\(", hdr))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.SIGNATURES)
    assert re.search(r"BCN_LORENZ = 5, BCN_VORTEX = 6", hdr)
    # the ctypes structs mirror the C structs field by field
    for cname, cls in (("bcn_lorenz_cfg", _lib.LorenzCfg), ("bcn_vortex_cfg", _lib.VortexCfg)):
        body = re.search(r"typedef struct \{([^{}]*)\} %s;" % cname, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                typ, names = decl.split(None, 1)
                fields += [(n.strip(), typ) for n in names.split(",")]
        assert [n for n, _ in fields] == [n for n, _ in cls._fields_], cname
        assert all((t == "int32_t") == (ct is _lib.C.c_int32) for (_, t), (_, ct) in zip(fields, cls._fields_)), cname
    if build.hipcc() is None and not os.path.exists(build.LIB):
        pytest.skip("no hipcc and no prebuilt library")
    L = _lib.load()
    for name in NEW:
        assert hasattr(L, name)
    assert L.bcn_api_version() == 4


def test_torch_extension_registers_the_ode_ops():
    """The four ODE ops are in the env's op table and registered by the extension (CUDA and Meta keys, outputs in place)."""
    import shutil
    from beacon_amd import build, torch_ext, vec
    ode = ("lorenz_reset", "lorenz_step", "vortex_reset", "vortex_step")
    assert vec._ODE_OPS == ode
    src = open(os.path.join(ROOT, "beacon_amd", "csrc", "torch", "beacon_torch.cpp")).read()
    for n in ode:
        assert 'm.def("%s(' % n in src and src.count('m.impl("%s"' % n) == 2, n     # CUDA and Meta
    if (shutil.which("g++") is None and torch_ext.stale()) or (build.hipcc() is None and not os.path.exists(build.LIB)):
        pytest.skip("no compiler and no prebuilt extension")
    path = torch_ext.build_ext()
    assert path and os.path.exists(path) and not torch_ext.stale()
    ops = torch_ext.load()
    table = vec._op_table()
    assert ops is not None and table is not None and set(ode) <= set(table)
    for n in ode:
        schema = str(getattr(ops, n).default._schema)
        assert schema.startswith("beacon::%s(int handle" % n) and schema.endswith("-> ()") and "Tensor(a!) obs" in schema, schema
    assert "Tensor? actions" in str(ops.lorenz_step.default._schema) and "Tensor? actions" in str(ops.vortex_step.default._schema)
    with pytest.raises((NotImplementedError, RuntimeError)):                # CUDA key only: CPU tensors find no kernel
        ops.lorenz_reset(0, torch.zeros(6))


def test_ode_envs_have_no_cpu_fallback():
    import beacon_amd
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for cls in (beacon_amd.VecLorenz, beacon_amd.VecVortex):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cls(4)
