"""CPU-side checks of the per-replica parameter variant of the register-resident 2D kernels (csrc/ns2d_prm.h, bcn_set_option
"params_kernel", bcn_set_fast_plugin_params): the C ABI's new entry point in the header, the binding and the built library; the
plain units' gfx950 code, which must be what it was before the variant existed; and the on-demand plugin built with
-DBCN_JIT_PRM=1."""
import importlib.util
import json
import os
import re
import subprocess

import pytest

from conftest import GOLD, ROOT


def _tool():
    spec = importlib.util.spec_from_file_location("params_fast_kernels", os.path.join(ROOT, "scripts", "params_fast_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _parent():
    return json.load(open(os.path.join(GOLD, "params_fast_parent_kernels.json")))


def test_header_binding_and_library_have_the_plugin_entry_point_and_the_option():
    from beacon_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "beacon_hip.h")).read()
    declared = set(re.findall(r"BCN_API\s+[\w\s\*]+?\b(bcn_\w+)\s*\(", hdr))
    assert "bcn_set_fast_plugin_params" in declared and "bcn_set_fast_plugin_params" in _lib.SIGNATURES
    assert re.search(r"bcn_set_fast_plugin_params\(bcn_env_t h, void\* launch_fn\)", hdr)
    assert "bcn_jit_launch_prm(const void* step_args, int batch, void* stream, const void* params_table_dev)" in hdr
    assert re.search(r'\*\s+"params_kernel" 0 / 1', hdr)                                     # in the option list of bcn_set_option
    assert hdr.index('"params_kernel" 0 / 1') < hdr.index("BCN_API int bcn_set_option")
    assert int(re.search(r"#define BCN_API_VERSION (\d+)", hdr).group(1)) == 4 and _lib.API_VERSION == 4     # no buffer changed size
    if build.hipcc() is None and not os.path.exists(build.LIB):
        pytest.skip("no hipcc and no prebuilt library")
    L = _lib.load()
    assert hasattr(L, "bcn_set_fast_plugin_params")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True)
    if out.returncode == 0:
        assert "bcn_set_fast_plugin_params" in set(line.split()[-1] for line in out.stdout.splitlines() if line.strip())
    assert L.bcn_set_fast_plugin_params(None, None) == 1 and b"null handle" in L.bcn_last_error()


def test_the_variant_is_a_macro_of_new_units_with_their_siblings_flags():
    """The parameter instantiations live in translation units of their own that define BCN_PRM_KERNELS before the include and are
    built with the per-file flags of their siblings; the plain units neither define the macro nor mention params.h, ns2d.h does not
    know the table, and the impl headers have no template parameter for it."""
    from beacon_amd import build
    csrc = build.CSRC
    units = [os.path.basename(f) for f in build.sources()]
    for new, old in (("ns2d_fast_prm.hip", "ns2d_fast.hip"), ("ns2d_fast_prm_f64.hip", "ns2d_fast_f64.hip"), ("ns2d_fast2_prm.hip", "ns2d_fast2.hip")):
        assert new in units and build.FILE_FLAGS[new] == build.FILE_FLAGS[old]
        text = open(os.path.join(csrc, old)).read()
        assert "params.h" not in text and not re.search(r"#\s*define\s+BCN_PRM_KERNELS", text)
    for new in ("ns2d_fast_prm.hip", "ns2d_fast2_prm.hip"):
        text = open(os.path.join(csrc, new)).read()
        assert text.index("#define BCN_PRM_KERNELS") < text.index("#include")
    assert "prm" not in open(os.path.join(csrc, "ns2d.h")).read()
    jit = open(os.path.join(csrc, "jit", "ns2d_jit.hip")).read()
    assert "params.h" not in jit and "BCN_JIT_PRM" in jit
    for h in ("ns2d_fast_impl.h", "ns2d_fast2_impl.h", "ns2d_fast4_impl.h"):
        text = open(os.path.join(csrc, h)).read()
        assert '#include "ns2d_prm.h"' in text and "BCN_PRM_LOCAL(KIND)" in text and not re.search(r"template <[^>]*PRM", text)


@pytest.mark.parametrize("unit", ["ns2d_fast.hip", "ns2d_fast_f64.hip", "ns2d_fast2.hip"])
def test_the_plain_units_kept_their_kernels(unit, tmp_path):
    """hipcc --offload-arch=gfx950 --cuda-device-only -S of the unit with the library's own flags against the table of the commit
    before the variant (tests/golden/params_fast_parent_kernels.json, written there by scripts/params_fast_kernels.py): the same
    kernel names, and for each the same VGPRs, SGPRs, private segment, LDS and number of instruction lines."""
    from beacon_amd import build
    if build.hipcc() is None:
        pytest.skip("no hipcc")
    T = _tool()
    now = T.kernel_table(T.unit_asm(build, unit, str(tmp_path / (unit + ".s"))))
    parent = _parent()[unit]
    assert set(now) == set(parent), set(now) ^ set(parent)
    assert now == parent, {k: (parent[k], now[k]) for k in parent if parent[k] != now[k]}


@pytest.mark.parametrize("grid", [(75, 50, False, 0), (100, 110, False, 1), (50, 150, False, 0)], ids=["rows1", "rows2", "rows4"])
def test_parameter_plugin_cross_compiles_and_exports_its_launcher(grid):
    """One grid of each kernel family: build_plugin(..., extra_defs={"BCN_JIT_PRM": 1}) cross-compiles a shared object of its own that
    exports bcn_jit_launch_prm next to the usual symbols; the plain plugin of the same grid does not export it."""
    from beacon_amd import build, jit
    if build.hipcc() is None:
        pytest.skip("no hipcc")
    assert dict(jit.PRM_DEFS) == {"BCN_JIT_PRM": 1} and grid in jit.PRM_TEST_GRIDS
    prm = jit.build_plugin(*grid, extra_defs=dict(jit.PRM_DEFS))
    plain = jit.build_plugin(*grid)
    assert prm and plain and prm != plain

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        return set(line.split()[-1] for line in out.stdout.splitlines() if line.strip())
    usual = {"bcn_jit_launch", "bcn_jit_scratch_elems", "bcn_jit_lds_bytes"}
    assert usual | {"bcn_jit_launch_prm"} <= exported(prm)
    assert usual <= exported(plain) and "bcn_jit_launch_prm" not in exported(plain)


def test_the_plain_plugin_kept_its_kernels(tmp_path):
    """The device code of a plain plugin (75x50 float32, one row per lane) against the commit before the variant: the same
    comparison as for the library's units."""
    from beacon_amd import build, jit
    if build.hipcc() is None:
        pytest.skip("no hipcc")
    T = _tool()
    g = T.PLUGIN_GRIDS[0]
    now = T.kernel_table(T.plugin_asm(build, T.plugin_defs(jit.choose, *g), str(tmp_path / "plugin.s")))
    parent = _parent()[T.plugin_key(g)]
    assert now == parent, (set(now) ^ set(parent), {k: (parent[k], now[k]) for k in parent if k in now and parent[k] != now[k]})
    # and with the flag: other kernels (the table is an argument), none of the plain ones
    prm = T.kernel_table(T.plugin_asm(build, T.plugin_defs(jit.choose, *g, extra=dict(jit.PRM_DEFS)), str(tmp_path / "plugin_prm.s")))
    steps = lambda t: {k for k in t if "NS2DArgs" in k}                     # (ns2d_rank_by_work takes no argument block: in both)
    assert len(steps(prm)) == len(steps(parent)) == 4 and not steps(prm) & steps(parent)


def test_prebuild_lists_the_parameter_plugins_of_the_gpu_tests():
    from beacon_amd import jit
    extra = [(g, d) for g, d in jit.EXTRA_BUILDS if d.get("BCN_JIT_PRM") == 1]
    assert [g for g, d in extra if "BCN_JIT_BREAK" not in d] == jit.PRM_TEST_GRIDS
    assert [(g, d) for g, d in extra if "BCN_JIT_BREAK" in d] == [(jit.PRM_BREAK_GRID, {"BCN_JIT_PRM": 1, "BCN_JIT_BREAK": 1})]
    for g in jit.PRM_TEST_GRIDS + [jit.PRM_BREAK_GRID]:
        assert g in jit.TEST_GRIDS and g not in jit.BUILTIN_GRIDS
    fam = [jit.choose(*g)["rows"] for g in jit.PRM_TEST_GRIDS]
    assert fam == [1, 2, 2, 4] and jit.choose(50, 75, True, 0)["gf"] == 1          # global scratch
