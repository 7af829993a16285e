"""CPU-side checks of the snapshot feature (VecEnv.snapshot / restore / fork): the Snapshot container without a GPU, the two
torch ops, the op tables, the C ABI version, and the copy kernels' build for gfx950 with 16-byte loads and stores."""
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT

NEW = ("bcn_snapshot_bytes", "bcn_snapshot_bytes_n", "bcn_snapshot_layout", "bcn_snapshot_signature", "bcn_snapshot_save",
       "bcn_snapshot_load")


def _snap(n=3, nx=5):
    """a burgers-like snapshot of n replicas, float32, built by hand"""
    from beacon_amd import _lib, vec
    lay, off = [], 0
    for name, elem, planes, row in (("fields", _lib.SNAP_REAL, 3, nx), ("a_last", _lib.SNAP_REAL, 1, 1), ("stp", _lib.SNAP_I32, 1, 1),
                                    ("nctr", _lib.SNAP_U32, 1, 1), ("obs", _lib.SNAP_REAL, 1, 2), ("done", _lib.SNAP_U8, 1, 1)):
        off = (off + 15) // 16 * 16
        lay.append(dict(name=name, offset=off, elem=elem, planes=planes, row_elems=row))
        off += planes * n * row * (1 if elem == _lib.SNAP_U8 else 4)
    buf = torch.arange((off + 15) // 16 * 16, dtype=torch.int64).to(torch.uint8)
    meta = dict(env="VecBurgers", kind=2, dtype="f32", batch=n, signature=0x1234567890abcdef, layout=lay, field_shape=[nx],
                ctor=dict(nx=nx, seed=0), version="test", noise=dict(sigma=0.1, seed=0, replica_offset=0),
                gen_state=torch.arange(16, dtype=torch.uint8))
    return vec.Snapshot(buf, meta)


def test_snapshot_container_views_save_load_and_to(tmp_path):
    import beacon_amd
    s = _snap()
    assert beacon_amd.Snapshot is type(s) and s.batch == 3 and s.signature == 0x1234567890abcdef
    assert s.names() == ["fields", "a_last", "stp", "nctr", "obs", "done"]
    f = s.view("fields")
    assert f.shape == (3, 3, 5) and f.dtype == torch.float32 and f.data_ptr() == s.buf.data_ptr()       # a view, no copy
    assert s.view("a_last").shape == (3, 1) and s.view("obs").shape == (3, 2)
    assert s.view("stp").shape == (3,) and s.view("stp").dtype == torch.int32 and s.view("nctr").dtype == torch.int32
    assert s.view("done").dtype == torch.uint8 and s.view("done").shape == (3,)
    for seg in s.meta["layout"]:
        assert seg["offset"] % 16 == 0
    assert torch.equal(s.view("done"), s.buf[s.meta["layout"][-1]["offset"]:][:3])
    with pytest.raises(KeyError):
        s.view("sweeps")
    with pytest.raises(ValueError):
        type(s)(torch.zeros(4), {})
    s.save(tmp_path / "s.pt")
    r = type(s).load(tmp_path / "s.pt")
    assert torch.equal(r.buf, s.buf) and r.buf.device.type == "cpu"
    assert {k: v for k, v in r.meta.items() if k != "gen_state"} == {k: v for k, v in s.meta.items() if k != "gen_state"}
    assert torch.equal(r.meta["gen_state"], s.meta["gen_state"])
    assert torch.equal(r.view("fields"), f)
    assert s.to("cpu") is s
    t = type(s).load(tmp_path / "s.pt", device="cpu")
    assert torch.equal(t.buf, s.buf) and t.meta["ctor"] == s.meta["ctor"]


def test_env_surface_exists():
    from beacon_amd import vec
    for m in ("snapshot", "restore", "fork", "snapshot_signature"):
        assert callable(getattr(vec.VecEnv, m))


def test_op_tables_and_api_version():
    from beacon_amd import _lib, build, vec
    assert len(vec._OPS) == 10
    assert vec._ODE_OPS == ("lorenz_reset", "lorenz_step", "vortex_reset", "vortex_step")
    assert vec._STATE_OPS == ("snapshot_save", "snapshot_load")
    hdr = open(os.path.join(ROOT, "include", "beacon_hip.h")).read()
    declared = set(re.findall(r"BCN_API\s+[\w\s\*]+?\b(bcn_\w+)\s*\(", hdr))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.SIGNATURES)
    assert int(re.search(r"#define BCN_API_VERSION (\d+)", hdr).group(1)) == 4 and _lib.API_VERSION == 4
    # the ctypes struct mirrors bcn_snapshot_seg
    body = re.search(r"typedef struct \{([^{}]*)\} bcn_snapshot_seg;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[\d+\]", "", d.split()[-1]) for d in body.split(";") if d.strip()]
    assert names == [n for n, _ in _lib.SnapshotSeg._fields_]
    if build.hipcc() is None and not os.path.exists(build.LIB):
        pytest.skip("no hipcc and no prebuilt library")
    L = _lib.load()
    for name in NEW:
        assert hasattr(L, name)
    assert L.bcn_api_version() == 4
    assert L.bcn_snapshot_bytes(None) == 0 and L.bcn_snapshot_signature(None) == 0                       # null handles are refused
    assert L.bcn_snapshot_save(None, None, None, None) == 1 and L.bcn_snapshot_load(None, None, 1, None, None, None, None) == 1


def test_torch_extension_defines_and_registers_the_snapshot_ops():
    from beacon_amd import build, torch_ext, vec
    src = open(os.path.join(ROOT, "beacon_amd", "csrc", "torch", "beacon_torch.cpp")).read()
    for n in vec._STATE_OPS:
        assert src.count('m.def("%s(' % n) == 1 and src.count('m.impl("%s"' % n) == 2, n                  # CUDA and Meta
    if (shutil.which("g++") is None and torch_ext.stale()) or (build.hipcc() is None and not os.path.exists(build.LIB)):
        pytest.skip("no compiler and no prebuilt extension")
    path = torch_ext.build_ext()
    assert path and os.path.exists(path) and not torch_ext.stale()
    ops = torch_ext.load()
    table = vec._op_table()
    assert ops is not None and table is not None and set(vec._STATE_OPS) <= set(table)
    assert str(ops.snapshot_save.default._schema) == "beacon::snapshot_save(int handle, Tensor(a!) snap, Tensor out_buf) -> ()"
    assert str(ops.snapshot_load.default._schema) == ("beacon::snapshot_load(int handle, Tensor snap, int n_src, Tensor? src, "
                                                      "Tensor? mask, Tensor(a!) out_buf) -> ()")
    with pytest.raises((NotImplementedError, RuntimeError)):                # CUDA key only: CPU tensors find no kernel
        ops.snapshot_save(0, torch.zeros(16, dtype=torch.uint8), torch.zeros(16, dtype=torch.uint8))


def test_copy_kernels_compile_for_gfx950_with_16_byte_accesses(tmp_path):
    """csrc/snapshot.hip with the library's own flags: both kernels are there, the aligned path loads and stores 16 bytes per
    lane, nothing spills to scratch (the segment table is indexed in the kernel arguments, not copied), and the only stores
    are vector stores to global memory."""
    from beacon_amd import build
    cc = build.hipcc()
    if cc is None:
        pytest.skip("no hipcc")
    src = os.path.join(build.CSRC, "snapshot.hip")
    assert src in build.sources()
    asm = str(tmp_path / "snapshot.s")
    subprocess.check_call(build.compile_cmd(src, asm, mode=("--cuda-device-only", "-S")))
    text = open(asm).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    assert len(kernels) == 2 and all("snapshot_copy_k" in k for k in kernels), kernels
    assert text.count("global_load_dwordx4") >= 8 and text.count("global_store_dwordx4") >= 8      # 4 in flight per lane, 2 kernels
    assert re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text) == ["0", "0"]
    stores = set(re.findall(r"^\s*((?:global|flat|scratch|buffer|s)_\w*store\w*)", text, flags=re.M))
    assert stores and all(s.startswith("global_store_") for s in stores), stores
