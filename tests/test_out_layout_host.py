"""The packed output buffer [obs | rwd | status | done | trunc] has ONE definition in C (include/beacon_hip.h: bcn_out_layout,
which the library indexes device memory with and the torch ops bounds-check with) and one in Python (beacon_amd.vec.out_layout,
which allocates the buffer): a plain C program prints the first and it is compared with the second.  No GPU."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

BATCHES, OBS, ESZ = (1, 3, 17, 1024), (1, 5, 192), (4, 8)

PROGRAM = r"""
#include <stdio.h>
#include "beacon_hip.h"
int main(void) {
  const size_t B[] = {%s}, N[] = {%s}, E[] = {%s};
  for (size_t i = 0; i < sizeof(B) / sizeof(B[0]); i++)
    for (size_t j = 0; j < sizeof(N) / sizeof(N[0]); j++)
      for (size_t k = 0; k < sizeof(E) / sizeof(E[0]); k++) {
        const bcn_out_layout_t o = bcn_out_layout(B[i], N[j], E[k]);
        printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\n", B[i], N[j], E[k], o.obs, o.rwd, o.status, o.done, o.trunc, o.bytes);
      }
  return 0;
}
"""


def test_python_out_layout_is_the_c_helpers(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    from beacon_amd import vec
    src, exe = tmp_path / "out_layout.c", tmp_path / "out_layout"
    src.write_text(PROGRAM % tuple(", ".join(map(str, v)) for v in (BATCHES, OBS, ESZ)))
    subprocess.check_call([cc, "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    rows = [tuple(map(int, ln.split())) for ln in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert [r[:3] for r in rows] == [(b, n, e) for b in BATCHES for n in OBS for e in ESZ]
    for b, n, e, *c in rows:
        lay = vec.out_layout(b, n, e)
        assert [lay[k] for k in ("obs", "rwd", "status", "done", "trunc", "bytes")] == c, (b, n, e)
        assert all(v % 16 == 0 for v in c) and lay["bytes"] >= lay["trunc"] + b
