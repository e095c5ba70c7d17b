"""CPU tier: the statistics phase of the separable transform writes each row's Ψ into the LDS once (psi[sd_swz(j)],
mioc_sdt.hip: sdt_stats), checked on the compiled gfx950 code by the kernels' static count of `ds_write_b64`.

The parent of this change wrote Ψ twice per statistics site (by rank, and raw at the swizzled position for pass 0): eight
stores more per site, and a ninth for the seam lanes' straddle element at M = 4.  Its counts are recorded here;
k_sdt_run1 and k_sdt_run hold two statistics sites (the first item's and the tail's), k_sdt_step one.

Source: mioc_sdt.hip, compiled with the library's own flags (as tests/test_isa_guard.py does).
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mixed-integer-optimal-control---algorithm-tools_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import isa_vmcnt as iv  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950"]
# symbol: (the parent's ds_write_b64 count, statistics sites)
PARENT = {"k_sdt_run1ILi4": (142, 2), "k_sdt_runILi4": (135, 2), "k_sdt_stepILi4": (110, 1),
          "k_sdt_run1ILi3": (121, 2), "k_sdt_runILi3": (114, 2), "k_sdt_stepILi3": (94, 1)}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    o = str(tmp_path_factory.mktemp("isa_psi") / "mioc_sdt.s")
    p = subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", "-o", o, "mioc_sdt.hip"], cwd=CSRC,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    return o


@pytest.mark.parametrize("sym", list(PARENT))
def test_one_lds_copy_of_psi(listing, sym):
    ops = [l.split(";")[0].split() for l in iv.function_lines(listing, sym)]
    n = sum(1 for t in ops if t and t[0] == "ds_write_b64")
    was, sites = PARENT[sym]
    print(sym, "ds_write_b64", n, "parent", was)
    assert n <= was - 8 * sites, (sym, n, was)
