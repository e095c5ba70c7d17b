"""CPU tier: listing facts of the one-row persistent separable-transform kernel k_sdt_run1<3> / <4>, checked on the
compiled gfx950 code -- the same facts tests/test_isa_item.py and tests/test_isa_guard.py hold k_sdt_run to:

  * no SGPR spills, no VGPR spills, no scratch;
  * no `s_nop` directly after a `v_min_f64`;
  * exactly one hand-written row start `s_waitcnt vmcnt(5)`, and on every path exactly the previous item's five stores
    lie between the last load and it (six on wave 0's path through the `done` flag store: slack 1, as for k_sdt_run).

Source: mioc_sdt.hip, compiled with the library's own flags.
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
SDT_RUN1 = ["k_sdt_run1ILi3", "k_sdt_run1ILi4"]

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    o = str(tmp_path_factory.mktemp("isa_row_owner") / "mioc_sdt.s")
    p = subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", "-o", o, "mioc_sdt.hip"], cwd=CSRC,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    return o


def _opcodes(lines):
    out = []
    for n, l in enumerate(lines):
        t = l.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        out.append((n, t.split()[0]))
    return out


@pytest.mark.parametrize("sym", SDT_RUN1)
def test_row_owner_is_its_own_kernel(listing, sym):
    """The symbol is not one the general kernel's listing tests would pick up."""
    lines = open(listing).read().split("\n")
    names = [l.split(":")[0] for l in lines if l.startswith("_Z") and sym in l.split(":")[0] and ":" in l]
    assert names, sym
    assert not [n for n in names if "k_sdt_runILi" in n], names


@pytest.mark.parametrize("sym", SDT_RUN1)
def test_row_owner_no_spills_no_scratch(listing, sym):
    meta = iv.kernel_meta(listing, sym)
    assert meta.get("sgpr_spill_count") == 0, meta
    assert meta.get("vgpr_spill_count") == 0, meta
    assert meta.get("private_segment_fixed_size") == 0, meta
    ins, _ = iv.parse(iv.function_lines(listing, sym))
    assert not [t for op, t in ins if op.startswith("scratch_")], "scratch access"


@pytest.mark.parametrize("sym", SDT_RUN1)
def test_row_owner_no_nop_after_min(listing, sym):
    lines = iv.function_lines(listing, sym)
    ops = _opcodes(lines)
    assert sum(op == "v_min_f64" for _, op in ops) > 100, "not the kernel's listing"
    bad = [lines[n].strip() + f" (function line {n})" for (_, a), (n, b) in zip(ops, ops[1:])
           if a == "v_min_f64" and b == "s_nop"]
    assert not bad, bad[:5]


@pytest.mark.parametrize("sym", SDT_RUN1)
def test_row_owner_row_start_wait(listing, sym):
    res, bad = iv.check_wait(listing, sym, 5, "load", slack=1)
    assert len(res) == 1, res
    assert not bad, bad
