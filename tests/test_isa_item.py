"""CPU tier: listing facts of the persistent separable-transform kernel k_sdt_run<3> / <4> (the C4 headline kernel),
checked on the compiled gfx950 code.

The kernel's row loop uses every scalar register the hardware has (106).  When the register allocator runs out, it
parks launch constants in the lanes of a vector register and reads them back with v_readlane_b32 inside the row --
about fifty per row before this file existed.  And every separate inline-asm v_min_f64 draws the compiler's boundary
wait state (`s_nop`) before a dependent instruction, which in the merge sweeps of the transform came to one per merge.
So, for both instantiations:

  * no SGPR spills, no VGPR spills, no scratch;
  * no `s_nop` directly after a `v_min_f64` (comment lines such as the asm-statement markers in between ignored).

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
SDT_RUN = ["k_sdt_runILi3", "k_sdt_runILi4"]

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    o = str(tmp_path_factory.mktemp("isa_item") / "mioc_sdt.s")
    p = subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", "-o", o, "mioc_sdt.hip"], cwd=CSRC,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    return o


@pytest.mark.parametrize("sym", SDT_RUN)
def test_sdt_run_no_spills(listing, sym):
    meta = iv.kernel_meta(listing, sym)
    assert meta.get("sgpr_spill_count") == 0, meta
    assert meta.get("vgpr_spill_count") == 0, meta
    assert meta.get("private_segment_fixed_size") == 0, meta


def _opcodes(lines):
    """(line number, opcode) of every instruction: labels, directives, comment-only and empty lines dropped."""
    out = []
    for n, l in enumerate(lines):
        t = l.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        out.append((n, t.split()[0]))
    return out


@pytest.mark.parametrize("sym", SDT_RUN)
def test_sdt_run_no_nop_after_min(listing, sym):
    lines = iv.function_lines(listing, sym)
    ops = _opcodes(lines)
    assert sum(op == "v_min_f64" for _, op in ops) > 100, "not the kernel's listing"
    bad = [lines[n].strip() + f" (function line {n})" for (_, a), (n, b) in zip(ops, ops[1:])
           if a == "v_min_f64" and b == "s_nop"]
    assert not bad, bad[:5]


def test_nop_check_sees_a_nop():
    """The check itself: a wait state after a v_min_f64 is found through the asm-statement comment lines."""
    lines = ["\tv_add_f64 v[0:1], v[2:3], 1.0", "\t;;#ASMSTART", "\tv_min_f64 v[0:1], v[0:1], v[2:3]", "\t;;#ASMEND",
             "\ts_nop 0", "\tv_add_f64 v[4:5], v[0:1], 1.0"]
    ops = _opcodes(lines)
    assert [(a, b) for (_, a), (_, b) in zip(ops, ops[1:]) if a == "v_min_f64" and b == "s_nop"]
