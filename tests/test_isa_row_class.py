"""CPU tier: per-class listing facts of the one-row persistent kernel k_sdt_run1<3> / <4> (compiled gfx950 code) that
tests/test_isa_row_owner.py does not look at.  The kernel decides its row's class once (lowc: a source row may be below
0; highc: a target may lie outside the trust region) and branches on it at the class-dependent sites of the one item
loop:

  * the load issue has a short arm: one straight-line block that forms all four 16-byte load offsets without a signed
    compare of a source row against 0 / 1 and with no v_cndmask but the straddle tests' (one mask bit per pair; at
    M = 3 also one second-element offset per pair).  The general kernel k_sdt_run<M>, which does not know the class,
    has no such block;
  * the arms share the loads and stores: the kernel has as many vector-memory instructions of each kind as before the
    class branches (no load or store hoisted into an arm or duplicated);
  * no spill, no scratch, and a vector register count that keeps two waves per SIMD (at most 256 of the 512 per lane),
    the parent's occupancy (it had 244 / 214).

Source: mioc_sdt.hip, compiled with the library's own flags.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mixed-integer-optimal-control---algorithm-tools_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import isa_vmcnt as iv  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950"]
# symbol, the general kernel's symbol, v_cndmask allowed in the short arm
KERNELS = [("k_sdt_run1ILi3", "k_sdt_runILi3", 8), ("k_sdt_run1ILi4", "k_sdt_runILi4", 4)]
# vector-memory instructions of the kernel by kind, as before the class branches
VM = {
    "k_sdt_run1ILi3": {"buffer_load_dwordx4": 8, "buffer_load_dwordx2": 8, "buffer_store_dwordx4": 4},
    "k_sdt_run1ILi4": {"buffer_load_dwordx4": 8, "buffer_load_dwordx2": 2, "buffer_store_dwordx4": 4},
}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    o = str(tmp_path_factory.mktemp("isa_row_class") / "mioc_sdt.s")
    p = subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", "-o", o, "mioc_sdt.hip"], cwd=CSRC,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    return o


def _offset_blocks(path, sym):
    """The straight-line blocks between the item loop's row start (the hand-written vmcnt(5)) and its four 16-byte
    loads that write all four of the loads' offset registers: (VALU, v_cndmask, signed compares) of each."""
    marks = []
    ins, labels = iv.parse(iv.function_lines(path, sym), marks)
    starts = set(labels.values())
    row = [i for i in marks if ins[i][0] == "s_waitcnt" and iv.vmcnt_of(ins[i][1]) == 5]
    assert len(row) == 1, row
    loads = [i for i in range(row[0], len(ins)) if ins[i][0] == "buffer_load_dwordx4"][:4]
    assert len(loads) == 4 and loads[3] - loads[0] < 16, loads  # one group
    offs = [re.match(r"buffer_load_dwordx4 v\[\d+:\d+\], (v\d+),", ins[i][1]).group(1) for i in loads]
    blocks, cur = [], []
    for i in range(row[0], loads[0]):
        if i in starts and cur:
            blocks.append(cur)
            cur = []
        cur.append(i)
        if ins[i][0].startswith(("s_cbranch", "s_branch")):
            blocks.append(cur)
            cur = []
    blocks.append(cur)
    out = []
    for b in blocks:
        defs = {m.group(1) for m in (re.match(r"v_\S+ (v\d+),", ins[i][1]) for i in b) if m}
        if all(r in defs for r in offs):
            ops = [ins[i][0] for i in b]
            out.append((sum(o.startswith("v_") for o in ops), sum(o.startswith("v_cndmask") for o in ops),
                        sum(bool(re.match(r"v_cmp_(gt|lt|ge|le)_i32", o)) for o in ops)))
    return out


@pytest.mark.parametrize("sym,general,sel", KERNELS)
def test_row_class_load_issue_short_arm(listing, sym, general, sel):
    short = [b for b in _offset_blocks(listing, sym) if b[2] == 0]
    assert len(short) == 1, _offset_blocks(listing, sym)
    valu, cnd, _ = short[0]
    assert cnd <= sel, short
    assert valu <= 40, short  # the general form is 59 (M = 4) and more
    # the general kernel forms its offsets with the source-row tests on every path
    assert not [b for b in _offset_blocks(listing, general) if b[2] == 0], _offset_blocks(listing, general)


@pytest.mark.parametrize("sym,general,sel", KERNELS)
def test_row_class_arms_share_loads_and_stores(listing, sym, general, sel):
    inv = iv.vm_inventory(listing, sym)
    for op, n in VM[sym].items():
        assert inv.get(op, 0) == n, (op, inv)


@pytest.mark.parametrize("sym,general,sel", KERNELS)
def test_row_class_registers(listing, sym, general, sel):
    meta = iv.kernel_meta(listing, sym)
    assert meta.get("sgpr_spill_count") == 0 and meta.get("vgpr_spill_count") == 0, meta
    assert meta.get("private_segment_fixed_size") == 0, meta
    assert 0 < meta.get("vgpr_count") <= 256, meta  # two waves per SIMD, as the parent's 244 / 214
