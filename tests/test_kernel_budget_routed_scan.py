"""Pass 2's scan form over a routed shadow (k_partition_agg_lean<RowsNarrow8, ACC_ADD_F64, false, SCAN>, csrc/dfx_k_pass2.hip) keeps
its budget: no spilled vector register and no scratch in any of its six comparison forms, the hand-scheduled row registers v88..v119
allocated (118 registers: 8-byte rows end at v117), and no more instructions than the two-pass form it stands in for -- the scan
loop is ONE body behind a scalar switch over the slot pairs, so the stage and the probe path exist three times, not once per slot
(unrolled over the eight slots the compiler stopped inlining the probe path; the row cursor then lived in memory, and the loads'
scalar base address with it).  Its dynamic LDS (8192 x 12 + 24 KB of parked rows + 24 KB of stage = 147 456 bytes) is pinned by
tests/native/routed_shadow_rule.cpp.  The device assembly of the unit is produced as the library builds it (no GPU needed)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCANS = {"no predicate": 1, "x > a AND x < b": 4 | (1 << 3), "x >= a AND x < b": 6 | (1 << 3), "x > a AND x <= b": 4 | (3 << 3),
         "x >= a AND x <= b": 6 | (3 << 3), "run-time operators": 0}


def test_routed_shadow_scan_kernels_register_spill_and_instruction_budget():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_meta.py"), "dfx_k_pass2", "--all"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows8 = [ln for ln in r.stdout.splitlines() if "k_partition_agg_lean<dfx::RowForm<8u, true, false, false>, 0, false, " in ln]

    def fields(line):
        f = {k: int(v) for k, v in re.findall(r"(spilled_sgpr|spilled_vgpr|vgpr|instructions)\s+(\d+)", line)}
        f["scratch"] = int(re.search(r"scratch\s+(\d+) B", line).group(1))
        return f

    parent = [ln for ln in rows8 if "false, -1>" in ln]
    assert len(parent) == 1, r.stdout[-2000:]
    two_pass = fields(parent[0])
    for what, scan in SCANS.items():
        line = [ln for ln in rows8 if f"false, {scan}>" in ln]
        assert len(line) == 1, (what, r.stdout[-2000:])
        f = fields(line[0])
        print(what, f)
        assert f["spilled_vgpr"] == 0 and f["scratch"] == 0, line[0]
        assert f["vgpr"] == 118, line[0]
        assert f["instructions"] <= two_pass["instructions"] * 102 // 100, (line[0], parent[0])
        if scan != 0:  # (the run-time form carries both terms' three compares and selects in scalar registers; it is not the headline's)
            assert f["spilled_sgpr"] <= two_pass["spilled_sgpr"], (line[0], parent[0])
