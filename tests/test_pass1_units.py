"""CPU test of the list of pass-1 units of the partitioned GROUP BY and of the choice of the scan plan's unit
(csrc/dfx_pass1_units.hpp): plan_unit over every (column count, gen, pair, one_value, PTF_KEY4) against a table written out by hand,
and one distinct name and one launcher slot per unit.  tests/native/pass1_units_check.cpp is a stand-alone program: built and run
once plain, once under the host sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pass1_units_check.cpp")


def test_pass1_units_program(tmp_path):
    for name, flags in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / f"pass1_units_check_{name}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.startswith("ok:"), name + ":\n" + r.stdout[-2000:] + r.stderr[-2000:]


def test_every_pass1_unit_has_its_translation_unit():
    from datafusion_archive_amd import build as B

    units = B._pass1_units()
    assert len(units) == len(set(units)) == 29
    for u in units:
        assert os.path.exists(os.path.join(B.CSRC, f"dfx_k_partition_{u}.hip")), u
        assert f"dfx_k_partition_{u}.hip" in B.SOURCES
    stray = [f for f in os.listdir(B.CSRC) if f.startswith("dfx_k_partition_") and f.endswith(".hip") and f[len("dfx_k_partition_"):-4] not in units]
    assert not stray, stray
