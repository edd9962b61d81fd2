"""CPU test of the 8-byte routed row form (PTF_ROW8): choose_routed_layout and choose_pass2 against values written out by hand for
the headline's table, the shapes that must keep their 12-byte (or other) rows, and pass 1's LDS bytes for both scanner splits.
tests/native/row8_layout_check.cpp is a stand-alone program: built and run once plain, once under the host sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "row8_layout_check.cpp")


def test_row8_layout_program(tmp_path):
    for name, flags in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / f"row8_layout_check_{name}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.startswith("ok:"), name + ":\n" + r.stdout[-2000:] + r.stderr[-2000:]


def test_row8_option_and_counter_are_wired():
    from datafusion_archive_amd import build as B

    table = open(os.path.join(B.CSRC, "dfx_options.cpp")).read()
    assert '"agg.routed_row8"' in table and '"agg_row8_launches"' in table
    assert "int routed_row8 = -1;" in open(os.path.join(B.CSRC, "dfx_relation.hpp")).read()
