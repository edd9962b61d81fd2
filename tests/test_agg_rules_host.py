"""CPU test of the grouped aggregate's numeric rules (csrc/dfx_agg_rules.hpp): the probing block of a table, the size a table grows
to, the rebuild and replay-in-place conditions, the fill bound after a control-block snapshot, when a pass-2 window closes, the LDS
front cache's slots and copies, the spill list's window rows -- each against a table of inputs and expected outputs written out by
hand.  tests/native/agg_rules_check.cpp is a stand-alone program: once plain, once under the host sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "agg_rules_check.cpp")


def test_agg_rules_program(tmp_path):
    for name, flags in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / f"agg_rules_check_{name}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.startswith("ok:"), name + ":\n" + r.stdout[-2000:] + r.stderr[-2000:]


def test_agg_rules_header_is_free_of_hip():
    text = open(os.path.join(ROOT, "datafusion_archive_amd", "csrc", "dfx_agg_rules.hpp")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<stdint.h>", "<algorithm>"], includes
