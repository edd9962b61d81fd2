"""CPU test of the rule a Utf8 column's byte total is judged by and of the slot where a scan leaves its 64-bit grand total
(csrc/dfx_scan_rules.hpp): the sort, the resident table, the CSV source and the filter read that slot and ask that rule, so a total of
2^32 bytes or more is refused instead of wrapping to a small positive int32.  tests/native/utf8_total_rule_check.cpp is a stand-alone
program: once plain, once under the host sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "utf8_total_rule_check.cpp")


def test_utf8_total_rule_program(tmp_path):
    for name, flags in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / f"utf8_total_rule_check_{name}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.startswith("ok:"), name + ":\n" + r.stdout[-2000:] + r.stderr[-2000:]


def test_scan_rules_header_is_free_of_hip():
    text = open(os.path.join(ROOT, "datafusion_archive_amd", "csrc", "dfx_scan_rules.hpp")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<stdint.h>"], includes
