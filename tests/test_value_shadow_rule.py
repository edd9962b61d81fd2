"""CPU test of the value shadow's decision rule (csrc/dfx_value_shadow.hpp): when the Float32 copy of a resident Float64 operand
column is built (agg.value_shadow, the second qualifying query), the memory rule, the silent drops and the refusal for good of a
column that is not Float32-exact.  tests/native/value_shadow_rule.cpp runs it with the device stubbed, as a stand-alone program:
once plain, once under the host sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "value_shadow_rule.cpp")


def test_value_shadow_rule_program(tmp_path):
    for name, flags in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / f"value_shadow_rule_{name}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.startswith("ok:"), name + ":\n" + r.stdout[-2000:] + r.stderr[-2000:]
