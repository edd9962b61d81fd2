"""CPU test of the routed shadow's decision rule (csrc/dfx_routed_shadow.hpp) and of the choice of pass 2's scan form
(choose_pass2_scan, csrc/dfx_pass2_forms.hpp): the option's three values, the build point, the memory rule at its edge, the silent
drops, the refusal for good after a spilled row, which launches bind a window (aligned and unaligned slices, the tail window, a
geometry mismatch, a second column pair), and the scan form against a table written out by hand.
tests/native/routed_shadow_rule.cpp runs it with the device stubbed, as a stand-alone program: once plain, once under the host
sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "routed_shadow_rule.cpp")


def test_routed_shadow_rule_program(tmp_path):
    for name, flags in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / f"routed_shadow_rule_{name}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.startswith("ok:"), name + ":\n" + r.stdout[-2000:] + r.stderr[-2000:]
