"""CPU test of the forms of pass 2 of the partitioned GROUP BY and of their choice (csrc/dfx_pass2_forms.hpp): choose_pass2 over
every combination of the five flags that matter, na, kw, n_words, two block sizes and the pair forms' operand patterns against
tables written out by hand.  tests/native/pass2_forms_check.cpp is a stand-alone program: built and run once plain, once under
the host sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pass2_forms_check.cpp")


def test_pass2_forms_program(tmp_path):
    for name, flags in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / f"pass2_forms_check_{name}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.startswith("ok:"), name + ":\n" + r.stdout[-2000:] + r.stderr[-2000:]


def test_pass2_has_its_translation_unit():
    from datafusion_archive_amd import build as B

    assert B.GUARD_SRC == "dfx_k_pass2.hip" and B.GUARD_SRC in B.SOURCES
    assert "dfx_pass2_forms.hpp" in B.HEADERS
    text = open(os.path.join(B.CSRC, B.GUARD_SRC)).read()
    assert "DFX_PARTITION_MAIN_TU" not in text  # (the macro that once kept pass 1's sizing functions in one translation unit; they are inline in dfx_pass1_layout.hpp now)
