"""CPU test of the row source of the scan kernels (csrc/dfx_row_source.hpp): wants_scan_plan and choose_row_source of every
ScanKernel against the ladders of the launchers the header replaced, written out by hand; the oddities of those ladders by name;
distinct, non-empty names.  tests/native/row_source_check.cpp is a stand-alone program: built and run once plain, once under the
host sanitizers.  And the wiring: the header and the units that came out of dfx_k_core.hip are in the build's lists, and no
launcher keeps a ladder of its own."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "row_source_check.cpp")


def test_row_source_program(tmp_path):
    for name, flags in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / f"row_source_check_{name}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.startswith("ok:"), name + ":\n" + r.stdout[-2000:] + r.stderr[-2000:]


def test_row_source_is_wired_into_the_build():
    from datafusion_archive_amd import build as B

    assert "dfx_row_source.hpp" in B.HEADERS
    for unit in ("dfx_k_filter.hip", "dfx_launch.cpp", "dfx_k_core.hip"):
        assert unit in B.SOURCES and os.path.exists(os.path.join(B.CSRC, unit)), unit
    assert len(B.SOURCES) == len(set(B.SOURCES))
    # the header is host only: the two headers it is built on, nothing else of the project
    text = open(os.path.join(B.CSRC, "dfx_row_source.hpp")).read()
    assert sorted(re.findall(r'#include\s+"([^"]+)"', text)) == ["dfx_device.hpp", "dfx_sigs.hpp"]
    assert not re.search(r"#include\s+<hip", text)


def test_no_launcher_keeps_a_ladder_of_its_own():
    from datafusion_archive_amd import build as B

    sites = ["dfx_k_filter.hip", "dfx_k_core.hip", "dfx_k_reduce.hip", "dfx_k_table_inl.hpp", "dfx_k_fewgroup.hip", "dfx_k_distinct_inl.hpp",
             "dfx_k_partition.hip"]
    for f in sites:
        text = open(os.path.join(B.CSRC, f)).read()
        assert "choose_row_source" in text or "bind_row_source" in text, f
        for gone in ("use_fast", "DFX_MASK", "DFX_FUSED", "DFX_REDUCE_NA", "DFX_HA", "DFX_FG", "DFX_FGP", "DFX_ARG"):
            assert not re.search(r"\b" + gone + r"\b", text), (f, gone)
