"""CPU test of the routed layout of the partitioned GROUP BY (csrc/dfx_pass1_layout.hpp): the LDS arithmetic of pass 1 and
choose_routed_layout against tables written out by hand, and the regions' containment and separation over the tables' shapes, the
three scratch layouts and two pads.  tests/native/pass1_layout_check.cpp is a stand-alone program: built and run once plain, once
under the host sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pass1_layout_check.cpp")


def test_pass1_layout_program(tmp_path):
    for name, flags in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / f"pass1_layout_check_{name}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.startswith("ok:"), name + ":\n" + r.stdout[-2000:] + r.stderr[-2000:]


def test_pass1_layout_has_one_home():
    from datafusion_archive_amd import build as B

    assert "dfx_pass1_layout.hpp" in B.HEADERS
    header = open(os.path.join(B.CSRC, "dfx_pass1_layout.hpp")).read()
    assert "#include <hip" not in header and "__global__" not in header and "__device__" not in header  # host only, free of HIP
    for src in ("dfx_k_partition.hip", "dfx_k_partition_inl.hpp", "dfx_k_partition_ws_inl.hpp", "dfx_kernels.hpp"):
        text = open(os.path.join(B.CSRC, src)).read()
        assert "DFX_PARTITION_MAIN_TU" not in text  # the sizing functions are inline in the one header: no macro to define them once
        assert "size_t partition_ring_bytes(" not in text and "size_t partition_ws_bytes(" not in text
