"""CPU test of what the FastPolicy / PlanPolicy kernels read (csrc/dfx_scan_plan.hpp): the terms' ranges and the host's
restatement of PlanPolicy::pass against the comparison operators, bind_scan_plan against the function it was taken apart
from (every refusal, every gen flavour, the key-4 rule through both of its doors), the recogniser against the former one.
tests/native/scan_plan_check.cpp is a stand-alone program: built and run once plain, once under the host sanitizers.  And
the wiring: the header is in the build's lists and free of HIP, and dfx_expr.cpp is split by its jobs."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "scan_plan_check.cpp")


def test_scan_plan_program(tmp_path):
    for name, flags in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / f"scan_plan_check_{name}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.startswith("ok:"), name + ":\n" + r.stdout[-2000:] + r.stderr[-2000:]
        assert int(re.match(r"ok: (\d+) cells \(bind_scan_plan: (\d+) compared", r.stdout).group(2)) >= 100000, r.stdout


def test_scan_plan_is_wired_into_the_build():
    from datafusion_archive_amd import build as B

    assert "dfx_scan_plan.hpp" in B.HEADERS
    # the header is host only: dfx_device.hpp and standard headers, nothing else of the project, nothing of HIP
    text = open(os.path.join(B.CSRC, "dfx_scan_plan.hpp")).read()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["dfx_device.hpp"]
    assert not re.search(r"#include\s+<hip", text)
    for unit in ("dfx_expr.cpp", "dfx_expr_utf8.cpp", "dfx_expr_program.cpp"):
        assert B.SOURCES.count(unit) == 1 and os.path.exists(os.path.join(B.CSRC, unit)), unit
    assert len(B.SOURCES) == len(set(B.SOURCES))


def test_dfx_expr_is_split_by_its_jobs():
    from datafusion_archive_amd import build as B

    text = open(os.path.join(B.CSRC, "dfx_expr.cpp")).read()
    for gone in ("plan_term_range", "fast_terms", "Utf8Terms::"):
        assert gone not in text, gone
    # the planner lives in the header alone: the library's own entry points call it, they do not restate it
    program = open(os.path.join(B.CSRC, "dfx_expr_program.cpp")).read()
    assert '#include "dfx_scan_plan.hpp"' in program
    for name in ("plan_term_passes", "build_fast_plan", "host_plan::bind_scan_plan", "host_plan::scan_plan_shape_ok", "device_ones_block()"):
        assert name in program, name
    assert "img_hi" not in program  # (no copy of PlanPolicy::pass beside the C ABI)
    assert "Utf8Terms::compile" in open(os.path.join(B.CSRC, "dfx_expr_utf8.cpp")).read()
