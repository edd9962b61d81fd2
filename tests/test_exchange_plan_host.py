"""CPU test of the multi-GPU exchange's host arithmetic (csrc/dfx_exchange_plan.hpp): the slab layout, the payload plan every
rank derives from round 1's count matrix (need_more must come out the same on every rank, or the ranks part ways between two
collectives) and the verdict on the peers' state words.  tests/native/exchange_plan_check.cpp holds them against naive
restatements at worlds 1, 2, 3, 8 and 64 (the slab at every world up to 1024), as a stand-alone program: once plain, once
under the host sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "exchange_plan_check.cpp")


def test_exchange_plan_check_program(tmp_path):
    for name, flags in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / f"exchange_plan_check_{name}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.startswith("ok:"), name + ":\n" + r.stdout[-2000:] + r.stderr[-2000:]
