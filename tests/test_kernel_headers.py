"""CPU test of the device-side headers of the kernel units (csrc/dfx_k_base_inl.hpp, dfx_k_interp_inl.hpp, dfx_k_policy_inl.hpp,
dfx_k_plan_policy_inl.hpp, dfx_k_acc_inl.hpp: one job each, no umbrella): they are in the build's list, the header they came out
of is gone, the kernel units that scan no rows by a policy reach neither the interpreter nor a policy through their includes, the
base header stands on dfx_kernels.hpp alone, and the kernels read a policy's optional flags directly (no detector templates).
That no kernel changed is not tested here: tools/kernel_ab.py compares the device assembly (profiles/r12_kernel_headers_ab.txt)."""
import os
import re

from datafusion_archive_amd import build as B

HEADERS = ["dfx_k_base_inl.hpp", "dfx_k_interp_inl.hpp", "dfx_k_policy_inl.hpp", "dfx_k_plan_policy_inl.hpp", "dfx_k_acc_inl.hpp"]
SMALL_UNITS = ["dfx_k_csv.hip", "dfx_k_csvwrite.hip", "dfx_k_sort.hip", "dfx_k_dict.hip", "dfx_k_utf8pred.hip", "dfx_k_parquet.hip"]
OLD = "dfx_kernels_inl.hpp"


def project_includes(name):
    """the `#include "dfx_..."` lines of one file of csrc/"""
    return re.findall(r'^\s*#\s*include\s+"(dfx_[^"]+)"', open(os.path.join(B.CSRC, name)).read(), re.M)


def reachable(name):
    seen, todo = set(), [name]
    while todo:
        for inc in project_includes(todo.pop()):
            if inc not in seen:
                assert os.path.exists(os.path.join(B.CSRC, inc)), (name, inc)
                seen.add(inc)
                todo.append(inc)
    return seen


def csrc_files():
    return sorted(f for f in os.listdir(B.CSRC) if os.path.isfile(os.path.join(B.CSRC, f)))


def test_the_five_headers_are_in_the_build():
    for h in HEADERS:
        assert h in B.HEADERS and os.path.exists(os.path.join(B.CSRC, h)), h
    assert len(B.HEADERS) == len(set(B.HEADERS))
    for h in B.HEADERS:
        assert os.path.exists(os.path.join(B.CSRC, h)), h


def test_the_old_header_is_gone():
    assert OLD not in B.HEADERS and not os.path.exists(os.path.join(B.CSRC, OLD))
    for f in csrc_files():
        assert OLD not in open(os.path.join(B.CSRC, f), errors="replace").read(), f


def test_small_units_reach_neither_interpreter_nor_policies():
    for unit in SMALL_UNITS:
        assert unit in B.SOURCES, unit
        reached = reachable(unit)
        assert "dfx_k_base_inl.hpp" in reached, unit
        for h in ("dfx_k_interp_inl.hpp", "dfx_k_policy_inl.hpp", "dfx_k_plan_policy_inl.hpp"):
            assert h not in reached, (unit, h)


def test_base_header_stands_on_dfx_kernels_alone():
    assert project_includes("dfx_k_base_inl.hpp") == ["dfx_kernels.hpp"]
    # ... and the layering of the others: each names the header below it
    assert project_includes("dfx_k_interp_inl.hpp") == ["dfx_k_base_inl.hpp"]
    assert project_includes("dfx_k_acc_inl.hpp") == ["dfx_k_base_inl.hpp"]
    assert sorted(project_includes("dfx_k_policy_inl.hpp")) == ["dfx_k_interp_inl.hpp", "dfx_sigs.hpp"]
    assert project_includes("dfx_k_plan_policy_inl.hpp") == ["dfx_k_policy_inl.hpp"]


def test_policy_flag_detectors_are_gone():
    for f in csrc_files():
        text = open(os.path.join(B.CSRC, f), errors="replace").read()
        for gone in ("Row8Of", "RowPairsOf", "KeyPairsOf"):
            assert gone not in text, (f, gone)
    ws = open(os.path.join(B.CSRC, "dfx_k_partition_ws_inl.hpp")).read()
    for flag in ("POL::kRow8", "POL::kRowPairs", "POL::kKeyPairs"):
        assert flag in ws, flag
