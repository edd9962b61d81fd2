"""Builds the HIP extension in-tree: datafusion_archive_amd/lib/libdfx_hip.so (gfx950 only).

hipcc cross-compiles without a GPU.  The built library is git-ignored but travels to the GPU box
with the repo snapshot.  No JIT, no torch extension machinery: a plain C-ABI shared object.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from typing import List

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
OBJDIR = os.path.join(HERE, "build")
LIB = os.path.join(LIBDIR, "libdfx_hip.so")


def _pass1_units() -> List[str]:
    """the pass-1 units of the partitioned GROUP BY: the names in DFX_PASS1_UNITS (csrc/dfx_pass1_units.hpp), one translation unit each"""
    import re
    text = open(os.path.join(CSRC, "dfx_pass1_units.hpp")).read()
    return re.findall(r"\bX\((\w+)\)", re.search(r"#define DFX_PASS1_UNITS\(X\)((?:.*\\\n)*.*)", text).group(1))


# kernel translation units first (slowest): they compile in parallel
SOURCES = ["dfx_k_table1.hip", "dfx_k_table2.hip", "dfx_k_table3.hip", "dfx_k_table4.hip", "dfx_k_table8.hip", "dfx_k_core.hip", "dfx_k_filter.hip",
           "dfx_k_reduce.hip", "dfx_k_pass2.hip", "dfx_k_partition.hip"] + [f"dfx_k_partition_{u}.hip" for u in _pass1_units()] + [
           "dfx_k_fewgroup.hip", "dfx_k_distinct1.hip", "dfx_k_distinct2.hip", "dfx_k_distinct3.hip", "dfx_k_distinct4.hip",
           "dfx_k_distinct8.hip", "dfx_k_csv.hip", "dfx_k_sort.hip", "dfx_k_dict.hip", "dfx_k_utf8pred.hip", "dfx_k_utf8agg.hip", "dfx_k_csvwrite.hip", "dfx_k_parquet.hip", "dfx_k_parquet_write.hip", "dfx_k_parquet_write_dict.hip", "dfx_k_parquet_write_lz4.hip", "dfx_launch.cpp", "dfx_host.cpp", "dfx_expr.cpp", "dfx_expr_program.cpp", "dfx_expr_utf8.cpp", "dfx_relation.cpp", "dfx_host_stream.cpp", "dfx_export.cpp",
           "dfx_filter.cpp", "dfx_project.cpp", "dfx_aggregate.cpp", "dfx_aggregate_strategy.cpp",
           "dfx_aggregate_table.cpp", "dfx_aggregate_ctrl.cpp", "dfx_aggregate_shadow.cpp", "dfx_aggregate_launch.cpp", "dfx_aggregate_emit.cpp", "dfx_aggregate_partial.cpp", "dfx_utf8_dict.cpp",
           "dfx_gather.cpp", "dfx_table.cpp", "dfx_options.cpp", "dfx_csv.cpp", "dfx_sort.cpp", "dfx_comm.cpp", "dfx_exchange.cpp", "dfx_distinct.cpp", "dfx_distinct_sets.cpp", "dfx_distinct_emit.cpp",
           "dfx_csv_write.cpp", "dfx_parquet.cpp", "dfx_parquet_write.cpp"]
HEADERS = ["dfx_device.hpp", "dfx_sigs.hpp", "dfx_row_source.hpp", "dfx_scan_plan.hpp", "dfx_numparse.hpp", "dfx_utf8_match.hpp", "dfx_pow5_table.hpp", "dfx_numfmt.hpp", "dfx_pow10_table.hpp", "dfx_csvwrite.hpp", "dfx_csv_walk.hpp", "dfx_parquet_rle.hpp", "dfx_parquet_lz4.hpp", "dfx_parquet_meta.hpp", "dfx_parquet_thrift_write.hpp", "dfx_parquet_enc.hpp", "dfx_parquet_dict_enc.hpp", "dfx_parquet_lz4_enc.hpp", "dfx_parquet_write.hpp", "dfx_k_parquet_write_inl.hpp", "dfx_scan_rules.hpp", "dfx_kernels.hpp", "dfx_k_base_inl.hpp", "dfx_k_interp_inl.hpp", "dfx_k_policy_inl.hpp", "dfx_k_plan_policy_inl.hpp", "dfx_k_acc_inl.hpp", "dfx_k_table_inl.hpp", "dfx_k_partition_inl.hpp", "dfx_k_partition_ws_inl.hpp", "dfx_k_distinct_inl.hpp", "dfx_launch.hpp",
           "dfx_host.hpp", "dfx_pass1_units.hpp", "dfx_pass1_layout.hpp", "dfx_agg_rules.hpp", "dfx_pass2_forms.hpp", "dfx_key_shadow.hpp", "dfx_value_shadow.hpp", "dfx_routed_shadow.hpp", "dfx_relation.hpp", "dfx_gather.hpp", "dfx_utf8_dict.hpp", "dfx_exchange_plan.hpp", "dfx_comm.hpp", "dfx_aggregate_impl.hpp", "dfx_distinct_impl.hpp", "../../include/dfx.h"]

# -ffp-contract=off : the reference never fuses a*b+c; projections must be bit-exact
# -munsafe-fp-atomics: hardware global_atomic_add_f64 / ds_add_f64 instead of CAS loops
CXXFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
            "-munsafe-fp-atomics", "-Wall", "-Wno-unused-result", "-fno-gpu-rdc"]
CXXFLAGS += os.environ.get("DFX_EXTRA_CXXFLAGS", "").split()  # debug builds


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm for the gfx950 build)")


def _stale(target: str, deps: List[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def _depfile_deps(depfile: str):
    """Prerequisites recorded by the compiler (-MD -MF) the last time this object was built; None if there is no record."""
    try:
        text = open(depfile).read()
    except OSError:
        return None
    text = text.replace("\\\n", " ")
    if ":" not in text:
        return None
    deps = [d for d in text.split(":", 1)[1].split() if d.startswith(HERE) or d.startswith(os.path.dirname(HERE))]
    return deps or None


def _recorded_flags(obj: str) -> str:
    try:
        return open(obj + ".flags").read()
    except OSError:
        return ""


# ---- build-time guard: hand-scheduled registers of pass 2 ------------------------------------------------------------------
# k_partition_agg_lean (csrc/dfx_k_pass2.hip) issues its row loads by inline assembly into VGPRs v88..v119, which the kernel
# withholds from the register allocator (amdgpu_num_vgpr(88)).  That is only sound while (a) the code object ALLOCATES those
# registers (its .vgpr_count covers them: a wave that was given fewer would have its loads land in another wave's registers) and
# (b) nothing the compiler generates touches them.  Round 2 found a silent-corruption bug of exactly this kind on the GPU;
# build() refuses to produce a library that has the next one (tests/test_build_guards.py runs the same check).
GUARD_SRC = "dfx_k_pass2.hip"
RESERVED_VGPRS = range(88, 120)


def _asm_registers(operand_text: str):
    import re
    regs = set()
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]", operand_text):
        regs.update(range(int(m.group(1)), int(m.group(2)) + 1))
    for m in re.finditer(r"\bv(\d+)\b", operand_text):
        regs.add(int(m.group(1)))
    return regs


def check_pass2_reserved_registers(asm: str) -> int:
    """Raises RuntimeError naming the kernel and the instruction; returns the number of instantiations checked."""
    import re
    kernels = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN3dfx\d+k_partition_agg_lean\w*):.*?\n(.*?)\n\s*s_endpgm", asm, re.S | re.M)}
    if len(kernels) < 8:
        raise RuntimeError(f"build guard: expected every k_partition_agg_lean instantiation, found {len(kernels)}")
    meta = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.name:\s+(\S+)\n(?:(?!\.name:).*\n)*?\s+\.vgpr_count:\s+(\d+)", asm)}
    reserved = set(RESERVED_VGPRS)
    for k, body in kernels.items():
        if k not in meta:
            raise RuntimeError(f"build guard: no metadata for {k}")
        # v117 with 8-byte rows (dwordx2 loads: the rows of two shadows), v118 with 12-byte rows (dwordx3), v119 with 16-byte rows
        used = max(_asm_registers(body) & reserved, default=0)
        widths = {int(m.group(1)) for m in re.finditer(r"\bglobal_load_dwordx([234])\s+v\[(?:8[89]|9\d|1[01]\d):", body)}
        if not widths or used < 115 + max(widths):
            raise RuntimeError(f"build guard: {k}: the in-flight row registers v88..v119 are gone")
        if meta[k] <= used:
            raise RuntimeError(f"build guard: {k}: .vgpr_count = {meta[k]} does not cover v{used} (the in-flight row registers v88..v{used}): "
                               "a wave would be allocated fewer registers than the hand-written loads write")
        for line in body.split("\n"):
            ins = line.split(";")[0].strip()
            if not ins or ins.endswith(":") or ins.startswith("."):
                continue
            op, _, rest = ins.partition(" ")
            ops = [o.strip() for o in rest.split(",")]
            if not (_asm_registers(rest) & reserved):
                continue
            if op in ("global_load_dwordx2", "global_load_dwordx3", "global_load_dwordx4"):
                ok = _asm_registers(ops[0]) <= reserved and not (_asm_registers(",".join(ops[1:])) & reserved)
            elif op in ("v_mov_b32", "v_mov_b32_e32"):
                ok = not (_asm_registers(ops[0]) & reserved) and _asm_registers(ops[1]) <= reserved
            else:
                ok = False
            if not ok:
                raise RuntimeError(f"build guard: {k}: compiler-generated instruction touches a reserved register: {ins}")
    return len(kernels)


def pass2_guard_asm(hipcc: str, out_path: str) -> str:
    """device assembly of the pass-2 translation unit, with the flags the library is built with"""
    flags = [f for f in CXXFLAGS if f not in ("-fPIC",)]
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-o", out_path, os.path.join(CSRC, GUARD_SRC)], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("build guard: hipcc -S failed:\n" + r.stderr[-2000:])
    return open(out_path).read()


def build(force: bool = False, verbose: bool = False) -> str:
    os.makedirs(LIBDIR, exist_ok=True)
    os.makedirs(OBJDIR, exist_ok=True)
    hipcc = _hipcc()
    hdrs = [os.path.join(CSRC, h) for h in HEADERS] + [os.path.abspath(__file__)]
    jobs = []
    objs = []
    for src in SOURCES:
        sp = os.path.join(CSRC, src)
        obj = os.path.join(OBJDIR, os.path.splitext(src)[0] + ".o")
        objs.append(obj)
        depfile = obj + ".d"
        recorded = _depfile_deps(depfile)  # exact per-object prerequisites when known, else every header
        deps = ([sp] + recorded + [os.path.abspath(__file__)]) if recorded else ([sp] + hdrs)
        if force or _stale(obj, deps) or os.environ.get("DFX_EXTRA_CXXFLAGS", "") != _recorded_flags(obj):
            cmd = [hipcc] + CXXFLAGS + (["-x", "hip"] if src.endswith(".cpp") else []) + ["-MD", "-MF", depfile, "-c", sp, "-o", obj]
            jobs.append(cmd)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        if "-c" in cmd:  # remember the extra flags this object was built with (a -D switch must rebuild it)
            with open(cmd[-1] + ".flags", "w") as fh:
                fh.write(os.environ.get("DFX_EXTRA_CXXFLAGS", ""))
        return r

    guard_obj = os.path.join(OBJDIR, os.path.splitext(GUARD_SRC)[0] + ".o")
    guard_stamp = guard_obj + ".guard"
    guard_due = any(cmd[-1] == guard_obj for cmd in jobs) or not os.path.exists(guard_stamp) or \
        (os.path.exists(guard_obj) and os.path.getmtime(guard_stamp) < os.path.getmtime(guard_obj))

    def guard(_unused=None):
        n = check_pass2_reserved_registers(pass2_guard_asm(hipcc, os.path.join(OBJDIR, os.path.splitext(GUARD_SRC)[0] + ".guard.s")))
        if verbose:
            print(f"build guard: {n} instantiations of k_partition_agg_lean keep v88..v119 to the hand-written loads", flush=True)

    if jobs or guard_due:
        with ThreadPoolExecutor(max_workers=min(8, len(jobs) + 1)) as ex:
            guard_future = ex.submit(guard) if guard_due else None  # (beside the compile jobs: ~15 s of its own)
            list(ex.map(run, jobs))
            if guard_future is not None:
                guard_future.result()  # raises: no library from a translation unit that fails the guard
        if guard_due:
            with open(guard_stamp, "w") as fh:
                fh.write("ok\n")
    if jobs or force or _stale(LIB, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
