"""Scan plans (csrc/dfx_device.hpp: DevScanPlan) on the host: every `column <op> literal` term is planned as an unsigned
range test on an order-preserving 64-bit image of the value.  `dfx_debug_plan_term` runs the planner and the kernels'
arithmetic on the host; here it is compared with the comparison it restates (arrow 0.12 array_ops over the reference's
`comparison_ops!`, expression.rs:171-210) for every operator over NaN, +-0.0, +-inf, subnormals and the integer extremes.
No GPU needed."""
import itertools
import struct

import numpy as np
import pytest

from datafusion_archive_amd import _ffi

DT = {"i32": 4, "i64": 5, "u32": 8, "u64": 9, "f32": 10, "f64": 11}  # dfx_dtype
OPS = ["eq", "ne", "lt", "le", "gt", "ge"]  # dfx_operator 0..5


def canon(kind, v):
    """canonical 64-bit form of a value of the column's type (signed: sign-extended, Float32: bits in the low word)"""
    if kind in ("i32", "i64"):
        return int(v) & 0xFFFFFFFFFFFFFFFF
    if kind in ("u32", "u64"):
        return int(v)
    if kind == "f32":
        return struct.unpack("<I", struct.pack("<f", v))[0]
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def expect(op, a, b):
    with np.errstate(invalid="ignore"):
        return bool({"eq": a == b, "ne": a != b, "lt": a < b, "le": a <= b, "gt": a > b, "ge": a >= b}[op])


F64 = [float("nan"), -float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308,
       1.0, -1.0, 1.0000000000000002, 0.9999999999999999, 204.8, 409.6, 1.7976931348623157e308, -1.7976931348623157e308, 3.5, -3.5]
F32 = [float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 1e-45, -1e-45, 1.0, -1.0, 1.0000001, 3.4028235e38, -3.4028235e38, 16777216.0]
I64 = [0, 1, -1, 2, -2, 2**63 - 1, -(2**63), 2**63 - 2, -(2**63) + 1, 2**31, -(2**31), 2**32, 12345, -12345]
I32 = [0, 1, -1, 2**31 - 1, -(2**31), 2**31 - 2, -(2**31) + 1, 65536, -65536, 7]
U64 = [0, 1, 2, 2**63, 2**63 - 1, 2**64 - 1, 2**64 - 2, 2**32, 2**32 - 1]
U32 = [0, 1, 2, 2**31, 2**31 - 1, 2**32 - 1, 2**32 - 2]
VALUES = {"f64": F64, "f32": F32, "i64": I64, "i32": I32, "u64": U64, "u32": U32}
NP = {"f64": np.float64, "f32": np.float32, "i64": np.int64, "i32": np.int32, "u64": np.uint64, "u32": np.uint32}


@pytest.mark.parametrize("kind", list(VALUES))
def test_plan_terms_restate_the_comparison_operators(kind):
    L = _ffi.lib()
    t = NP[kind]
    for lit, val in itertools.product(VALUES[kind], VALUES[kind]):
        for oi, op in enumerate(OPS):
            got = L.dfx_debug_plan_term(DT[kind], oi, canon(kind, lit), canon(kind, val), 0)
            want = expect(op, t(val), t(lit))
            assert got == int(want), f"{kind}: {val!r} {op} {lit!r}: plan {got}, comparison {want}"


def test_plan_terms_on_random_doubles_and_integers():
    L = _ffi.lib()
    rng = np.random.default_rng(20260925)
    bits = rng.integers(0, 2**64, 4000, dtype=np.uint64)
    d = bits.view(np.float64)
    i = bits.view(np.int64)
    for a, b in zip(range(0, 4000, 2), range(1, 4000, 2)):
        for oi, op in enumerate(OPS):
            assert L.dfx_debug_plan_term(DT["f64"], oi, int(bits[b]), int(bits[a]), 0) == int(expect(op, d[a], d[b]))
            assert L.dfx_debug_plan_term(DT["i64"], oi, int(bits[b]), int(bits[a]), 0) == int(expect(op, i[a], i[b]))
            assert L.dfx_debug_plan_term(DT["u64"], oi, int(bits[b]), int(bits[a]), 0) == int(expect(op, bits[a], bits[b]))


def test_plan_terms_null_values_follow_arrow_0_12():
    """bool_op compares Option<T>: None sorts below every value and the result is never null (oracle/dfx_oracle.c
    compare_arrays; the device interpreter's table in dfx_k_interp_inl.hpp): null == x false, != true, < true, <= true,
    > false, >= false -- whatever the literal."""
    L = _ffi.lib()
    want = {"eq": 0, "ne": 1, "lt": 1, "le": 1, "gt": 0, "ge": 0}
    for kind in VALUES:
        for lit in VALUES[kind]:
            for oi, op in enumerate(OPS):
                assert L.dfx_debug_plan_term(DT[kind], oi, canon(kind, lit), 0, 1) == want[op]


def test_plan_terms_reject_types_the_plans_do_not_cover():
    L = _ffi.lib()
    for dt in (1, 2, 3, 6, 7, 12):  # Boolean, Int8, Int16, UInt8, UInt16, Utf8
        assert L.dfx_debug_plan_term(dt, 0, 0, 0, 0) == -1
