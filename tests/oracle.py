"""ctypes binding of the CPU oracle (oracle/libdfx_oracle.so) -- TEST INFRASTRUCTURE ONLY.

The product package never imports this module.  It converts pyarrow arrays to the oracle's
``orc_array`` views, runs the reference-shaped CPU restatement and converts results back.
"""
from __future__ import annotations

import ctypes
import math
import os
import subprocess
from typing import List, Optional, Sequence

import numpy as np
import pyarrow as pa

from datafusion_archive_amd.logicalplan import DataType, Expr, ExprNode, serialize

_HERE = os.path.dirname(os.path.abspath(__file__))
_ORACLE_DIR = os.path.join(os.path.dirname(_HERE), "oracle")
_LIB_PATH = os.path.join(_ORACLE_DIR, "libdfx_oracle.so")


class OracleError(Exception):
    def __init__(self, code: int, message: str):
        super().__init__(f"[{code}] {message}")
        self.code = code
        self.message = message


class OrcArray(ctypes.Structure):
    _fields_ = [
        ("dtype", ctypes.c_int32),
        ("owned", ctypes.c_int32),
        ("length", ctypes.c_int64),
        ("values", ctypes.c_void_p),
        ("validity", ctypes.c_void_p),
        ("offsets", ctypes.c_void_p),
        ("data", ctypes.c_void_p),
    ]


class OrcBatch(ctypes.Structure):
    _fields_ = [
        ("num_rows", ctypes.c_int64),
        ("num_columns", ctypes.c_int32),
        ("owned", ctypes.c_int32),
        ("columns", ctypes.POINTER(ctypes.POINTER(OrcArray))),
    ]


class SynthColumn(ctypes.Structure):
    _fields_ = [
        ("name", ctypes.c_char_p),
        ("kind", ctypes.c_int32),
        ("column_id", ctypes.c_int32),
        ("p0", ctypes.c_double),
        ("p1", ctypes.c_double),
    ]


def build_oracle() -> str:
    """Compile the oracle if needed (gcc, seconds). Returns the library path.  DFX_ORACLE_SO: use this build instead
    (tests/test_oracle_sanitized.py runs the oracle's own tests over an ASan + UBSan build)."""
    if os.environ.get("DFX_ORACLE_SO"):
        return os.environ["DFX_ORACLE_SO"]
    src = os.path.join(_ORACLE_DIR, "dfx_oracle.c")
    if (not os.path.exists(_LIB_PATH)) or os.path.getmtime(_LIB_PATH) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", _ORACLE_DIR, "-s"])
    return _LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build_oracle())
        _lib.orc_synth_u64.restype = ctypes.c_uint64
        _lib.orc_synth_u64.argtypes = [ctypes.c_uint64, ctypes.c_int32, ctypes.c_int64]
        _lib.orc_synth_fill.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_double,
                                        ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
        _lib.orc_array_free.argtypes = [ctypes.POINTER(OrcArray)]
        _lib.orc_batch_free.argtypes = [ctypes.POINTER(OrcBatch)]
        _lib.orc_agg_free.argtypes = [ctypes.c_void_p]
        _lib.orc_csv_close.argtypes = [ctypes.c_void_p]
        _lib.orc_csv_next.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.POINTER(OrcBatch)), ctypes.c_char_p, ctypes.c_size_t]
    return _lib


_PA_TO_DT = {
    pa.bool_(): DataType.Boolean, pa.int8(): DataType.Int8, pa.int16(): DataType.Int16,
    pa.int32(): DataType.Int32, pa.int64(): DataType.Int64, pa.uint8(): DataType.UInt8,
    pa.uint16(): DataType.UInt16, pa.uint32(): DataType.UInt32, pa.uint64(): DataType.UInt64,
    pa.float32(): DataType.Float32, pa.float64(): DataType.Float64, pa.string(): DataType.Utf8,
}
_DT_TO_PA = {v: k for k, v in _PA_TO_DT.items()}
_DT_TO_NP = {
    DataType.Int8: np.int8, DataType.Int16: np.int16, DataType.Int32: np.int32, DataType.Int64: np.int64,
    DataType.UInt8: np.uint8, DataType.UInt16: np.uint16, DataType.UInt32: np.uint32,
    DataType.UInt64: np.uint64, DataType.Float32: np.float32, DataType.Float64: np.float64,
}


def _normalize(arr: pa.Array) -> pa.Array:
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks()
    if arr.offset != 0:
        arr = pa.concat_arrays([arr])
        if arr.offset != 0:  # pragma: no cover - concat_arrays always rebases
            arr = pa.array(arr.to_pylist(), type=arr.type)
    return arr


class _ArrayView:
    """Keeps the pyarrow buffers alive while the oracle reads them."""

    def __init__(self, arr: pa.Array):
        arr = _normalize(arr)
        self.arr = arr
        self.c = OrcArray()
        self.c.dtype = int(_PA_TO_DT[arr.type])
        self.c.owned = 0
        self.c.length = len(arr)
        bufs = arr.buffers()
        self.c.validity = bufs[0].address if (bufs[0] is not None and arr.null_count > 0) else None
        if arr.type == pa.string():
            self.c.offsets = bufs[1].address
            self.c.data = bufs[2].address if bufs[2] is not None else None
        else:
            self.c.values = bufs[1].address if bufs[1] is not None else None


class _BatchView:
    def __init__(self, batch: pa.RecordBatch):
        self.views = [_ArrayView(batch.column(i)) for i in range(batch.num_columns)]
        self.ptrs = (ctypes.POINTER(OrcArray) * max(1, len(self.views)))(
            *[ctypes.pointer(v.c) for v in self.views])
        self.c = OrcBatch()
        self.c.num_rows = batch.num_rows
        self.c.num_columns = batch.num_columns
        self.c.owned = 0
        self.c.columns = ctypes.cast(self.ptrs, ctypes.POINTER(ctypes.POINTER(OrcArray)))


def _array_to_arrow(a: OrcArray) -> pa.Array:
    n = a.length
    dt = DataType(a.dtype)
    validity = None
    null_count = 0
    if a.validity:
        raw = ctypes.string_at(a.validity, (n + 7) // 8)
        validity = pa.py_buffer(raw)
        bits = np.unpackbits(np.frombuffer(raw, dtype=np.uint8), bitorder="little")[:n]
        null_count = int(n - bits.sum())
    if dt == DataType.Utf8:
        offs = ctypes.string_at(a.offsets, 4 * (n + 1))
        nbytes = int(np.frombuffer(offs, dtype=np.int32)[-1]) if n >= 0 else 0
        data = ctypes.string_at(a.data, nbytes) if (a.data and nbytes) else b""
        return pa.Array.from_buffers(pa.string(), n, [validity, pa.py_buffer(offs), pa.py_buffer(data)],
                                     null_count=null_count)
    if dt == DataType.Boolean:
        vals = ctypes.string_at(a.values, (n + 7) // 8)
        return pa.Array.from_buffers(pa.bool_(), n, [validity, pa.py_buffer(vals)], null_count=null_count)
    width = np.dtype(_DT_TO_NP[dt]).itemsize
    vals = ctypes.string_at(a.values, width * n) if n else b""
    return pa.Array.from_buffers(_DT_TO_PA[dt], n, [validity, pa.py_buffer(vals)], null_count=null_count)


def _batch_to_arrow(bp, names: Optional[Sequence[str]] = None) -> pa.RecordBatch:
    b = bp.contents
    cols = [_array_to_arrow(b.columns[i].contents) for i in range(b.num_columns)]
    if names is None:
        names = [f"c{i}" for i in range(len(cols))]
    return pa.RecordBatch.from_arrays(cols, names=list(names))


def _check(code: int, err) -> None:
    if code != 0:
        raise OracleError(code, err.value.decode(errors="replace"))


def eval_expr(expr: Expr, batch: pa.RecordBatch) -> pa.Array:
    """compile_scalar_expr(expr)(batch) on the CPU oracle."""
    s = serialize([expr])
    bv = _BatchView(batch)
    out = ctypes.POINTER(OrcArray)()
    err = ctypes.create_string_buffer(512)
    code = lib().orc_eval(s.nodes, s.n_nodes, s.roots[0], ctypes.byref(bv.c), ctypes.byref(out), err, 512)
    _check(code, err)
    try:
        return _array_to_arrow(out.contents)
    finally:
        lib().orc_array_free(out)


def filter_next(expr: Expr, batch: pa.RecordBatch) -> pa.RecordBatch:
    """FilterRelation::next for one input batch."""
    s = serialize([expr])
    bv = _BatchView(batch)
    out = ctypes.POINTER(OrcBatch)()
    err = ctypes.create_string_buffer(512)
    code = lib().orc_filter_next(s.nodes, s.n_nodes, s.roots[0], ctypes.byref(bv.c), ctypes.byref(out), err, 512)
    _check(code, err)
    try:
        return _batch_to_arrow(out, batch.schema.names)
    finally:
        lib().orc_batch_free(out)


def project_next(exprs: Sequence[Expr], batch: pa.RecordBatch) -> pa.RecordBatch:
    """ProjectRelation::next for one input batch."""
    s = serialize(list(exprs))
    roots = (ctypes.c_int32 * len(s.roots))(*s.roots)
    bv = _BatchView(batch)
    out = ctypes.POINTER(OrcBatch)()
    err = ctypes.create_string_buffer(512)
    code = lib().orc_project_next(s.nodes, s.n_nodes, roots, len(s.roots), ctypes.byref(bv.c),
                                  ctypes.byref(out), err, 512)
    _check(code, err)
    try:
        return _batch_to_arrow(out)
    finally:
        lib().orc_batch_free(out)


def aggregate(group_exprs: Sequence[Expr], aggr_exprs: Sequence[Expr],
              batches: Sequence[pa.RecordBatch]) -> pa.RecordBatch:
    """AggregateRelation over a sequence of input batches (one output batch)."""
    s = serialize(list(group_exprs) + list(aggr_exprs))
    ng, na = len(group_exprs), len(aggr_exprs)
    groots = (ctypes.c_int32 * max(1, ng))(*s.roots[:ng])
    aroots = (ctypes.c_int32 * max(1, na))(*s.roots[ng:])
    agg = ctypes.c_void_p()
    err = ctypes.create_string_buffer(512)
    code = lib().orc_agg_new(s.nodes, s.n_nodes, groots, ng, aroots, na, ctypes.byref(agg), err, 512)
    _check(code, err)
    try:
        for b in batches:
            bv = _BatchView(b)
            code = lib().orc_agg_push(agg, ctypes.byref(bv.c), err, 512)
            _check(code, err)
        out = ctypes.POINTER(OrcBatch)()
        code = lib().orc_agg_finish(agg, ctypes.byref(out), err, 512)
        _check(code, err)
        try:
            return _batch_to_arrow(out)
        finally:
            lib().orc_batch_free(out)
    finally:
        lib().orc_agg_free(agg)


# ---------------------------------------------------------------------------------------------
# synthetic data (definition shared with the device generator)
# ---------------------------------------------------------------------------------------------
SYNTH_F64_UNIFORM, SYNTH_F64_EXACT, SYNTH_I64_UNIFORM, SYNTH_I64_ZIPF, SYNTH_I32_UNIFORM, SYNTH_I64_WIDE = 0, 1, 2, 3, 4, 5


def synth_column(kind: int, column_id: int, p0: float, p1: float, seed: int, row_begin: int, n: int) -> np.ndarray:
    kind &= 0xFF
    out = np.empty(n, dtype=np.int64 if kind in (SYNTH_I64_UNIFORM, SYNTH_I64_ZIPF, SYNTH_I64_WIDE) else np.int32 if kind == SYNTH_I32_UNIFORM else np.float64)
    code = lib().orc_synth_fill(kind, column_id, p0, p1, seed, row_begin, n, out.ctypes.data_as(ctypes.c_void_p))
    if code != 0:
        raise OracleError(code, "orc_synth_fill")
    return out


def synth_validity(kind: int, column_id: int, seed: int, row_begin: int, n: int):
    """Boolean numpy array (True = valid) of a synthetic column with nulls (kind | permille << 8), or None"""
    permille = (kind >> 8) & 0x3FF
    if permille == 0:
        return None
    bits = np.zeros((n + 7) // 8, dtype=np.uint8)
    L = lib()
    L.orc_synth_validity.restype = ctypes.c_int64
    L.orc_synth_validity.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    L.orc_synth_validity(column_id, permille, seed, row_begin, n, bits.ctypes.data_as(ctypes.c_void_p))
    return np.unpackbits(bits, bitorder="little")[:n].astype(bool)


def synth_batch(cols: Sequence[tuple], seed: int, row_begin: int, n: int) -> pa.RecordBatch:
    """cols: (name, kind, column_id, p0, p1)."""
    arrays = []
    for (_, k, cid, p0, p1) in cols:
        v = synth_column(k, cid, p0, p1, seed, row_begin, n)
        valid = synth_validity(k, cid, seed, row_begin, n)
        arrays.append(pa.array(v) if valid is None else pa.array(v, mask=~valid))
    return pa.RecordBatch.from_arrays(arrays, names=[c[0] for c in cols])


def run_synth_query(cols: Sequence[tuple], seed: int, row_begin: int, n_rows: int, batch_rows: int,
                    filter_expr: Optional[Expr], group_exprs: Sequence[Expr], aggr_exprs: Sequence[Expr],
                    mask_only: bool = False, want_result: bool = True):
    """Reference-shaped CPU baseline over generated batches. Returns (seconds, kept_rows, result batch)."""
    exprs: List[Expr] = ([filter_expr] if filter_expr is not None else []) + list(group_exprs) + list(aggr_exprs)
    s = serialize(exprs)
    off = 1 if filter_expr is not None else 0
    ng, na = len(group_exprs), len(aggr_exprs)
    groots = (ctypes.c_int32 * max(1, ng))(*s.roots[off:off + ng])
    aroots = (ctypes.c_int32 * max(1, na))(*s.roots[off + ng:])
    names = [c[0].encode() for c in cols]
    carr = (SynthColumn * len(cols))()
    for i, (_, k, cid, p0, p1) in enumerate(cols):
        carr[i].name = names[i]
        carr[i].kind, carr[i].column_id, carr[i].p0, carr[i].p1 = k, cid, p0, p1
    secs = ctypes.c_double()
    kept = ctypes.c_int64()
    out = ctypes.POINTER(OrcBatch)()
    err = ctypes.create_string_buffer(512)
    code = lib().orc_run_synth_query(
        carr, len(cols), ctypes.c_uint64(seed), ctypes.c_int64(row_begin), ctypes.c_int64(n_rows),
        ctypes.c_int64(batch_rows), s.nodes, s.n_nodes, s.roots[0] if filter_expr is not None else -1,
        groots, ng, aroots, na, 1 if mask_only else 0, ctypes.byref(secs),
        ctypes.byref(out) if want_result else None, ctypes.byref(kept), err, 512)
    _check(code, err)
    res = None
    if want_result and out:
        try:
            res = _batch_to_arrow(out)
        finally:
            lib().orc_batch_free(out)
    return secs.value, kept.value, res


def run_synth_filter(cols: Sequence[tuple], seed: int, row_begin: int, n_rows: int, batch_rows: int, filter_expr: Expr,
                     want_columns: Sequence[int] = (0,), want_mask: bool = True):
    """FilterRelation reference-shaped (batch_rows-row batches through orc_filter_next) over generated batches.
    Returns (seconds, kept, {column index: compacted values as numpy}, mask bits as numpy uint8 or None)."""
    s = serialize([filter_expr])
    names = [c[0].encode() for c in cols]
    carr = (SynthColumn * len(cols))()
    for i, (_, k, cid, p0, p1) in enumerate(cols):
        carr[i].name = names[i]
        carr[i].kind, carr[i].column_id, carr[i].p0, carr[i].p1 = k, cid, p0, p1
    outs = {}
    ptrs = (ctypes.c_void_p * len(cols))()
    for c in want_columns:
        k = cols[c][1]
        outs[c] = np.empty(n_rows, dtype=np.int64 if k in (SYNTH_I64_UNIFORM, SYNTH_I64_ZIPF) else np.float64)
        ptrs[c] = outs[c].ctypes.data
    mask = np.empty((n_rows + 7) // 8, dtype=np.uint8) if want_mask else None
    secs = ctypes.c_double()
    kept = ctypes.c_int64()
    err = ctypes.create_string_buffer(512)
    L = lib()
    L.orc_run_synth_filter.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                       ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double), ctypes.c_char_p, ctypes.c_size_t]
    code = L.orc_run_synth_filter(ctypes.cast(carr, ctypes.c_void_p), len(cols), seed, row_begin, n_rows, batch_rows,
                                  ctypes.cast(s.nodes, ctypes.c_void_p), s.n_nodes, s.roots[0], ctypes.cast(ptrs, ctypes.c_void_p),
                                  mask.ctypes.data if mask is not None else None, ctypes.byref(kept), ctypes.byref(secs), err, 512)
    _check(code, err)
    return secs.value, kept.value, {c: v[:kept.value] for c, v in outs.items()}, mask


def read_csv(filename: str, schema: pa.Schema, batch_size: int = 1024) -> List[pa.RecordBatch]:
    """CsvDataSource::new(filename, schema, batch_size) drained (datasource.rs:33-58): every batch next() yields."""
    dts = (ctypes.c_int32 * len(schema))(*[int(_PA_TO_DT[f.type]) for f in schema])
    h = ctypes.c_void_p()
    err = ctypes.create_string_buffer(512)
    L = lib()
    _check(L.orc_csv_open(os.fsencode(filename), dts, len(schema), ctypes.c_int64(batch_size), ctypes.byref(h), err, 512), err)
    out: List[pa.RecordBatch] = []
    try:
        while True:
            bp = ctypes.POINTER(OrcBatch)()
            _check(L.orc_csv_next(h, ctypes.byref(bp), err, 512), err)
            if not bp:
                break
            try:
                out.append(_batch_to_arrow(bp, schema.names))
            finally:
                L.orc_batch_free(bp)
    finally:
        L.orc_csv_close(h)
    return out


# ---------------------------------------------------------------------------------------------------
# ORDER BY / LIMIT (LogicalPlan::Sort / Limit, logicalplan.rs:313-338).  The reference's executor has neither
# (context.rs:113,194: unimplemented!()), so this restates the SEMANTICS THE LIBRARY DEFINES,
# independently and naively (pure Python, small inputs only): stable; NULL larger than every value; every NaN equal and
# larger than every number; -0.0 < +0.0; one result batch.  No reference behaviour pins it; a second restatement of
# another construction does (tests/sort_cases.py reference_sort, compared on the CPU by tests/test_sort_cases_host.py).
# ---------------------------------------------------------------------------------------------------
def sort_order(batches: Sequence[pa.RecordBatch], keys: Sequence[tuple]) -> List[int]:
    """The permutation behind sort_batches: output row i is row order[i] of the concatenated non-empty batches."""
    batches = [b for b in batches if b.num_rows]
    key_cols = []
    for e, _asc in keys:
        key_cols.append(pa.concat_arrays([eval_expr(e, b) for b in batches]).to_pylist())
    order = list(range(sum(b.num_rows for b in batches)))
    for (_e, asc), col in reversed(list(zip(keys, key_cols))):  # least significant key first, stable sorts
        def rank(i, col=col):
            v = col[i]
            if v is None:
                return (1, 0, 0, 0)
            if isinstance(v, float):
                if v != v:
                    return (0, 1, 0, 0)  # every NaN, whatever its sign or payload
                return (0, 0, v, math.copysign(1.0, v))  # Python's -0.0 == 0.0: the sign orders the two zeros, -0.0 first
            return (0, 0, v, 0)
        order = sorted(order, key=rank, reverse=not asc)  # reverse=True keeps the input order of equal elements
    return order


def sort_batches(batches: Sequence[pa.RecordBatch], keys: Sequence[tuple]) -> Optional[pa.RecordBatch]:
    """keys: [(Expr, asc)] -- the inner expressions of Expr::Sort, evaluated with the oracle's own evaluator.
    The order is DESIGN.md section 9's, signed zeros included (-0.0 < +0.0).  tests/sort_cases.py holds a second reference
    of another construction (numpy ranks + lexsort) and tests/test_sort_cases_host.py holds the two against each other,
    bit for bit, on every case the device is later checked with."""
    batches = [b for b in batches if b.num_rows]
    if not batches:
        return None
    table = pa.Table.from_batches(batches).combine_chunks()
    order = sort_order(batches, keys)
    return table.take(pa.array(order, pa.int64())).to_batches()[0] if table.num_rows else None


def limit_batches(batches: Sequence[pa.RecordBatch], limit: int) -> List[pa.RecordBatch]:
    out, left = [], limit
    for b in batches:
        if left <= 0:
            break
        out.append(b.slice(0, min(left, b.num_rows)))
        left -= out[-1].num_rows
    return out


# ---------------------------------------------------------------------------------------------
# exact ("truth") group sums of doubles, and the tolerance every Float64 SUM is held to
# ---------------------------------------------------------------------------------------------
class ExactGroupSums:
    """Correctly rounded EXACT per-group sums of non-negative doubles, accumulated slice by slice in integer arithmetic.

    Every value must be a multiple of 2^-scale and below 2^(78 - scale) (the synthetic columns are: uniform doubles on a
    2^-53 grid, products of bounded factors).  v * 2^scale is split into four 26-bit limbs; numpy.bincount adds a limb of
    every row to its group in float64 -- exact while a sum stays below 2^53, i.e. for fewer than 2^27 rows per group --
    and the limbs are recombined as Python integers at the end: truth = round_to_nearest(sum / 2^scale), one rounding."""

    def __init__(self, n_groups: int, scale: int = 53):
        self.n_groups, self.scale = int(n_groups), int(scale)
        self.limbs = [np.zeros(self.n_groups, dtype=np.float64) for _ in range(4)]
        self.count = np.zeros(self.n_groups, dtype=np.int64)

    def add(self, group_ids: np.ndarray, values: np.ndarray) -> None:
        g = np.asarray(group_ids, dtype=np.int64)
        v = np.asarray(values, dtype=np.float64)
        if v.size == 0:
            return
        assert np.all(v >= 0.0) and np.all(np.isfinite(v)), "ExactGroupSums: non-negative finite values only"
        m, e = np.frexp(v)                      # v = m * 2^e, m in [0.5, 1) (0 for v == 0)
        big = (m * 9007199254740992.0).astype(np.int64)   # 53-bit integer mantissa, exact
        shift = e.astype(np.int64) - 53 + self.scale        # v * 2^scale = big << shift
        shift = np.where(big == 0, 0, shift)
        assert shift.max() <= 25, f"ExactGroupSums: value above the fixed-point window (shift {shift.max()})"
        down = np.maximum(-shift, 0)             # small values: the mantissa's low bits must be zeros (a multiple of 2^-scale)
        assert down.max() <= 62 and np.all((big & ((np.int64(1) << down) - 1)) == 0), "ExactGroupSums: a value is not a multiple of 2^-scale"
        big = big >> down
        up = np.maximum(shift, 0)
        hi, lo = big >> 26, big & ((1 << 26) - 1)
        a, b = hi << up, lo << up                # value * 2^scale = a * 2^26 + b, both below 2^52
        for k, part in enumerate((b & ((1 << 26) - 1), b >> 26, a & ((1 << 26) - 1), a >> 26)):
            self.limbs[k] += np.bincount(g, weights=part.astype(np.float64), minlength=self.n_groups)
        self.count += np.bincount(g, minlength=self.n_groups)
        assert self.count.max() < (1 << 27), "ExactGroupSums: too many rows in one group for exact float64 limb sums"

    def result(self) -> np.ndarray:
        """float64 array: the correctly rounded exact sum of every group"""
        l0, l1, l2, l3 = (x.astype(np.int64) for x in self.limbs)
        out = np.empty(self.n_groups, dtype=np.float64)
        den = 1 << self.scale
        for i in range(self.n_groups):
            total = int(l0[i]) + (int(l1[i]) << 26) + (int(l2[i]) << 26) + (int(l3[i]) << 52)
            out[i] = total / den  # int / int true division: correctly rounded
        return out


# the working bound of check_float_sums in units of sqrt(n) ULP.  Round 4: 64 (150 x the worst distance observed).  Round 5: 8 --
# still 7 x the largest distance seen over 10^6 groups of ~270 rows (19 ULP = 1.16 sqrt(n)) and 17 x the 0.46 sqrt(n) of groups
# of 1.6 x 10^7 rows, and tight enough that a single lost row of a 10^7-row group of uniform doubles is 20 000 x outside it
WORKING_SQRT_N_ULP = 8.0


def exact_sums_q1(cols: Sequence[tuple], seed: int, row_begin: int, n_rows: int, step: int = 1 << 23):
    """Correctly rounded EXACT sums of the four aggregates of BASELINE config 5's query (SUM(qty), SUM(price), SUM(price * (1 - disc)),
    SUM(price * (1 - disc) * (1 + tax)) WHERE ship <= 2436 AND disc >= 0 GROUP BY rf, ls) over rows [row_begin, row_begin + n_rows) of
    the synthetic columns `cols` (rf, ls, qty, price, disc, tax, ship): the arguments are computed as the reference computes them (one
    IEEE rounding per operator, numpy), then added in integer arithmetic (ExactGroupSums).  Returns (four arrays indexed by
    rf * 2 + ls, the rows per group)."""
    accs = [ExactGroupSums(6, scale=52) for _ in range(4)]
    for r0 in range(0, n_rows, step):
        m = min(step, n_rows - r0)
        c = [synth_column(k_, cid, p0, p1, seed, row_begin + r0, m) for (_n, k_, cid, p0, p1) in cols]
        rf, ls, qty, price, disc, tax, ship = c
        keep = (ship <= 2436.0) & (disc >= 0.0)
        g = (rf * 2 + ls)[keep]
        dp = price * (1.0 - disc)
        for a_, arg in zip(accs, (qty, price, dp, dp * (1.0 + tax))):
            a_.add(g, arg[keep])
    return [a_.result() for a_ in accs], accs[0].count.copy()


def check_float_sums(got: np.ndarray, ref: np.ndarray, n: np.ndarray, abs_sum: np.ndarray, truth: Optional[np.ndarray] = None, what: str = "") -> dict:
    """The tolerance a Float64 SUM of the product is held to, per group of n rows:
      proven     |got - ref| <= n * eps * sum|v|      both are sums of the same n terms in different orders (eps = 2^-52);
      working    |got - ref| <= 8 * sqrt(n) ULP(ref)  rounding errors of a sequential sum behave like a random walk: the
                 reference's own distance from the exact sum is ~0.3 sqrt(n) ULP, the product's (tree / per-lane partial
                 sums) far smaller.  8 sqrt(n) (WORKING_SQRT_N_ULP) is 7 - 17 x what is observed and n / (8 sqrt(n)) tighter
                 than the proven bound;
      vs truth   |got - truth| <= (sqrt(n) + 8) ULP   when the exact sums are known (ExactGroupSums): the product must not be
                 further from the exact sum than a sequential sum typically is.
    Raises AssertionError naming the first offending group; returns the observed maxima (in ULP and in sqrt(n) units)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)
    eps = 2.0 ** -52
    err = np.abs(got - ref)
    ulp = np.spacing(np.abs(ref))
    proven = n * eps * np.asarray(abs_sum, dtype=np.float64)
    bad = np.nonzero(err > proven)[0]
    assert bad.size == 0, f"{what}: {bad.size} groups outside n * eps * sum|v|, e.g. group {bad[0]}: got {got[bad[0]]!r} reference {ref[bad[0]]!r}"
    emp = WORKING_SQRT_N_ULP * np.sqrt(n) * ulp
    bad = np.nonzero(err > emp)[0]
    assert bad.size == 0, (f"{what}: {bad.size} groups further than {WORKING_SQRT_N_ULP:g} sqrt(n) ULP from the reference's sum, e.g. group {bad[0]} ({int(n[bad[0]])} rows): "
                           f"got {got[bad[0]]!r} reference {ref[bad[0]]!r} = {err[bad[0]] / ulp[bad[0]]:.0f} ULP")
    out = {"max_ulp_vs_reference": float((err / ulp).max()) if err.size else 0.0,
           "max_over_sqrt_n": float((err / ulp / np.sqrt(np.maximum(n, 1.0))).max()) if err.size else 0.0}
    if truth is not None:
        truth = np.asarray(truth, dtype=np.float64)
        tulp = np.spacing(np.abs(truth))
        terr = np.abs(got - truth)
        bad = np.nonzero(terr > (np.sqrt(n) + 8.0) * tulp)[0]
        assert bad.size == 0, (f"{what}: {bad.size} groups further than (sqrt(n) + 8) ULP from the EXACT sum, e.g. group {bad[0]} ({int(n[bad[0]])} rows): "
                               f"got {got[bad[0]]!r} exact {truth[bad[0]]!r} = {terr[bad[0]] / tulp[bad[0]]:.0f} ULP")
        out["max_ulp_vs_exact"] = float((terr / tulp).max()) if terr.size else 0.0
        out["reference_max_ulp_vs_exact"] = float((np.abs(ref - truth) / tulp).max()) if terr.size else 0.0
    return out
