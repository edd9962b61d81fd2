"""Case matrix of ORDER BY / LIMIT: a deterministic generator and a second reference.  No GPU import, no
library import: tests/test_sort_cases_host.py checks this module on the CPU, tests/test_gpu_sort_cases.py binds the device to it.

The operator has no reference behaviour to be identical to, so its order is pinned by TWO restatements of DESIGN.md section 9 that
share no method and are held against each other on every case:
  * tests/oracle.py sort_batches: Python's sorted() over per-row key tuples, one stable sort per key, values from the C oracle's
    expression evaluator;
  * reference_sort() here: numpy only.  Per key the columns (is_null, is_nan, value with NaN -> 0, not signbit) are ranked densely
    (np.lexsort + a change mask; Utf8 through np.unique over `bytes`), the ranks are negated for DESC and ONE np.lexsort over
    (row number, rank of the last key, ..., rank of the first key) gives the permutation.  Key expressions are evaluated by the
    numpy function every Key carries.  No bit images, no sorted(key=...).

The order: stable; NULL larger than every value (last ASC, first DESC); every NaN equal to every other NaN and larger than +inf;
-0.0 < +0.0; integers by value in their own type; false < true; Utf8 byte-wise, a proper prefix first (NUL bytes are bytes); DESC
is the reverse order of DISTINCT keys, equal keys stay in input order.

A family is a function returning a list of Case; FAMILIES maps the names.  Everything is seeded: cases are the same in every
process, and Case.line names family, case and seed.
"""
import numpy as np
import pyarrow as pa
import pyarrow.compute  # noqa: F401

from datafusion_archive_amd.logicalplan import BinaryExpr, Cast, Column, DataType, Literal, Operator, ScalarValue

SEED = 0x50F7

# (DataType, numpy type, arrow type) of the ten numeric types
NUMERIC = [(DataType.Int8, np.int8, pa.int8()), (DataType.Int16, np.int16, pa.int16()), (DataType.Int32, np.int32, pa.int32()),
           (DataType.Int64, np.int64, pa.int64()), (DataType.UInt8, np.uint8, pa.uint8()), (DataType.UInt16, np.uint16, pa.uint16()),
           (DataType.UInt32, np.uint32, pa.uint32()), (DataType.UInt64, np.uint64, pa.uint64()),
           (DataType.Float32, np.float32, pa.float32()), (DataType.Float64, np.float64, pa.float64())]
NP_OF = {dt: t for dt, t, _ in NUMERIC}
SLICE_LO = (1, 7, 63, 65)        # first rows of the sliced batches: value, validity-bit and Utf8 offsets non-zero, not byte-aligned
ROW_EDGES = (1, 2, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768, 32769)
TOPK_TYPES = (DataType.Int8, DataType.UInt64, DataType.Float32, DataType.Float64, DataType.Boolean)
# a resident scan starts at a multiple of 64 rows and rounds its batch length up to one (dfx_table_scan_range_new: slices stay
# byte-aligned in every bitmap), so "odd" is an odd multiple of 64 and batches of 1000 rows arrive as 1024
RESIDENT_BEGIN, RESIDENT_BATCH = 192, 1000

F64_NANS = (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000123)
F32_NANS = (0x7FC00000, 0xFFC00000, 0x7FC00123)


# ---------------------------------------------------------------------------------------------------------------------------
# arrays and batches
# ---------------------------------------------------------------------------------------------------------------------------
def utf8_array(values, mask=None, keep_null_bytes=False):
    """Utf8 array from buffers.  values: bytes per row; mask: True = NULL.  keep_null_bytes: a NULL row keeps its bytes, so its
    slot has a non-empty range (legal Arrow; a reader that forgets the validity sees text there)."""
    n = len(values)
    mask = np.zeros(n, bool) if mask is None else np.asarray(mask, bool)
    kept = [v if (keep_null_bytes or not m) else b"" for v, m in zip(values, mask)]
    offs = np.zeros(n + 1, np.int32)
    if n:
        offs[1:] = np.cumsum([len(v) for v in kept])
    validity = pa.py_buffer(np.packbits(~mask, bitorder="little").tobytes()) if mask.any() else None
    return pa.Array.from_buffers(pa.string(), n, [validity, pa.py_buffer(offs.tobytes()), pa.py_buffer(b"".join(kept))],
                                 null_count=int(mask.sum()))


def _array(values, mask, lo, hi, raw=False):
    m = None if mask is None else np.asarray(mask[lo:hi], bool)
    if m is not None and not m.any():
        m = None  # a batch without nulls has no validity buffer: the nullptr beside a real bitmap
    if isinstance(values, list):
        return utf8_array(values[lo:hi], m, raw)
    return pa.array(values[lo:hi], mask=m)


def build_batches(columns, lens):
    """columns: [(name, values, mask or None[, keep_null_bytes])], values a numpy array or a list of bytes (Utf8); one RecordBatch
    per entry of lens, every array built on its own (offset 0)."""
    out, lo = [], 0
    for n in lens:
        arrays = [_array(c[1], c[2], lo, lo + n, len(c) > 3 and c[3]) for c in columns]
        out.append(pa.RecordBatch.from_arrays(arrays, names=[c[0] for c in columns]))
        lo += n
    assert lo == len(columns[0][1]), (lo, len(columns[0][1]))
    return out


def ragged(rng, n):
    """lengths adding up to n: a leading 0-row batch, 1-row and 0-row batches among uneven ones"""
    lens, left = [0], n
    for step in (1, 0):
        if left > step:
            lens.append(int(rng.integers(1, max(2, left // 3))) if left > 3 else 1)
            left -= lens[-1]
        lens.append(step if left >= step else 0)
        left -= lens[-1]
    if left > 4:
        a = int(rng.integers(1, left))
        lens += [a, 0, left - a]
    else:
        lens.append(left)
    assert sum(lens) == n and min(lens) == 0
    return lens


def sliced(batches, rot=0):
    """the same rows as slices: batch j becomes whole.slice(lo, len) of a longer batch, lo = SLICE_LO[(j + rot) % 4]; the rows
    around the slice are other rows of the input"""
    table = pa.Table.from_batches(batches).combine_chunks()
    total, out, at = table.num_rows, [], 0
    # the rows in front of a slice hold text in every Utf8 column (where such rows exist), so the slice's first offset is not 0
    text = np.ones(total, bool)
    for col in table.columns:
        if col.type == pa.string() and total:
            text &= np.asarray(pa.compute.utf8_length(col.chunk(0)).fill_null(0).to_numpy(zero_copy_only=False)) > 0
    pool = np.nonzero(text)[0] if text.any() else np.arange(max(total, 1), dtype=np.int64)
    for j, b in enumerate(batches):
        n = b.num_rows
        if n == 0 or total == 0:
            out.append(b)
            continue
        lo = SLICE_LO[(j + rot) % len(SLICE_LO)]
        junk = lambda m, salt: pool[(np.arange(m, dtype=np.int64) * 7 + 3 + salt) % len(pool)]  # noqa: E731
        idx = np.concatenate([junk(lo, at), np.arange(at, at + n, dtype=np.int64), junk(3, at + 11)])
        whole = table.take(pa.array(idx)).combine_chunks().to_batches()[0]
        out.append(whole.slice(lo, n))
        at += n
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# keys: an Expr for the library and the oracle, a numpy function for the second reference
# ---------------------------------------------------------------------------------------------------------------------------
class K:
    def __init__(self, expr, fn, dtype=None):
        self.expr, self.fn, self.dtype = expr, fn, dtype  # dtype: DataType of the result where the builder knows it

    def __repr__(self):
        return repr(self.expr)


def kcol(i, dtype=None):
    return K(Column(i), lambda col: col(i), dtype)


def klit_f64(v):
    return K(Literal(ScalarValue.Float64(float(v))), lambda col: (np.full(col.n, float(v)), np.ones(col.n, bool)), DataType.Float64)


def klit_i64(v):
    return K(Literal(ScalarValue.Int64(int(v))), lambda col: (np.full(col.n, int(v), np.int64), np.ones(col.n, bool)), DataType.Int64)


def _rust_as(x, to):
    """numeric `as` of Rust: integers truncate / extend in two's complement, float -> integer saturates with NaN -> 0"""
    t = NP_OF[to]
    with np.errstate(all="ignore"):
        if x.dtype.kind in "iu" or np.dtype(t).kind == "f":
            return x.astype(t)
        info = np.iinfo(t)
        d = x.astype(np.float64)
        out = np.zeros(len(d), t)
        inside = (d > float(info.min)) & (d < float(info.max))  # (float(max) of the 64-bit types is 2^63 / 2^64: >= saturates)
        out[inside] = np.trunc(d[inside]).astype(t)
        out[d <= float(info.min)] = info.min
        out[d >= float(info.max)] = info.max
        return out  # NaN: 0


def kcast(k, to):
    def fn(col):
        v, ok = k.fn(col)
        return _rust_as(v, to), ok
    return K(Cast(k.expr, to), fn, to)


_NP_OP = {Operator.Plus: np.add, Operator.Minus: np.subtract, Operator.Multiply: np.multiply}


def kbin(a, op, b):
    def fn(col):
        (x, xo), (y, yo) = a.fn(col), b.fn(col)
        assert x.dtype == y.dtype, (x.dtype, y.dtype)
        with np.errstate(all="ignore"):
            return _NP_OP[op](x, y), xo & yo  # integers wrap, floats round once in their own type; NULL if either side is
    return K(BinaryExpr(a.expr, op, b.expr), fn, a.dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy reference
# ---------------------------------------------------------------------------------------------------------------------------
def np_values(arr):
    """(values, valid) of an Arrow array: numeric / bool numpy values with NULL slots zeroed, Utf8 as an object array of bytes"""
    valid = np.asarray(arr.is_valid().to_numpy(zero_copy_only=False), bool)
    if arr.type == pa.string():
        vals = np.empty(len(arr), object)
        vals[:] = [b"" if x is None else x for x in arr.cast(pa.binary()).to_pylist()]
        return vals, valid
    if arr.type == pa.bool_():
        return np.asarray(arr.fill_null(False).to_numpy(zero_copy_only=False), bool), valid
    return np.asarray(arr.fill_null(0).to_numpy(zero_copy_only=False)), valid


class _Columns:
    def __init__(self, batches):
        self.table = pa.Table.from_batches(batches).combine_chunks()
        self.n = self.table.num_rows
        self._cache = {}

    def __call__(self, i):
        if i not in self._cache:
            self._cache[i] = np_values(self.table.column(i).chunk(0))
        return self._cache[i]


def dense_rank(vals, valid):
    """rank of every row's key in section 9's ascending order, equal keys equal ranks (int64, 0-based)"""
    n = len(vals)
    isnull = ~np.asarray(valid, bool)
    if vals.dtype == object:                       # Utf8: bytes compare byte-wise, a prefix first
        filled = vals.copy()
        filled[isnull] = b""
        _u, inv = np.unique(filled, return_inverse=True)
        cols = [np.asarray(inv).reshape(n), isnull]
    elif vals.dtype.kind == "f":
        isnan = np.isnan(vals) & ~isnull
        v = np.where(isnan | isnull, vals.dtype.type(0), vals)
        cols = [~np.signbit(v), v, isnan, isnull]  # least significant first: -0.0 == +0.0 as numbers, the sign decides
    else:
        cols = [np.where(isnull, vals.dtype.type(0), vals), isnull]
    order = np.lexsort(cols)
    changed = np.zeros(n, bool)
    for c in cols:
        s = c[order]
        changed[1:] |= s[1:] != s[:-1]
    rank = np.empty(n, np.int64)
    rank[order] = np.cumsum(changed)
    return rank


def reference_order(batches, keys):
    """keys: [(K, asc)].  The permutation: output row i is row order[i] of the concatenated non-empty batches."""
    cols = _Columns([b for b in batches if b.num_rows])
    ranks = []
    for k, asc in keys:
        r = dense_rank(*k.fn(cols))
        ranks.append(r if asc else -r)
    return np.lexsort([np.arange(cols.n, dtype=np.int64)] + ranks[::-1]), cols.table


def reference_sort(batches, keys, limit=None):
    """one sorted RecordBatch (its first `limit` rows), or None for no rows"""
    if not any(b.num_rows for b in batches) or limit == 0:
        return None
    order, table = reference_order(batches, keys)
    if limit is not None:
        order = order[:limit]
    return table.take(pa.array(order, pa.int64())).to_batches()[0]


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
class Data:
    """the rows of one or more cases, built once (cases that share a Data share its reference results)"""

    def __init__(self, name, build):
        self.name, self._build, self._batches = name, build, None

    @property
    def batches(self):
        if self._batches is None:
            self._batches = self._build()
        return self._batches

    @property
    def schema(self):
        return self.batches[0].schema

    @property
    def num_rows(self):
        return sum(b.num_rows for b in self.batches)


class Case:
    def __init__(self, family, name, seed, data, keys, limit=None, source="host", rot=0, tags=()):
        self.family, self.name, self.seed, self.data = family, name, seed, data
        self.key_specs = list(keys)     # [(K, asc)]
        self.limit, self.source, self.rot, self.tags = limit, source, rot, tuple(tags)
        self._fed = None

    @property
    def keys(self):
        """[(Expr, asc)]: what SortRelation and oracle.sort_batches take"""
        return [(k.expr, asc) for k, asc in self.key_specs]

    @property
    def key_text(self):
        return ", ".join("%r %s" % (k, "ASC" if asc else "DESC") for k, asc in self.key_specs)

    @property
    def line(self):
        return "sort_cases %s/%s seed=%#x source=%s limit=%s ORDER BY %s" % (self.family, self.name, self.seed, self.source, self.limit,
                                                                           self.key_text)

    @property
    def schema(self):
        return self.data.schema

    def batches(self):
        """the host batches the operator is fed ("resident": the rows the scan delivers, see table_batches)"""
        if self.source != "sliced":
            return self.data.batches
        if self._fed is None:
            self._fed = sliced(self.data.batches, self.rot)
        return self._fed

    def table_batches(self):
        """"resident": the table's content: RESIDENT_BEGIN other rows, the case's rows, 37 more; scanned with
        scan(RESIDENT_BATCH, RESIDENT_BEGIN, num_rows)"""
        table = pa.Table.from_batches(self.data.batches).combine_chunks()
        n = table.num_rows
        pad = lambda m, salt: table.take(pa.array((np.arange(m, dtype=np.int64) * 5 + salt) % n)).combine_chunks().to_batches()  # noqa: E731
        return pad(RESIDENT_BEGIN, 1) + [b for b in self.data.batches if b.num_rows] + pad(37, 2)

    def selects(self):
        """whether the radix select applies, from the documented rule alone: 1 <= k <= n // 8, k < n, first key not Utf8 and
        without nulls (in the rows the operator sees)"""
        n, k = self.data.num_rows, self.limit
        if k is None or k < 1 or k > n // 8 or k >= n:
            return False
        vals, valid = self.key_specs[0][0].fn(_Columns([b for b in self.batches() if b.num_rows]))
        return vals.dtype != object and bool(valid.all())


def _int_specials(t):
    i = np.iinfo(t)
    return np.array(sorted({i.min, i.min + 1, 0, 1, i.max - 1, i.max} | ({-1} if i.min < 0 else set())), dtype=t)


def _float_specials(t):
    u, nans = (np.uint64, F64_NANS) if t == np.float64 else (np.uint32, F32_NANS)
    f = np.finfo(t)
    plain = np.array([0.0, -0.0, np.inf, -np.inf, f.smallest_subnormal, f.smallest_normal - f.smallest_subnormal, f.smallest_normal,
                      f.max, -f.max, -f.smallest_subnormal, 1.0, np.nextafter(t(1.0), t(2.0)), -1.0, np.nextafter(t(-1.0), t(-2.0))], dtype=t)
    if t == np.float64:  # neighbours in the lowest mantissa bit, far from 1
        plain = np.concatenate([plain, np.array([1e300, np.nextafter(1e300, np.inf), 3.5e-200, np.nextafter(3.5e-200, 1.0)])])
    return np.concatenate([plain, np.array(nans, dtype=u).view(t)])


def _random_values(rng, t, m):
    if np.dtype(t).kind == "f":
        with np.errstate(all="ignore"):
            return (rng.standard_normal(m) * 10.0 ** rng.integers(-30, 30, m)).astype(t)
    i = np.iinfo(t)
    return rng.integers(i.min, i.max, m, dtype=t, endpoint=True)


def _payload(rng, n):
    """row number + Utf8, Boolean and UInt8 columns with nulls of their own"""
    words = [b"", b"a", b"bc", "Zürich".encode(), b"payload-longer-than-8", b"x\x00y"]
    s = [words[int(i)] + str(int(j)).encode() * int(j % 3) for i, j in zip(rng.integers(0, len(words), n), rng.integers(0, 50, n))]
    return [("row", np.arange(n, dtype=np.int64), None), ("s", s, rng.random(n) < 0.2), ("t", rng.random(n) < 0.5, rng.random(n) < 0.2),
            ("u", rng.integers(0, 256, n, dtype=np.uint8), rng.random(n) < 0.2)]


def _typed_key_column(rng, dt, with_nulls):
    """(values, mask, specials): every value at least three times, the specials valid at least once"""
    if dt == DataType.Boolean:
        base, specials = np.array([False, True] * 150), np.array([False, True])
    else:
        t = NP_OF[dt]
        specials = _float_specials(t) if np.dtype(t).kind == "f" else _int_specials(t)
        base = np.concatenate([specials, _random_values(rng, t, 300)])
    copies = 4 if with_nulls else 3  # nulls only in a fourth copy: every value, the specials included, stays valid three times
    perm = rng.permutation(copies * len(base))
    vals = np.tile(base, copies)[perm]
    mask = ((perm >= 3 * len(base)) & (rng.random(len(perm)) < 0.6)) if with_nulls else None
    return vals, mask, specials


def _types_data(seed, dt, with_nulls):
    def build():
        rng = np.random.default_rng([seed, int(dt), int(with_nulls)])
        vals, mask, _s = _typed_key_column(rng, dt, with_nulls)
        n = len(vals)
        a = int(rng.integers(1, n - 2))
        return build_batches([("k", vals, mask)] + _payload(rng, n), [a, 1, n - a - 1])
    return Data("types:%s:%d" % (dt.name, with_nulls), build)


def family_types(seed=SEED):
    """(a) every numeric type and Boolean as the single key, both directions, with and without nulls"""
    out = []
    for dt in [DataType.Boolean] + [d for d, _t, _p in NUMERIC]:
        for with_nulls in (False, True):
            data = _types_data(seed, dt, with_nulls)
            for asc in (True, False):
                out.append(Case("types", "%s-%s-%s" % (dt.name, "asc" if asc else "desc", "nulls" if with_nulls else "dense"), seed, data,
                                [(kcol(0, dt), asc)], tags=("type:" + dt.name,)))
    return out


def _edge_data(seed, n, split):
    def build():
        rng = np.random.default_rng([seed, n])  # the same rows for both splits
        cols = [("k32", rng.integers(-3, 4, n, dtype=np.int32), None),
                ("k64", rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64, endpoint=True), None),
                ("f32", (rng.integers(-40, 40, n) * 0.25).astype(np.float32), rng.random(n) < 0.1),
                ("row", np.arange(n, dtype=np.int64), None)]
        return build_batches(cols, [n] if split == "one" else ragged(np.random.default_rng([seed, n, 1]), n))
    return Data("edges:%d:%s" % (n, split), build)


def family_row_edges(seed=SEED):
    """(b) totals at the tile, block and scan-chunk edges, as one batch and as ragged batches"""
    out = []
    for n in ROW_EDGES:
        for split in ("one", "ragged"):
            data = _edge_data(seed, n, split)
            for c, (name, asc) in enumerate((("i32ties", True), ("i64full", False), ("f32nulls", True))):
                out.append(Case("row_edges", "%d-%s-%s" % (n, split, name), seed, data, [(kcol(c), asc)], tags=("rows:%d" % n, "split:" + split)))
    return out


def _offsets_data(seed):
    def build():
        rng = np.random.default_rng([seed, 0xC])
        n = 2900
        words = [b"", b"k", b"key", b"key-eight", "ключ".encode(), b"key\x00", b"a-much-longer-key-string"]
        s = [words[int(i)] + bytes([97 + int(j)]) * int(j) for i, j in zip(rng.integers(0, len(words), n), rng.integers(0, 4, n))]
        p = [b"p%d" % int(j) for j in rng.integers(0, 500, n)]
        cols = [("b", rng.random(n) < 0.5, None), ("i16", rng.integers(-2 ** 15, 2 ** 15, n).astype(np.int16), rng.random(n) < 0.2),
                ("s", s, None), ("pb", rng.random(n) < 0.5, rng.random(n) < 0.25), ("ps", p, rng.random(n) < 0.25),
                ("row", np.arange(n, dtype=np.int64), None)]
        return build_batches(cols, [1024, 1024, n - 2048])
    return Data("offsets", build)


def family_offsets(seed=SEED):
    """(c) the same rows as built, as slices at odd offsets and from a resident table scanned from row RESIDENT_BEGIN"""
    data = _offsets_data(seed)
    keysets = [("bool", [(kcol(0), True)]), ("i16", [(kcol(1), False)]), ("utf8", [(kcol(2), True)]),
               ("all", [(kcol(0), False), (kcol(1), True), (kcol(2), False)])]
    out = []
    for kname, keys in keysets:
        for source, rot in (("host", 0), ("sliced", 0), ("sliced", 2), ("resident", 0)):
            out.append(Case("offsets", "%s-%s%d" % (kname, source, rot), seed, data, keys, source=source, rot=rot, tags=("keys:" + kname,)))
    return out


def _null_layout_data(seed, where):
    def build():
        rng = np.random.default_rng([seed, 0xD])
        lens = [900, 700, 1, 850]
        n = sum(lens)
        starts = np.cumsum([0] + lens)
        mask = np.zeros(n, bool)
        if where == "all":
            mask[:] = True
        elif where != "none":
            j = {"first": 0, "middle": 1, "last": 3}[where]
            mask[starts[j]:starts[j + 1]] = rng.random(lens[j]) < 0.3
        f = (rng.integers(-300, 300, n) * 0.5)
        cols = [("k", rng.integers(-50, 50, n).astype(np.int64), mask), ("same", np.full(n, -7, np.int32), None),
                ("f64", f, mask if where != "all" else None), ("i32", rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32), mask if where != "all" else None),
                ("i32b", rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32), None),
                ("f32", (rng.integers(-9, 9, n) * 2.0 ** rng.integers(-3, 120, n)).astype(np.float32), mask if where != "all" else None),
                ("f32b", (rng.integers(-9, 9, n) * 2.0 ** rng.integers(-3, 120, n)).astype(np.float32), None)] + _payload(rng, n)
        return build_batches(cols, lens)
    return Data("nulls:" + where, build)


def family_null_layout(seed=SEED):
    """(d) nulls in one batch only, all-null / all-equal / literal keys, one column twice, nullable computed keys"""
    out = []
    for where in ("first", "middle", "last"):
        data = _null_layout_data(seed, where)
        for asc in (True, False):
            out.append(Case("null_layout", "nulls-%s-%s" % (where, "asc" if asc else "desc"), seed, data, [(kcol(0), asc)], tags=("nulls:" + where,)))
        f64, i32, i32b, f32, f32b = kcol(2), kcol(3), kcol(4), kcol(5), kcol(6)
        out.append(Case("null_layout", "cast-f64-i8-" + where, seed, data, [(kcast(f64, DataType.Int8), True)], tags=("computed",)))
        out.append(Case("null_layout", "i32-mul-wraps-" + where, seed, data, [(kbin(i32, Operator.Multiply, i32b), False)], tags=("computed",)))
        out.append(Case("null_layout", "f32-plus-f32-" + where, seed, data, [(kbin(f32, Operator.Plus, f32b), True)], tags=("computed",)))
    data = _null_layout_data(seed, "middle")
    out.append(Case("null_layout", "same-column-twice", seed, data, [(kcol(0), True), (kcol(0), False)], tags=("twice",)))
    for asc in (True, False):
        d = "asc" if asc else "desc"
        out.append(Case("null_layout", "all-null-" + d, seed, _null_layout_data(seed, "all"), [(kcol(0), asc)], tags=("no-pass",)))
        out.append(Case("null_layout", "all-equal-" + d, seed, data, [(kcol(1), asc)], tags=("no-pass",)))
        out.append(Case("null_layout", "literal-f64-" + d, seed, data, [(klit_f64(2.5), asc)], tags=("no-pass",)))
    out.append(Case("null_layout", "literal-i64", seed, data, [(klit_i64(-3), True)], tags=("no-pass",)))
    return out


UTF8_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 24, 25)


def _utf8_words():
    stem = b"abcdefghijklmnopqrstuvwxyz"
    words = [stem[:n] for n in UTF8_LENGTHS]
    words += [stem[:n - 1] + b"~" for n in UTF8_LENGTHS if n]                          # differ in the last byte only
    words += [stem[:8] + b"A", stem[:8] + b"B", stem[:16] + b"A", stem[:16] + b"B", stem[:24] + b"A", stem[:24] + b"B"]  # ... only past a chunk boundary
    words += [b"a", b"a\x00", b"a\x00\x00", b"a\x00b", b"\x00", stem[:8] + b"\x00", stem[:7] + b"\x00"]
    words += ["Zürich".encode(), "zebra".encode(), "éa".encode(), "日本語".encode(), "日本".encode(), "\U0001F600".encode(), "￿".encode()]
    return words


def _utf8_data(seed, kind):
    def build():
        rng = np.random.default_rng([seed, 0xE])
        n, words = 1500, _utf8_words()
        s = [words[int(i)] for i in rng.integers(0, len(words), n)]
        mask = rng.random(n) < 0.12
        if kind == "empty":
            s, mask = [b""] * n, None
        elif kind == "null":
            mask = np.ones(n, bool)  # (the slots still hold the words)
        elif kind == "dense":
            mask = None
        cols = [("s", s, mask, True), ("i8", rng.integers(-2, 3, n).astype(np.int8), None), ("row", np.arange(n, dtype=np.int64), None),
                ("ps", [b"<" + w + b">" for w in s], rng.random(n) < 0.2, True)]
        return build_batches(cols, [600, 0, 1, 899])
    return Data("utf8:" + kind, build)


def family_utf8(seed=SEED):
    """(e) Utf8 keys: chunk-edge lengths, differences past a chunk boundary, NUL bytes, empty / NULL columns, non-ASCII text, NULL
    slots that still hold bytes; first key and second key after an Int8 key"""
    out = []
    for kind in ("nulls", "dense", "empty", "null"):
        data = _utf8_data(seed, kind)
        for asc in (True, False):
            d = "asc" if asc else "desc"
            out.append(Case("utf8", "%s-first-%s" % (kind, d), seed, data, [(kcol(0), asc)], tags=("utf8:" + kind,)))
            out.append(Case("utf8", "%s-second-%s" % (kind, d), seed, data, [(kcol(1), not asc), (kcol(0), asc)], tags=("utf8:" + kind,)))
    out.append(Case("utf8", "nulls-first-asc-sliced", seed, _utf8_data(seed, "nulls"), [(kcol(0), True)], source="sliced", rot=1, tags=("utf8:nulls",)))
    return out


def _ks(n):
    return sorted({k for k in (1, 2, 64, n // 8 - 1, n // 8, n // 8 + 1, n - 1, n, n + 3) if k >= 1})


def _tile_tie_data(seed):
    def build():
        rng = np.random.default_rng([seed, 0xF])
        n = 16384
        k = rng.integers(100, 10000, n).astype(np.int32)
        k[rng.choice(4000, 10, replace=False)] = 5   # the 10 smallest, all in the first tile
        k[4090:4102] = 50                            # ranks 11..22: rank 16 is row 4095, rank 17 is row 4096 -- a 4096-row tile edge between them
        cols = [("k", k, None), ("tie", (np.arange(n) * 7919 % 104729).astype(np.int64), None), ("row", np.arange(n, dtype=np.int64), None)]
        return build_batches(cols, [5000, 1, 11383])
    return Data("topk:tile-tie", build)


def family_topk(seed=SEED):
    """(f) ORDER BY ... LIMIT k: the prefix of the full sort for every k around n // 8 and n"""
    out = []
    for dt in TOPK_TYPES:
        for with_nulls in (False, True):
            data = _types_data(seed, dt, with_nulls)
            for asc in (True, False):
                for k in _ks(data_rows(dt, with_nulls)):
                    out.append(Case("topk", "%s-%s-%s-k%d" % (dt.name, "asc" if asc else "desc", "nulls" if with_nulls else "dense", k), seed, data,
                                    [(kcol(0, dt), asc)], limit=k, tags=("group:types",)))
    for j, n in enumerate(x for x in ROW_EDGES if x >= 2048):
        data = _edge_data(seed, n, "ragged" if j % 2 else "one")
        c, asc = ((0, True), (1, False), (2, True))[j % 3]  # (the Float32 key has nulls: the full sort)
        for k in _ks(n):
            out.append(Case("topk", "rows%d-col%d-k%d" % (n, c, k), seed, data, [(kcol(c), asc)], limit=k, tags=("group:edges",)))
    tie = _tile_tie_data(seed)
    for k in (10, 15, 16, 17, 22, 23, 2048):
        out.append(Case("topk", "tile-tie-k%d" % k, seed, tie, [(kcol(0), True)], limit=k, tags=("group:ties",)))
        out.append(Case("topk", "tile-tie-second-key-k%d" % k, seed, tie, [(kcol(0), True), (kcol(1), False)], limit=k, tags=("group:ties",)))
        out.append(Case("topk", "tile-tie-sliced-k%d" % k, seed, tie, [(kcol(0), True), (kcol(1), True)], limit=k, source="sliced", rot=k % 4,
                        tags=("group:ties",)))
    for dt in (DataType.Boolean, DataType.Float32):
        data = _types_data(seed, dt, False)
        for k in (1, data_rows(dt, False) // 8, data_rows(dt, False) // 8 + 1):
            out.append(Case("topk", "%s-sliced-k%d" % (dt.name, k), seed, data, [(kcol(0, dt), False)], limit=k, source="sliced", rot=3, tags=("group:ties",)))
    return out


def data_rows(dt, with_nulls):
    """rows of a _types_data input (known without building it)"""
    copies = 4 if with_nulls else 3
    if dt == DataType.Boolean:
        return copies * 300
    t = NP_OF[dt]
    return copies * (len(_float_specials(t) if np.dtype(t).kind == "f" else _int_specials(t)) + 300)


def _mix_data(seed, index):
    def build():
        rng = np.random.default_rng([seed, 0x6, index])
        n = int(rng.choice([1, 2, 65, 700, 2049, 4097])) if rng.random() < 0.3 else int(rng.integers(3, 6001))
        cols = []
        for dt in [DataType.Boolean] + [d for d, _t, _p in NUMERIC]:
            vals, _m, _s = _typed_key_column(rng, dt, False)
            narrow = rng.random() < 0.5  # half of the columns draw from a few values: ties for the later keys to break
            pick = rng.integers(0, min(len(vals), 12) if narrow else len(vals), n)
            cols.append((dt.name.lower(), vals[pick], (rng.random(n) < 0.1) if rng.random() < 0.5 else None))
        words = _utf8_words()
        cols.append(("s", [words[int(i)] for i in rng.integers(0, len(words), n)], (rng.random(n) < 0.1) if rng.random() < 0.5 else None, True))
        cols.append(("i32b", rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32), None))
        cols.append(("f32b", _random_values(rng, np.float32, n), None))
        cols.append(("f64b", rng.integers(-8, 8, n) * 0.5, (rng.random(n) < 0.1) if rng.random() < 0.5 else None))
        cols.append(("row", np.arange(n, dtype=np.int64), None))
        lens = [n] if rng.random() < 0.25 else ragged(rng, n)
        return build_batches(cols, lens)
    return Data("mix:%d" % index, build)


MIX_COLUMNS = ["boolean"] + [d.name.lower() for d, _t, _p in NUMERIC] + ["s", "i32b", "f32b", "f64b", "row"]


def _mix_key(rng):
    c = {name: i for i, name in enumerate(MIX_COLUMNS)}
    numeric = [(kcol(c[d.name.lower()], d), d) for d, _t, _p in NUMERIC]
    r = rng.random()
    if r < 0.5:
        return kcol(int(rng.integers(0, c["i32b"])))          # any column, Utf8 and Boolean included
    if r < 0.68:
        k, _d = numeric[int(rng.integers(0, len(numeric)))]
        return kcast(k, NUMERIC[int(rng.integers(0, len(NUMERIC)))][0])
    if r < 0.76:
        return kbin(kcol(c["int32"], DataType.Int32), Operator.Multiply, kcol(c["i32b"], DataType.Int32))
    if r < 0.84:
        return kbin(kcol(c["float32"], DataType.Float32), Operator.Plus, kcol(c["f32b"], DataType.Float32))
    if r < 0.92:
        return kbin(kcol(c["float64"], DataType.Float64), Operator.Minus, kcol(c["f64b"], DataType.Float64))  # inf - inf: a NaN made on the device
    if r < 0.97:
        return kcast(kbin(kcol(c["int32"], DataType.Int32), Operator.Plus, kcol(c["i32b"], DataType.Int32)), DataType.Int16)
    return klit_f64(1.0)


N_MIXES = 150


def family_mixes(seed=SEED):
    """(g) seeded random mixes: 1-4 keys from all column types and small expression trees, random directions, splits, slices, limits"""
    out = []
    for index in range(N_MIXES):
        rng = np.random.default_rng([seed, 0x9, index])
        keys = [(_mix_key(rng), bool(rng.random() < 0.5)) for _ in range(int(rng.integers(1, 5)))]
        source = "sliced" if rng.random() < 0.35 else "host"
        limit = None
        if rng.random() < 0.5:
            limit = int(rng.choice([0, 1, 3, 64, 100, 700, 7000])) if rng.random() < 0.7 else int(rng.integers(1, 6000))
        out.append(Case("mixes", "mix%03d" % index, seed, _mix_data(seed, index), keys, limit=limit, source=source, rot=index % 4))
    return out


def witness_passes(seed=SEED):
    """DESIGN.md section 9's own example: 5000 rows, a non-null Int64 key uniform in [0, 2^20), ASC: digits 0-2 vary (3 passes), digits
    3-6 are 0 and digit 7 is the flipped sign bit (5 skipped)"""
    def build():
        rng = np.random.default_rng([seed, 0x20])
        return build_batches([("k", rng.integers(0, 1 << 20, 5000).astype(np.int64), None), ("row", np.arange(5000, dtype=np.int64), None)], [5000])
    return Case("witness", "int64-below-2^20", seed, Data("witness", build), [(kcol(0), True)])


FAMILIES = {"types": family_types, "row_edges": family_row_edges, "offsets": family_offsets, "null_layout": family_null_layout,
            "utf8": family_utf8, "topk": family_topk, "mixes": family_mixes}


def expected(case, full):
    """the result the operator must give, from the full sort `full` of the case's rows (a RecordBatch or None): one batch, or
    None for no rows / LIMIT 0"""
    if full is None or case.limit == 0:
        return None
    return full if case.limit is None else full.slice(0, min(case.limit, full.num_rows))
