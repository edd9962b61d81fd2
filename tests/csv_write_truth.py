"""The CSV writer's format (deviation D11) restated in Python, independent of csrc/dfx_numfmt.hpp: `repr` (Float64) and
numpy's unique scientific formatting (Float32) supply the shortest digits and the exponent, this module lays them out by the
D11 rule and builds whole files from Arrow batches.  Shared by tests/test_csv_write_host.py and tests/test_gpu_csv_write.py."""
import math
import struct

import numpy as np
import pyarrow as pa

SPECIAL_BYTES = b',"\r\n'


def _digits_exp(text):
    """'1.5e-05' / '123.25' / '1.e+16' -> ('15', -6) / ('12325', -2) / ('1', 16): significant digits and the power of ten of the last"""
    mant, _, e = text.partition("e")
    ip, _, fp = mant.partition(".")
    digs, exp10 = ip + fp, (int(e) if e else 0) - len(fp)
    digs = digs.lstrip("0")
    stripped = digs.rstrip("0")
    return stripped, exp10 + len(digs) - len(stripped)


def layout(neg, digs, exp10):
    """Rust's {:?}: positional with at least one digit after the point for 1e-4 <= |x| < 1e16, else d[.ddd]e[-]x"""
    nd = len(digs)
    e = nd - 1 + exp10
    if -4 <= e < 16:
        if e < 0:
            body = "0." + "0" * (-e - 1) + digs
        elif exp10 >= 0:
            body = digs + "0" * exp10 + ".0"
        else:
            body = digs[:e + 1] + "." + digs[e + 1:]
    else:
        body = digs[0] + ("." + digs[1:] if nd > 1 else "") + "e" + str(e)
    return ("-" if neg else "") + body


def _special(x):
    if x != x:
        return "NaN"
    if math.isinf(x):
        return "-inf" if x < 0 else "inf"
    if x == 0:
        return "-0.0" if math.copysign(1.0, x) < 0 else "0.0"
    return None


def f64_cell(x):
    s = _special(x)
    if s is not None:
        return s
    return layout(x < 0, *_digits_exp(repr(abs(x))))


def f32_cell(x):
    x = np.float32(x)
    s = _special(float(x))
    if s is not None:
        return s
    return layout(bool(x < 0), *_digits_exp(np.format_float_scientific(abs(x), unique=True)))


def utf8_cell(b, one_column=False):
    if any(c in SPECIAL_BYTES for c in b):
        return b'"' + b.replace(b'"', b'""') + b'"'
    return b'""' if (one_column and not b) else b


def cell(value, typ, one_column=False):
    """one value of an Arrow column (None: null) as its cell, bytes"""
    if value is None:
        return b'""' if one_column else b""
    if pa.types.is_string(typ):
        return utf8_cell(value.encode() if isinstance(value, str) else value, one_column)
    if pa.types.is_boolean(typ):
        return b"true" if value else b"false"
    if typ == pa.float64():
        return f64_cell(value).encode()
    if typ == pa.float32():
        return f32_cell(value).encode()
    return str(int(value)).encode()


def column_values(arr):
    """python values of a column, floats without a detour that could change their bits"""
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks()
    if pa.types.is_floating(arr.type):
        vals = arr.fill_null(0).to_numpy(zero_copy_only=False)
        valid = arr.is_valid().to_pylist()
        return [(v if arr.type == pa.float32() else float(v)) if ok else None for v, ok in zip(vals, valid)]
    return arr.to_pylist()


def expected_file(schema, batches):
    one = len(schema) == 1
    out = [b",".join(utf8_cell(f.name.encode(), one) for f in schema) + b"\n"]
    for b in batches:
        cols = [[cell(v, f.type, one) for v in column_values(b.column(i))] for i, f in enumerate(schema)]
        out.extend(b",".join(row) + b"\n" for row in zip(*cols))
    return b"".join(out)


def f64_from_bits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def f32_from_bits(u):
    return np.frombuffer(struct.pack("<I", u), dtype=np.float32)[0]


def special_f64_bits():
    out = [0, 1 << 63, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF,
           1, 2, 0x000FFFFFFFFFFFFF, 0x0010000000000000, 0x0010000000000001, 0x7FEFFFFFFFFFFFFF]
    for v in [1e-4, 1e16, 1.0, 0.1, 123456.789, 1.5e-5, 5e-324, 9007199254740993.0, 0.3, 2.0 ** 53] + [float("1e%d" % k) for k in range(-323, 309, 7)]:
        u = struct.unpack("<Q", struct.pack("<d", v))[0]
        out += [u - 1, u, u + 1, (u + 1) | (1 << 63)] if u else [u]
    out += [e << 52 for e in range(1, 2047, 13)]
    return out


def special_f32_bits():
    out = [0, 1 << 31, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF, 1, 2, 0x007FFFFF, 0x00800000, 0x00800001, 0x7F7FFFFF]
    for v in [1e-4, 1e16, 1.0, 0.1, 123456.789, 1.5e-5, 1e-45, 16777217.0, 0.3] + [float("1e%d" % k) for k in range(-44, 39, 3)]:
        u = struct.unpack("<I", struct.pack("<f", v))[0]
        out += [u - 1, u, u + 1, (u + 1) | (1 << 31)] if u else [u]
    out += [e << 23 for e in range(1, 255, 5)]
    return out
