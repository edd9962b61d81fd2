"""MIN / MAX of a Utf8 column (deviation D10) restated in plain Python: per group, `min` / `max` over `str.encode()` of the non-null
values -- Python orders `bytes` as Rust orders `str`: unsigned byte-wise lexicographic, a proper prefix first, the empty string the
smallest.  A group without a non-null value reports None for both.  The C oracle has no such aggregate."""
from collections import defaultdict


def key_value(k):
    return k if k is None or isinstance(k, str) else int(k)


def utf8_extrema(keys, values):
    """{key tuple: (min bytes | None, max bytes | None)} over every key tuple that occurs; keys: a list of columns (any
    sequences), values: a sequence of str | None.  Ungrouped: keys == [] and the one entry is ()."""
    groups = defaultdict(list)
    for i, v in enumerate(values):
        g = groups[tuple(key_value(k[i]) for k in keys)]
        if v is not None:
            g.append(v.encode())
    if not keys:
        groups[()]  # the ungrouped row exists whatever the input
    return {kt: ((min(g), max(g)) if g else (None, None)) for kt, g in groups.items()}


def encoded(column):
    """a result column as bytes | None"""
    return [None if v is None else v.encode() for v in column.to_pylist()]


def extrema_as_dict(batch, kw, min_col, max_col):
    """{key tuple: (min, max)} of a result batch; a column index of None reads as None throughout"""
    keys = [batch.column(i).to_pylist() for i in range(kw)]
    lo = encoded(batch.column(min_col)) if min_col is not None else [None] * batch.num_rows
    hi = encoded(batch.column(max_col)) if max_col is not None else [None] * batch.num_rows
    out = {}
    for r in range(batch.num_rows):
        kt = tuple(k[r] for k in keys)
        assert kt not in out, f"duplicate group {kt}"
        out[kt] = (lo[r], hi[r])
    return out
