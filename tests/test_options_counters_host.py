"""CPU test of the option and counter tables (csrc/dfx_options.cpp) against the structs they name: every field of `struct Counters`
answers dfx_counter_get by its own name, every `int` field of `struct AggOptions` has exactly one key, and every key is accepted by the
per-operator option validation and rejected with one letter changed.  Loads the built library; no GPU needed (the constructors
do no device work, the counters are host memory)."""
import os
import re

import pyarrow as pa
import pytest

from datafusion_archive_amd import build as B
from datafusion_archive_amd import execution as ex
from datafusion_archive_amd.logicalplan import BinaryExpr, Column, Literal, Operator, ScalarValue


def _struct_body(header, name):
    text = open(os.path.join(B.CSRC, header)).read()
    return re.search(r"^struct %s \{.*?\n(.*?)^\};" % name, text, re.S | re.M).group(1)


def test_every_counter_field_answers_by_its_name():
    fields = re.findall(r"^\s*long long (\w+) = 0;", _struct_body("dfx_host.hpp", "Counters"), re.M)
    assert len(fields) >= 78 and len(set(fields)) == len(fields)
    ex.counter_reset()
    for f in fields:
        assert ex.counter_get(f) == 0, f
    assert ex.counter_get("no_such") == -1


def test_every_option_field_has_one_key_and_every_key_is_validated():
    fields = re.findall(r"^\s*int (\w+) = ", _struct_body("dfx_relation.hpp", "AggOptions"), re.M)
    table = open(os.path.join(B.CSRC, "dfx_options.cpp")).read()
    table = table[table.index("kOptionKeys[] = {"):table.index("static_assert")]
    rows = re.findall(r'\{"([\w.]+)",\s*&AggOptions::(\w+)\}', table)
    keys = [k for k, _ in rows]
    assert len(fields) >= 49 and len(keys) == len(fields)
    assert len(set(keys)) == len(keys)
    assert sorted(f for _, f in rows) == sorted(fields)  # ... and no field twice

    schema = pa.schema([("k", pa.int64()), ("v", pa.float64())])
    b = pa.RecordBatch.from_pydict({"k": [1], "v": [2.0]}, schema=schema)
    pred = ex.compile_scalar_expr(None, BinaryExpr(Column(1), Operator.Gt, Literal(ScalarValue.Float64(1.0))), schema)

    def operator_with(key):  # its own option set: the process defaults are not touched
        return ex.FilterRelation(ex.DataSourceRelation(schema, [b]), pred, schema, options={key: 0})
    for key in keys:
        operator_with(key)  # accepted
        wrong = key[:-1] + ("x" if key[-1] != "x" else "y")
        assert wrong not in keys
        with pytest.raises(ex.ExecutionError) as e:
            operator_with(wrong)
        assert e.value.kind == "General" and wrong in e.value.message
