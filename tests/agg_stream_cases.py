"""Streams for the oracle-bound fuzz of the grouped aggregate's strategy state machine (tests/test_gpu_agg_state_machine.py on
the device, tests/test_agg_stream_cases_host.py for the generator and the reference side).  No GPU import.

AggregateRelation decides how a GROUP BY runs from the first 2^18 rows of a first batch of more than 2^21 rows (the calibration
slice) and carries that decision through the stream; every decision has a "turned out wrong later" path.  A case here is a
stream whose CHARACTER CHANGES after the decision: right behind the slice (row 2^18 of the first batch), at a batch boundary,
or both.  Each stream has three phases -- A: rows [0, 2^18) of the first batch, B: the rest of the first batch, C: the later
batches -- and a phase fixes the key distribution, the pass rate of the predicate and whether the operands carry nulls.

Values are exact: Float64 operands are integers below 2^20 times 2^-10 (any partial sum over <= 2^23 rows is representable, so
a sum has the same bits in every order of additions), Int64 operands wrap.  No NaN, no signed zeros.

cases(seed) is deterministic.  A Case is light (a recipe and a seed of its own); Case.batches() builds the host RecordBatches.
Case.line is enough to replay it alone: cases(seed)[index].
"""
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

from datafusion_archive_amd.logicalplan import AggregateFunction, BinaryExpr, Column, DataType, Literal, Operator, ScalarValue

SLICE = 1 << 18          # rows of the calibration slice
BIG = 1 << 21            # a first batch longer than this gets a slice
I64_MIN = -(2 ** 63)
F64, I64, U64 = DataType.Float64, DataType.Int64, DataType.UInt64
LO, HI = 204.8, 409.6    # the predicate: LO < column < HI (values are m * 2^-10, 0 <= m < 2^20: a fifth of a uniform column passes)

# thresholds the operator tests the group count against: few-group registers, the LDS front cache, the partitioned strategy,
# and the load limit of the default table of 256 blocks x 8192 slots (beyond it the table grows and the pair / plane blocks stop applying)
THRESHOLDS = (8, 8192, 16384, 1 << 20)

AGG_SETS = {
    # name: [(function, operand column)], the host-side family it lands in when there are many groups and one narrow key
    "one_sum": [("SUM", "v")],                                            # headline path
    "one_min_w": [("MIN", "w")],
    "planes3": [("SUM", "v"), ("MIN", "v"), ("MAX", "v")],                 # one operand: a pass 2 per accumulator plane
    "planes_avg": [("AVG", "v")],                                          # AVG = SUM + COUNT of one operand
    "shared2": [("SUM", "v"), ("MIN", "v")],
    "pair": [("SUM", "v"), ("MIN", "w")],                                  # two operands: the pair scan
    "pair_raw": [("AVG", "v"), ("MAX", "w")],                              # ... three accumulators: raw operands in the pair rows
    "three_ops": [("SUM", "v"), ("MIN", "w"), ("MAX", "x")],               # a scan per aggregate, held batches
    "chunks": [("SUM", "v"), ("MIN", "v"), ("MAX", "v"), ("COUNT", "v"), ("SUM", "w"), ("MIN", "w"), ("MAX", "w"), ("COUNT", "w"),
               ("AVG", "x"), ("MAX", "x")],                                # 11 accumulators: more than one fused program takes
    "distinct": [("SUM", "v"), ("COUNT_DISTINCT", "d"), ("MAX", "w")],
}

# options drawn 2-3 together for the cases without a fixed recipe (and added one at a time to some recipes)
OPTION_POOL = [("agg.capacity_log2", (9, 11, 13, 14, 16)), ("agg.partition_cap_rows", (128, 640)), ("agg.partition_defer", (1, 4)),
               ("agg.partition_defer_batches", (1, 2, 8)), ("agg.hot_keys", (0, 1)), ("agg.narrow_keys", (0, 1)), ("agg.pair_scan", (0,)),
               ("agg.shared_planes", (0,)), ("agg.shared_operand", (0,)), ("agg.split_aggregates", (0,)), ("agg.chunk_hold", (1, 2)),
               ("agg.replay_in_place", (0,)), ("agg.pass1_ws", (0,)), ("agg.pass2_stream", (0,)), ("agg.fewgroup", (0,)),
               ("agg.strategy", (1, 3)), ("scan.plan", (0, 2)), ("scan.fast", (0,)), ("agg.calibration_memo", (0,))]


def _phase_text(p):
    return p[0] + "(" + ",".join(str(x) for x in p[1:]) + ")"


class Case:
    def __init__(self, seed, index, name, keys, aggs, rates=None, pred_col="v", nulls_from=None, null_cols=("v",), empty=None,
                 first_big=True, key_kind="i64", options=None, n_batches=4, rows=None, resident=False, crosses=None, scale=1.0):
        self.seed, self.index, self.name = seed, index, name
        self.keys = keys              # (A, B, C): key phases -- ("uni", G) | ("wide", G) | ("skew", G, permille of the hot key) | ("hot", G, H)
        self.agg_set = aggs
        self.rates = rates            # (A, B, C) pass rates of the predicate in permille, or None: no predicate
        self.pred_col = pred_col if rates else None
        self.nulls_from = nulls_from  # index of the first non-empty batch whose operands in `null_cols` carry nulls
        self.null_cols = tuple(null_cols)
        self.empty = empty            # "first" | "middle" | "last" | None: where an empty batch goes
        self.first_big = first_big
        self.key_kind = key_kind      # "i64" | "two" (a second small key column) | "utf8"
        self.options = dict(options or {})
        self.n_batches = n_batches
        self.rows = rows              # total rows at scale 1
        self.resident = resident      # also run over a resident table, twice
        self.crosses = crosses        # (threshold, "few->many" | "many->few") or None
        self.scale = scale
        self.n_keys = 2 if key_kind == "two" else 1

    # ---- the query -----------------------------------------------------------------------------------------------------------
    @property
    def columns(self):
        names = ["k"] + (["k2"] if self.key_kind == "two" else [])
        for _f, c in AGG_SETS[self.agg_set]:
            if c not in names:
                names.append(c)
        if self.pred_col and self.pred_col not in names:
            names.append(self.pred_col)
        return names

    @property
    def schema(self):
        t = {"k": pa.string() if self.key_kind == "utf8" else pa.int64(), "k2": pa.int64(), "v": pa.float64(), "w": pa.int64(),
             "x": pa.float64(), "p": pa.float64(), "d": pa.int64()}
        return pa.schema([(c, t[c]) for c in self.columns])

    def col(self, name):
        return Column(self.columns.index(name))

    @property
    def group(self):
        return [Column(i) for i in range(self.n_keys)]

    @property
    def aggs(self):
        """every aggregate, COUNT_DISTINCT included, in result order"""
        out = []
        for f, c in AGG_SETS[self.agg_set]:
            t = U64 if f in ("COUNT", "COUNT_DISTINCT") else (I64 if c in ("w", "d") else F64)
            out.append(AggregateFunction(f, [self.col(c)], t))
        return out

    @property
    def distinct_positions(self):
        return [i for i, (f, _c) in enumerate(AGG_SETS[self.agg_set]) if f == "COUNT_DISTINCT"]

    @property
    def plain_aggs(self):
        """the aggregates the oracle knows (it has no COUNT_DISTINCT)"""
        d = set(self.distinct_positions)
        return [a for i, a in enumerate(self.aggs) if i not in d]

    @property
    def pred(self):
        if not self.rates:
            return None
        c = self.col(self.pred_col)
        return BinaryExpr(BinaryExpr(c, Operator.Gt, Literal(ScalarValue.Float64(LO))), Operator.And,
                          BinaryExpr(c, Operator.Lt, Literal(ScalarValue.Float64(HI))))

    # ---- the description -----------------------------------------------------------------------------------------------------
    @property
    def tags(self):
        """the families this case belongs to (what test_agg_stream_cases_host.py counts)"""
        A, B, C = self.keys
        t = {"aggs:" + self.agg_set, "keys:" + self.key_kind, "first:" + ("big" if self.first_big else "small")}
        kinds = [p[0] for p in (A, B, C)]
        for a, b, where in ((A, B, "slice"), (B, C, "batch")):
            if a != b:
                t.add("change@" + where)
            if a[0] != "wide" and b[0] == "wide":
                t.add("narrow->wide@" + where)
            if a[0] in ("uni", "wide") and b[0] in ("skew", "hot"):
                t.add("uniform->skew")
            if a[0] in ("skew", "hot") and b[0] == "uni":
                t.add("skew->uniform")
        if self.crosses:
            t.add("crosses:%d:%s" % self.crosses)
        if self.rates:
            rA, rB, rC = self.rates
            for a, b in ((rA, rB), (rB, rC)):
                if a < 500 <= b:
                    t.add("selective->dense")
                if b < 500 <= a:
                    t.add("dense->selective")
            t.add("pred:" + self.pred_col)
        else:
            t.add("pred:none")
        if self.nulls_from is not None:
            t.add("nulls@batch%d" % (self.nulls_from + 1))
            if self.rates:
                t.add("nulls-under-predicate")
        if self.empty:
            t.add("empty:" + self.empty)
        if self.resident:
            t.add("resident")
        t.add("options:%d" % len(self.options))
        for k in self.options:
            t.add("opt:" + k)
        del kinds
        return t

    @property
    def line(self):
        return ("agg_stream_cases.cases(%d)[%d] %s: rows=%s batches=%d first=%s keys[%s] %s | %s | %s aggs=%s pred=%s rates=%s nulls_from=%s%s "
                "empty=%s crosses=%s resident=%d options=%s" % (
                    self.seed, self.index, self.name, self.rows, self.n_batches, "big" if self.first_big else "small", self.key_kind,
                    _phase_text(self.keys[0]), _phase_text(self.keys[1]), _phase_text(self.keys[2]),
                    "+".join("%s(%s)" % fc for fc in AGG_SETS[self.agg_set]), self.pred_col, self.rates, self.nulls_from,
                    "/".join(self.null_cols) if self.nulls_from is not None else "", self.empty, self.crosses, int(self.resident),
                    sorted(self.options.items())))

    # ---- the data ------------------------------------------------------------------------------------------------------------
    def _lengths(self, rng):
        """ragged batch lengths (never multiples of 64), the first one above 2^21 rows when first_big"""
        s = self.scale
        total = int(self.rows * s)
        big = int(BIG * s)
        if self.first_big:
            first = big + int(rng.integers(int(big * 0.02), int(big * 0.2)))
        else:
            first = int(rng.integers(int(big * 0.1), int(big * 0.45)))
        rest = max(total - first, 3 * (self.n_batches - 1))
        cuts = np.sort(rng.integers(rest // (4 * self.n_batches), rest, self.n_batches - 2)) if self.n_batches > 2 else np.array([], dtype=np.int64)
        edges = np.concatenate([[0], cuts, [rest]]).astype(np.int64)
        lens = [first] + [int(x) for x in np.diff(edges)]
        return [max(n, 3) + 1 if max(n, 3) % 64 == 0 else max(n, 3) for n in lens]

    def _keys(self, rng, phase, n):
        kind, G = phase[0], int(phase[1])
        k = rng.integers(0, G, n).astype(np.int64)
        if kind == "wide":  # keys without a 32-bit image: at or above 2^32, and negative ones
            sel = rng.integers(0, 3, n)
            k = np.where(sel == 0, k + (1 << 32), np.where(sel == 1, -k - 1, k))
        elif kind == "skew":  # one key takes phase[2] permille of the rows
            k[rng.random(n) < phase[2] / 1000.0] = G // 3
        elif kind == "hot":   # half of the rows on phase[2] keys, the rest uniform
            hot = rng.random(n) < 0.5
            k[hot] = rng.integers(0, int(phase[2]), int(hot.sum())) * 7 + 1
        return k

    def _rated(self, rng, rate, n):
        """a column of m * 2^-10 of which `rate` permille lie inside (LO, HI)"""
        lo_m, hi_m = int(LO * 1024) + 1, int(HI * 1024)   # m in [lo_m, hi_m) passes: 204.8 * 1024 = 209715.2
        inside = rng.integers(lo_m, hi_m, n)
        below = rng.integers(0, lo_m, n)
        above = rng.integers(hi_m + 1, 1 << 20, n)
        u = rng.random(n)
        m = np.where(u < rate / 1000.0, inside, np.where(rng.random(n) < 0.4, below, above))
        return m.astype(np.float64) * 2.0 ** -10

    def batches(self):
        rng = np.random.default_rng([self.seed, self.index])
        lens = self._lengths(rng)
        n = sum(lens)
        n0 = min(int(SLICE * self.scale), lens[0])
        spans = [(0, n0, 0), (n0, lens[0], 1), (lens[0], n, 2)]
        cols = {}
        k = np.empty(n, dtype=np.int64)
        for a, b, ph in spans:
            k[a:b] = self._keys(rng, self.keys[ph], b - a)
        A, _B, C = self.keys
        if "wide" in (self.keys[1][0], C[0]) and n > n0 + 8:
            # the edges of the 32-bit image, wherever the wide phase starts: the table's sentinel, 2^32 itself; 0 and 2^32 - 1 are narrow
            w0 = n0 if self.keys[1][0] == "wide" else lens[0]
            k[w0 + 3], k[w0 + 5], k[n - 2] = I64_MIN, 1 << 32, I64_MIN
            k[1], k[2] = 0, (1 << 32) - 1
        cols["k"] = k
        if self.key_kind == "two":
            cols["k2"] = rng.integers(0, 4, n).astype(np.int64)
        names = self.columns
        for c in ("v", "x", "p"):
            if c in names:
                if c == self.pred_col:
                    cols[c] = np.concatenate([self._rated(rng, self.rates[ph], b - a) for a, b, ph in spans])
                else:
                    cols[c] = rng.integers(0, 1 << 20, n).astype(np.float64) * 2.0 ** -10
        if "w" in names:
            cols["w"] = rng.integers(-(1 << 62), 1 << 62, n).astype(np.int64)  # sums wrap
        if "d" in names:
            cols["d"] = rng.integers(0, 600, n).astype(np.int64)
        starts = np.concatenate([[0], np.cumsum(lens)])
        arrays = []
        for c in names:
            a = cols[c]
            if self.nulls_from is not None and c in self.null_cols:
                valid = np.ones(n, dtype=bool)
                s0 = int(starts[self.nulls_from])
                valid[s0:] = rng.random(n - s0) > 0.1
                arrays.append(pa.Array.from_buffers(self.schema.field(c).type, n, [pa.py_buffer(np.packbits(valid, bitorder="little").tobytes()),
                                                                                  pa.py_buffer(a)], null_count=int(n - valid.sum())))
            elif c == "k" and self.key_kind == "utf8":
                arrays.append(pc.binary_join_element_wise(pa.scalar("key"), pc.cast(pa.array(a), pa.string()), "-"))
            else:
                arrays.append(pa.array(a))
        whole = pa.RecordBatch.from_arrays(arrays, schema=self.schema)
        out = [whole.slice(int(starts[i]), lens[i]) for i in range(len(lens))]  # every batch but the first has a non-zero Arrow offset
        if self.empty:
            at = {"first": 0, "middle": len(out) // 2, "last": len(out)}[self.empty]
            out.insert(at, whole.slice(int(starts[min(at, len(lens) - 1)]), 0))
        return out


def _recipes(seed, scale):
    """The cases with a purpose: each is built to cross one decision.  Rows are sized by the thresholds, not by taste."""
    M = 1 << 20
    sel, dense = (200, 200, 200), (900, 900, 900)
    R = []

    def add(name, keys, aggs, **kw):
        kw.setdefault("rows", 3 * M)
        R.append(Case(seed, len(R), name, keys, aggs, scale=scale, **kw))

    U = lambda g: ("uni", g)
    # -- few -> many groups, the slice's count and the final one on opposite sides of each threshold; change behind the slice / at a batch boundary
    add("few8_slice", (U(5), U(300), U(300)), "one_sum", rates=sel, crosses=(8, "few->many"), resident=True)
    add("few8_batch", (U(6), U(6), U(5000)), "planes3", rates=(200, 200, 900), crosses=(8, "few->many"), empty="middle", options={'agg.partition_defer_batches': 2, 'scan.plan': 2})
    add("lds8192_slice", (U(3000), U(12000), U(12000)), "one_min_w", crosses=(8192, "few->many"), options={"agg.fewgroup": 0, "scan.fast": 0})
    add("lds8192_batch", (U(4000), U(4000), U(150000)), "pair", rates=sel, crosses=(8192, "few->many"), options={'agg.narrow_keys': 1, 'agg.replay_in_place': 0})
    add("part16384_slice", (U(12000), U(200000), U(200000)), "one_sum", rates=(900, 200, 200), crosses=(16384, "few->many"), options={'agg.strategy': 1, 'agg.capacity_log2': 16})
    add("part16384_batch", (U(9000), U(9000), U(300000)), "pair_raw", crosses=(16384, "few->many"), empty="last")
    add("blocks_pair_batch", (U(200000), U(200000), U(1700000)), "pair", rows=int(7.6 * M), n_batches=3, crosses=(1 << 20, "few->many"))
    add("blocks_planes_slice", (U(100000), U(1600000), U(1600000)), "planes_avg", rows=int(7.2 * M), n_batches=3, crosses=(1 << 20, "few->many"))
    # -- many -> few
    add("many_few_batch", (U(200000), U(200000), U(5)), "one_sum", rates=(200, 900, 900), crosses=(16384, "many->few"))
    add("many_few_slice", (U(60000), U(7), U(7)), "shared2", rates=sel, crosses=(16384, "many->few"), options={"agg.shared_planes": 0, "agg.partition_defer": 4})
    # -- narrow -> wide keys
    add("wide_batch", (U(100000), U(100000), ("wide", 100000)), "one_sum", rates=sel, n_batches=5, resident=True)
    add("wide_slice", (U(50000), ("wide", 50000), ("wide", 50000)), "one_sum", options={"agg.pass2_stream": 0, "agg.partition_defer": 1})
    add("wide_late_pair", (U(200000), U(200000), ("wide", 200000)), "pair", rates=sel, n_batches=6, rows=6 * M)
    add("wide_planes", (U(80000), U(80000), ("wide", 80000)), "planes3", rates=(200, 200, 900), options={'agg.partition_defer_batches': 1, 'agg.pass1_ws': 0})
    # -- uniform -> skew and back
    add("skew_pair_spill", (U(100000), U(100000), ("skew", 100000, 400)), "pair", rates=(200, 200, 900), options={"agg.hot_keys": 0, "agg.partition_cap_rows": 640})
    add("skew_hot_forced", (U(100000), ("skew", 100000, 350), ("skew", 100000, 350)), "one_sum", rates=sel, options={"agg.hot_keys": 1, "agg.partition_cap_rows": 128})
    add("skew_seen_then_uniform", (("hot", 100000, 24), ("hot", 100000, 24), U(100000)), "one_sum", rates=dense)
    add("uniform_then_skew_default", (U(150000), U(150000), ("skew", 150000, 450)), "one_sum", rates=(200, 200, 900), resident=True)
    # -- a table that starts small: the slice itself overflows it
    add("small_table_one", (U(200000), U(200000), U(200000)), "one_sum", rates=sel, options={"agg.capacity_log2": 11, "agg.pass1_ws": 0})
    add("small_table_pair", (U(200000), U(200000), U(400000)), "pair", rates=sel, options={"agg.capacity_log2": 14, "agg.partition_defer_batches": 2})
    add("small_table_planes", (U(150000), U(150000), U(150000)), "planes3", options={"agg.capacity_log2": 13, "agg.replay_in_place": 0}, empty="first")
    # -- nulls arrive in a later batch
    add("nulls_pair_forced", (U(50000), U(50000), U(50000)), "pair_raw", first_big=False, rows=2 * M, nulls_from=1, null_cols=("v",),
        options={"agg.strategy": 3, "agg.narrow_keys": 1, "agg.capacity_log2": 14})
    add("nulls_pair_default", (U(120000), U(120000), U(120000)), "pair", nulls_from=2, null_cols=("w",))
    add("nulls_planes", (U(120000), U(120000), U(120000)), "planes_avg", nulls_from=1, null_cols=("v",), options={'agg.partition_defer': 4, 'agg.narrow_keys': 1})
    add("nulls_unfused", (U(100000), U(100000), U(100000)), "one_sum", rates=sel, pred_col="p", nulls_from=1, null_cols=("v",), options={"scan.plan": 0, "agg.calibration_memo": 0})
    add("nulls_unfused_pair", (U(100000), U(100000), U(100000)), "pair", rates=(200, 900, 200), pred_col="p", nulls_from=2, null_cols=("v", "w"), options={"scan.fast": 0, "agg.chunk_hold": 2})
    add("nulls_planned", (U(30000), U(30000), ("wide", 30000)), "pair", rates=sel, pred_col="v", nulls_from=1, null_cols=("w",), options={"scan.plan": 2, "agg.hot_keys": 0})
    # -- the other host-side families
    add("three_operands", (U(100000), U(100000), U(250000)), "three_ops", rates=sel, n_batches=6, rows=4 * M)
    add("three_operands_hold1", (U(100000), ("wide", 100000), U(100000)), "three_ops", options={"agg.chunk_hold": 1, "agg.narrow_keys": 0})
    add("chunks", (U(3000), U(3000), U(60000)), "chunks", rates=sel, n_batches=5, options={'agg.fewgroup': 0, 'agg.chunk_hold': 1})
    add("chunks_partitioned", (U(70000), U(70000), U(70000)), "chunks", rows=int(2.5 * M), options={"agg.chunk_hold": 2, "agg.split_aggregates": 0})
    add("shared_operand", (U(100000), U(100000), ("skew", 100000, 300)), "shared2", rates=sel, options={"agg.shared_planes": 0, "agg.partition_defer_batches": 8})
    add("pair_scan_off", (U(100000), U(100000), ("wide", 100000)), "pair", rates=sel, options={"agg.pair_scan": 0, "agg.chunk_hold": 2})
    add("shared_rows_off", (U(90000), ("skew", 90000, 300), U(90000)), "shared2", rates=(200, 900, 900), options={"agg.shared_operand": 0, "agg.shared_planes": 0})
    add("distinct_beside_plain", (U(4096), U(4096), U(20000)), "distinct", rows=int(2.2 * M), options={"agg.distinct_capacity_log2": 9, "agg.capacity_log2": 12})
    add("distinct_predicate", (U(500), U(500), U(500)), "distinct", rates=sel, first_big=False, rows=2 * M, options={"agg.distinct_capacity_log2": 10})
    add("two_keys", (U(20000), U(20000), U(90000)), "pair", rates=sel, key_kind="two", options={'agg.split_aggregates': 0, 'agg.capacity_log2': 9})
    add("two_keys_small_table", (U(50), U(30000), U(30000)), "one_sum", key_kind="two", options={"agg.capacity_log2": 10, "agg.strategy": 3})
    add("utf8_key", (U(2000), U(2000), U(40000)), "pair", rates=sel, key_kind="utf8", rows=2 * M + 300000, options={"agg.dict_capacity_log2": 6})
    add("utf8_key_small", (U(90), U(90), U(5000)), "one_sum", key_kind="utf8", first_big=False, rows=2 * M, options={"agg.dict_capacity_log2": 4, "agg.capacity_log2": 9})
    # -- "decide after the first batch": a first batch too small for a slice
    add("first_small", (U(100), U(100), U(50000)), "one_sum", rates=(200, 200, 900), first_big=False, rows=2 * M + 5000)
    add("first_small_wide", (U(40000), U(40000), ("wide", 40000)), "pair", first_big=False, rows=2 * M + 77, empty="first")
    return R


def cases(seed, scale=1.0):
    """The deterministic list of cases of `seed`.  scale < 1 shrinks the row counts (and the slice) for the CPU test of the
    generator and the oracle; the GPU test runs scale 1 only: the thresholds are the operator's, they do not scale."""
    out = _recipes(seed, scale)
    rng = np.random.default_rng([seed, 0xA66])
    shapes = [(("uni", 40000), ("uni", 40000), ("wide", 300000)), (("uni", 7), ("uni", 90000), ("skew", 90000, 400)),
              (("uni", 250000), ("skew", 250000, 320), ("uni", 600000)), (("hot", 60000, 16), ("uni", 60000), ("wide", 60000)),
              (("uni", 10000), ("uni", 20000), ("uni", 500000)), (("uni", 300000), ("uni", 300000), ("uni", 3))]
    sets = ["one_sum", "planes3", "pair", "pair_raw", "three_ops", "shared2"]
    rate_choices = [None, (200, 200, 900), (900, 200, 200), (200, 900, 200), (100, 100, 100)]
    for i in range(6):  # drawn: phases, aggregates and 2-3 options together (a quarter with the defaults only)
        keys = shapes[int(rng.integers(0, len(shapes)))]
        aggs = sets[int(rng.integers(0, len(sets)))]
        rates = rate_choices[int(rng.integers(0, len(rate_choices)))]
        opts = {}
        if i % 4 != 3:
            for j in rng.choice(len(OPTION_POOL), int(rng.integers(2, 4)), replace=False):
                k, vals = OPTION_POOL[int(j)]
                opts[k] = int(vals[int(rng.integers(0, len(vals)))])
        nulls = [None, None, 1, 2][int(rng.integers(0, 4))]
        out.append(Case(seed, len(out), "drawn%d" % i, keys, aggs, rates=rates, pred_col="v",
                        nulls_from=nulls, null_cols=("w",) if rates else ("v",), empty=[None, "first", "middle", "last"][int(rng.integers(0, 4))],
                        first_big=bool(rng.random() < 0.8), options=opts, n_batches=int(rng.integers(3, 7)),
                        rows=int(rng.integers(2 * (1 << 20) + 400000, 4 * (1 << 20))), scale=scale))
    return out


# ---- numpy truths (no oracle, no device) ---------------------------------------------------------------------------------------
def concat_filtered(case, batches):
    """{column: numpy values}, {column: validity} of the rows that pass the predicate, over the whole stream.  Under a predicate every
    surviving slot counts as valid and holds whatever the slot held (the reference's filter ignores value nulls)."""
    t = pa.Table.from_batches(batches, schema=case.schema)
    vals, valid = {}, {}
    for name in case.columns:
        a = t.column(name).combine_chunks()
        if pa.types.is_string(a.type):
            vals[name] = np.array(a.to_pylist(), dtype=object)
            valid[name] = np.ones(len(a), dtype=bool)
            continue
        valid[name] = np.asarray(a.is_valid()) if a.null_count else np.ones(len(a), dtype=bool)
        np_t = a.type.to_pandas_dtype()
        vals[name] = np.frombuffer(a.buffers()[1], dtype=np_t, count=len(a), offset=a.offset * np.dtype(np_t).itemsize)
    if case.rates:
        c = vals[case.pred_col]
        keep = (c > LO) & (c < HI)
        vals = {k: v[keep] for k, v in vals.items()}
        valid = {k: np.ones(int(keep.sum()), dtype=bool) for k in valid}
    return vals, valid


def group_ids(case, vals):
    """(number of groups, group id per row, the key columns of each group)"""
    if case.key_kind == "two":
        comb = vals["k"] * 4 + vals["k2"]
        u, inv = np.unique(comb, return_inverse=True)
        return len(u), inv, [u // 4, u % 4]
    u, inv = np.unique(vals["k"], return_inverse=True)
    return len(u), inv, [u]


def distinct_truth(case, batches, column):
    """{key tuple: number of distinct valid values of `column`}"""
    vals, valid = concat_filtered(case, batches)
    g, inv, keys = group_ids(case, vals)
    out = np.zeros(g, dtype=np.int64)
    ok = valid[column]
    pairs = np.unique(inv[ok].astype(np.int64) * (1 << 20) + vals[column][ok])  # (values of `d` are below 600)
    np.add.at(out, pairs >> 20, 1)
    return {tuple(int(k[i]) for k in keys): int(out[i]) for i in range(g)}
