/*
 * dfx.h -- C ABI of the MI355X-native filter / projection / aggregate execution path.
 *
 * This is the drop-in boundary for andygrove/datafusion-archive's src/execution::{filter,
 * projection,aggregate} and its RecordBatch expression evaluator.  Every entry point below
 * names the reference interface it replaces (paths relative to the reference repo root).
 *
 * Conventions
 *  - plain C, no C++/HIP/torch types in any signature;
 *  - RecordBatches cross the boundary as Arrow C Data Interface structs; the pull-based
 *    `trait Relation { next(); schema() }` (src/execution/relation.rs:27-32) crosses it as the
 *    Arrow C Stream Interface: get_next()==Relation::next() (a released array == Ok(None)),
 *    get_schema()==Relation::schema();
 *  - every function returns a dfx_status (0 = OK); the code mirrors the variant of
 *    `ExecutionError` (src/execution/error.rs:26-36) the reference would have produced.  Message
 *    text goes to the caller-provided `err` buffer (or ArrowArrayStream.get_last_error for
 *    stream callbacks).  No C++ exception, HIP error or panic crosses this ABI;
 *  - handles are thread-confined (the reference is Rc<RefCell<..>>, i.e. !Send + !Sync).
 */
#ifndef DFX_H
#define DFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Arrow C Data / C Stream / C Device interfaces (standard ABI, verbatim struct layouts).
 * ---------------------------------------------------------------------------------------- */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
#define ARROW_FLAG_DICTIONARY_ORDERED 1
#define ARROW_FLAG_NULLABLE 2
#define ARROW_FLAG_MAP_KEYS_SORTED 4
struct ArrowSchema {
  const char* format;
  const char* name;
  const char* metadata;
  int64_t flags;
  int64_t n_children;
  struct ArrowSchema** children;
  struct ArrowSchema* dictionary;
  void (*release)(struct ArrowSchema*);
  void* private_data;
};
struct ArrowArray {
  int64_t length;
  int64_t null_count;
  int64_t offset;
  int64_t n_buffers;
  int64_t n_children;
  const void** buffers;
  struct ArrowArray** children;
  struct ArrowArray* dictionary;
  void (*release)(struct ArrowArray*);
  void* private_data;
};
#endif

#ifndef ARROW_C_STREAM_INTERFACE
#define ARROW_C_STREAM_INTERFACE
struct ArrowArrayStream {
  int (*get_schema)(struct ArrowArrayStream*, struct ArrowSchema* out);
  int (*get_next)(struct ArrowArrayStream*, struct ArrowArray* out);
  const char* (*get_last_error)(struct ArrowArrayStream*);
  void (*release)(struct ArrowArrayStream*);
  void* private_data;
};
#endif

/* ------------------------------------------------------------------------------------------
 * Status codes == ExecutionError variants (src/execution/error.rs:26-36), same order.
 * ---------------------------------------------------------------------------------------- */
typedef enum dfx_status {
  DFX_OK = 0,
  DFX_IO_ERROR = 1,        /* ExecutionError::IoError        */
  DFX_PARSER_ERROR = 2,    /* ExecutionError::ParserError    */
  DFX_GENERAL = 3,         /* ExecutionError::General        */
  DFX_INVALID_COLUMN = 4,  /* ExecutionError::InvalidColumn  */
  DFX_NOT_IMPLEMENTED = 5, /* ExecutionError::NotImplemented (also the reference's unimplemented!()) */
  DFX_INTERNAL_ERROR = 6,  /* ExecutionError::InternalError  (also the reference's panic!()/unwrap()) */
  DFX_ARROW_ERROR = 7,     /* ExecutionError::ArrowError     (e.g. arrow DivideByZero) */
  DFX_EXECUTION_ERROR = 8  /* ExecutionError::ExecutionError (also HIP / RCCL failures) */
} dfx_status;

/* arrow::datatypes::DataType subset used by the path (expression.rs:135-166). */
typedef enum dfx_dtype {
  DFX_TYPE_NONE = 0,
  DFX_BOOLEAN = 1,
  DFX_INT8 = 2,
  DFX_INT16 = 3,
  DFX_INT32 = 4,
  DFX_INT64 = 5,
  DFX_UINT8 = 6,
  DFX_UINT16 = 7,
  DFX_UINT32 = 8,
  DFX_UINT64 = 9,
  DFX_FLOAT32 = 10,
  DFX_FLOAT64 = 11,
  DFX_UTF8 = 12
} dfx_dtype;

/* logicalplan::Operator (src/logicalplan.rs:67-84), same order. */
typedef enum dfx_operator {
  DFX_OP_EQ = 0,
  DFX_OP_NOT_EQ = 1,
  DFX_OP_LT = 2,
  DFX_OP_LT_EQ = 3,
  DFX_OP_GT = 4,
  DFX_OP_GT_EQ = 5,
  DFX_OP_PLUS = 6,
  DFX_OP_MINUS = 7,
  DFX_OP_MULTIPLY = 8,
  DFX_OP_DIVIDE = 9,
  DFX_OP_MODULUS = 10,
  DFX_OP_AND = 11,
  DFX_OP_OR = 12,
  DFX_OP_NOT = 13,
  DFX_OP_LIKE = 14,
  DFX_OP_NOT_LIKE = 15
} dfx_operator;

/* logicalplan::Expr variants (src/logicalplan.rs:136-167), same order. */
typedef enum dfx_expr_kind {
  DFX_EXPR_COLUMN = 0,
  DFX_EXPR_LITERAL = 1,
  DFX_EXPR_BINARY = 2,
  DFX_EXPR_IS_NOT_NULL = 3,
  DFX_EXPR_IS_NULL = 4,
  DFX_EXPR_CAST = 5,
  DFX_EXPR_SORT = 6,
  DFX_EXPR_SCALAR_FUNCTION = 7,
  DFX_EXPR_AGGREGATE_FUNCTION = 8
} dfx_expr_kind;

/*
 * One node of a serialised logicalplan::Expr tree.  A tree is an array of nodes in any order
 * with child links by index; `root` selects the top node.  This is what a Rust shim derives
 * from the `&Expr` it is handed by ExecutionContext::execute (src/execution/context.rs:132,
 * :155,:174,:180) -- the reference's RuntimeExpr holds opaque closures, so the tree itself has
 * to cross the boundary.
 */
typedef struct dfx_expr_node {
  int32_t kind;   /* dfx_expr_kind */
  int32_t op;     /* BINARY: dfx_operator */
  int32_t dtype;  /* LITERAL: literal's type (DFX_TYPE_NONE == ScalarValue::Null);
                     CAST: target type; AGGREGATE_FUNCTION / SCALAR_FUNCTION: return_type */
  int32_t left;   /* BINARY: left child; CAST / AGGREGATE / IS_NULL / IS_NOT_NULL / SORT: the child; else -1 */
  int32_t right;  /* BINARY: right child; else -1 */
  int32_t column; /* COLUMN: column index */
  int32_t n_args; /* AGGREGATE_FUNCTION / SCALAR_FUNCTION: number of arguments (reference asserts 1,
                     expression.rs:91); the first argument is `left` */
  int32_t reserved;
  union {
    int64_t i64;  /* Int8..Int64 literals, sign-extended */
    uint64_t u64; /* UInt8..UInt64 literals, zero-extended; Boolean: 0/1 */
    double f64;   /* Float64 literal */
    float f32;    /* Float32 literal */
  } lit;
  const char* name; /* AGGREGATE_FUNCTION / SCALAR_FUNCTION: function name (matched case-insensitively,
                       expression.rs:98); Utf8 literal: the string; else NULL */
} dfx_expr_node;

/* ------------------------------------------------------------------------------------------
 * Library / device
 * ---------------------------------------------------------------------------------------- */
/* ABI version of this header. */
#define DFX_ABI_VERSION 1
int32_t dfx_abi_version(void);

/* Bind the calling process to one GPU (one process per GPU).  Must precede any other call that
 * touches the device; default device is 0.  No reference equivalent (reference is CPU-only). */
int32_t dfx_init(int32_t device_ordinal, char* err, size_t errlen);
/* Device facts for reports: name, CU count, HBM bytes, wavefront size. */
int32_t dfx_device_info(char* name, size_t namelen, int32_t* n_cu, int64_t* hbm_bytes,
                        int32_t* wavefront, char* err, size_t errlen);
/* Block until every stream of the library is idle (bench bracketing). */
int32_t dfx_synchronize(char* err, size_t errlen);

/* ------------------------------------------------------------------------------------------
 * Expression compiler.
 *   replaces: compile_scalar_expr (src/execution/expression.rs:283-505)
 *             compile_expr        (src/execution/expression.rs:80-121)
 *             RuntimeExpr::{get_name,get_type} (expression.rs:56-77)
 * Validation errors map 1:1 on the reference's Err cases (unsupported literal type :306-309,
 * unsupported operator :494-497, unsupported expression :500-503, cast rules :316-379,
 * unsupported aggregate :103-106).
 * Aggregate names (matched case-insensitively): MIN, MAX, SUM, COUNT, AVG and COUNT_DISTINCT (one argument, return type
 * UInt64: the number of distinct non-null argument values; a Rust shim maps AggregateType::CountDistinct to this name).
 * MIN / MAX also take a bare Utf8 Column with return type Utf8 (deviation D10: the planner types them so, sqlplanner.rs:309-322,
 * the reference's executor panics): a nullable Utf8 result in Rust `str` ordering (the order of the string terms below; the empty
 * string is the smallest), null arguments skipped, NULL for a group without a non-null argument.
 * Utf8 string terms (deviation D9): a BinaryExpr of a bare Utf8 Column and a Utf8 Literal compiles -- Eq NotEq Lt LtEq Gt GtEq
 * with the literal on either side, Like / NotLike with the column on the left and the pattern on the right -- to a Boolean
 * expression named by its Debug form (`#4 Eq Utf8("CO")`), alone or anywhere under AND / OR beside numeric terms.  Ordering is
 * Rust `str` ordering (unsigned byte-wise, a proper prefix first), equality is byte equality.  LIKE: `%` any run of bytes, `_`
 * one UTF-8 encoded character, no escape character, anchored at both ends; NOT LIKE is the complement on non-null rows.  A null
 * slot gives Eq false, NotEq true, Lt / LtEq true, Gt / GtEq false, Like false, NotLike true (arrow 0.12 bool_op over
 * Option<T>; recalled, unpinned).  A literal of more than 4096 bytes is DFX_NOT_IMPLEMENTED.  Every other use of a Utf8
 * literal, Like on other operands and Utf8 column against Utf8 column are refused as the reference refuses them.
 * ---------------------------------------------------------------------------------------- */
typedef struct dfx_runtime_expr dfx_runtime_expr;

int32_t dfx_compile_scalar_expr(const dfx_expr_node* nodes, int32_t n_nodes, int32_t root,
                                const struct ArrowSchema* input_schema, dfx_runtime_expr** out,
                                char* err, size_t errlen);
int32_t dfx_compile_expr(const dfx_expr_node* nodes, int32_t n_nodes, int32_t root,
                         const struct ArrowSchema* input_schema, dfx_runtime_expr** out, char* err,
                         size_t errlen);
const char* dfx_runtime_expr_name(const dfx_runtime_expr* e); /* RuntimeExpr::get_name */
int32_t dfx_runtime_expr_type(const dfx_runtime_expr* e);     /* RuntimeExpr::get_type -> dfx_dtype */
int32_t dfx_runtime_expr_is_aggregate(const dfx_runtime_expr* e);
void dfx_runtime_expr_free(dfx_runtime_expr* e);

/* ------------------------------------------------------------------------------------------
 * Operators.  Each consumes (takes ownership of) an input stream and fills `out` with the
 * operator's own stream; out->release frees the whole sub-tree, like dropping the
 * Rc<RefCell<Relation>>.  When `input` is itself a stream produced by this library the operators
 * are chained on the device (no host round trip) and Filter feeding Aggregate is fused into one
 * kernel.  The runtime exprs are borrowed for the duration of the call only.
 * ---------------------------------------------------------------------------------------- */

/* replaces FilterRelation::new(input, expr, schema) + impl Relation (src/execution/filter.rs:36-77)
 * and fn filter (filter.rs:79-110). */
int32_t dfx_filter_relation_new(struct ArrowArrayStream* input, const dfx_runtime_expr* expr,
                                const struct ArrowSchema* schema, struct ArrowArrayStream* out,
                                char* err, size_t errlen);

/* replaces ProjectRelation::new(input, expr, schema) + impl Relation (src/execution/projection.rs:36-71). */
int32_t dfx_project_relation_new(struct ArrowArrayStream* input, const dfx_runtime_expr* const* exprs,
                                 int32_t n_exprs, const struct ArrowSchema* schema,
                                 struct ArrowArrayStream* out, char* err, size_t errlen);

/* replaces AggregateRelation::new(schema, input, group_expr, aggr_expr) + impl Relation
 * (src/execution/aggregate.rs:47-61, :614-631, :703-952).  `schema` may be NULL or empty
 * (context.rs:185 passes Schema::empty()).  With a COUNT_DISTINCT or a MIN / MAX of a Utf8 column among the aggregates the
 * stream is a distinct aggregate around a plain one (one distinct set per argument; the Utf8 extrema are folded from theirs at
 * emit): more than 7 GROUP BY expressions are DFX_NOT_IMPLEMENTED here, a MIN / MAX of Utf8 declared with another return type is
 * DFX_INTERNAL_ERROR here, and the partial / exchange calls below on such a stream are DFX_NOT_IMPLEMENTED (distinct counts do
 * not add across ranks; the extrema's dictionary ids are rank-local). */
int32_t dfx_aggregate_relation_new(const struct ArrowSchema* schema, struct ArrowArrayStream* input,
                                   const dfx_runtime_expr* const* group_exprs, int32_t n_group,
                                   const dfx_runtime_expr* const* aggr_exprs, int32_t n_aggr,
                                   struct ArrowArrayStream* out, char* err, size_t errlen);

/* Per-operator options.  The reference's operators take no tuning knobs; this library's strategy switches (dfx_set_option
 * below, process-wide defaults kept for benchmarks and debugging) can also be given to ONE operator: it starts from the
 * process defaults as they are when it first runs, applies `options` on top, and is not affected by later dfx_set_option
 * calls.  Keys are the ones dfx_set_option documents ("agg.strategy", "scan.fast", "filter.single_pass", ...); an unknown
 * key is DFX_GENERAL.  No global mutable state is involved (thread-confined handles). */
typedef struct dfx_option {
  const char* key;
  int64_t value;
} dfx_option;
int32_t dfx_filter_relation_new_with_options(struct ArrowArrayStream* input, const dfx_runtime_expr* expr,
                                             const struct ArrowSchema* schema, const dfx_option* options, int32_t n_options,
                                             struct ArrowArrayStream* out, char* err, size_t errlen);
int32_t dfx_aggregate_relation_new_with_options(const struct ArrowSchema* schema, struct ArrowArrayStream* input,
                                                const dfx_runtime_expr* const* group_exprs, int32_t n_group,
                                                const dfx_runtime_expr* const* aggr_exprs, int32_t n_aggr,
                                                const dfx_option* options, int32_t n_options,
                                                struct ArrowArrayStream* out, char* err, size_t errlen);

/* ------------------------------------------------------------------------------------------
 * HBM-resident tables: the in-memory DataSource (src/execution/datasource.rs:27-30 trait
 * DataSource; relation.rs:34-54 DataSourceRelation).  A table is uploaded (or generated) once
 * into HBM and can be scanned many times; the scan is a library stream, so operators stacked on
 * it never leave the device.
 * ---------------------------------------------------------------------------------------- */
typedef struct dfx_table dfx_table;

/* Drain `input` (host Arrow batches), copy every column to HBM. Consumes the stream. */
int32_t dfx_table_from_stream(struct ArrowArrayStream* input, dfx_table** out, char* err,
                              size_t errlen);

/* Synthetic column generators (deterministic per (seed, column id, global row index); the CPU
 * oracle reproduces any slice -- SURVEY.md section 8(d)). */
typedef enum dfx_synth_kind {
  DFX_SYNTH_F64_UNIFORM = 0, /* p0 + p1 * u,  u in [0,1) 53-bit          (dtype Float64) */
  DFX_SYNTH_F64_EXACT = 1,   /* m * 2^-S, m uniform integer in [0,2^B): B = p0 (0: 20), S = p1 (0: 10)  (dtype Float64) */
  DFX_SYNTH_I64_UNIFORM = 2, /* uniform integer in [0, (int64)p0)          (dtype Int64)   */
  DFX_SYNTH_I64_ZIPF = 3,    /* floor(p0 ^ u) - 1 clipped to [0,p0): log-uniform skew (dtype Int64) */
  DFX_SYNTH_I32_UNIFORM = 4, /* uniform integer in [0, (int32)p0): the same draw as I64_UNIFORM, stored in 4 bytes (dtype Int32) */
  DFX_SYNTH_I64_WIDE = 5     /* (u + 1) * 0x9E3779B97F4A7C15 mod 2^64 with u the I64_UNIFORM draw in [0, (int64)p0): p0 distinct keys
                              * spread over all of Int64 -- hashed ids, both signs, (almost) none below 2^32 (dtype Int64).  The
                              * reference takes any Int64 key (aggregate.rs:807-852) */
} dfx_synth_kind;
/* Nulls: `kind | (permille << 8)` gives the column a validity bitmap in which a row is NULL with probability permille / 1000
 * (1 .. 1000), decided by a draw of its own -- DFX_SYNTH_NULL_STREAM mixed into the column id -- so the values under the null
 * slots are ordinary values: grouped aggregates read value(row) without a null check (aggregate.rs:561-603). */
#define DFX_SYNTH_KIND(k) ((k) & 0xFF)
#define DFX_SYNTH_NULL_PERMILLE(k) (((k) >> 8) & 0x3FF)
#define DFX_SYNTH_NULL_STREAM 0x4E554C4C
typedef struct dfx_synth_column {
  const char* name;
  int32_t kind;      /* dfx_synth_kind, optionally | (null permille << 8) */
  int32_t column_id; /* stream id mixed into the generator */
  double p0, p1;
} dfx_synth_column;
int32_t dfx_table_synth(const dfx_synth_column* cols, int32_t n_cols, uint64_t seed,
                        int64_t row_begin, int64_t n_rows, dfx_table** out, char* err,
                        size_t errlen);

int64_t dfx_table_num_rows(const dfx_table* t);
int32_t dfx_table_num_columns(const dfx_table* t);
/* Raw device pointer of a column's values buffer (for torch/RCCL plumbing and debugging). */
const void* dfx_table_column_device_ptr(const dfx_table* t, int32_t column);

/* DataSourceRelation over a resident table: yields slices of `batch_rows` rows (<=0: one batch).
 * The table must outlive the stream. */
int32_t dfx_table_scan_new(const dfx_table* t, int64_t batch_rows, struct ArrowArrayStream* out,
                           char* err, size_t errlen);
/* ... over the rows [row_begin, row_begin + n_rows) of the table only (row_begin a multiple of 64: slices stay
 * byte-aligned in every bitmap; n_rows < 0: to the end).  A partition of a resident table as a DataSource of its own
 * (relation.rs:34-54 wraps whatever DataSource it is given): what bench.py uses to check the last rows of the
 * 10^10-row table -- row indices beyond 2^32 -- against the oracle. */
int32_t dfx_table_scan_range_new(const dfx_table* t, int64_t row_begin, int64_t n_rows, int64_t batch_rows,
                                 struct ArrowArrayStream* out, char* err, size_t errlen);
void dfx_table_free(dfx_table* t);

/* ------------------------------------------------------------------------------------------
 * CSV data source.  replaces CsvDataSource::new(filename, schema, batch_size) + impl DataSource
 * (src/execution/datasource.rs:33-58; wrapped by DataSourceRelation, relation.rs:34-54).  As in the
 * reference the arrow csv reader is created with has_headers = true: the FIRST RECORD IS ALWAYS
 * CONSUMED AS A HEADER.  The text is copied to HBM once; record boundaries, cell conversion
 * (Rust `str::parse` semantics, correctly rounded floats) and Utf8 extraction run on the device,
 * batch_size records per get_next().  Errors: a missing file is the reference's unwrap() panic
 * (DFX_INTERNAL_ERROR); a cell that does not parse is DFX_ARROW_ERROR "Error while parsing value
 * {cell} at line {n}"; a record with a different field count than the first is DFX_ARROW_ERROR.
 * The stream is a library stream: operators stacked on it never leave the device.
 * ---------------------------------------------------------------------------------------- */
int32_t dfx_csv_datasource_new(const char* filename, const struct ArrowSchema* schema, int64_t batch_size,
                               struct ArrowArrayStream* out, char* err, size_t errlen);

/* ------------------------------------------------------------------------------------------
 * Parquet data source.  The executor of DataSourceMeta::ParquetFile { filename, schema, projection } (src/execution/
 * datasource.rs:87-92; `STORED AS PARQUET`, dfparser.rs:177-178), which the reference declares and never runs.  Deviation D12,
 * parity unpinned; the contract is pyarrow's reader: the concatenated batches equal pyarrow.parquet.read_table bit for bit.
 *   schema      from the file ("a Parquet file that contains schema information"): names, Arrow types, nullable = the field is
 *               `optional`.  projection == NULL: every leaf column in file order; otherwise the named columns in the given order
 *               (an index out of range is DFX_INVALID_COLUMN).
 *   batches     a row group is decoded as a whole on the device, when the first get_next() needs it (so a consumer's projection
 *               push-down has been heard: the chunks of columns nobody reads are neither read from the file nor copied).
 *               batch_size <= 0: one batch per row group; > 0: zero-copy slices of batch_size rows rounded up to a multiple of
 *               64, the last of a row group short.  A batch never spans row groups; a row group of 0 rows yields none.
 *   subset      flat schemas (required / optional leaves under the root); BOOLEAN, INT32 (+ Int(8/16/32, s/u) by truncation), INT64
 *               (+ Int(64, s/u)), FLOAT, DOUBLE, BYTE_ARRAY annotated String; codec UNCOMPRESSED or LZ4_RAW (codec 7; its pages are
 *               inflated on the device); dictionary pages, data pages V1 and V2; PLAIN, RLE_DICTIONARY / PLAIN_DICTIONARY, RLE Booleans; a chunk
 *               that falls back from its dictionary to PLAIN pages.  Anything else is DFX_NOT_IMPLEMENTED at construction, naming
 *               the column and the thing -- also for a column the projection leaves out: the subset is a property of the file.
 *   errors      a missing or unreadable file is DFX_IO_ERROR; a file that is not Parquet or is damaged (magic, footer length,
 *               thrift overrunning its buffer, extents beyond the file or chunk, value counts that do not add up, a run overrunning
 *               its page, a malformed compressed block, a dictionary index beyond the dictionary, a string length overrunning its page) is DFX_PARSER_ERROR
 *               saying what and where; no device is DFX_EXECUTION_ERROR (there is no host decoding path).
 * The stream is a library stream: operators stacked on it never leave the device.
 * ---------------------------------------------------------------------------------------- */
int32_t dfx_parquet_datasource_new(const char* filename, const int32_t* projection, int32_t n_projection, int64_t batch_size,
                                   struct ArrowArrayStream* out, char* err, size_t errlen);

/* ------------------------------------------------------------------------------------------
 * CSV writer.  The executor of PhysicalPlan::Write { plan, filename, kind } -- "execute a logical plan and write the output
 * to a file" (src/execution/physicalplan.rs:24-29) -- which the reference declares and never runs; kind = CSV.  A sink: it
 * consumes `input` to its end (a stream of this library stays on the device, a foreign stream is uploaded like any operator
 * input), formats every batch as text on the device and writes `filename`.  rows_out / bytes_out (may be NULL): rows written,
 * bytes of the file (header included).  Deviation D11, parity unpinned (arrow 0.12 has no csv writer); the contract is the
 * library's own reader: the file read back by dfx_csv_datasource_new with the same schema gives the same rows bit for bit.
 *   layout    one header record with the field names (the reader always consumes the first record), one record per row,
 *             delimiter ',', terminator '\n' also after the last record
 *   integers  plain decimal, '-' for negatives;  Boolean  true / false
 *   floats    the shortest digits that parse back to the same bits IN THE COLUMN'S WIDTH (the closest such), laid out as Rust's
 *             {:?}: positional with at least one digit after the point for 1e-4 <= |x| < 1e16 and zero (1.0 0.1 -0.0), else
 *             d[.ddd]e[-]x (1e16 1.5e-5 5e-324); NaN, inf, -inf.  A Float64 cell is at most 24 bytes, a Float32 cell 19
 *   Utf8      the bytes as they are, quoted iff the cell holds ',' '"' CR or LF, every '"' doubled inside quotes; header names alike
 *   nulls     an empty cell;  a file of ONE column writes an empty cell as "" (the reader skips blank lines)
 *   exceptions to the round trip: a null Utf8 slot comes back as the empty string (the reader never produces Utf8 nulls);
 *             every NaN payload comes back as one NaN
 * `options`: none is defined, any key is DFX_GENERAL.  Errors: a path that cannot be created or written is DFX_IO_ERROR, a
 * column type outside Boolean .. Utf8 is DFX_NOT_IMPLEMENTED naming the type, no device is DFX_EXECUTION_ERROR (there is no
 * host formatting path).  The text goes to `filename` + ".dfx-partial" and is renamed at the end: a failed call leaves
 * nothing under the final name.
 * ---------------------------------------------------------------------------------------- */
int32_t dfx_csv_write(struct ArrowArrayStream* input, const char* filename, const dfx_option* options, int32_t n_options,
                      int64_t* rows_out, int64_t* bytes_out, char* err, size_t errlen);

/* ------------------------------------------------------------------------------------------
 * Parquet writer.  The same sink with kind = Parquet: PhysicalPlan::Write { plan, filename, kind } (src/execution/physicalplan.rs:24-29)
 * with FileType::Parquet beside CSV (dfparser.rs:31-36), which the reference declares and never runs.  It consumes `input` to its end
 * (a stream of this library stays on the device, a foreign stream is uploaded like any operator input), encodes every page body on
 * the device and writes `filename`.  rows_out / bytes_out (may be NULL): rows written, bytes of the file.  Deviation D13, parity
 * unpinned.  The contract: what it writes, pyarrow reads back as the table that went in, bit for bit (names, types, field
 * nullability, nulls, values by bit pattern: NaN payloads, -0.0 and null Utf8 slots included), and so does
 * dfx_parquet_datasource_new.
 *   format    PAR1; a flat schema, one leaf per input column, in order, with the input's names; a field the input schema flags
 *             nullable is OPTIONAL, else REQUIRED.  Codec UNCOMPRESSED, data pages V1, encoding PLAIN (dictionary pages and
 *             RLE_DICTIONARY data pages only under the "dictionary" option, below), no page CRC, no page index; chunk statistics
 *             carry null_count only; created_by names the library
 *   types     Boolean -> BOOLEAN;  Int8 .. Int32, UInt8 .. UInt32 -> INT32 with Int(bits, signed) and the matching converted type,
 *             values sign / zero extended to 4 bytes;  Int64 -> INT64;  UInt64 -> INT64 with Int(64, false);  Float32 -> FLOAT;
 *             Float64 -> DOUBLE;  Utf8 -> BYTE_ARRAY annotated String / UTF8
 *   levels    OPTIONAL columns: the V1 block {u32 length}{RLE / bit-packed hybrid, width 1} holding exactly ONE run per page: an RLE
 *             run of 1 when every row of the page is valid, an RLE run of 0 when none is, else one bit-packed run of ceil(n / 8)
 *             groups with zero padding bits -- by the page's own non-null count.  REQUIRED columns have no level block
 *   geometry  the input's rows are cut into row groups of exactly "row_group_rows" rows (the last shorter; a batch that crosses a
 *             boundary is split there); inside a group the rows of each batch are cut into pages of "page_rows" rows (the last
 *             shorter): a page never holds rows of two batches.  Zero rows: a valid file with the schema and no row group
 *   dictionary  "dictionary" = N > 0: every non-Boolean column chunk (row group and column) starts dictionary-encoded, its
 *             dictionary built on the device: keyed on the STORED bit pattern (fixed width: the widened value -- NaN payloads are
 *             entries of their own, -0.0 and +0.0 are two; Utf8: the bytes; null slots contribute nothing), ids in order of first
 *             occurrence in the chunk's row order.  The dictionary page is the chunk's first page (PageHeader type DICTIONARY_PAGE,
 *             DictionaryPageHeader { num_values = entries, encoding PLAIN }; the entries in id order: stored width each, LE32 length +
 *             bytes for Utf8; dictionary_page_offset set, data_page_offset the first data page, encodings PLAIN, RLE,
 *             RLE_DICTIONARY, total sizes with the dictionary page).  A dictionary data page (V1, RLE_DICTIONARY): the level block
 *             as above, one byte w, then ONE run over the page's nn non-null values: nothing when nn == 0; an RLE run when all its
 *             indices are equal (varint(nn << 1), the index in ceil(w / 8) bytes); else one bit-packed run (varint(ceil(nn / 8) << 1
 *             | 1), ceil(nn / 8) * w bytes, LSB first, padding bits zero).  w = max(1, bits(max(E, 1) - 1)), E the chunk's entries
 *             after the launch that holds the page.  The unit of decision is the LAUNCH -- the rows of one batch inside one row
 *             group, at most 2^20 of them (a whole number of pages; one page where page_rows is larger): a launch that would take the
 *             dictionary beyond N entries, or its body to 2^31 - 1 bytes, turns the chunk PLAIN from that launch to its end (the
 *             dictionary pages already held stay; a chunk that falls back in its first launch is byte for byte the chunk written
 *             without the option).  A new row group starts every column with an empty dictionary.  Boolean columns stay PLAIN
 *   compression  "compression" = 7 (LZ4_RAW): every column chunk carries codec 7 and every page body -- data pages stay V1, so the
 *             level block and the values together; under "dictionary" the dictionary page and the index pages as well -- is ONE raw
 *             LZ4 block (no frame, no length prefix), packed on the device by the rule of csrc/dfx_parquet_lz4_enc.hpp, which is
 *             deterministic: a file is byte for byte what the sequential host encoder of that header writes.  V1 has no "stored"
 *             form: a page that does not shrink is still a valid block (the reader accepts it: its header pass counts such pages as oversized_v1_pages); an
 *             empty body (the dictionary of an all-null chunk) is the one-byte block {0x00}.  PageHeader carries both sizes;
 *             ColumnMetaData's total_uncompressed_size and total_compressed_size both include the page headers
 * `options`: "row_group_rows" (default 2^20, any value >= 1), "page_rows" (default 2^15; a multiple of 64, 64 .. 2^30), "dictionary"
 * (default 0: PLAIN pages only, files byte for byte what they are without the key; 1 .. 2^20: the most entries of a chunk's
 * dictionary), "dictionary_hash_bits" (debug; 1 .. 64, default 64: the device's hash of a Utf8 value is cut to that many bits, so
 * that a test can make two strings collide and see the chunk fall back to PLAIN; means nothing without "dictionary"); "dictionary" > 0
 * takes "page_rows" of at most 2^20 (the dictionary kernels keep a word per row and column of a launch); "compression" (a Parquet
 * codec id; default 0, UNCOMPRESSED: nothing new runs and files are byte for byte what they are without the key; 7: LZ4_RAW; any other
 * value -- SNAPPY, GZIP, BROTLI, ZSTD, the deprecated LZ4 -- is refused: they are not written); any other key
 * or value is DFX_GENERAL naming the key, before a device is asked for.  Errors: a column type outside Boolean .. Utf8 is DFX_NOT_IMPLEMENTED naming the column and the type,
 * before a file exists and before a device is asked for; no device is DFX_EXECUTION_ERROR (there is no host encoding path); a path
 * that cannot be created or written is DFX_IO_ERROR; a REQUIRED field whose batch arrives with nulls is DFX_EXECUTION_ERROR naming
 * the column; a page body of 2^31 - 1 bytes or more is DFX_EXECUTION_ERROR (the page header's sizes are i32), and so is, under
 * "compression" = 7, a body whose block's bound, n + n / 255 + 16, exceeds 2^31 - 1.  The bytes go to
 * `filename` + ".dfx-partial" and are renamed at the end: a failed call leaves nothing under either name.
 * ---------------------------------------------------------------------------------------- */
int32_t dfx_parquet_write(struct ArrowArrayStream* input, const char* filename, const dfx_option* options, int32_t n_options,
                          int64_t* rows_out, int64_t* bytes_out, char* err, size_t errlen);

/* ------------------------------------------------------------------------------------------
 * ORDER BY / LIMIT.  The operators behind LogicalPlan::Sort { expr: [Expr::Sort { expr, asc }], input, schema } and
 * LogicalPlan::Limit { limit, input, schema } (src/logicalplan.rs:313-338), which the reference's planner emits
 * (sqlplanner.rs:142-183) and its executor leaves at unimplemented!() (context.rs:113,194): there is no reference
 * behaviour, the semantics are this library's (parity unpinned): stable sort, NULL larger than every value (last
 * when ascending, first when descending), NaN larger than every number, ONE result batch.  `exprs` are the sort
 * expressions compiled with dfx_compile_scalar_expr (the inner `expr` of Expr::Sort; compile_scalar_expr itself
 * rejects Expr::Sort like the reference, expression.rs:380-399), `ascending[i]` their direction.  Keys: any
 * fixed-width scalar expression, or a Utf8 column (byte-wise lexicographic).  LIMIT keeps the first `limit` rows.
 * ---------------------------------------------------------------------------------------- */
int32_t dfx_sort_relation_new(struct ArrowArrayStream* input, const dfx_runtime_expr* const* exprs,
                              const int32_t* ascending, int32_t n_exprs, const struct ArrowSchema* schema,
                              struct ArrowArrayStream* out, char* err, size_t errlen);
int32_t dfx_limit_relation_new(struct ArrowArrayStream* input, int64_t limit, const struct ArrowSchema* schema,
                               struct ArrowArrayStream* out, char* err, size_t errlen);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU GROUP BY exchange (no reference equivalent: the reference is single-process).
 * One process per GPU.  After draining its local input, an aggregate stream exports its partial
 * groups bucketed by hash(key) % world into one contiguous device buffer per payload word; the
 * host plumbing (torch.distributed / RCCL all-to-all) moves the buckets; the receiving side
 * imports them and merges.  Then get_next() on the stream emits the groups this rank owns.
 * ---------------------------------------------------------------------------------------- */
/* Drain the input and build the local partial table.  Fills n_words = key words + accumulator
 * words per group, and counts[world] = groups destined to each rank. */
int32_t dfx_aggregate_partial_build(struct ArrowArrayStream* agg, int32_t world, int32_t* n_words,
                                    int64_t* counts, char* err, size_t errlen);
/* Write the bucketed partials: `dst` is a device buffer of n_words * total int64 words laid out
 * word-major within each destination bucket: for rank r, bucket base = n_words * prefix(r), and
 * word w of group g of that bucket at base + w * counts[r] + g. */
int32_t dfx_aggregate_partial_export(struct ArrowArrayStream* agg, void* dst_device, int64_t dst_words,
                                     char* err, size_t errlen);
/* Replace the stream's state by the merge of `n_buckets` received buckets (same layout as
 * export: bucket b holds counts[b] groups starting at word offset n_words * prefix(b)). */
int32_t dfx_aggregate_partial_import(struct ArrowArrayStream* agg, const void* src_device,
                                     const int64_t* counts, int32_t n_buckets, char* err,
                                     size_t errlen);

/* The same exchange as ONE library call over RCCL (counts, then variable-length buckets, as
 * grouped ncclSend/ncclRecv on the library's stream; xGMI between the GPUs of a node).  One process per GPU:
 *   rank 0:      dfx_comm_unique_id(id)           -- ncclGetUniqueId; the host plumbing hands `id` to every rank
 *   every rank:  dfx_comm_init(id, world, rank)   -- ncclCommInitRank on the library's device (dfx_init)
 *   per query:   dfx_aggregate_exchange(agg, comm, stats)  then get_next() emits the groups this rank owns
 * dfx_aggregate_exchange drains the input, counts the groups per owner rank, and replaces the stream's table by the merge
 * of what it received in TWO collective rounds: one all-gather of world + 3 words per rank (its state and query shape, the
 * groups it can receive / send without allocating more, its group count per destination rank: every buffer of the second
 * round is allocated before the first), then the buckets, the last of them with a trailer word (the sender's state) --
 * one host read-back (the count matrix) plus the final synchronisation.  Only if some rank receives or holds more groups
 * than it announced do the ranks allocate again and agree in a round of their own.  Ungrouped aggregates are combined with an all-gather of the per-rank scalars (every rank then emits
 * the global row).  stats (may be NULL): [0] groups sent, [1] groups received, [2] bytes sent, [3] host synchronisations.
 * RCCL is bound at run time (dlopen librccl.so.1); without it these calls return ExecutionError.  Utf8 keys:
 * NotImplemented (dictionary ids are rank-local). */
#define DFX_COMM_ID_BYTES 128
typedef struct dfx_comm dfx_comm;
int32_t dfx_comm_unique_id(uint8_t* id /* [DFX_COMM_ID_BYTES] */, char* err, size_t errlen);
int32_t dfx_comm_init(const uint8_t* id, int32_t world, int32_t rank, dfx_comm** out, char* err, size_t errlen);
void dfx_comm_destroy(dfx_comm* comm);
/* The number of ranks the communicator ITSELF reports (ncclCommCount): what RCCL saw, not what the host asked for.
 * -1: not a communicator, or RCCL refused.  (bench.py puts it into the line's config.rccl_ranks.) */
int32_t dfx_comm_ranks(const dfx_comm* comm);
int32_t dfx_aggregate_exchange(struct ArrowArrayStream* agg, dfx_comm* comm, int64_t* stats, char* err, size_t errlen);

/* ------------------------------------------------------------------------------------------
 * Measurement hooks (used by bench.py; not part of the drop-in surface).
 * ---------------------------------------------------------------------------------------- */
/* The group hash of a single-word key (its 32 bits sit in the HIGH half: table slot = hash >> (64 - log2 capacity)) and,
 * for keys below 2^32, its inverse: the hash restricted to such keys is a bijection of the low word, which is what lets
 * the partitioned GROUP BY route 12-byte rows {hash image, operand} and turn claimed images back into keys.  Host code,
 * no GPU needed; used by the CPU tests. */
uint64_t dfx_debug_group_hash(uint64_t key);
uint32_t dfx_debug_unhash32(uint32_t image);
/* One `column <op> literal` term of a scan plan (csrc/dfx_device.hpp: DevScanPlan) evaluated on the host with the arithmetic
 * the kernels use: the range test on the order-preserving image of `value` (csrc/dfx_scan_plan.hpp: plan_term_range and
 * plan_term_passes; the entry point is in csrc/dfx_expr_program.cpp).  dtype: the column's dfx_dtype (Int32, UInt32,
 * Float32, Int64, UInt64, Float64); op: dfx_operator 0..5 (Eq NotEq Lt LtEq Gt GtEq); literal / value: canonical 64-bit
 * forms (signed ints sign-extended, unsigned zero-extended, Float32 bits in the low word, Float64 bits); is_null: the value
 * is null (arrow 0.12's rule for None decides).  Returns 0 / 1, or -1 for a type the plans do not cover.  Host code, no
 * GPU needed: the CPU tests compare it with the comparison it restates over NaN, +-0.0, +-inf and the integer extremes. */
int32_t dfx_debug_plan_term(int32_t dtype, int32_t op, uint64_t literal, uint64_t value, int32_t is_null);
/* Debug: one Utf8 string term (deviation D9, see dfx_compile_scalar_expr) over ONE value, evaluated on the host by the matcher
 * the term kernel runs per row (csrc/dfx_utf8_match.hpp).  op: DFX_OP_EQ .. DFX_OP_GT_EQ with the value on the left, DFX_OP_LIKE
 * or DFX_OP_NOT_LIKE; literal: the NUL-terminated literal / pattern; value, value_len: the value's bytes; is_null: the value is
 * null.  Returns 0 / 1, or -1 for a bad call (another operator, a null pointer, a literal of more than 4096 bytes).  No GPU needed. */
int32_t dfx_debug_utf8_term(int32_t op, const char* literal, const uint8_t* value, int64_t value_len, int32_t is_null);
/* Debug: one value formatted as dfx_csv_write formats a cell, on the host, by the code the kernel runs per cell
 * (csrc/dfx_numfmt.hpp); the twin of dfx_debug_utf8_term.  dtype DFX_BOOLEAN .. DFX_FLOAT64: `bits` is the value in its
 * canonical 64-bit form (Float32 bits in the low word; wider bits of a narrow integer are ignored), the cell is written to
 * buf.  dtype DFX_UTF8: buf holds the value's bytes on entry, `bits` is their number (bit 63 set: the file has one column,
 * so an empty cell is written ""), and the cell replaces them.  Returns the cell's length (a NUL follows if there is room),
 * or -1 for a bad call (another dtype, a null or too small buffer).  No GPU needed. */
int32_t dfx_debug_format_value(int32_t dtype, uint64_t bits, char* buf, size_t buflen);
/* Pulls every batch of a library stream and drops it on the device: no host RecordBatch, no D2H copy (what a stacked
 * operator would see).  rows / batches (may be NULL): what came out. */
int32_t dfx_relation_drain_device(struct ArrowArrayStream* stream, int64_t* rows, int64_t* batches, char* err, size_t errlen);
/* Test hook: the Arrow bitmap (LSB first) a FilterRelation computed for its most recent input batch -- the BooleanArray of
 * the reference's predicate closure (filter.rs:53-66), which the operator itself never hands out.  out == NULL: start
 * keeping it (call before next()); else copies (rows + 7) / 8 bytes to `out` (host memory). */
int32_t dfx_filter_debug_mask(struct ArrowArrayStream* filter_stream, uint8_t* out, int64_t out_bytes, int64_t* rows, char* err, size_t errlen);
/* When enabled every tracked kernel launch is bracketed by HIP events on its launch stream. */
int32_t dfx_profile_enable(int32_t on);
int32_t dfx_profile_reset(void);
/* Number of distinct kernels recorded so far; then per index: name, launches, total ms,
 * algorithmic bytes the launches covered. */
int32_t dfx_profile_count(void);
int32_t dfx_profile_get(int32_t index, char* name, size_t namelen, int64_t* launches,
                        double* total_ms, double* algo_bytes);

/* EXPLAIN of an operator tree created by this library: one line per operator, children indented by two spaces --
 * what was fused (a Filter under an Aggregate), how large the fused program is and which kernel family will run it
 * (a compile-time shape signature, the run-time decoded shape family, the SSA interpreter).  Host state only: works
 * before the first get_next and without a GPU.  (The reference prints its logical plan upstream of this boundary,
 * context.rs:105; this is the physical counterpart.)  Writes at most buflen - 1 bytes + NUL; returns the full length,
 * or -1 if `stream` was not produced by this library. */
int64_t dfx_relation_explain(struct ArrowArrayStream* stream, char* buf, size_t buflen);

/* Tunables (bench/test only; process-wide, read when an operator is created or a batch is launched).
 * Returns DFX_GENERAL for an unknown key.  Keys:
 *   "agg.strategy"           0 auto (calibrated on the first rows of a stream), 1 global-atomic table only,
 *                            2 LDS front cache, 3 partitioned (route rows to table blocks, aggregate blocks in LDS)
 *   "agg.capacity_log2"      initial GROUP BY table slots (0: 2^21)
 *   "agg.lds_slots" / "agg.lds_copies"   LDS front cache geometry (-1 auto)
 *   "agg.fewgroup"           1: <= 8 groups run on register accumulators (default), 0: LDS front cache
 *   "agg.partition_mode"     pass 1 of the partitioned strategy: 2 lock-free LDS rings (default), 1 LDS counting sort,
 *                            0 direct routing; "agg.partition_block", "agg.partition_pad", "agg.partition_cap_rows"
 *   "agg.replay_in_place"    experimental, default 0
 *   "agg.dict_capacity_log2" initial slots of a Utf8 key dictionary (0: 2^16)
 *   "filter.single_pass"     FilterRelation: 1 one kernel per batch (predicate, bitmap, look-back, compaction; default), 0 mask ->
 *                            scan -> compaction;  "filter.dense": the single-pass kernel's flavour that keeps a tile in registers
 *                            (one read of the column however many rows pass): -1 once the stream has kept > 22 % of a batch
 *                            (default), 0 never, 1 whenever the shape allows (one Float64 predicate column)
 *   "scan.fast"              0: always the generic SSA interpreter instead of the shape-specialised kernels
 *   "scan.plan"              scan plans (run-time query shapes evaluated as data: range tests on value images, 4-byte columns
 *                            widened, nulls by arrow's comparison rule): 1 wherever the shape is covered and no compile-time
 *                            signature matches (default), 0 never (round 3's dispatch), 2 also instead of the signatures
 *   "host.stream"            how HOST Arrow batches reach HBM (also a per-operator option: the first operator above a host
 *                            source decides): 0 pageable copies in order on the library's stream, the producer's array
 *                            released after the stream has passed them (default: 0.85 of the link, the fastest form measured);
 *                            1 pinned staging ring filled by library threads, DMA on a copy stream, the array released when its
 *                            bytes have been copied out; 2 one batch ahead on a copy stream; 3 = 2 + large buffers page-locked
 *                            in place.  "host.stage_threads" (8), "host.stage_mb" (16: bytes per pinned slot),
 *                            "host.stage_slots" (6) size the ring of form 1
 *   "pool.trim"              (any value) return the cached device buffers to the driver */
int32_t dfx_set_option(const char* key, int64_t value);
/* Measurement counters: "h2d_bytes" (column bytes the uploaders copied host -> device), "h2d_staged_bytes" (of which through
 * the pinned staging ring), "csv_cells" (cells the CSV source converted) -- what projection push-down saves, "csv_tiles" / "csv_general_tiles"
 * (64-record tiles converted by the CSV source / those that took the per-lane walk instead of the wave-cooperative path).  -1: unknown name.
 * "csv_write_cells" / "csv_write_bytes" / "csv_write_general_tiles" (dfx_csv_write: cells formatted, bytes of text written, 64-row
 * tiles whose text did not fit the LDS window and took the lane-per-row path).
 * Transitions of the grouped aggregate's strategy state machine (they observe only; tests/test_gpu_agg_state_machine.py asserts that
 * its streams reach every one of them):
 *   "agg_calibrations"            calibration slices run (first 2^18 rows of a first batch of more than 2^21 rows)
 *   "agg_memo_decisions"          strategy decisions taken from a resident table's memo instead of a slice
 *   "agg_calibration_replays"     slices that overflowed the table: grown / replayed before the decision read the group count
 *   "agg_growths"                 tables rebuilt larger (rehash + replay of the spill list)
 *   "agg_replays_in_place"        spill lists replayed into the table as it was (overflowing routing regions, no growth)
 *   "agg_narrow_to_wide"          streams that left the 12-byte routed rows: a key without a 32-bit image after a narrow decision
 *   "agg_pair_launches", "agg_plane_launches", "agg_shared_operand_launches"   pass-1 launches of the pair / plane / shared rows
 *   "agg_pair_fallbacks"          streams that left the pair scan (or the planes) for one scan per aggregate ...
 *   "agg_pair_fallbacks_pending"  ... of which with a deferred window still to aggregate
 *   "agg_pass2_launches", "agg_deferred_windows"   pass-2 launches / those over more than one pass-1 launch
 *   "agg_held_runs"               runs of every chunk of accumulators over the held batches (agg.chunk_hold)
 *   "agg_fewgroup_launches"       launches of the register-accumulator kernel (at most 8 groups known)
 *   "agg_hot_key_launches"        pass-1 launches that kept heavy keys in LDS
 *   "agg_unfused_batches"         batches filtered for real because of nulls under the absorbed predicate
 *   "distinct_set_growths", "distinct_spill_rows"  COUNT(DISTINCT) sets rehashed into larger ones / rows replayed from their spill lists
 * ORDER BY / LIMIT (they observe only; tests/test_gpu_sort_cases.py):
 *   "sort_passes_run", "sort_passes_skipped"   radix passes launched / digits found constant over the input and skipped
 *   "sort_topk_selects"           ORDER BY ... LIMIT k queries whose candidates were radix-selected by the first key
 * Parquet source (they observe only; tests/test_gpu_parquet.py):
 *   "parquet_chunk_bytes"         bytes of column chunks copied to the device -- what projection push-down saves
 *   "parquet_pages"               pages walked by the host (dictionary pages included)
 *   "parquet_dict_pages", "parquet_plain_pages"   data pages whose values are dictionary indices / PLAIN values
 *   "parquet_rle_runs", "parquet_bitpacked_runs"  runs of the RLE / bit-packed hybrid the kernels walked (levels, indices, RLE Booleans)
 *   "parquet_host_walked_strings" length prefixes of PLAIN byte arrays the host chased (dictionary pages always, PLAIN data pages)
 * Parquet writer (they observe only; tests/test_gpu_parquet_write.py):
 *   "parquet_write_pages", "parquet_write_row_groups"   data pages / row groups written
 *   "parquet_write_bytes"         bytes of the files written
 *   "parquet_write_rle_level_pages", "parquet_write_bitpacked_level_pages"   pages of OPTIONAL columns whose definition levels are
 *                                 one RLE run (every row valid, or none) / one bit-packed run (valid and null rows)
 *   "parquet_write_dict_pages", "parquet_write_dict_entries"   "dictionary" > 0 (tests/test_gpu_parquet_dict_write.py): dictionary
 *                                 pages written / the entries they hold ("parquet_write_pages" keeps counting data pages only)
 *   "parquet_write_dict_index_pages", "parquet_write_dict_rle_index_pages"   data pages of dictionary indices / of them, pages whose
 *                                 indices are one RLE run (all equal)
 *   "parquet_write_dict_fallback_chunks"   chunks that left dictionary mode for PLAIN, a fallback in the first launch included
 *   "parquet_write_lz4_pages", "parquet_write_lz4_bytes_in", "parquet_write_lz4_bytes_out", "parquet_write_lz4_sequences"
 *                                 "compression" = 7 (tests/test_gpu_parquet_lz4_write.py): page bodies packed into LZ4 blocks on the
 *                                 device, dictionary pages included / their bytes / the blocks' bytes / the blocks' sequences */
int64_t dfx_counter_get(const char* name);
void dfx_counter_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* DFX_H */
