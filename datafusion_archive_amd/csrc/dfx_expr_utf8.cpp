// dfx_expr_utf8.cpp -- Utf8 string terms of a predicate (deviation D9, stated at the top of dfx_expr.cpp): which nodes are
// string terms, one term compiled into its class and segment table, and Utf8Terms: the pass that rewrites each term of a
// predicate into a virtual Boolean column and launches its kernel (dfx_k_utf8pred.hip) per batch.
#include <string.h>

#include "dfx_host.hpp"
#include "dfx_kernels.hpp"

namespace dfx {

bool utf8_string_term(const std::vector<dfx_expr_node>& nodes, int32_t idx, const SchemaInfo& schema, bool* col_left) {
  if (idx < 0 || idx >= (int32_t)nodes.size()) return false;
  const dfx_expr_node& n = nodes[idx];
  if (n.kind != DFX_EXPR_BINARY) return false;
  const bool cmp = n.op >= DFX_OP_EQ && n.op <= DFX_OP_GT_EQ, like = n.op == DFX_OP_LIKE || n.op == DFX_OP_NOT_LIKE;
  if (!cmp && !like) return false;
  if (n.left < 0 || n.left >= (int32_t)nodes.size() || n.right < 0 || n.right >= (int32_t)nodes.size()) return false;
  auto is_col = [&](const dfx_expr_node& c) {
    return c.kind == DFX_EXPR_COLUMN && c.column >= 0 && c.column < (int32_t)schema.fields.size() && schema.fields[c.column].dtype == DFX_UTF8;
  };
  auto is_lit = [&](const dfx_expr_node& c) { return c.kind == DFX_EXPR_LITERAL && c.dtype == DFX_UTF8; };
  const dfx_expr_node &l = nodes[n.left], &r = nodes[n.right];
  if (is_col(l) && is_lit(r)) {
    if (col_left) *col_left = true;
    return true;
  }
  if (cmp && is_lit(l) && is_col(r)) {  // LIKE takes the column on the left and the pattern on the right only
    if (col_left) *col_left = false;
    return true;
  }
  return false;
}

Status utf8_compile_term(int op, const char* literal, size_t len, Utf8Term* t, std::vector<uint8_t>* image) {
  if (len > kUtf8MaxLiteral)
    return Status::Err(DFX_NOT_IMPLEMENTED, strfmt("Utf8 literal of more than %u bytes in a string term", kUtf8MaxLiteral));
  memset(t, 0, sizeof(*t));
  std::vector<uint8_t> bytes;
  std::vector<Utf8Seg> segs;
  if (op >= DFX_OP_EQ && op <= DFX_OP_GT_EQ) {
    t->cls = U8_CMP;
    t->m = utf8_cmp_mask(op);
    t->if_null = utf8_cmp_if_null(t->m);
    bytes.assign(literal, literal + len);
  } else if (op == DFX_OP_LIKE || op == DFX_OP_NOT_LIKE) {
    const bool negate = op == DFX_OP_NOT_LIKE;
    bool pct = false, underscore = false;
    size_t at = 0;
    while (at <= len) {  // the `%`-separated segments; empty ones (a leading / trailing / doubled %) carry nothing
      size_t to = at;
      while (to < len && literal[to] != '%') {
        underscore = underscore || literal[to] == '_';
        ++to;
      }
      if (to > at) {
        Utf8Seg sg;
        sg.off = (uint16_t)bytes.size();
        sg.len = (uint16_t)(to - at);
        segs.push_back(sg);
        bytes.insert(bytes.end(), literal + at, literal + to);
      }
      if (to < len) pct = true;
      at = to + 1;
    }
    t->flags = (pct ? U8F_PCT : 0u) | (len > 0 && literal[0] == '%' ? U8F_LEAD : 0u) | (len > 0 && literal[len - 1] == '%' ? U8F_TRAIL : 0u);
    t->min_len = (uint32_t)bytes.size();  // (`_` is at least one byte)
    if (!pct && !underscore) {  // no wildcards: Eq / NotEq
      t->cls = U8_CMP;
      t->m = negate ? 5u : 2u;
      t->if_null = negate ? 1u : 0u;
      segs.clear();
    } else {
      t->inv = negate ? 1u : 0u;
      t->if_null = negate ? 1u : 0u;  // by analogy with Eq / NotEq
      if (!underscore && segs.size() <= 1) {
        const bool lead = (t->flags & U8F_LEAD) != 0, trail = (t->flags & U8F_TRAIL) != 0;
        t->cls = segs.empty() ? U8_PREFIX : (lead && trail) ? U8_CONTAINS : lead ? U8_SUFFIX : U8_PREFIX;  // (`%` alone: the empty prefix)
        segs.clear();
      } else {
        t->cls = U8_GENERAL;
      }
    }
  } else {
    return Status::Err(DFX_INTERNAL_ERROR, "not a string term operator");
  }
  t->lit_len = (uint32_t)bytes.size();
  t->n_segs = (uint32_t)segs.size();
  image->assign((size_t)std::max<uint32_t>(utf8_term_image_bytes(*t), 4u), 0);  // (never empty: it becomes a device buffer)
  if (!bytes.empty()) memcpy(image->data(), bytes.data(), bytes.size());
  const size_t seg_at = utf8_term_segs_at(*t);
  if (!segs.empty()) memcpy(image->data() + seg_at, segs.data(), segs.size() * sizeof(Utf8Seg));
  return Status::OK();
}

Status Utf8Terms::compile(const dfx_runtime_expr& e, const SchemaInfo& schema, int first_virt) {
  terms_.clear();
  whole_ = false;
  rw_ = e;
  if (e.is_aggregate || e.root < 0 || e.root >= (int32_t)e.nodes.size()) return Status::OK();
  std::vector<int32_t> stack{e.root};
  std::vector<int32_t> found;
  int guard = 0;
  while (!stack.empty()) {
    const int32_t at = stack.back();
    stack.pop_back();
    if (at < 0 || at >= (int32_t)e.nodes.size() || ++guard > 1 << 20) continue;
    const dfx_expr_node& n = e.nodes[(size_t)at];
    if (utf8_string_term(e.nodes, at, schema, nullptr)) {
      found.push_back(at);
      continue;
    }
    if (n.kind == DFX_EXPR_BINARY) {
      stack.push_back(n.right);
      stack.push_back(n.left);
    } else if (n.kind == DFX_EXPR_CAST) {
      stack.push_back(n.left);
    }
  }
  for (int32_t at : found) {
    const dfx_expr_node& n = e.nodes[(size_t)at];
    bool col_left = true;
    (void)utf8_string_term(e.nodes, at, schema, &col_left);
    const dfx_expr_node& c = e.nodes[(size_t)(col_left ? n.left : n.right)];
    const dfx_expr_node& l = e.nodes[(size_t)(col_left ? n.right : n.left)];
    int op = n.op;
    if (!col_left)  // literal on the left: mirror the operator (as fast_terms does)
      op = op == DFX_OP_LT ? DFX_OP_GT : op == DFX_OP_LT_EQ ? DFX_OP_GT_EQ : op == DFX_OP_GT ? DFX_OP_LT : op == DFX_OP_GT_EQ ? DFX_OP_LT_EQ : op;
    const std::string lit = l.name ? l.name : "";
    int slot = -1;
    for (size_t k = 0; k < terms_.size(); ++k)
      if (terms_[k].src_col == c.column && terms_[k].op == op && terms_[k].literal == lit) slot = (int)k;
    if (slot < 0) {
      Utf8TermSpec sp;
      sp.src_col = c.column;
      sp.op = op;
      sp.literal = lit;
      DFX_RETURN_IF_ERROR(utf8_compile_term(op, lit.data(), lit.size(), &sp.term, &sp.image));
      sp.virt_col = first_virt + (int)terms_.size();
      slot = (int)terms_.size();
      terms_.push_back(std::move(sp));
    }
    dfx_expr_node& w = rw_.nodes[(size_t)at];
    memset(&w, 0, sizeof(w));
    w.kind = DFX_EXPR_COLUMN;
    w.column = terms_[(size_t)slot].virt_col;
    w.left = w.right = -1;
  }
  rw_.rebind();
  whole_ = found.size() == 1 && found[0] == e.root;
  return Status::OK();
}

void Utf8Terms::append_fields(SchemaInfo* s) const {
  for (size_t k = 0; k < terms_.size(); ++k) {
    Field f;
    f.name = "__utf8_term_" + std::to_string(k);
    f.dtype = DFX_BOOLEAN;
    f.nullable = false;
    s->fields.push_back(f);
  }
}

bool Utf8Terms::source_has_nulls(const DeviceBatch& in) const {
  for (const Utf8TermSpec& t : terms_)
    if (t.src_col < (int)in.columns.size() && in.columns[(size_t)t.src_col].validity && in.columns[(size_t)t.src_col].null_count != 0) return true;
  return false;
}

Status Utf8Terms::eval(const DeviceBatch& in, DeviceBatch* ext) {
  if (ext != &in) {
    const size_t keep = ext->columns.size();
    if (keep < in.columns.size()) *ext = in;
    ext->num_rows = in.num_rows;
  }
  if (terms_.empty()) return Status::OK();
  DFX_RETURN_IF_ERROR(ensure_init());
  hipStream_t s = ctx().stream;
  const int64_t n = in.num_rows;
  for (Utf8TermSpec& t : terms_) {
    if (t.src_col >= (int)in.columns.size() || in.columns[(size_t)t.src_col].dtype != DFX_UTF8 || in.columns[(size_t)t.src_col].absent)
      return Status::Err(DFX_INTERNAL_ERROR, strfmt("Column at index %d is not of expected type", t.src_col));
    const DeviceColumn& src = in.columns[(size_t)t.src_col];
    Status st;
    if (!t.dev) {
      t.dev = device_alloc(t.image.size(), &st);
      if (!t.dev) return st;
      DFX_HIP(hipMemcpyAsync(t.dev.get(), t.image.data(), t.image.size(), hipMemcpyHostToDevice, s));
    }
    auto words = device_alloc(sizeof(uint64_t) * (size_t)std::max<int64_t>((n + 63) / 64, 1), &st);
    if (!words) return st;
    if (n > 0) {
      DevUtf8Pred T;
      T.t = t.term;
      T.lit = (const uint8_t*)t.dev.get();
      const uint8_t* validity = src.null_count != 0 ? src.validity : nullptr;
      DFX_HIP(launch_utf8_pred(src.offsets, src.data, validity, src.bit_offset, n, T, (uint64_t*)words.get(),
                               (double)n * 4.0 + (double)src.data_bytes + (double)n / 8.0, s));
    }
    if ((int)ext->columns.size() <= t.virt_col) ext->columns.resize((size_t)t.virt_col + 1);
    DeviceColumn& vc = ext->columns[(size_t)t.virt_col];
    vc = DeviceColumn();
    vc.dtype = DFX_BOOLEAN;
    vc.length = n;
    vc.values = words.get();
    vc.owners = {words};
  }
  return Status::OK();
}

std::string Utf8Terms::explain() const {
  static const char* cls[] = {"compare", "prefix", "suffix", "contains", "general"};
  std::string out;
  for (const Utf8TermSpec& t : terms_) {
    if (!out.empty()) out += "; ";
    out += strfmt("#%d %s %s, literal of %zu bytes", t.src_col, op_debug(t.op), t.term.cls <= U8_GENERAL ? cls[t.term.cls] : "?", t.literal.size());
    if (t.term.cls == U8_GENERAL) out += strfmt(" in %u segments", t.term.n_segs);
  }
  return out;
}

}  // namespace dfx

// a term on the host: the planner and utf8_term_eval, the function a lane of k_utf8_pred runs over its row (include/dfx.h)
extern "C" int32_t dfx_debug_utf8_term(int32_t op, const char* literal, const uint8_t* value, int64_t value_len, int32_t is_null) {
  using namespace dfx;
  const bool known = (op >= DFX_OP_EQ && op <= DFX_OP_GT_EQ) || op == DFX_OP_LIKE || op == DFX_OP_NOT_LIKE;
  if (!known || !literal || value_len < 0 || value_len > (int64_t)INT32_MAX || (!value && value_len > 0 && !is_null)) return -1;
  Utf8Term t;
  std::vector<uint8_t> image;
  if (!utf8_compile_term(op, literal, strlen(literal), &t, &image).ok()) return -1;
  if (is_null) return (int32_t)t.if_null;
  const uint8_t none = 0;
  return utf8_term_eval(t, image.data(), (const Utf8Seg*)(image.data() + utf8_term_segs_at(t)), value ? value : &none, (uint32_t)value_len) ? 1 : 0;
}
