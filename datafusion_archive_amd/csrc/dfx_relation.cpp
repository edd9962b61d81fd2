// dfx_relation.cpp -- what the operator units share (dfx_filter.cpp, dfx_project.cpp, dfx_aggregate*.cpp, dfx_distinct_emit.cpp):
// the control block's error word, a small upload, the byte count of a fused program's input, the option list of a
// *_new_with_options call.
#include "dfx_relation.hpp"

namespace dfx {

Status error_from_ctrl(uint32_t bits) {
  if (bits & 1u) return Status::Err(DFX_ARROW_ERROR, "DivideByZero");  // arrow 0.12 array_ops::divide
  if (bits & 2u) return Status::Err(DFX_INTERNAL_ERROR, "attempt to divide with overflow");
  if (bits & 4u) return Status::Err(DFX_INTERNAL_ERROR, "partitioned aggregation: LDS ring stalled");
  if (bits & 8u) return Status::Err(DFX_INTERNAL_ERROR, "single-pass filter: look-back stalled");
  if (bits & PQ_ERR_INFLATE) return Status::Err(DFX_PARSER_ERROR, "Parquet: the compressed block of a page is malformed");
  if (bits & PQ_ERR_RUN) return Status::Err(DFX_PARSER_ERROR, "Parquet: a run of a page's levels or values overruns the page");
  if (bits & PQ_ERR_DICT_INDEX) return Status::Err(DFX_PARSER_ERROR, "Parquet: a dictionary index is beyond the dictionary");
  if (bits & PQ_ERR_VALUE) return Status::Err(DFX_PARSER_ERROR, "Parquet: a page holds fewer values than its non-null rows");
  return Status::OK();
}

Status alloc_zeroed_ctrl(std::shared_ptr<void>* ctrl) {
  Status st;
  *ctrl = device_alloc(sizeof(uint32_t) * CTRL_WORDS, &st);
  if (!*ctrl) return st;
  DFX_HIP(hipMemsetAsync(ctrl->get(), 0, sizeof(uint32_t) * CTRL_WORDS, ctx().stream));
  return Status::OK();
}

Status clear_ctrl_error(const std::shared_ptr<void>& ctrl, uint32_t bits, hipStream_t s) {
  DFX_HIP(hipMemsetAsync(ctrl.get(), 0, sizeof(uint32_t) * CTRL_WORDS, s));
  return error_from_ctrl(bits);
}

Status take_ctrl_error(const std::shared_ptr<void>& ctrl, hipStream_t s) {
  uint32_t errbits = 0;
  DFX_HIP(hipMemcpyAsync(&errbits, (uint32_t*)ctrl.get() + CTRL_ERROR, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  DFX_HIP(hipStreamSynchronize(s));
  return errbits ? clear_ctrl_error(ctrl, errbits, s) : Status::OK();
}

Status upload_small(const void* host, size_t bytes, std::shared_ptr<void>* dev) {
  Status st;
  *dev = device_alloc(std::max<size_t>(bytes, 8), &st);
  if (!*dev) return st;
  DFX_HIP(hipMemcpyAsync(dev->get(), host, bytes, hipMemcpyHostToDevice, ctx().stream));
  DFX_HIP(hipStreamSynchronize(ctx().stream));
  return Status::OK();
}

double program_input_bytes(const ProgramBuilder& builder, const DeviceBatch& batch, int64_t n) {
  double bytes = 0;
  for (int ci : builder.columns()) bytes += (double)n * (batch.columns[ci].dtype == DFX_BOOLEAN ? 0.125 : dtype_width(batch.columns[ci].dtype));
  return bytes;
}

Status parse_option_overrides(const dfx_option* options, int32_t n_options, OptionOverrides* overrides) {
  AggOptions probe = agg_options();  // a copy: only asked whether it knows the key
  for (int i = 0; i < n_options; ++i) {
    if (!options[i].key || !set_option_in(probe, options[i].key, options[i].value))
      return Status::Err(DFX_GENERAL, std::string("unknown option ") + (options[i].key ? options[i].key : "(null)"));
    overrides->emplace_back(options[i].key, options[i].value);
  }
  return Status::OK();
}

}  // namespace dfx
