// vfm_ops_common.hpp -- what the TORCH_LIBRARY fragments of this directory (vfm_*_ops.cpp) share: the tensor checks,
// and the parts of a session struct and of a fold-in struct that every form names alike, each checked and filled in one
// place.  Host C++ for the shim only: no .hip unit includes it.
#pragma once

#include <ATen/ATen.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <string.h>

#include "vfm_elicit.h"

namespace vfm_ops {

using at::Tensor;
using c10::optional;

inline const Tensor& dev_tensor(const Tensor& t, at::ScalarType dt, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on the GPU (vae_amd has no CPU fallback)");
  TORCH_CHECK(t.scalar_type() == dt, name, " has the wrong dtype");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  return t;
}

inline bool given(const optional<Tensor>& t) { return t.has_value() && t->defined(); }

inline void check(int rc, const char* what) {
  TORCH_CHECK(rc == 0, what, " failed (code ", rc, "): ", vfm_last_error());
}

inline void* stream_of(const Tensor& t) { return (void*)c10::hip::getCurrentHIPStream(t.get_device()).stream(); }

// ---- the parts of a session struct S (vfm_elicit_t, vfm_elicit_field_t, vfm_elicit_solve_t, vfm_elicit_bound_t,
// vfm_design_t), after VFM_STRUCT_INIT.  An op is a sequence of them plus its own scalars; the rows come first: the
// outputs and the history are sized by the U, P and F they set.

// the model's tables: T, d and the three pointers.  S: a session struct, or any struct with these five members (the
// ranking ops, whose C entry points take plain arguments, keep one of their own: vfm_rank_ops.cpp)
template <class S>
void fill_tables(S& p, const Tensor& entity, const Tensor& bias, const Tensor& scalars) {
  dev_tensor(entity, at::kFloat, "entity_params"); dev_tensor(bias, at::kFloat, "bias_params");
  dev_tensor(scalars, at::kFloat, "scalars");
  TORCH_CHECK(entity.dim() == 2 && bias.dim() == 2 && bias.size(1) == 2 && bias.size(0) == entity.size(0) &&
              entity.size(1) % 2 == 0 && scalars.numel() >= 3, "table shapes");
  p.T = entity.size(0); p.d = (int32_t)(entity.size(1) / 2);
  p.entity_params = entity.data_ptr<float>(); p.bias_params = bias.data_ptr<float>();
  p.scalars = scalars.data_ptr<float>();
}

template <class S>
void fill_workspace(S& p, const Tensor& workspace) {
  dev_tensor(workspace, at::kByte, "workspace");
  p.workspace = workspace.data_ptr();
  p.workspace_bytes = workspace.numel();
}

// the field form's rows: the ids, the pool's full rows and one operand per distinct context (pool_y NULL: the op has none)
template <class S>
void fill_field_rows(S& p, const Tensor& entities, const Tensor& pool_ptr, const Tensor& pool_x, const Tensor* pool_y,
                     const Tensor& op_x, const Tensor& pool_op) {
  dev_tensor(entities, at::kLong, "entities"); dev_tensor(pool_ptr, at::kLong, "pool_ptr");
  dev_tensor(pool_x, at::kLong, "pool_x");
  if (pool_y) dev_tensor(*pool_y, at::kFloat, "pool_y");
  dev_tensor(op_x, at::kLong, "op_x"); dev_tensor(pool_op, at::kLong, "pool_op");
  TORCH_CHECK(pool_x.dim() == 2 && pool_x.size(1) >= 2 && pool_x.size(1) <= VFM_MAX_FIELDS, "pool_x must be [P, F]");
  const int64_t U = entities.numel(), P = pool_x.size(0), F = pool_x.size(1);
  TORCH_CHECK(pool_ptr.numel() == U + 1 && (!pool_y || pool_y->numel() == P), "pool_ptr [U + 1], pool_y [P]");
  TORCH_CHECK(op_x.dim() == 2 && op_x.size(1) == F && pool_op.numel() == P,
              "op_x must be [n_ops, F], pool_op must hold one operand per pool row");
  p.U = U; p.P = P; p.F = (int32_t)F; p.n_ops = op_x.size(0);
  p.entities = entities.data_ptr<int64_t>(); p.pool_ptr = pool_ptr.data_ptr<int64_t>();
  p.pool_x = pool_x.data_ptr<int64_t>();
  if (pool_y) p.pool_y = pool_y->data_ptr<float>();
  p.op_x = op_x.data_ptr<int64_t>(); p.pool_op = pool_op.data_ptr<int64_t>();
}

// the field form's history (rows false: the op reads the history's operands only and has no hist_x, hist_y)
template <class S>
void fill_field_history(S& p, const optional<Tensor>& hist_ptr, const optional<Tensor>& hist_x,
                        const optional<Tensor>& hist_y, const optional<Tensor>& hist_op, bool rows = true) {
  if (!given(hist_ptr)) return;
  TORCH_CHECK((!rows || (given(hist_x) && given(hist_y))) && given(hist_op), "hist_ptr needs hist_x, hist_y and hist_op");
  dev_tensor(*hist_ptr, at::kLong, "hist_ptr"); dev_tensor(*hist_op, at::kLong, "hist_op");
  p.H = hist_op->numel();
  if (rows) {
    dev_tensor(*hist_x, at::kLong, "hist_x"); dev_tensor(*hist_y, at::kFloat, "hist_y");
    TORCH_CHECK(hist_x->dim() == 2 && hist_x->size(1) == p.F, "hist_x must be [H, F]");
    p.hist_x = hist_x->data_ptr<int64_t>(); p.hist_y = hist_y->data_ptr<float>();
  }
  TORCH_CHECK(hist_ptr->numel() == p.U + 1 && (!rows || (hist_x->size(0) == p.H && hist_y->numel() == p.H)),
              "hist_ptr [U + 1], hist_y [H], hist_op [H]");
  p.hist_ptr = hist_ptr->data_ptr<int64_t>(); p.hist_op = hist_op->data_ptr<int64_t>();
}

// the outputs of a session of n_rounds rounds over the p.U ids and p.P pool rows (p.d: fill_tables)
template <class S>
void fill_session_outputs(S& p, int64_t n_rounds, const Tensor& out_row, const Tensor& out_score, const Tensor& out_loss,
                          const optional<Tensor>& out_theta, const optional<Tensor>& out_mean,
                          const optional<Tensor>& out_var) {
  dev_tensor(out_row, at::kLong, "out_row"); dev_tensor(out_score, at::kFloat, "out_score");
  dev_tensor(out_loss, at::kFloat, "out_loss");
  TORCH_CHECK(n_rounds >= 0 && n_rounds <= VFM_ELICIT_MAX_ROUNDS, "n_rounds out of range");
  const int64_t U = p.U, P = p.P, Q = n_rounds;
  TORCH_CHECK(out_row.numel() >= U * Q && out_score.numel() >= U * Q && out_loss.numel() >= U * Q,
              "out_row, out_score, out_loss must be [U, Q]");
  p.n_rounds = (int32_t)Q;
  p.out_row = out_row.data_ptr<int64_t>(); p.out_score = out_score.data_ptr<float>();
  p.out_loss = out_loss.data_ptr<float>();
  if (given(out_theta)) {
    TORCH_CHECK(dev_tensor(*out_theta, at::kFloat, "out_theta").numel() >= U * Q * (2 * (int64_t)p.d + 2),
                "out_theta must be [U, Q, 2d + 2]");
    p.out_theta = out_theta->data_ptr<float>();
  }
  if (given(out_mean) || given(out_var)) {
    TORCH_CHECK(given(out_mean) && given(out_var), "out_mean and out_var: both or neither");
    TORCH_CHECK(dev_tensor(*out_mean, at::kFloat, "out_mean").numel() >= (Q + 1) * P &&
                dev_tensor(*out_var, at::kFloat, "out_var").numel() >= (Q + 1) * P,
                "out_mean, out_var must be [Q + 1, P]");
    p.out_mean = out_mean->data_ptr<float>();
    p.out_var = out_var->data_ptr<float>();
  }
}

// ---- the parts of a fold-in struct S (vfm_foldin_solve_t, vfm_foldin_split_t, vfm_foldin_bound_t,
// vfm_foldin_bound_split_t; vfm_foldin_t takes the row list), after a memset.  The rows come first: they set E.

// the folded ids, the rows' targets and operands and the loss: E, R, F, n_ops and the five pointers
template <class S>
void fill_fold_rows(S& p, const Tensor& entities, const Tensor& y, const Tensor& op_x, const Tensor& row_op,
                    const Tensor& loss) {
  dev_tensor(entities, at::kLong, "entities"); dev_tensor(y, at::kFloat, "y");
  dev_tensor(op_x, at::kLong, "op_x"); dev_tensor(row_op, at::kLong, "row_op"); dev_tensor(loss, at::kFloat, "loss");
  TORCH_CHECK(op_x.dim() == 2 && row_op.numel() == y.numel(), "op_x must be [n_ops, F], row_op [R] with y [R]");
  TORCH_CHECK(loss.numel() >= entities.numel(), "loss [E]");
  p.E = entities.numel(); p.R = y.numel(); p.F = (int32_t)op_x.size(1); p.n_ops = op_x.size(0);
  p.entities = entities.data_ptr<int64_t>(); p.y = y.data_ptr<float>();
  p.op_x = op_x.data_ptr<int64_t>(); p.row_op = row_op.data_ptr<int64_t>(); p.out_loss = loss.data_ptr<float>();
}

// the row list of the p.E ids
template <class S>
void fill_row_list(S& p, const Tensor& row_ptr) {
  TORCH_CHECK(dev_tensor(row_ptr, at::kLong, "row_ptr").numel() == p.E + 1, "row_ptr [E + 1]");
  p.row_ptr = row_ptr.data_ptr<int64_t>();
}

// the chunk table of the p.E ids: n_chunks and the two pointers
template <class S>
void fill_chunk_table(S& p, const Tensor& chunk_ptr, const Tensor& chunks) {
  dev_tensor(chunk_ptr, at::kLong, "chunk_ptr"); dev_tensor(chunks, at::kLong, "chunks");
  TORCH_CHECK(chunks.dim() == 2 && chunks.size(1) == 3, "chunks must be [n_chunks, 3]");
  TORCH_CHECK(chunk_ptr.numel() == p.E + 1, "chunk_ptr [E + 1]");
  p.n_chunks = chunks.size(0);
  p.chunk_ptr = chunk_ptr.data_ptr<int64_t>(); p.chunks = chunks.data_ptr<int64_t>();
}

// the folded field's prior, mean | precision, for tables of width d (fill_tables)
inline const float* prior_of(const Tensor& prior, int64_t d) {
  dev_tensor(prior, at::kFloat, "prior");
  TORCH_CHECK(prior.dim() == 2 && prior.size(0) == 2 && prior.size(1) == d + 1, "prior must be [2, d + 1]");
  return prior.data_ptr<float>();
}

// a *_workspace_bytes result: negative is the library's "bad arguments"
inline int64_t checked_bytes(int64_t b, const char* what) {
  TORCH_CHECK(b >= 0, what, ": bad arguments");
  return b;
}

}  // namespace vfm_ops
