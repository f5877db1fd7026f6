// vfm_design_ops.cpp -- torch.ops.vfm_hip.{design_workspace_bytes, design_scores, design_elicit, design_scores_prior,
// design_elicit_prior}: the TORCH_LIBRARY fragment over include/vfm_design.h and its forms under a field prior
// (include/vfm_elicit_prior.h).  Like vfm_elicit_ops.cpp it only validates tensors, takes the current HIP stream
// of the tensors' device and forwards raw pointers; all arithmetic is in the HIP kernels.  The rows, tables, workspace,
// outputs and history are the session parts of vfm_ops_common.hpp; the targets are this form's own.
#include "vfm_ops_common.hpp"

#include "vfm_design.h"
#include "vfm_elicit_prior.h"

namespace {

using namespace vfm_ops;

int64_t design_workspace_bytes(int64_t U, int64_t P, int64_t n_ops, int64_t d, int64_t lds_dim) {
  const int64_t b = vfm_design_workspace_bytes(U, P, n_ops, (int32_t)d, (int32_t)lds_dim);
  TORCH_CHECK(b >= 0, "vfm_design_workspace_bytes: bad arguments");
  return b;
}

// what both ops share: the rows (pool_y NULL: the scores read none), the targets, the model's tables, the workspace
void fill_design(vfm_design_t& p, const Tensor& entities, const Tensor& pool_ptr, const Tensor& pool_x,
                 const Tensor* pool_y, const Tensor& tgt_ptr, const Tensor& tgt_op, const Tensor& op_x,
                 const Tensor& pool_op, const Tensor& entity, const Tensor& bias, const Tensor& scalars,
                 const Tensor& workspace, int64_t field, int64_t flags, int64_t lds_dim, double kl_weight) {
  VFM_STRUCT_INIT(p);
  fill_field_rows(p, entities, pool_ptr, pool_x, pool_y, op_x, pool_op);
  dev_tensor(tgt_ptr, at::kLong, "tgt_ptr"); dev_tensor(tgt_op, at::kLong, "tgt_op");
  TORCH_CHECK(tgt_ptr.numel() == p.U + 1, "pool_ptr [U + 1], tgt_ptr [U + 1]");
  p.n_targets = tgt_op.numel();
  p.tgt_ptr = tgt_ptr.data_ptr<int64_t>(); p.tgt_op = tgt_op.data_ptr<int64_t>();
  fill_tables(p, entity, bias, scalars);
  fill_workspace(p, workspace);
  p.field = (int32_t)field; p.flags = (int32_t)flags; p.lds_dim = (int32_t)lds_dim; p.kl_weight = (float)kl_weight;
}

// every pool row's score with R = the respondent's history; prior: NULL, or the respondents' field prior [2, d + 1]
// (design_scores_prior)
void design_scores_call(const Tensor* prior, const Tensor& entities, const Tensor& pool_ptr, const Tensor& pool_x, const optional<Tensor>& hist_ptr,
                   const optional<Tensor>& hist_op, const Tensor& tgt_ptr, const Tensor& tgt_op, const Tensor& op_x,
                   const Tensor& pool_op, Tensor entity, Tensor bias, const Tensor& scalars, Tensor workspace,
                   Tensor out_pool_score, int64_t field, int64_t flags, double kl_weight) {
  vfm_design_t p;
  fill_design(p, entities, pool_ptr, pool_x, nullptr, tgt_ptr, tgt_op, op_x, pool_op, entity, bias, scalars, workspace,
              field, flags, -1, kl_weight);
  fill_field_history(p, hist_ptr, c10::nullopt, c10::nullopt, hist_op, /*rows=*/false);
  TORCH_CHECK(dev_tensor(out_pool_score, at::kFloat, "out_pool_score").numel() >= p.P, "out_pool_score must be [P]");
  p.out_pool_score = out_pool_score.data_ptr<float>();
  c10::hip::HIPGuard guard(entities.get_device());
  if (prior) check(vfm_design_scores_prior_f32(&p, prior_of(*prior, p.d), stream_of(entities)), "vfm_design_scores_prior_f32");
  else check(vfm_design_scores_f32(&p, stream_of(entities)), "vfm_design_scores_f32");
}

#define VFM_SCORES_TENSORS                                                                                               \
  const Tensor &entities, const Tensor &pool_ptr, const Tensor &pool_x, const optional<Tensor>&hist_ptr,                 \
      const optional<Tensor>&hist_op, const Tensor &tgt_ptr, const Tensor &tgt_op, const Tensor &op_x,                   \
      const Tensor &pool_op, Tensor entity, Tensor bias, const Tensor &scalars, Tensor workspace, Tensor out_pool_score
#define VFM_SCORES_TENSOR_NAMES                                                                                          \
  entities, pool_ptr, pool_x, hist_ptr, hist_op, tgt_ptr, tgt_op, op_x, pool_op, entity, bias, scalars, workspace,       \
      out_pool_score

void design_scores(VFM_SCORES_TENSORS, int64_t field, int64_t flags, double kl_weight) {
  design_scores_call(nullptr, VFM_SCORES_TENSOR_NAMES, field, flags, kl_weight);
}

void design_scores_prior(VFM_SCORES_TENSORS, const Tensor& prior, int64_t field, int64_t flags, double kl_weight) {
  design_scores_call(&prior, VFM_SCORES_TENSOR_NAMES, field, flags, kl_weight);
}

// the sessions: elicit_solve's tensors without the strategy's, plus the targets; prior: as design_scores_call's
// (design_elicit_prior)
void design_elicit_call(const Tensor* prior, const Tensor& entities, const Tensor& pool_ptr, const Tensor& pool_x, const Tensor& pool_y,
                   const optional<Tensor>& hist_ptr, const optional<Tensor>& hist_x, const optional<Tensor>& hist_y,
                   const optional<Tensor>& hist_op, const Tensor& tgt_ptr, const Tensor& tgt_op, const Tensor& op_x,
                   const Tensor& pool_op, Tensor entity, Tensor bias, const Tensor& scalars, Tensor workspace,
                   Tensor out_row, Tensor out_score, Tensor out_loss, const optional<Tensor>& out_theta,
                   const optional<Tensor>& out_mean, const optional<Tensor>& out_var, int64_t field, int64_t n_rounds,
                   int64_t flags, int64_t reset, int64_t write, int64_t lds_dim, double kl_weight) {
  vfm_design_t p;
  fill_design(p, entities, pool_ptr, pool_x, &pool_y, tgt_ptr, tgt_op, op_x, pool_op, entity, bias, scalars, workspace,
              field, flags, lds_dim, kl_weight);
  fill_session_outputs(p, n_rounds, out_row, out_score, out_loss, out_theta, out_mean, out_var);
  fill_field_history(p, hist_ptr, hist_x, hist_y, hist_op);
  p.reset = (int32_t)reset; p.write = (int32_t)write;
  c10::hip::HIPGuard guard(entities.get_device());
  if (prior) check(vfm_design_elicit_prior_f32(&p, prior_of(*prior, p.d), stream_of(entities)), "vfm_design_elicit_prior_f32");
  else check(vfm_design_elicit_f32(&p, stream_of(entities)), "vfm_design_elicit_f32");
}

#define VFM_DESIGN_TENSORS                                                                                               \
  const Tensor &entities, const Tensor &pool_ptr, const Tensor &pool_x, const Tensor &pool_y,                            \
      const optional<Tensor>&hist_ptr, const optional<Tensor>&hist_x, const optional<Tensor>&hist_y,                     \
      const optional<Tensor>&hist_op, const Tensor &tgt_ptr, const Tensor &tgt_op, const Tensor &op_x,                   \
      const Tensor &pool_op, Tensor entity, Tensor bias, const Tensor &scalars, Tensor workspace, Tensor out_row,        \
      Tensor out_score, Tensor out_loss, const optional<Tensor>&out_theta, const optional<Tensor>&out_mean,              \
      const optional<Tensor>&out_var
#define VFM_DESIGN_TENSOR_NAMES                                                                                          \
  entities, pool_ptr, pool_x, pool_y, hist_ptr, hist_x, hist_y, hist_op, tgt_ptr, tgt_op, op_x, pool_op, entity, bias,   \
      scalars, workspace, out_row, out_score, out_loss, out_theta, out_mean, out_var

void design_elicit(VFM_DESIGN_TENSORS, int64_t field, int64_t n_rounds, int64_t flags, int64_t reset, int64_t write,
                   int64_t lds_dim, double kl_weight) {
  design_elicit_call(nullptr, VFM_DESIGN_TENSOR_NAMES, field, n_rounds, flags, reset, write, lds_dim, kl_weight);
}

void design_elicit_prior(VFM_DESIGN_TENSORS, const Tensor& prior, int64_t field, int64_t n_rounds, int64_t flags,
                         int64_t reset, int64_t write, int64_t lds_dim, double kl_weight) {
  design_elicit_call(&prior, VFM_DESIGN_TENSOR_NAMES, field, n_rounds, flags, reset, write, lds_dim, kl_weight);
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(vfm_hip, m) {
  m.def("design_workspace_bytes(int U, int P, int n_ops, int d, int lds_dim) -> int", &design_workspace_bytes);
  m.def("design_scores(Tensor entities, Tensor pool_ptr, Tensor pool_x, Tensor? hist_ptr, Tensor? hist_op, "
        "Tensor tgt_ptr, Tensor tgt_op, Tensor op_x, Tensor pool_op, Tensor entity_params, Tensor bias_params, "
        "Tensor scalars, Tensor(a!) workspace, Tensor(b!) out_pool_score, int field, int flags, float kl_weight) -> ()",
        &design_scores);
  m.def("design_elicit(Tensor entities, Tensor pool_ptr, Tensor pool_x, Tensor pool_y, Tensor? hist_ptr, Tensor? hist_x, "
        "Tensor? hist_y, Tensor? hist_op, Tensor tgt_ptr, Tensor tgt_op, Tensor op_x, Tensor pool_op, "
        "Tensor(a!) entity_params, Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) out_row, "
        "Tensor(e!) out_score, Tensor(f!) out_loss, Tensor(g!)? out_theta, Tensor(h!)? out_mean, Tensor(i!)? out_var, "
        "int field, int n_rounds, int flags, int reset, int write, int lds_dim, float kl_weight) -> ()",
        &design_elicit);
  m.def("design_scores_prior(Tensor entities, Tensor pool_ptr, Tensor pool_x, Tensor? hist_ptr, Tensor? hist_op, "
        "Tensor tgt_ptr, Tensor tgt_op, Tensor op_x, Tensor pool_op, Tensor entity_params, Tensor bias_params, "
        "Tensor scalars, Tensor(a!) workspace, Tensor(b!) out_pool_score, Tensor prior, int field, int flags, "
        "float kl_weight) -> ()",
        &design_scores_prior);
  m.def("design_elicit_prior(Tensor entities, Tensor pool_ptr, Tensor pool_x, Tensor pool_y, Tensor? hist_ptr, "
        "Tensor? hist_x, Tensor? hist_y, Tensor? hist_op, Tensor tgt_ptr, Tensor tgt_op, Tensor op_x, Tensor pool_op, "
        "Tensor(a!) entity_params, Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) out_row, "
        "Tensor(e!) out_score, Tensor(f!) out_loss, Tensor(g!)? out_theta, Tensor(h!)? out_mean, Tensor(i!)? out_var, "
        "Tensor prior, int field, int n_rounds, int flags, int reset, int write, int lds_dim, float kl_weight) -> ()",
        &design_elicit_prior);
}
