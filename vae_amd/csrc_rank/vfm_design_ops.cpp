// vfm_design_ops.cpp -- torch.ops.vfm_hip.{design_workspace_bytes, design_scores, design_elicit}: the TORCH_LIBRARY
// fragment over include/vfm_design.h.  Like vfm_elicit_ops.cpp it only validates tensors, takes the current HIP stream
// of the tensors' device and forwards raw pointers; all arithmetic is in the HIP kernels.
#include <ATen/ATen.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <string.h>

#include "vfm_design.h"

namespace {

using at::Tensor;
using c10::optional;

const Tensor& dev_tensor(const Tensor& t, at::ScalarType dt, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on the GPU (vae_amd has no CPU fallback)");
  TORCH_CHECK(t.scalar_type() == dt, name, " has the wrong dtype");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  return t;
}

bool given(const optional<Tensor>& t) { return t.has_value() && t->defined(); }

int64_t design_workspace_bytes(int64_t U, int64_t P, int64_t n_ops, int64_t d, int64_t lds_dim) {
  const int64_t b = vfm_design_workspace_bytes(U, P, n_ops, (int32_t)d, (int32_t)lds_dim);
  TORCH_CHECK(b >= 0, "vfm_design_workspace_bytes: bad arguments");
  return b;
}

// what both ops share: the ids, the pool, the history's operands, the targets, the operand table, the model's tables
void fill_design(vfm_design_t& p, const Tensor& entities, const Tensor& pool_ptr, const Tensor& pool_x,
                 const optional<Tensor>& hist_ptr, const optional<Tensor>& hist_op, const Tensor& tgt_ptr,
                 const Tensor& tgt_op, const Tensor& op_x, const Tensor& pool_op, Tensor& entity, Tensor& bias,
                 const Tensor& scalars, Tensor& workspace, int64_t field, int64_t flags, int64_t lds_dim,
                 double kl_weight) {
  dev_tensor(entities, at::kLong, "entities"); dev_tensor(pool_ptr, at::kLong, "pool_ptr");
  dev_tensor(pool_x, at::kLong, "pool_x"); dev_tensor(tgt_ptr, at::kLong, "tgt_ptr");
  dev_tensor(tgt_op, at::kLong, "tgt_op"); dev_tensor(op_x, at::kLong, "op_x"); dev_tensor(pool_op, at::kLong, "pool_op");
  dev_tensor(entity, at::kFloat, "entity_params"); dev_tensor(bias, at::kFloat, "bias_params");
  dev_tensor(scalars, at::kFloat, "scalars"); dev_tensor(workspace, at::kByte, "workspace");
  TORCH_CHECK(entity.dim() == 2 && bias.dim() == 2 && bias.size(1) == 2 && bias.size(0) == entity.size(0) &&
              entity.size(1) % 2 == 0 && scalars.numel() >= 3, "table shapes");
  TORCH_CHECK(pool_x.dim() == 2 && pool_x.size(1) >= 2 && pool_x.size(1) <= VFM_MAX_FIELDS, "pool_x must be [P, F]");
  const int64_t U = entities.numel(), P = pool_x.size(0), F = pool_x.size(1);
  TORCH_CHECK(pool_ptr.numel() == U + 1 && tgt_ptr.numel() == U + 1, "pool_ptr [U + 1], tgt_ptr [U + 1]");
  TORCH_CHECK(op_x.dim() == 2 && op_x.size(1) == F && pool_op.numel() == P,
              "op_x must be [n_ops, F], pool_op must hold one operand per pool row");
  VFM_STRUCT_INIT(p);
  p.U = U; p.P = P; p.T = entity.size(0); p.F = (int32_t)F; p.d = (int32_t)(entity.size(1) / 2);
  p.field = (int32_t)field; p.flags = (int32_t)flags; p.lds_dim = (int32_t)lds_dim; p.kl_weight = (float)kl_weight;
  p.n_ops = op_x.size(0); p.n_targets = tgt_op.numel();
  p.entities = entities.data_ptr<int64_t>(); p.pool_ptr = pool_ptr.data_ptr<int64_t>();
  p.pool_x = pool_x.data_ptr<int64_t>();
  p.tgt_ptr = tgt_ptr.data_ptr<int64_t>(); p.tgt_op = tgt_op.data_ptr<int64_t>();
  p.op_x = op_x.data_ptr<int64_t>(); p.pool_op = pool_op.data_ptr<int64_t>();
  p.entity_params = entity.data_ptr<float>(); p.bias_params = bias.data_ptr<float>();
  p.scalars = scalars.data_ptr<float>();
  if (given(hist_ptr)) {
    TORCH_CHECK(given(hist_op), "hist_ptr needs hist_op");
    dev_tensor(*hist_ptr, at::kLong, "hist_ptr"); dev_tensor(*hist_op, at::kLong, "hist_op");
    p.H = hist_op->numel();
    TORCH_CHECK(hist_ptr->numel() == U + 1, "hist_ptr [U + 1]");
    p.hist_ptr = hist_ptr->data_ptr<int64_t>(); p.hist_op = hist_op->data_ptr<int64_t>();
  }
  p.workspace = workspace.data_ptr();
  p.workspace_bytes = workspace.numel();
}

// every pool row's score with R = the respondent's history
void design_scores(const Tensor& entities, const Tensor& pool_ptr, const Tensor& pool_x, const optional<Tensor>& hist_ptr,
                   const optional<Tensor>& hist_op, const Tensor& tgt_ptr, const Tensor& tgt_op, const Tensor& op_x,
                   const Tensor& pool_op, Tensor entity, Tensor bias, const Tensor& scalars, Tensor workspace,
                   Tensor out_pool_score, int64_t field, int64_t flags, double kl_weight) {
  vfm_design_t p;
  fill_design(p, entities, pool_ptr, pool_x, hist_ptr, hist_op, tgt_ptr, tgt_op, op_x, pool_op, entity, bias, scalars,
              workspace, field, flags, -1, kl_weight);
  TORCH_CHECK(dev_tensor(out_pool_score, at::kFloat, "out_pool_score").numel() >= p.P, "out_pool_score must be [P]");
  p.out_pool_score = out_pool_score.data_ptr<float>();
  c10::hip::HIPGuard guard(entities.get_device());
  const int rc = vfm_design_scores_f32(&p, (void*)c10::hip::getCurrentHIPStream(entities.get_device()).stream());
  TORCH_CHECK(rc == 0, "vfm_design_scores_f32 failed (code ", rc, "): ", vfm_last_error());
}

// the sessions: elicit_solve's tensors without the strategy's, plus the targets
void design_elicit(const Tensor& entities, const Tensor& pool_ptr, const Tensor& pool_x, const Tensor& pool_y,
                   const optional<Tensor>& hist_ptr, const optional<Tensor>& hist_x, const optional<Tensor>& hist_y,
                   const optional<Tensor>& hist_op, const Tensor& tgt_ptr, const Tensor& tgt_op, const Tensor& op_x,
                   const Tensor& pool_op, Tensor entity, Tensor bias, const Tensor& scalars, Tensor workspace,
                   Tensor out_row, Tensor out_score, Tensor out_loss, const optional<Tensor>& out_theta,
                   const optional<Tensor>& out_mean, const optional<Tensor>& out_var, int64_t field, int64_t n_rounds,
                   int64_t flags, int64_t reset, int64_t write, int64_t lds_dim, double kl_weight) {
  vfm_design_t p;
  fill_design(p, entities, pool_ptr, pool_x, hist_ptr, hist_op, tgt_ptr, tgt_op, op_x, pool_op, entity, bias, scalars,
              workspace, field, flags, lds_dim, kl_weight);
  const int64_t U = p.U, P = p.P, Q = n_rounds;
  TORCH_CHECK(Q >= 0 && Q <= VFM_ELICIT_MAX_ROUNDS, "n_rounds out of range");
  TORCH_CHECK(dev_tensor(pool_y, at::kFloat, "pool_y").numel() == P, "pool_y [P]");
  dev_tensor(out_row, at::kLong, "out_row"); dev_tensor(out_score, at::kFloat, "out_score");
  dev_tensor(out_loss, at::kFloat, "out_loss");
  TORCH_CHECK(out_row.numel() >= U * Q && out_score.numel() >= U * Q && out_loss.numel() >= U * Q,
              "out_row, out_score, out_loss must be [U, Q]");
  p.n_rounds = (int32_t)Q; p.reset = (int32_t)reset; p.write = (int32_t)write;
  p.pool_y = pool_y.data_ptr<float>();
  p.out_row = out_row.data_ptr<int64_t>(); p.out_score = out_score.data_ptr<float>();
  p.out_loss = out_loss.data_ptr<float>();
  if (given(hist_ptr)) {
    TORCH_CHECK(given(hist_x) && given(hist_y), "hist_ptr needs hist_x and hist_y");
    dev_tensor(*hist_x, at::kLong, "hist_x"); dev_tensor(*hist_y, at::kFloat, "hist_y");
    TORCH_CHECK(hist_x->dim() == 2 && hist_x->size(1) == p.F && hist_x->size(0) == p.H && hist_y->numel() == p.H,
                "hist_x must be [H, F], hist_y [H]");
    p.hist_x = hist_x->data_ptr<int64_t>(); p.hist_y = hist_y->data_ptr<float>();
  }
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
  c10::hip::HIPGuard guard(entities.get_device());
  const int rc = vfm_design_elicit_f32(&p, (void*)c10::hip::getCurrentHIPStream(entities.get_device()).stream());
  TORCH_CHECK(rc == 0, "vfm_design_elicit_f32 failed (code ", rc, "): ", vfm_last_error());
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
}
