// vfm_prior_ops.cpp -- torch.ops.vfm_hip.{foldin_solve_prior, foldin_solve_split_prior}: the TORCH_LIBRARY fragment over
// include/vfm_prior.h, next to foldin_solve (vfm_foldin_ops.cpp) and foldin_solve_split (vfm_sweep_ops.cpp).  It only
// validates tensors, takes the current HIP stream of the tensors' device and forwards raw pointers; all arithmetic is in
// the HIP kernels.  The workspaces are the parent calls' (foldin_solve_workspace_bytes, foldin_split_workspace_bytes).
#include "vfm_ops_common.hpp"

#include "vfm_prior.h"

namespace {

using namespace vfm_ops;

// the rows' tables, operands and outputs that both ops check alike; returns d
int64_t check_common(const Tensor& entities, const Tensor& y, const Tensor& op_x, const Tensor& row_op, const Tensor& entity,
                     const Tensor& bias, const Tensor& scalars, const Tensor& workspace, const Tensor& loss,
                     const Tensor& prior) {
  dev_tensor(entities, at::kLong, "entities");
  dev_tensor(y, at::kFloat, "y"); dev_tensor(op_x, at::kLong, "op_x"); dev_tensor(row_op, at::kLong, "row_op");
  dev_tensor(entity, at::kFloat, "entity_params"); dev_tensor(bias, at::kFloat, "bias_params");
  dev_tensor(scalars, at::kFloat, "scalars"); dev_tensor(loss, at::kFloat, "loss");
  dev_tensor(workspace, at::kByte, "workspace"); dev_tensor(prior, at::kFloat, "prior");
  TORCH_CHECK(entity.dim() == 2 && bias.dim() == 2 && bias.size(1) == 2 && bias.size(0) == entity.size(0) &&
              entity.size(1) % 2 == 0 && scalars.numel() >= 3, "table shapes");
  TORCH_CHECK(op_x.dim() == 2 && row_op.numel() == y.numel(), "op_x must be [n_ops, F], row_op [R] with y [R]");
  const int64_t d = entity.size(1) / 2;
  TORCH_CHECK(prior.dim() == 2 && prior.size(0) == 2 && prior.size(1) == d + 1, "prior must be [2, d + 1]");
  return d;
}

void foldin_solve_prior(const Tensor& entities, const Tensor& row_ptr, const Tensor& y, const Tensor& op_x,
                        const Tensor& row_op, Tensor entity, Tensor bias, const Tensor& scalars, Tensor workspace,
                        Tensor loss, const Tensor& prior, int64_t col, int64_t objective, int64_t likelihood, int64_t flags,
                        int64_t lds_dim, double kl_weight) {
  const int64_t d = check_common(entities, y, op_x, row_op, entity, bias, scalars, workspace, loss, prior);
  dev_tensor(row_ptr, at::kLong, "row_ptr");
  const int64_t E = entities.numel();
  TORCH_CHECK(row_ptr.numel() == E + 1 && loss.numel() >= E, "row_ptr [E + 1], loss [E]");
  vfm_foldin_solve_t p;
  memset(&p, 0, sizeof(p));
  p.E = E; p.R = y.numel(); p.T = entity.size(0); p.n_ops = op_x.size(0);
  p.F = (int32_t)op_x.size(1); p.d = (int32_t)d;
  p.col = (int32_t)col; p.objective = (int32_t)objective; p.likelihood = (int32_t)likelihood; p.flags = (int32_t)flags;
  p.lds_dim = (int32_t)lds_dim; p.kl_weight = (float)kl_weight;
  p.entities = entities.data_ptr<int64_t>(); p.row_ptr = row_ptr.data_ptr<int64_t>(); p.y = y.data_ptr<float>();
  p.op_x = op_x.data_ptr<int64_t>(); p.row_op = row_op.data_ptr<int64_t>();
  p.entity_params = entity.data_ptr<float>(); p.bias_params = bias.data_ptr<float>();
  p.scalars = scalars.data_ptr<float>(); p.out_loss = loss.data_ptr<float>();
  p.workspace = workspace.data_ptr(); p.workspace_bytes = workspace.numel();
  c10::hip::HIPGuard guard(y.get_device());
  check(vfm_foldin_solve_prior_f32(&p, prior.data_ptr<float>(), stream_of(y)), "vfm_foldin_solve_prior_f32");
}

void foldin_solve_split_prior(const Tensor& entities, const Tensor& chunk_ptr, const Tensor& chunks, const Tensor& y,
                              const Tensor& op_x, const Tensor& row_op, Tensor entity, Tensor bias, const Tensor& scalars,
                              Tensor workspace, Tensor loss, const Tensor& prior, int64_t col, int64_t flags,
                              int64_t lds_dim, double kl_weight) {
  const int64_t d = check_common(entities, y, op_x, row_op, entity, bias, scalars, workspace, loss, prior);
  dev_tensor(chunk_ptr, at::kLong, "chunk_ptr"); dev_tensor(chunks, at::kLong, "chunks");
  TORCH_CHECK(chunks.dim() == 2 && chunks.size(1) == 3, "chunks must be [n_chunks, 3]");
  const int64_t E = entities.numel();
  TORCH_CHECK(chunk_ptr.numel() == E + 1 && loss.numel() >= E, "chunk_ptr [E + 1], loss [E]");
  vfm_foldin_split_t p;
  memset(&p, 0, sizeof(p));
  p.E = E; p.R = y.numel(); p.T = entity.size(0); p.n_ops = op_x.size(0); p.n_chunks = chunks.size(0);
  p.F = (int32_t)op_x.size(1); p.d = (int32_t)d;
  p.col = (int32_t)col; p.flags = (int32_t)flags; p.lds_dim = (int32_t)lds_dim; p.kl_weight = (float)kl_weight;
  p.entities = entities.data_ptr<int64_t>(); p.chunk_ptr = chunk_ptr.data_ptr<int64_t>();
  p.chunks = chunks.data_ptr<int64_t>(); p.y = y.data_ptr<float>();
  p.op_x = op_x.data_ptr<int64_t>(); p.row_op = row_op.data_ptr<int64_t>();
  p.entity_params = entity.data_ptr<float>(); p.bias_params = bias.data_ptr<float>();
  p.scalars = scalars.data_ptr<float>(); p.out_loss = loss.data_ptr<float>();
  p.workspace = workspace.data_ptr(); p.workspace_bytes = workspace.numel();
  c10::hip::HIPGuard guard(y.get_device());
  check(vfm_foldin_solve_split_prior_f32(&p, prior.data_ptr<float>(), stream_of(y)), "vfm_foldin_solve_split_prior_f32");
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(vfm_hip, m) {
  m.def("foldin_solve_prior(Tensor entities, Tensor row_ptr, Tensor y, Tensor op_x, Tensor row_op, "
        "Tensor(a!) entity_params, Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) loss, "
        "Tensor prior, int col, int objective, int likelihood, int flags, int lds_dim, float kl_weight) -> ()",
        &foldin_solve_prior);
  m.def("foldin_solve_split_prior(Tensor entities, Tensor chunk_ptr, Tensor chunks, Tensor y, Tensor op_x, "
        "Tensor row_op, Tensor(a!) entity_params, Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, "
        "Tensor(d!) loss, Tensor prior, int col, int flags, int lds_dim, float kl_weight) -> ()",
        &foldin_solve_split_prior);
}
