// vfm_foldin_ops.cpp -- torch.ops.vfm_hip.{foldin, foldin_workspace_bytes, foldin_solve, foldin_solve_workspace_bytes,
// foldin_bound, foldin_bound_workspace_bytes}: the TORCH_LIBRARY fragment over include/vfm_foldin.h and include/vfm_bound.h.  Like vfm_rank_ops.cpp it only validates tensors, takes the current HIP stream of the tensors'
// device and forwards raw pointers; all arithmetic is in the HIP kernels.
#include "vfm_ops_common.hpp"

#include "vfm_bound.h"
#include "vfm_foldin.h"

namespace {

using namespace vfm_ops;

int64_t foldin_workspace_bytes(int64_t n_ops, int64_t d, int64_t objective) {
  const int64_t b = vfm_foldin_workspace_bytes(n_ops, (int32_t)d, (int32_t)objective);
  TORCH_CHECK(b >= 0, "vfm_foldin_workspace_bytes: bad arguments");
  return b;
}

void foldin(const Tensor& entities, const Tensor& row_ptr, const Tensor& x, const Tensor& y,
            const optional<Tensor>& op_x, const optional<Tensor>& row_op, Tensor entity, Tensor bias,
            const Tensor& scalars, const optional<Tensor>& workspace, Tensor loss, const optional<Tensor>& grad,
            int64_t col, int64_t objective, int64_t likelihood, int64_t flags, int64_t mode, int64_t n_steps,
            int64_t n_samples, int64_t reset, int64_t lds_rows, double lr, double kl_weight, int64_t seed, int64_t t0) {
  dev_tensor(entities, at::kLong, "entities"); dev_tensor(row_ptr, at::kLong, "row_ptr");
  dev_tensor(x, at::kLong, "x"); dev_tensor(y, at::kFloat, "y");
  dev_tensor(entity, at::kFloat, "entity_params"); dev_tensor(bias, at::kFloat, "bias_params");
  dev_tensor(scalars, at::kFloat, "scalars"); dev_tensor(loss, at::kFloat, "loss");
  TORCH_CHECK(entity.dim() == 2 && bias.dim() == 2 && bias.size(1) == 2 && bias.size(0) == entity.size(0) &&
              entity.size(1) % 2 == 0 && scalars.numel() >= 3, "table shapes");
  TORCH_CHECK(x.dim() == 2 && y.numel() == x.size(0), "x must be [R, F] with y [R]");
  const int64_t E = entities.numel();
  TORCH_CHECK(row_ptr.numel() == E + 1 && loss.numel() >= E, "row_ptr [E + 1], loss [E]");
  vfm_foldin_t p;
  memset(&p, 0, sizeof(p));
  p.E = E; p.R = x.size(0); p.T = entity.size(0); p.F = (int32_t)x.size(1); p.d = (int32_t)(entity.size(1) / 2);
  p.col = (int32_t)col; p.objective = (int32_t)objective; p.likelihood = (int32_t)likelihood; p.flags = (int32_t)flags;
  p.mode = (int32_t)mode; p.n_steps = (int32_t)n_steps; p.n_samples = (int32_t)n_samples; p.reset = (int32_t)reset;
  p.lds_rows = (int32_t)lds_rows; p.lr = (float)lr; p.kl_weight = (float)kl_weight; p.seed = (uint64_t)seed; p.t0 = t0;
  p.entities = entities.data_ptr<int64_t>(); p.row_ptr = row_ptr.data_ptr<int64_t>();
  p.x = x.data_ptr<int64_t>(); p.y = y.data_ptr<float>();
  if (given(op_x)) {
    TORCH_CHECK(dev_tensor(*op_x, at::kLong, "op_x").dim() == 2 && op_x->size(1) == x.size(1), "op_x must be [n_ops, F]");
    TORCH_CHECK(given(row_op) && dev_tensor(*row_op, at::kLong, "row_op").numel() == p.R,
                "row_op must hold one operand per row");
    p.n_ops = op_x->size(0);
    p.op_x = op_x->data_ptr<int64_t>();
    p.row_op = row_op->data_ptr<int64_t>();
  }
  if (given(workspace)) {
    dev_tensor(*workspace, at::kByte, "workspace");
    p.workspace = workspace->data_ptr();
    p.workspace_bytes = workspace->numel();
  }
  p.entity_params = entity.data_ptr<float>(); p.bias_params = bias.data_ptr<float>();
  p.scalars = scalars.data_ptr<float>(); p.out_loss = loss.data_ptr<float>();
  if (given(grad)) {
    TORCH_CHECK(dev_tensor(*grad, at::kFloat, "grad").numel() >= E * (2 * (int64_t)p.d + 2), "grad must be [E, 2d + 2]");
    p.out_grad = grad->data_ptr<float>();
  }
  c10::hip::HIPGuard guard(x.get_device());
  check(vfm_foldin_f32(&p, stream_of(x)), "vfm_foldin_f32");
}

int64_t foldin_solve_workspace_bytes(int64_t E, int64_t n_ops, int64_t d, int64_t lds_dim) {
  const int64_t b = vfm_foldin_solve_workspace_bytes(E, n_ops, (int32_t)d, (int32_t)lds_dim);
  TORCH_CHECK(b >= 0, "vfm_foldin_solve_workspace_bytes: bad arguments");
  return b;
}

void foldin_solve(const Tensor& entities, const Tensor& row_ptr, const Tensor& y, const Tensor& op_x,
                  const Tensor& row_op, Tensor entity, Tensor bias, const Tensor& scalars, Tensor workspace, Tensor loss,
                  int64_t col, int64_t objective, int64_t likelihood, int64_t flags, int64_t lds_dim, double kl_weight) {
  dev_tensor(entities, at::kLong, "entities"); dev_tensor(row_ptr, at::kLong, "row_ptr");
  dev_tensor(y, at::kFloat, "y"); dev_tensor(op_x, at::kLong, "op_x"); dev_tensor(row_op, at::kLong, "row_op");
  dev_tensor(entity, at::kFloat, "entity_params"); dev_tensor(bias, at::kFloat, "bias_params");
  dev_tensor(scalars, at::kFloat, "scalars"); dev_tensor(loss, at::kFloat, "loss");
  dev_tensor(workspace, at::kByte, "workspace");
  TORCH_CHECK(entity.dim() == 2 && bias.dim() == 2 && bias.size(1) == 2 && bias.size(0) == entity.size(0) &&
              entity.size(1) % 2 == 0 && scalars.numel() >= 3, "table shapes");
  TORCH_CHECK(op_x.dim() == 2 && row_op.numel() == y.numel(), "op_x must be [n_ops, F], row_op [R] with y [R]");
  const int64_t E = entities.numel();
  TORCH_CHECK(row_ptr.numel() == E + 1 && loss.numel() >= E, "row_ptr [E + 1], loss [E]");
  vfm_foldin_solve_t p;
  memset(&p, 0, sizeof(p));
  p.E = E; p.R = y.numel(); p.T = entity.size(0); p.n_ops = op_x.size(0);
  p.F = (int32_t)op_x.size(1); p.d = (int32_t)(entity.size(1) / 2);
  p.col = (int32_t)col; p.objective = (int32_t)objective; p.likelihood = (int32_t)likelihood; p.flags = (int32_t)flags;
  p.lds_dim = (int32_t)lds_dim; p.kl_weight = (float)kl_weight;
  p.entities = entities.data_ptr<int64_t>(); p.row_ptr = row_ptr.data_ptr<int64_t>(); p.y = y.data_ptr<float>();
  p.op_x = op_x.data_ptr<int64_t>(); p.row_op = row_op.data_ptr<int64_t>();
  p.entity_params = entity.data_ptr<float>(); p.bias_params = bias.data_ptr<float>();
  p.scalars = scalars.data_ptr<float>(); p.out_loss = loss.data_ptr<float>();
  p.workspace = workspace.data_ptr(); p.workspace_bytes = workspace.numel();
  c10::hip::HIPGuard guard(y.get_device());
  check(vfm_foldin_solve_f32(&p, stream_of(y)), "vfm_foldin_solve_f32");
}

int64_t foldin_bound_workspace_bytes(int64_t E, int64_t R, int64_t n_ops, int64_t d, int64_t lds_dim) {
  const int64_t b = vfm_foldin_bound_workspace_bytes(E, R, n_ops, (int32_t)d, (int32_t)lds_dim);
  TORCH_CHECK(b >= 0, "vfm_foldin_bound_workspace_bytes: bad arguments");
  return b;
}

void foldin_bound(const Tensor& entities, const Tensor& row_ptr, const Tensor& y, const Tensor& op_x,
                  const Tensor& row_op, Tensor entity, Tensor bias, const Tensor& scalars, Tensor workspace, Tensor loss,
                  int64_t col, int64_t objective, int64_t likelihood, int64_t flags, int64_t lds_dim, double kl_weight,
                  int64_t n_iters, int64_t reset, int64_t mode) {
  dev_tensor(entities, at::kLong, "entities"); dev_tensor(row_ptr, at::kLong, "row_ptr");
  dev_tensor(y, at::kFloat, "y"); dev_tensor(op_x, at::kLong, "op_x"); dev_tensor(row_op, at::kLong, "row_op");
  dev_tensor(entity, at::kFloat, "entity_params"); dev_tensor(bias, at::kFloat, "bias_params");
  dev_tensor(scalars, at::kFloat, "scalars"); dev_tensor(loss, at::kFloat, "loss");
  dev_tensor(workspace, at::kByte, "workspace");
  TORCH_CHECK(entity.dim() == 2 && bias.dim() == 2 && bias.size(1) == 2 && bias.size(0) == entity.size(0) &&
              entity.size(1) % 2 == 0 && scalars.numel() >= 3, "table shapes");
  TORCH_CHECK(op_x.dim() == 2 && row_op.numel() == y.numel(), "op_x must be [n_ops, F], row_op [R] with y [R]");
  const int64_t E = entities.numel();
  TORCH_CHECK(row_ptr.numel() == E + 1 && loss.numel() >= E, "row_ptr [E + 1], loss [E]");
  vfm_foldin_bound_t p;
  memset(&p, 0, sizeof(p));
  p.E = E; p.R = y.numel(); p.T = entity.size(0); p.n_ops = op_x.size(0);
  p.F = (int32_t)op_x.size(1); p.d = (int32_t)(entity.size(1) / 2);
  p.col = (int32_t)col; p.objective = (int32_t)objective; p.likelihood = (int32_t)likelihood; p.flags = (int32_t)flags;
  p.lds_dim = (int32_t)lds_dim; p.kl_weight = (float)kl_weight;
  p.n_iters = (int32_t)n_iters; p.reset = (int32_t)reset; p.mode = (int32_t)mode;
  p.entities = entities.data_ptr<int64_t>(); p.row_ptr = row_ptr.data_ptr<int64_t>(); p.y = y.data_ptr<float>();
  p.op_x = op_x.data_ptr<int64_t>(); p.row_op = row_op.data_ptr<int64_t>();
  p.entity_params = entity.data_ptr<float>(); p.bias_params = bias.data_ptr<float>();
  p.scalars = scalars.data_ptr<float>(); p.out_loss = loss.data_ptr<float>();
  p.workspace = workspace.data_ptr(); p.workspace_bytes = workspace.numel();
  c10::hip::HIPGuard guard(y.get_device());
  check(vfm_foldin_bound_f32(&p, stream_of(y)), "vfm_foldin_bound_f32");
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(vfm_hip, m) {
  m.def("foldin_workspace_bytes(int n_ops, int d, int objective) -> int", &foldin_workspace_bytes);
  m.def("foldin(Tensor entities, Tensor row_ptr, Tensor x, Tensor y, Tensor? op_x, Tensor? row_op, "
        "Tensor(a!) entity_params, Tensor(b!) bias_params, Tensor scalars, Tensor(c!)? workspace, Tensor(d!) loss, "
        "Tensor(e!)? grad, int col, int objective, int likelihood, int flags, int mode, int n_steps, int n_samples, "
        "int reset, int lds_rows, float lr, float kl_weight, int seed, int t0) -> ()",
        &foldin);
  m.def("foldin_solve_workspace_bytes(int E, int n_ops, int d, int lds_dim) -> int", &foldin_solve_workspace_bytes);
  m.def("foldin_solve(Tensor entities, Tensor row_ptr, Tensor y, Tensor op_x, Tensor row_op, "
        "Tensor(a!) entity_params, Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) loss, "
        "int col, int objective, int likelihood, int flags, int lds_dim, float kl_weight) -> ()",
        &foldin_solve);
  m.def("foldin_bound_workspace_bytes(int E, int R, int n_ops, int d, int lds_dim) -> int", &foldin_bound_workspace_bytes);
  m.def("foldin_bound(Tensor entities, Tensor row_ptr, Tensor y, Tensor op_x, Tensor row_op, "
        "Tensor(a!) entity_params, Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) loss, "
        "int col, int objective, int likelihood, int flags, int lds_dim, float kl_weight, int n_iters, int reset, "
        "int mode) -> ()",
        &foldin_bound);
}
