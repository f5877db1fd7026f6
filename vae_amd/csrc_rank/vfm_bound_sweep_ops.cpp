// vfm_bound_sweep_ops.cpp -- torch.ops.vfm_hip.{foldin_bound_split, foldin_bound_split_workspace_bytes}: the
// TORCH_LIBRARY fragment over include/vfm_bound_sweep.h.  Like vfm_sweep_ops.cpp it only validates tensors, takes the
// current HIP stream of the tensors' device and forwards raw pointers; all arithmetic is in the HIP kernels.
#include "vfm_ops_common.hpp"

#include "vfm_bound_sweep.h"

namespace {

using namespace vfm_ops;

int64_t foldin_bound_split_workspace_bytes(int64_t n_chunks, int64_t n_heavy, int64_t R, int64_t n_ops, int64_t d,
                                           int64_t lds_dim) {
  const int64_t b = vfm_foldin_bound_split_workspace_bytes(n_chunks, n_heavy, R, n_ops, (int32_t)d, (int32_t)lds_dim);
  TORCH_CHECK(b >= 0, "vfm_foldin_bound_split_workspace_bytes: bad arguments");
  return b;
}

void foldin_bound_split(const Tensor& entities, const Tensor& chunk_ptr, const Tensor& chunks, const Tensor& y,
                        const Tensor& op_x, const Tensor& row_op, Tensor entity, Tensor bias, const Tensor& scalars,
                        Tensor workspace, Tensor loss, int64_t col, int64_t flags, int64_t lds_dim, double kl_weight,
                        int64_t n_iters, int64_t reset) {
  dev_tensor(entities, at::kLong, "entities"); dev_tensor(chunk_ptr, at::kLong, "chunk_ptr");
  dev_tensor(chunks, at::kLong, "chunks");
  dev_tensor(y, at::kFloat, "y"); dev_tensor(op_x, at::kLong, "op_x"); dev_tensor(row_op, at::kLong, "row_op");
  dev_tensor(entity, at::kFloat, "entity_params"); dev_tensor(bias, at::kFloat, "bias_params");
  dev_tensor(scalars, at::kFloat, "scalars"); dev_tensor(loss, at::kFloat, "loss");
  dev_tensor(workspace, at::kByte, "workspace");
  TORCH_CHECK(entity.dim() == 2 && bias.dim() == 2 && bias.size(1) == 2 && bias.size(0) == entity.size(0) &&
              entity.size(1) % 2 == 0 && scalars.numel() >= 3, "table shapes");
  TORCH_CHECK(op_x.dim() == 2 && row_op.numel() == y.numel(), "op_x must be [n_ops, F], row_op [R] with y [R]");
  TORCH_CHECK(chunks.dim() == 2 && chunks.size(1) == 3, "chunks must be [n_chunks, 3]");
  const int64_t E = entities.numel();
  TORCH_CHECK(chunk_ptr.numel() == E + 1 && loss.numel() >= E, "chunk_ptr [E + 1], loss [E]");
  TORCH_CHECK(n_iters >= INT32_MIN && n_iters <= INT32_MAX, "n_iters out of range");
  vfm_foldin_bound_split_t p;
  memset(&p, 0, sizeof(p));
  p.E = E; p.R = y.numel(); p.T = entity.size(0); p.n_ops = op_x.size(0); p.n_chunks = chunks.size(0);
  p.F = (int32_t)op_x.size(1); p.d = (int32_t)(entity.size(1) / 2);
  p.col = (int32_t)col; p.flags = (int32_t)flags; p.lds_dim = (int32_t)lds_dim; p.kl_weight = (float)kl_weight;
  p.n_iters = (int32_t)n_iters; p.reset = reset != 0;
  p.entities = entities.data_ptr<int64_t>(); p.chunk_ptr = chunk_ptr.data_ptr<int64_t>();
  p.chunks = chunks.data_ptr<int64_t>(); p.y = y.data_ptr<float>();
  p.op_x = op_x.data_ptr<int64_t>(); p.row_op = row_op.data_ptr<int64_t>();
  p.entity_params = entity.data_ptr<float>(); p.bias_params = bias.data_ptr<float>();
  p.scalars = scalars.data_ptr<float>(); p.out_loss = loss.data_ptr<float>();
  p.workspace = workspace.data_ptr(); p.workspace_bytes = workspace.numel();
  c10::hip::HIPGuard guard(y.get_device());
  check(vfm_foldin_bound_split_f32(&p, stream_of(y)), "vfm_foldin_bound_split_f32");
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(vfm_hip, m) {
  m.def("foldin_bound_split_workspace_bytes(int n_chunks, int n_heavy, int R, int n_ops, int d, int lds_dim) -> int",
        &foldin_bound_split_workspace_bytes);
  m.def("foldin_bound_split(Tensor entities, Tensor chunk_ptr, Tensor chunks, Tensor y, Tensor op_x, Tensor row_op, "
        "Tensor(a!) entity_params, Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) loss, "
        "int col, int flags, int lds_dim, float kl_weight, int n_iters, int reset) -> ()",
        &foldin_bound_split);
}
