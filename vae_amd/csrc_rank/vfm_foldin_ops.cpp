// vfm_foldin_ops.cpp -- the fold-in family of torch.ops.vfm_hip: foldin (include/vfm_foldin.h), foldin_solve and
// foldin_solve_split (vfm_foldin.h, vfm_sweep.h), their *_prior forms (vfm_prior.h), foldin_bound and foldin_bound_split
// (vfm_bound.h, vfm_bound_sweep.h), their *_prior forms (vfm_bound_prior.h), the five *_workspace_bytes, implicit_base
// and foldin_solve_implicit with their size functions (vfm_implicit.h), foldin_solve_implicit_prior
// (vfm_implicit_prior.h) and foldin_solve_implicit_weights (vfm_implicit_weights.h).  Like vfm_rank_ops.cpp this TORCH_LIBRARY fragment
// only validates tensors, takes the current HIP stream of the tensors' device and forwards raw pointers; all arithmetic
// is in the HIP kernels.  Every solve is its parts (vfm_ops_common.hpp) plus its own scalars plus one call.
#include "vfm_ops_common.hpp"

#include "vfm_bound.h"
#include "vfm_bound_prior.h"
#include "vfm_bound_sweep.h"
#include "vfm_foldin.h"
#include "vfm_implicit.h"
#include "vfm_implicit_prior.h"
#include "vfm_implicit_weights.h"
#include "vfm_prior.h"
#include "vfm_sweep.h"

namespace {

using namespace vfm_ops;

int64_t foldin_workspace_bytes(int64_t n_ops, int64_t d, int64_t objective) {
  return checked_bytes(vfm_foldin_workspace_bytes(n_ops, (int32_t)d, (int32_t)objective), "vfm_foldin_workspace_bytes");
}

int64_t foldin_solve_workspace_bytes(int64_t E, int64_t n_ops, int64_t d, int64_t lds_dim) {
  return checked_bytes(vfm_foldin_solve_workspace_bytes(E, n_ops, (int32_t)d, (int32_t)lds_dim),
                       "vfm_foldin_solve_workspace_bytes");
}

int64_t foldin_bound_workspace_bytes(int64_t E, int64_t R, int64_t n_ops, int64_t d, int64_t lds_dim) {
  return checked_bytes(vfm_foldin_bound_workspace_bytes(E, R, n_ops, (int32_t)d, (int32_t)lds_dim),
                       "vfm_foldin_bound_workspace_bytes");
}

int64_t foldin_split_workspace_bytes(int64_t n_chunks, int64_t n_heavy, int64_t n_ops, int64_t d, int64_t lds_dim) {
  return checked_bytes(vfm_foldin_split_workspace_bytes(n_chunks, n_heavy, n_ops, (int32_t)d, (int32_t)lds_dim),
                       "vfm_foldin_split_workspace_bytes");
}

int64_t foldin_bound_split_workspace_bytes(int64_t n_chunks, int64_t n_heavy, int64_t R, int64_t n_ops, int64_t d,
                                           int64_t lds_dim) {
  return checked_bytes(vfm_foldin_bound_split_workspace_bytes(n_chunks, n_heavy, R, n_ops, (int32_t)d, (int32_t)lds_dim),
                       "vfm_foldin_bound_split_workspace_bytes");
}

void foldin(const Tensor& entities, const Tensor& row_ptr, const Tensor& x, const Tensor& y,
            const optional<Tensor>& op_x, const optional<Tensor>& row_op, Tensor entity, Tensor bias,
            const Tensor& scalars, const optional<Tensor>& workspace, Tensor loss, const optional<Tensor>& grad,
            int64_t col, int64_t objective, int64_t likelihood, int64_t flags, int64_t mode, int64_t n_steps,
            int64_t n_samples, int64_t reset, int64_t lds_rows, double lr, double kl_weight, int64_t seed, int64_t t0) {
  dev_tensor(entities, at::kLong, "entities"); dev_tensor(x, at::kLong, "x"); dev_tensor(y, at::kFloat, "y");
  dev_tensor(loss, at::kFloat, "loss");
  TORCH_CHECK(x.dim() == 2 && y.numel() == x.size(0), "x must be [R, F] with y [R]");
  TORCH_CHECK(loss.numel() >= entities.numel(), "loss [E]");
  vfm_foldin_t p;
  memset(&p, 0, sizeof(p));
  p.E = entities.numel(); p.R = x.size(0); p.F = (int32_t)x.size(1);
  p.entities = entities.data_ptr<int64_t>(); p.x = x.data_ptr<int64_t>(); p.y = y.data_ptr<float>();
  p.out_loss = loss.data_ptr<float>();
  fill_row_list(p, row_ptr);
  fill_tables(p, entity, bias, scalars);
  p.col = (int32_t)col; p.objective = (int32_t)objective; p.likelihood = (int32_t)likelihood; p.flags = (int32_t)flags;
  p.mode = (int32_t)mode; p.n_steps = (int32_t)n_steps; p.n_samples = (int32_t)n_samples; p.reset = (int32_t)reset;
  p.lds_rows = (int32_t)lds_rows; p.lr = (float)lr; p.kl_weight = (float)kl_weight; p.seed = (uint64_t)seed; p.t0 = t0;
  if (given(op_x)) {
    TORCH_CHECK(dev_tensor(*op_x, at::kLong, "op_x").dim() == 2 && op_x->size(1) == x.size(1), "op_x must be [n_ops, F]");
    TORCH_CHECK(given(row_op) && dev_tensor(*row_op, at::kLong, "row_op").numel() == p.R,
                "row_op must hold one operand per row");
    p.n_ops = op_x->size(0);
    p.op_x = op_x->data_ptr<int64_t>();
    p.row_op = row_op->data_ptr<int64_t>();
  }
  if (given(workspace)) fill_workspace(p, *workspace);
  if (given(grad)) {
    TORCH_CHECK(dev_tensor(*grad, at::kFloat, "grad").numel() >= p.E * (2 * (int64_t)p.d + 2), "grad must be [E, 2d + 2]");
    p.out_grad = grad->data_ptr<float>();
  }
  c10::hip::HIPGuard guard(x.get_device());
  check(vfm_foldin_f32(&p, stream_of(x)), "vfm_foldin_f32");
}

// what the six solves name alike: the rows, the tables, the workspace and four scalars
template <class S>
void fill_solve(S& p, const Tensor& entities, const Tensor& y, const Tensor& op_x, const Tensor& row_op,
                const Tensor& entity, const Tensor& bias, const Tensor& scalars, const Tensor& workspace, const Tensor& loss,
                int64_t col, int64_t flags, int64_t lds_dim, double kl_weight) {
  memset(&p, 0, sizeof(p));
  fill_fold_rows(p, entities, y, op_x, row_op, loss);
  fill_tables(p, entity, bias, scalars);
  fill_workspace(p, workspace);
  p.col = (int32_t)col; p.flags = (int32_t)flags; p.lds_dim = (int32_t)lds_dim; p.kl_weight = (float)kl_weight;
}

void foldin_solve(const Tensor& entities, const Tensor& row_ptr, const Tensor& y, const Tensor& op_x,
                  const Tensor& row_op, Tensor entity, Tensor bias, const Tensor& scalars, Tensor workspace, Tensor loss,
                  int64_t col, int64_t objective, int64_t likelihood, int64_t flags, int64_t lds_dim, double kl_weight) {
  vfm_foldin_solve_t p;
  fill_solve(p, entities, y, op_x, row_op, entity, bias, scalars, workspace, loss, col, flags, lds_dim, kl_weight);
  fill_row_list(p, row_ptr);
  p.objective = (int32_t)objective; p.likelihood = (int32_t)likelihood;
  c10::hip::HIPGuard guard(y.get_device());
  check(vfm_foldin_solve_f32(&p, stream_of(y)), "vfm_foldin_solve_f32");
}

void foldin_solve_prior(const Tensor& entities, const Tensor& row_ptr, const Tensor& y, const Tensor& op_x,
                        const Tensor& row_op, Tensor entity, Tensor bias, const Tensor& scalars, Tensor workspace,
                        Tensor loss, const Tensor& prior, int64_t col, int64_t objective, int64_t likelihood, int64_t flags,
                        int64_t lds_dim, double kl_weight) {
  vfm_foldin_solve_t p;
  fill_solve(p, entities, y, op_x, row_op, entity, bias, scalars, workspace, loss, col, flags, lds_dim, kl_weight);
  fill_row_list(p, row_ptr);
  p.objective = (int32_t)objective; p.likelihood = (int32_t)likelihood;
  c10::hip::HIPGuard guard(y.get_device());
  check(vfm_foldin_solve_prior_f32(&p, prior_of(prior, p.d), stream_of(y)), "vfm_foldin_solve_prior_f32");
}

void foldin_bound(const Tensor& entities, const Tensor& row_ptr, const Tensor& y, const Tensor& op_x,
                  const Tensor& row_op, Tensor entity, Tensor bias, const Tensor& scalars, Tensor workspace, Tensor loss,
                  int64_t col, int64_t objective, int64_t likelihood, int64_t flags, int64_t lds_dim, double kl_weight,
                  int64_t n_iters, int64_t reset, int64_t mode) {
  vfm_foldin_bound_t p;
  fill_solve(p, entities, y, op_x, row_op, entity, bias, scalars, workspace, loss, col, flags, lds_dim, kl_weight);
  fill_row_list(p, row_ptr);
  p.objective = (int32_t)objective; p.likelihood = (int32_t)likelihood;
  p.n_iters = (int32_t)n_iters; p.reset = (int32_t)reset; p.mode = (int32_t)mode;
  c10::hip::HIPGuard guard(y.get_device());
  check(vfm_foldin_bound_f32(&p, stream_of(y)), "vfm_foldin_bound_f32");
}

void foldin_bound_prior(const Tensor& entities, const Tensor& row_ptr, const Tensor& y, const Tensor& op_x,
                        const Tensor& row_op, Tensor entity, Tensor bias, const Tensor& scalars, Tensor workspace,
                        Tensor loss, const Tensor& prior, int64_t col, int64_t objective, int64_t likelihood, int64_t flags,
                        int64_t lds_dim, double kl_weight, int64_t n_iters, int64_t reset, int64_t mode) {
  vfm_foldin_bound_t p;
  fill_solve(p, entities, y, op_x, row_op, entity, bias, scalars, workspace, loss, col, flags, lds_dim, kl_weight);
  fill_row_list(p, row_ptr);
  p.objective = (int32_t)objective; p.likelihood = (int32_t)likelihood;
  p.n_iters = (int32_t)n_iters; p.reset = (int32_t)reset; p.mode = (int32_t)mode;
  c10::hip::HIPGuard guard(y.get_device());
  check(vfm_foldin_bound_prior_f32(&p, prior_of(prior, p.d), stream_of(y)), "vfm_foldin_bound_prior_f32");
}

void foldin_solve_split(const Tensor& entities, const Tensor& chunk_ptr, const Tensor& chunks, const Tensor& y,
                        const Tensor& op_x, const Tensor& row_op, Tensor entity, Tensor bias, const Tensor& scalars,
                        Tensor workspace, Tensor loss, int64_t col, int64_t flags, int64_t lds_dim, double kl_weight) {
  vfm_foldin_split_t p;
  fill_solve(p, entities, y, op_x, row_op, entity, bias, scalars, workspace, loss, col, flags, lds_dim, kl_weight);
  fill_chunk_table(p, chunk_ptr, chunks);
  c10::hip::HIPGuard guard(y.get_device());
  check(vfm_foldin_solve_split_f32(&p, stream_of(y)), "vfm_foldin_solve_split_f32");
}

void foldin_solve_split_prior(const Tensor& entities, const Tensor& chunk_ptr, const Tensor& chunks, const Tensor& y,
                              const Tensor& op_x, const Tensor& row_op, Tensor entity, Tensor bias, const Tensor& scalars,
                              Tensor workspace, Tensor loss, const Tensor& prior, int64_t col, int64_t flags,
                              int64_t lds_dim, double kl_weight) {
  vfm_foldin_split_t p;
  fill_solve(p, entities, y, op_x, row_op, entity, bias, scalars, workspace, loss, col, flags, lds_dim, kl_weight);
  fill_chunk_table(p, chunk_ptr, chunks);
  c10::hip::HIPGuard guard(y.get_device());
  check(vfm_foldin_solve_split_prior_f32(&p, prior_of(prior, p.d), stream_of(y)), "vfm_foldin_solve_split_prior_f32");
}

void foldin_bound_split(const Tensor& entities, const Tensor& chunk_ptr, const Tensor& chunks, const Tensor& y,
                        const Tensor& op_x, const Tensor& row_op, Tensor entity, Tensor bias, const Tensor& scalars,
                        Tensor workspace, Tensor loss, int64_t col, int64_t flags, int64_t lds_dim, double kl_weight,
                        int64_t n_iters, int64_t reset) {
  vfm_foldin_bound_split_t p;
  fill_solve(p, entities, y, op_x, row_op, entity, bias, scalars, workspace, loss, col, flags, lds_dim, kl_weight);
  fill_chunk_table(p, chunk_ptr, chunks);
  TORCH_CHECK(n_iters >= INT32_MIN && n_iters <= INT32_MAX, "n_iters out of range");
  p.n_iters = (int32_t)n_iters; p.reset = reset != 0;
  c10::hip::HIPGuard guard(y.get_device());
  check(vfm_foldin_bound_split_f32(&p, stream_of(y)), "vfm_foldin_bound_split_f32");
}

void foldin_bound_split_prior(const Tensor& entities, const Tensor& chunk_ptr, const Tensor& chunks, const Tensor& y,
                              const Tensor& op_x, const Tensor& row_op, Tensor entity, Tensor bias, const Tensor& scalars,
                              Tensor workspace, Tensor loss, const Tensor& prior, int64_t col, int64_t flags,
                              int64_t lds_dim, double kl_weight, int64_t n_iters, int64_t reset) {
  vfm_foldin_bound_split_t p;
  fill_solve(p, entities, y, op_x, row_op, entity, bias, scalars, workspace, loss, col, flags, lds_dim, kl_weight);
  fill_chunk_table(p, chunk_ptr, chunks);
  TORCH_CHECK(n_iters >= INT32_MIN && n_iters <= INT32_MAX, "n_iters out of range");
  p.n_iters = (int32_t)n_iters; p.reset = reset != 0;
  c10::hip::HIPGuard guard(y.get_device());
  check(vfm_foldin_bound_split_prior_f32(&p, prior_of(prior, p.d), stream_of(y)), "vfm_foldin_bound_split_prior_f32");
}

int64_t implicit_base_doubles(int64_t d) {
  return checked_bytes(vfm_implicit_base_doubles((int32_t)d), "vfm_implicit_base_doubles");
}

int64_t implicit_base_workspace_bytes(int64_t n, int64_t chunk_rows, int64_t d) {
  return checked_bytes(vfm_implicit_base_workspace_bytes(n, chunk_rows, (int32_t)d), "vfm_implicit_base_workspace_bytes");
}

int64_t implicit_solve_workspace_bytes(int64_t E, int64_t n_chunks, int64_t d, int64_t lds_dim) {
  return checked_bytes(vfm_implicit_solve_workspace_bytes(E, n_chunks, (int32_t)d, (int32_t)lds_dim),
                       "vfm_implicit_solve_workspace_bytes");
}

void implicit_base(const Tensor& entity, const Tensor& bias, const Tensor& scalars, Tensor workspace, Tensor base,
                   int64_t lo, int64_t n, int64_t chunk_rows, int64_t flags) {
  vfm_implicit_base_t p;
  memset(&p, 0, sizeof(p));
  dev_tensor(entity, at::kFloat, "entity_params"); dev_tensor(bias, at::kFloat, "bias_params");
  dev_tensor(scalars, at::kFloat, "scalars"); dev_tensor(base, at::kDouble, "base");
  TORCH_CHECK(entity.dim() == 2 && bias.dim() == 2 && bias.size(1) == 2 && bias.size(0) == entity.size(0) &&
              entity.size(1) % 2 == 0 && entity.size(1) >= 2 && scalars.numel() >= 3, "table shapes");
  p.T = entity.size(0); p.d = (int32_t)(entity.size(1) / 2);
  p.entity_params = entity.data_ptr<float>(); p.bias_params = bias.data_ptr<float>(); p.scalars = scalars.data_ptr<float>();
  TORCH_CHECK(base.numel() >= checked_bytes(vfm_implicit_base_doubles(p.d), "vfm_implicit_base_doubles"),
              "base [vfm_implicit_base_doubles(d)]");
  p.out_base = base.data_ptr<double>();
  fill_workspace(p, workspace);
  p.lo = lo; p.n = n; p.chunk_rows = chunk_rows; p.flags = (int32_t)flags;
  c10::hip::HIPGuard guard(entity.get_device());
  check(vfm_implicit_base_f32(&p, stream_of(entity)), "vfm_implicit_base_f32");
}

// what the implicit solve and its *_prior form name alike: everything but the prior
void fill_implicit_solve(vfm_implicit_solve_t& p, const Tensor& entities, const optional<Tensor>& row_ptr,
                         const optional<Tensor>& chunk_ptr, const optional<Tensor>& chunks, const Tensor& y,
                         const Tensor& partner, const Tensor& base, const Tensor& entity, const Tensor& bias,
                         const Tensor& scalars, const Tensor& workspace, const Tensor& loss, int64_t lo, int64_t n,
                         int64_t flags, int64_t lds_dim, double kl_weight, double w0, double w1) {
  memset(&p, 0, sizeof(p));
  dev_tensor(entities, at::kLong, "entities"); dev_tensor(y, at::kFloat, "y"); dev_tensor(partner, at::kLong, "partner");
  dev_tensor(base, at::kDouble, "base"); dev_tensor(loss, at::kFloat, "loss");
  TORCH_CHECK(partner.numel() == y.numel(), "partner [R] with y [R]");
  TORCH_CHECK(loss.numel() >= entities.numel(), "loss [E]");
  p.E = entities.numel(); p.R = y.numel();
  p.entities = entities.data_ptr<int64_t>(); p.y = y.data_ptr<float>(); p.partner = partner.data_ptr<int64_t>();
  p.out_loss = loss.data_ptr<float>();
  fill_tables(p, entity, bias, scalars);
  TORCH_CHECK(p.d >= 1 && base.numel() >= checked_bytes(vfm_implicit_base_doubles(p.d), "vfm_implicit_base_doubles"),
              "base [vfm_implicit_base_doubles(d)]");
  p.base = base.data_ptr<double>();
  fill_workspace(p, workspace);
  TORCH_CHECK(given(row_ptr) != given(chunk_ptr), "one of row_ptr and chunk_ptr");
  if (given(row_ptr)) {
    TORCH_CHECK(dev_tensor(*row_ptr, at::kLong, "row_ptr").numel() == p.E + 1, "row_ptr [E + 1]");
    p.row_ptr = row_ptr->data_ptr<int64_t>();
  } else {
    TORCH_CHECK(given(chunks), "chunk_ptr needs chunks");
    fill_chunk_table(p, *chunk_ptr, *chunks);
  }
  p.lo = lo; p.n = n; p.flags = (int32_t)flags; p.lds_dim = (int32_t)lds_dim;
  p.kl_weight = (float)kl_weight; p.w0 = (float)w0; p.w1 = (float)w1;
}

void foldin_solve_implicit(const Tensor& entities, const optional<Tensor>& row_ptr, const optional<Tensor>& chunk_ptr,
                           const optional<Tensor>& chunks, const Tensor& y, const Tensor& partner, const Tensor& base,
                           Tensor entity, Tensor bias, const Tensor& scalars, Tensor workspace, Tensor loss, int64_t lo,
                           int64_t n, int64_t flags, int64_t lds_dim, double kl_weight, double w0, double w1) {
  vfm_implicit_solve_t p;
  fill_implicit_solve(p, entities, row_ptr, chunk_ptr, chunks, y, partner, base, entity, bias, scalars, workspace, loss,
                      lo, n, flags, lds_dim, kl_weight, w0, w1);
  c10::hip::HIPGuard guard(y.get_device());
  check(vfm_foldin_solve_implicit_f32(&p, stream_of(y)), "vfm_foldin_solve_implicit_f32");
}

void foldin_solve_implicit_prior(const Tensor& entities, const optional<Tensor>& row_ptr,
                                 const optional<Tensor>& chunk_ptr, const optional<Tensor>& chunks, const Tensor& y,
                                 const Tensor& partner, const Tensor& base, Tensor entity, Tensor bias,
                                 const Tensor& scalars, Tensor workspace, Tensor loss, const Tensor& prior, int64_t lo,
                                 int64_t n, int64_t flags, int64_t lds_dim, double kl_weight, double w0, double w1) {
  vfm_implicit_solve_t p;
  fill_implicit_solve(p, entities, row_ptr, chunk_ptr, chunks, y, partner, base, entity, bias, scalars, workspace, loss,
                      lo, n, flags, lds_dim, kl_weight, w0, w1);
  c10::hip::HIPGuard guard(y.get_device());
  check(vfm_foldin_solve_implicit_prior_f32(&p, prior_of(prior, p.d), stream_of(y)), "vfm_foldin_solve_implicit_prior_f32");
}

// prior: the folded field's, or none for N(0, 1).  weights [R]: a weight per observed row, in y's order; there is no w1
void foldin_solve_implicit_weights(const Tensor& entities, const optional<Tensor>& row_ptr,
                                   const optional<Tensor>& chunk_ptr, const optional<Tensor>& chunks, const Tensor& y,
                                   const Tensor& partner, const Tensor& base, Tensor entity, Tensor bias,
                                   const Tensor& scalars, Tensor workspace, Tensor loss, const optional<Tensor>& prior,
                                   const Tensor& weights, int64_t lo, int64_t n, int64_t flags, int64_t lds_dim,
                                   double kl_weight, double w0) {
  vfm_implicit_solve_t p;
  // (w1 = w0: a call without rows has no weights array to point at and runs the call of one w1, which reads none)
  fill_implicit_solve(p, entities, row_ptr, chunk_ptr, chunks, y, partner, base, entity, bias, scalars, workspace, loss,
                      lo, n, flags, lds_dim, kl_weight, w0, w0);
  TORCH_CHECK(dev_tensor(weights, at::kFloat, "weights").numel() == y.numel(), "weights [R] with y [R]");
  c10::hip::HIPGuard guard(y.get_device());
  check(vfm_foldin_solve_implicit_weights_f32(&p, given(prior) ? prior_of(*prior, p.d) : nullptr,
                                              p.R > 0 ? weights.data_ptr<float>() : nullptr, stream_of(y)),
        "vfm_foldin_solve_implicit_weights_f32");
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
  m.def("foldin_solve_prior(Tensor entities, Tensor row_ptr, Tensor y, Tensor op_x, Tensor row_op, "
        "Tensor(a!) entity_params, Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) loss, "
        "Tensor prior, int col, int objective, int likelihood, int flags, int lds_dim, float kl_weight) -> ()",
        &foldin_solve_prior);
  m.def("foldin_bound_workspace_bytes(int E, int R, int n_ops, int d, int lds_dim) -> int", &foldin_bound_workspace_bytes);
  m.def("foldin_bound(Tensor entities, Tensor row_ptr, Tensor y, Tensor op_x, Tensor row_op, "
        "Tensor(a!) entity_params, Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) loss, "
        "int col, int objective, int likelihood, int flags, int lds_dim, float kl_weight, int n_iters, int reset, "
        "int mode) -> ()",
        &foldin_bound);
  m.def("foldin_bound_prior(Tensor entities, Tensor row_ptr, Tensor y, Tensor op_x, Tensor row_op, "
        "Tensor(a!) entity_params, Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) loss, "
        "Tensor prior, int col, int objective, int likelihood, int flags, int lds_dim, float kl_weight, int n_iters, "
        "int reset, int mode) -> ()",
        &foldin_bound_prior);
  m.def("foldin_split_workspace_bytes(int n_chunks, int n_heavy, int n_ops, int d, int lds_dim) -> int",
        &foldin_split_workspace_bytes);
  m.def("foldin_solve_split(Tensor entities, Tensor chunk_ptr, Tensor chunks, Tensor y, Tensor op_x, Tensor row_op, "
        "Tensor(a!) entity_params, Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) loss, "
        "int col, int flags, int lds_dim, float kl_weight) -> ()",
        &foldin_solve_split);
  m.def("foldin_solve_split_prior(Tensor entities, Tensor chunk_ptr, Tensor chunks, Tensor y, Tensor op_x, "
        "Tensor row_op, Tensor(a!) entity_params, Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, "
        "Tensor(d!) loss, Tensor prior, int col, int flags, int lds_dim, float kl_weight) -> ()",
        &foldin_solve_split_prior);
  m.def("foldin_bound_split_workspace_bytes(int n_chunks, int n_heavy, int R, int n_ops, int d, int lds_dim) -> int",
        &foldin_bound_split_workspace_bytes);
  m.def("foldin_bound_split(Tensor entities, Tensor chunk_ptr, Tensor chunks, Tensor y, Tensor op_x, Tensor row_op, "
        "Tensor(a!) entity_params, Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) loss, "
        "int col, int flags, int lds_dim, float kl_weight, int n_iters, int reset) -> ()",
        &foldin_bound_split);
  m.def("foldin_bound_split_prior(Tensor entities, Tensor chunk_ptr, Tensor chunks, Tensor y, Tensor op_x, "
        "Tensor row_op, Tensor(a!) entity_params, Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, "
        "Tensor(d!) loss, Tensor prior, int col, int flags, int lds_dim, float kl_weight, int n_iters, int reset) -> ()",
        &foldin_bound_split_prior);
  m.def("implicit_base_doubles(int d) -> int", &implicit_base_doubles);
  m.def("implicit_base_workspace_bytes(int n, int chunk_rows, int d) -> int", &implicit_base_workspace_bytes);
  m.def("implicit_base(Tensor entity_params, Tensor bias_params, Tensor scalars, Tensor(a!) workspace, Tensor(b!) base, "
        "int lo, int n, int chunk_rows, int flags) -> ()",
        &implicit_base);
  m.def("implicit_solve_workspace_bytes(int E, int n_chunks, int d, int lds_dim) -> int", &implicit_solve_workspace_bytes);
  m.def("foldin_solve_implicit(Tensor entities, Tensor? row_ptr, Tensor? chunk_ptr, Tensor? chunks, Tensor y, "
        "Tensor partner, Tensor base, Tensor(a!) entity_params, Tensor(b!) bias_params, Tensor scalars, "
        "Tensor(c!) workspace, Tensor(d!) loss, int lo, int n, int flags, int lds_dim, float kl_weight, float w0, "
        "float w1) -> ()",
        &foldin_solve_implicit);
  m.def("foldin_solve_implicit_prior(Tensor entities, Tensor? row_ptr, Tensor? chunk_ptr, Tensor? chunks, Tensor y, "
        "Tensor partner, Tensor base, Tensor(a!) entity_params, Tensor(b!) bias_params, Tensor scalars, "
        "Tensor(c!) workspace, Tensor(d!) loss, Tensor prior, int lo, int n, int flags, int lds_dim, float kl_weight, "
        "float w0, float w1) -> ()",
        &foldin_solve_implicit_prior);
  m.def("foldin_solve_implicit_weights(Tensor entities, Tensor? row_ptr, Tensor? chunk_ptr, Tensor? chunks, Tensor y, "
        "Tensor partner, Tensor base, Tensor(a!) entity_params, Tensor(b!) bias_params, Tensor scalars, "
        "Tensor(c!) workspace, Tensor(d!) loss, Tensor? prior, Tensor weights, int lo, int n, int flags, int lds_dim, "
        "float kl_weight, float w0) -> ()",
        &foldin_solve_implicit_weights);
}
