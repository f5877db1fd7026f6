// vfm_elicit_ops.cpp -- torch.ops.vfm_hip.{elicit, elicit_workspace_bytes, elicit_field, elicit_field_workspace_bytes,
// elicit_solve, elicit_solve_workspace_bytes, elicit_bound, elicit_bound_workspace_bytes}: the TORCH_LIBRARY fragment over
// include/vfm_elicit.h and the session of include/vfm_bound.h.  Like vfm_foldin_ops.cpp it only validates tensors, takes the current HIP stream of the tensors'
// device and forwards raw pointers; all arithmetic is in the HIP kernels.
#include <ATen/ATen.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <string.h>

#include <initializer_list>

#include "vfm_bound.h"
#include "vfm_elicit.h"

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

// The checks both ops make first, in their old order: every required tensor (the op names its own: rows, operands),
// the table shapes, n_rounds.
struct Named {
  const Tensor& t;
  at::ScalarType dt;
  const char* name;
};

void check_session_tensors(std::initializer_list<Named> own, const Tensor& entity, const Tensor& bias,
                           const Tensor& scalars, const Tensor& workspace, const Tensor& out_row, const Tensor& out_score,
                           const Tensor& out_loss, int64_t n_rounds) {
  for (const Named& n : own) dev_tensor(n.t, n.dt, n.name);
  dev_tensor(entity, at::kFloat, "entity_params"); dev_tensor(bias, at::kFloat, "bias_params");
  dev_tensor(scalars, at::kFloat, "scalars"); dev_tensor(workspace, at::kByte, "workspace");
  dev_tensor(out_row, at::kLong, "out_row"); dev_tensor(out_score, at::kFloat, "out_score");
  dev_tensor(out_loss, at::kFloat, "out_loss");
  TORCH_CHECK(entity.dim() == 2 && bias.dim() == 2 && bias.size(1) == 2 && bias.size(0) == entity.size(0) &&
              entity.size(1) % 2 == 0 && scalars.numel() >= 3, "table shapes");
  TORCH_CHECK(n_rounds >= 0 && n_rounds <= VFM_ELICIT_MAX_ROUNDS, "n_rounds out of range");
}

// The sizes, options, tables, outputs and workspace of p, which both structs name alike, with their size checks.
// P: vfm_elicit_t or vfm_elicit_field_t; U ids, n_pool pool rows.  The op adds its ids, rows, history and operands.
template <class P>
void fill_session(P& p, int64_t U, int64_t n_pool, int64_t F, const Tensor& pool_ptr, const Tensor& pool_y, Tensor& entity,
                  Tensor& bias, const Tensor& scalars, Tensor& workspace, Tensor& out_row, Tensor& out_score,
                  Tensor& out_loss, const optional<Tensor>& out_theta, const optional<Tensor>& out_mean,
                  const optional<Tensor>& out_var, int64_t Q, int64_t strategy, int64_t objective, int64_t likelihood,
                  int64_t flags, int64_t n_steps, int64_t n_samples, int64_t reset, int64_t write, int64_t lds_rows,
                  double lr, double kl_weight, int64_t seed, int64_t t0) {
  TORCH_CHECK(out_row.numel() >= U * Q && out_score.numel() >= U * Q && out_loss.numel() >= U * Q,
              "out_row, out_score, out_loss must be [U, Q]");
  VFM_STRUCT_INIT(p);
  p.U = U; p.P = n_pool; p.T = entity.size(0); p.F = (int32_t)F; p.d = (int32_t)(entity.size(1) / 2);
  p.n_rounds = (int32_t)Q; p.strategy = (int32_t)strategy; p.objective = (int32_t)objective;
  p.likelihood = (int32_t)likelihood; p.flags = (int32_t)flags; p.n_steps = (int32_t)n_steps;
  p.n_samples = (int32_t)n_samples; p.reset = (int32_t)reset; p.write = (int32_t)write; p.lds_rows = (int32_t)lds_rows;
  p.lr = (float)lr; p.kl_weight = (float)kl_weight; p.seed = (uint64_t)seed; p.t0 = t0;
  p.pool_ptr = pool_ptr.data_ptr<int64_t>(); p.pool_y = pool_y.data_ptr<float>();
  p.entity_params = entity.data_ptr<float>(); p.bias_params = bias.data_ptr<float>();
  p.scalars = scalars.data_ptr<float>();
  p.out_row = out_row.data_ptr<int64_t>(); p.out_score = out_score.data_ptr<float>();
  p.out_loss = out_loss.data_ptr<float>();
  if (given(out_theta)) {
    TORCH_CHECK(dev_tensor(*out_theta, at::kFloat, "out_theta").numel() >= U * Q * (2 * (int64_t)p.d + 2),
                "out_theta must be [U, Q, 2d + 2]");
    p.out_theta = out_theta->data_ptr<float>();
  }
  if (given(out_mean) || given(out_var)) {
    TORCH_CHECK(given(out_mean) && given(out_var), "out_mean and out_var: both or neither");
    TORCH_CHECK(dev_tensor(*out_mean, at::kFloat, "out_mean").numel() >= (Q + 1) * n_pool &&
                dev_tensor(*out_var, at::kFloat, "out_var").numel() >= (Q + 1) * n_pool,
                "out_mean, out_var must be [Q + 1, P]");
    p.out_mean = out_mean->data_ptr<float>();
    p.out_var = out_var->data_ptr<float>();
  }
  p.workspace = workspace.data_ptr();
  p.workspace_bytes = workspace.numel();
}

int64_t elicit_workspace_bytes(int64_t P, int64_t n_ops, int64_t d, int64_t objective) {
  const int64_t b = vfm_elicit_workspace_bytes(P, n_ops, (int32_t)d, (int32_t)objective);
  TORCH_CHECK(b >= 0, "vfm_elicit_workspace_bytes: bad arguments");
  return b;
}

void elicit(const Tensor& users, const Tensor& pool_ptr, const Tensor& pool_items, const Tensor& pool_y,
            const optional<Tensor>& hist_ptr, const optional<Tensor>& hist_items, const optional<Tensor>& hist_y,
            const optional<Tensor>& op_x, const optional<Tensor>& pool_op, const optional<Tensor>& hist_op,
            Tensor entity, Tensor bias, const Tensor& scalars, Tensor workspace, Tensor out_row, Tensor out_score,
            Tensor out_loss, const optional<Tensor>& out_theta, const optional<Tensor>& out_mean,
            const optional<Tensor>& out_var, int64_t n_rounds, int64_t strategy, int64_t objective, int64_t likelihood,
            int64_t flags, int64_t n_steps, int64_t n_samples, int64_t reset, int64_t write, int64_t lds_rows, double lr,
            double kl_weight, int64_t seed, int64_t t0) {
  check_session_tensors({{users, at::kLong, "users"}, {pool_ptr, at::kLong, "pool_ptr"},
                         {pool_items, at::kLong, "pool_items"}, {pool_y, at::kFloat, "pool_y"}},
                        entity, bias, scalars, workspace, out_row, out_score, out_loss, n_rounds);
  const int64_t U = users.numel(), P = pool_items.numel();
  TORCH_CHECK(pool_ptr.numel() == U + 1 && pool_y.numel() == P, "pool_ptr [U + 1], pool_y [P]");
  vfm_elicit_t p;
  fill_session(p, U, P, 2, pool_ptr, pool_y, entity, bias, scalars, workspace, out_row, out_score, out_loss, out_theta,
               out_mean, out_var, n_rounds, strategy, objective, likelihood, flags, n_steps, n_samples, reset, write,
               lds_rows, lr, kl_weight, seed, t0);
  p.users = users.data_ptr<int64_t>(); p.pool_items = pool_items.data_ptr<int64_t>();
  if (given(hist_ptr)) {
    TORCH_CHECK(given(hist_items) && given(hist_y), "hist_ptr needs hist_items and hist_y");
    dev_tensor(*hist_ptr, at::kLong, "hist_ptr"); dev_tensor(*hist_items, at::kLong, "hist_items");
    dev_tensor(*hist_y, at::kFloat, "hist_y");
    p.H = hist_items->numel();
    TORCH_CHECK(hist_ptr->numel() == p.U + 1 && hist_y->numel() == p.H, "hist_ptr [U + 1], hist_y [H]");
    p.hist_ptr = hist_ptr->data_ptr<int64_t>(); p.hist_items = hist_items->data_ptr<int64_t>();
    p.hist_y = hist_y->data_ptr<float>();
  }
  if (given(op_x)) {
    TORCH_CHECK(dev_tensor(*op_x, at::kLong, "op_x").dim() == 2 && op_x->size(1) == 2, "op_x must be [n_ops, 2]");
    TORCH_CHECK(given(pool_op) && dev_tensor(*pool_op, at::kLong, "pool_op").numel() == p.P,
                "pool_op must hold one operand per pool row");
    p.n_ops = op_x->size(0);
    p.op_x = op_x->data_ptr<int64_t>();
    p.pool_op = pool_op->data_ptr<int64_t>();
    if (p.H > 0) {
      TORCH_CHECK(given(hist_op) && dev_tensor(*hist_op, at::kLong, "hist_op").numel() == p.H,
                  "hist_op must hold one operand per history row");
      p.hist_op = hist_op->data_ptr<int64_t>();
    }
  }
  c10::hip::HIPGuard guard(users.get_device());
  const int rc = vfm_elicit_f32(&p, (void*)c10::hip::getCurrentHIPStream(users.get_device()).stream());
  TORCH_CHECK(rc == 0, "vfm_elicit_f32 failed (code ", rc, "): ", vfm_last_error());
}

int64_t elicit_field_workspace_bytes(int64_t P, int64_t n_ops, int64_t d, int64_t objective) {
  const int64_t b = vfm_elicit_field_workspace_bytes(P, n_ops, (int32_t)d, (int32_t)objective);
  TORCH_CHECK(b >= 0, "vfm_elicit_field_workspace_bytes: bad arguments");
  return b;
}

// the field form: pool_x [P, F] and hist_x [H, F] full rows, op_x [n_ops, F] the distinct contexts (both objectives)
void elicit_field(const Tensor& entities, const Tensor& pool_ptr, const Tensor& pool_x, const Tensor& pool_y,
                  const optional<Tensor>& hist_ptr, const optional<Tensor>& hist_x, const optional<Tensor>& hist_y,
                  const Tensor& op_x, const Tensor& pool_op, const optional<Tensor>& hist_op, Tensor entity, Tensor bias,
                  const Tensor& scalars, Tensor workspace, Tensor out_row, Tensor out_score, Tensor out_loss,
                  const optional<Tensor>& out_theta, const optional<Tensor>& out_mean, const optional<Tensor>& out_var,
                  int64_t field, int64_t key_col, int64_t n_rounds, int64_t strategy, int64_t objective,
                  int64_t likelihood, int64_t flags, int64_t n_steps, int64_t n_samples, int64_t reset, int64_t write,
                  int64_t lds_rows, double lr, double kl_weight, int64_t seed, int64_t t0) {
  check_session_tensors({{entities, at::kLong, "entities"}, {pool_ptr, at::kLong, "pool_ptr"}, {pool_x, at::kLong, "pool_x"},
                         {pool_y, at::kFloat, "pool_y"}, {op_x, at::kLong, "op_x"}, {pool_op, at::kLong, "pool_op"}},
                        entity, bias, scalars, workspace, out_row, out_score, out_loss, n_rounds);
  TORCH_CHECK(pool_x.dim() == 2 && pool_x.size(1) >= 2 && pool_x.size(1) <= VFM_MAX_FIELDS, "pool_x must be [P, F]");
  const int64_t U = entities.numel(), P = pool_x.size(0), F = pool_x.size(1);
  TORCH_CHECK(pool_ptr.numel() == U + 1 && pool_y.numel() == P, "pool_ptr [U + 1], pool_y [P]");
  TORCH_CHECK(op_x.dim() == 2 && op_x.size(1) == F && pool_op.numel() == P,
              "op_x must be [n_ops, F], pool_op must hold one operand per pool row");
  vfm_elicit_field_t p;
  fill_session(p, U, P, F, pool_ptr, pool_y, entity, bias, scalars, workspace, out_row, out_score, out_loss, out_theta,
               out_mean, out_var, n_rounds, strategy, objective, likelihood, flags, n_steps, n_samples, reset, write,
               lds_rows, lr, kl_weight, seed, t0);
  p.field = (int32_t)field; p.key_col = (int32_t)key_col;
  p.entities = entities.data_ptr<int64_t>(); p.pool_x = pool_x.data_ptr<int64_t>();
  p.n_ops = op_x.size(0);
  p.op_x = op_x.data_ptr<int64_t>(); p.pool_op = pool_op.data_ptr<int64_t>();
  if (given(hist_ptr)) {
    TORCH_CHECK(given(hist_x) && given(hist_y) && given(hist_op), "hist_ptr needs hist_x, hist_y and hist_op");
    dev_tensor(*hist_ptr, at::kLong, "hist_ptr"); dev_tensor(*hist_x, at::kLong, "hist_x");
    dev_tensor(*hist_y, at::kFloat, "hist_y"); dev_tensor(*hist_op, at::kLong, "hist_op");
    TORCH_CHECK(hist_x->dim() == 2 && hist_x->size(1) == F, "hist_x must be [H, F]");
    p.H = hist_x->size(0);
    TORCH_CHECK(hist_ptr->numel() == p.U + 1 && hist_y->numel() == p.H && hist_op->numel() == p.H,
                "hist_ptr [U + 1], hist_y [H], hist_op [H]");
    p.hist_ptr = hist_ptr->data_ptr<int64_t>(); p.hist_x = hist_x->data_ptr<int64_t>();
    p.hist_y = hist_y->data_ptr<float>(); p.hist_op = hist_op->data_ptr<int64_t>();
  }
  c10::hip::HIPGuard guard(entities.get_device());
  const int rc = vfm_elicit_field_f32(&p, (void*)c10::hip::getCurrentHIPStream(entities.get_device()).stream());
  TORCH_CHECK(rc == 0, "vfm_elicit_field_f32 failed (code ", rc, "): ", vfm_last_error());
}

int64_t elicit_solve_workspace_bytes(int64_t U, int64_t P, int64_t n_ops, int64_t d, int64_t lds_dim) {
  const int64_t b = vfm_elicit_solve_workspace_bytes(U, P, n_ops, (int32_t)d, (int32_t)lds_dim);
  TORCH_CHECK(b >= 0, "vfm_elicit_solve_workspace_bytes: bad arguments");
  return b;
}

// The tensors, sizes and options that the exact and the bound field-form sessions name alike, checked and put into p.
// S: vfm_elicit_solve_t or vfm_elicit_bound_t; the op adds its own options and the workspace check is the library's.
template <class S>
void fill_exact_session(S& p, const Tensor& entities, const Tensor& pool_ptr, const Tensor& pool_x, const Tensor& pool_y,
                        const optional<Tensor>& hist_ptr, const optional<Tensor>& hist_x, const optional<Tensor>& hist_y,
                        const Tensor& op_x, const Tensor& pool_op, const optional<Tensor>& hist_op, Tensor& entity,
                        Tensor& bias, const Tensor& scalars, Tensor& workspace, Tensor& out_row, Tensor& out_score,
                        Tensor& out_loss, const optional<Tensor>& out_theta, const optional<Tensor>& out_mean,
                        const optional<Tensor>& out_var, int64_t field, int64_t key_col, int64_t n_rounds, int64_t strategy,
                        int64_t flags, int64_t reset, int64_t write, int64_t lds_dim, double kl_weight, int64_t seed) {
  check_session_tensors({{entities, at::kLong, "entities"}, {pool_ptr, at::kLong, "pool_ptr"}, {pool_x, at::kLong, "pool_x"},
                         {pool_y, at::kFloat, "pool_y"}, {op_x, at::kLong, "op_x"}, {pool_op, at::kLong, "pool_op"}},
                        entity, bias, scalars, workspace, out_row, out_score, out_loss, n_rounds);
  TORCH_CHECK(pool_x.dim() == 2 && pool_x.size(1) >= 2 && pool_x.size(1) <= VFM_MAX_FIELDS, "pool_x must be [P, F]");
  const int64_t U = entities.numel(), P = pool_x.size(0), F = pool_x.size(1), Q = n_rounds;
  TORCH_CHECK(pool_ptr.numel() == U + 1 && pool_y.numel() == P, "pool_ptr [U + 1], pool_y [P]");
  TORCH_CHECK(op_x.dim() == 2 && op_x.size(1) == F && pool_op.numel() == P,
              "op_x must be [n_ops, F], pool_op must hold one operand per pool row");
  TORCH_CHECK(out_row.numel() >= U * Q && out_score.numel() >= U * Q && out_loss.numel() >= U * Q,
              "out_row, out_score, out_loss must be [U, Q]");
  VFM_STRUCT_INIT(p);
  p.U = U; p.P = P; p.T = entity.size(0); p.F = (int32_t)F; p.d = (int32_t)(entity.size(1) / 2);
  p.field = (int32_t)field; p.key_col = (int32_t)key_col; p.n_rounds = (int32_t)Q; p.strategy = (int32_t)strategy;
  p.flags = (int32_t)flags; p.reset = (int32_t)reset; p.write = (int32_t)write; p.lds_dim = (int32_t)lds_dim;
  p.kl_weight = (float)kl_weight; p.seed = (uint64_t)seed;
  p.entities = entities.data_ptr<int64_t>(); p.pool_ptr = pool_ptr.data_ptr<int64_t>();
  p.pool_x = pool_x.data_ptr<int64_t>(); p.pool_y = pool_y.data_ptr<float>();
  p.n_ops = op_x.size(0);
  p.op_x = op_x.data_ptr<int64_t>(); p.pool_op = pool_op.data_ptr<int64_t>();
  p.entity_params = entity.data_ptr<float>(); p.bias_params = bias.data_ptr<float>();
  p.scalars = scalars.data_ptr<float>();
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
  if (given(hist_ptr)) {
    TORCH_CHECK(given(hist_x) && given(hist_y) && given(hist_op), "hist_ptr needs hist_x, hist_y and hist_op");
    dev_tensor(*hist_ptr, at::kLong, "hist_ptr"); dev_tensor(*hist_x, at::kLong, "hist_x");
    dev_tensor(*hist_y, at::kFloat, "hist_y"); dev_tensor(*hist_op, at::kLong, "hist_op");
    TORCH_CHECK(hist_x->dim() == 2 && hist_x->size(1) == F, "hist_x must be [H, F]");
    p.H = hist_x->size(0);
    TORCH_CHECK(hist_ptr->numel() == p.U + 1 && hist_y->numel() == p.H && hist_op->numel() == p.H,
                "hist_ptr [U + 1], hist_y [H], hist_op [H]");
    p.hist_ptr = hist_ptr->data_ptr<int64_t>(); p.hist_x = hist_x->data_ptr<int64_t>();
    p.hist_y = hist_y->data_ptr<float>(); p.hist_op = hist_op->data_ptr<int64_t>();
  }
  p.workspace = workspace.data_ptr();
  p.workspace_bytes = workspace.numel();
}

// the exact field-form session: elicit_field's tensors, the exact fold-in's options in place of Adam's
void elicit_solve(const Tensor& entities, const Tensor& pool_ptr, const Tensor& pool_x, const Tensor& pool_y,
                  const optional<Tensor>& hist_ptr, const optional<Tensor>& hist_x, const optional<Tensor>& hist_y,
                  const Tensor& op_x, const Tensor& pool_op, const optional<Tensor>& hist_op, Tensor entity, Tensor bias,
                  const Tensor& scalars, Tensor workspace, Tensor out_row, Tensor out_score, Tensor out_loss,
                  const optional<Tensor>& out_theta, const optional<Tensor>& out_mean, const optional<Tensor>& out_var,
                  int64_t field, int64_t key_col, int64_t n_rounds, int64_t strategy, int64_t flags, int64_t reset,
                  int64_t write, int64_t lds_dim, double kl_weight, int64_t seed) {
  vfm_elicit_solve_t p;
  fill_exact_session(p, entities, pool_ptr, pool_x, pool_y, hist_ptr, hist_x, hist_y, op_x, pool_op, hist_op, entity, bias,
                     scalars, workspace, out_row, out_score, out_loss, out_theta, out_mean, out_var, field, key_col,
                     n_rounds, strategy, flags, reset, write, lds_dim, kl_weight, seed);
  c10::hip::HIPGuard guard(entities.get_device());
  const int rc = vfm_elicit_solve_f32(&p, (void*)c10::hip::getCurrentHIPStream(entities.get_device()).stream());
  TORCH_CHECK(rc == 0, "vfm_elicit_solve_f32 failed (code ", rc, "): ", vfm_last_error());
}

int64_t elicit_bound_workspace_bytes(int64_t U, int64_t P, int64_t H, int64_t n_ops, int64_t d, int64_t n_rounds,
                                     int64_t lds_dim) {
  const int64_t b = vfm_elicit_bound_workspace_bytes(U, P, H, n_ops, (int32_t)d, (int32_t)n_rounds, (int32_t)lds_dim);
  TORCH_CHECK(b >= 0, "vfm_elicit_bound_workspace_bytes: bad arguments");
  return b;
}

// the bound field-form session ('class' models): elicit_solve's tensors and options, and the rounds of the bound per fold
void elicit_bound(const Tensor& entities, const Tensor& pool_ptr, const Tensor& pool_x, const Tensor& pool_y,
                  const optional<Tensor>& hist_ptr, const optional<Tensor>& hist_x, const optional<Tensor>& hist_y,
                  const Tensor& op_x, const Tensor& pool_op, const optional<Tensor>& hist_op, Tensor entity, Tensor bias,
                  const Tensor& scalars, Tensor workspace, Tensor out_row, Tensor out_score, Tensor out_loss,
                  const optional<Tensor>& out_theta, const optional<Tensor>& out_mean, const optional<Tensor>& out_var,
                  int64_t field, int64_t key_col, int64_t n_rounds, int64_t strategy, int64_t flags, int64_t reset,
                  int64_t write, int64_t lds_dim, double kl_weight, int64_t seed, int64_t n_iters) {
  vfm_elicit_bound_t p;
  fill_exact_session(p, entities, pool_ptr, pool_x, pool_y, hist_ptr, hist_x, hist_y, op_x, pool_op, hist_op, entity, bias,
                     scalars, workspace, out_row, out_score, out_loss, out_theta, out_mean, out_var, field, key_col,
                     n_rounds, strategy, flags, reset, write, lds_dim, kl_weight, seed);
  TORCH_CHECK(n_iters >= 1 && n_iters <= INT32_MAX, "n_iters must be >= 1");
  p.n_iters = (int32_t)n_iters;
  c10::hip::HIPGuard guard(entities.get_device());
  const int rc = vfm_elicit_bound_f32(&p, (void*)c10::hip::getCurrentHIPStream(entities.get_device()).stream());
  TORCH_CHECK(rc == 0, "vfm_elicit_bound_f32 failed (code ", rc, "): ", vfm_last_error());
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(vfm_hip, m) {
  m.def("elicit_workspace_bytes(int P, int n_ops, int d, int objective) -> int", &elicit_workspace_bytes);
  m.def("elicit(Tensor users, Tensor pool_ptr, Tensor pool_items, Tensor pool_y, Tensor? hist_ptr, Tensor? hist_items, "
        "Tensor? hist_y, Tensor? op_x, Tensor? pool_op, Tensor? hist_op, Tensor(a!) entity_params, "
        "Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) out_row, Tensor(e!) out_score, "
        "Tensor(f!) out_loss, Tensor(g!)? out_theta, Tensor(h!)? out_mean, Tensor(i!)? out_var, int n_rounds, "
        "int strategy, int objective, int likelihood, int flags, int n_steps, int n_samples, int reset, int write, "
        "int lds_rows, float lr, float kl_weight, int seed, int t0) -> ()",
        &elicit);
  m.def("elicit_field_workspace_bytes(int P, int n_ops, int d, int objective) -> int", &elicit_field_workspace_bytes);
  m.def("elicit_field(Tensor entities, Tensor pool_ptr, Tensor pool_x, Tensor pool_y, Tensor? hist_ptr, Tensor? hist_x, "
        "Tensor? hist_y, Tensor op_x, Tensor pool_op, Tensor? hist_op, Tensor(a!) entity_params, "
        "Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) out_row, Tensor(e!) out_score, "
        "Tensor(f!) out_loss, Tensor(g!)? out_theta, Tensor(h!)? out_mean, Tensor(i!)? out_var, int field, int key_col, "
        "int n_rounds, int strategy, int objective, int likelihood, int flags, int n_steps, int n_samples, int reset, "
        "int write, int lds_rows, float lr, float kl_weight, int seed, int t0) -> ()",
        &elicit_field);
  m.def("elicit_solve_workspace_bytes(int U, int P, int n_ops, int d, int lds_dim) -> int", &elicit_solve_workspace_bytes);
  m.def("elicit_solve(Tensor entities, Tensor pool_ptr, Tensor pool_x, Tensor pool_y, Tensor? hist_ptr, Tensor? hist_x, "
        "Tensor? hist_y, Tensor op_x, Tensor pool_op, Tensor? hist_op, Tensor(a!) entity_params, "
        "Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) out_row, Tensor(e!) out_score, "
        "Tensor(f!) out_loss, Tensor(g!)? out_theta, Tensor(h!)? out_mean, Tensor(i!)? out_var, int field, int key_col, "
        "int n_rounds, int strategy, int flags, int reset, int write, int lds_dim, float kl_weight, int seed) -> ()",
        &elicit_solve);
  m.def("elicit_bound_workspace_bytes(int U, int P, int H, int n_ops, int d, int n_rounds, int lds_dim) -> int",
        &elicit_bound_workspace_bytes);
  m.def("elicit_bound(Tensor entities, Tensor pool_ptr, Tensor pool_x, Tensor pool_y, Tensor? hist_ptr, Tensor? hist_x, "
        "Tensor? hist_y, Tensor op_x, Tensor pool_op, Tensor? hist_op, Tensor(a!) entity_params, "
        "Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) out_row, Tensor(e!) out_score, "
        "Tensor(f!) out_loss, Tensor(g!)? out_theta, Tensor(h!)? out_mean, Tensor(i!)? out_var, int field, int key_col, "
        "int n_rounds, int strategy, int flags, int reset, int write, int lds_dim, float kl_weight, int seed, "
        "int n_iters) -> ()",
        &elicit_bound);
}
