// vfm_elicit_ops.cpp -- torch.ops.vfm_hip.{elicit, elicit_workspace_bytes, elicit_field, elicit_field_workspace_bytes,
// elicit_solve, elicit_solve_workspace_bytes, elicit_bound, elicit_bound_workspace_bytes, elicit_solve_prior,
// elicit_bound_prior, elicit_implicit, elicit_implicit_prior, elicit_implicit_workspace_bytes}: the TORCH_LIBRARY fragment
// over include/vfm_elicit.h, the session of include/vfm_bound.h, their forms under a field prior
// (include/vfm_elicit_prior.h) and the implicit session (include/vfm_elicit_implicit.h).  Like vfm_foldin_ops.cpp it only validates tensors, takes
// the current HIP stream of the tensors' device and forwards raw pointers; all arithmetic is in the HIP kernels.  Each
// session op is the parts of vfm_ops_common.hpp in sequence (rows, tables, workspace, outputs, history) plus its own
// options.
#include "vfm_ops_common.hpp"

#include "vfm_bound.h"
#include "vfm_elicit.h"
#include "vfm_elicit_implicit.h"
#include "vfm_elicit_prior.h"

namespace {

using namespace vfm_ops;

// the options of the two Adam forms (S: vfm_elicit_t or vfm_elicit_field_t)
template <class S>
void adam_options(S& p, int64_t strategy, int64_t objective, int64_t likelihood, int64_t flags, int64_t n_steps,
                  int64_t n_samples, int64_t reset, int64_t write, int64_t lds_rows, double lr, double kl_weight,
                  int64_t seed, int64_t t0) {
  p.strategy = (int32_t)strategy; p.objective = (int32_t)objective; p.likelihood = (int32_t)likelihood;
  p.flags = (int32_t)flags; p.n_steps = (int32_t)n_steps; p.n_samples = (int32_t)n_samples; p.reset = (int32_t)reset;
  p.write = (int32_t)write; p.lds_rows = (int32_t)lds_rows; p.lr = (float)lr; p.kl_weight = (float)kl_weight;
  p.seed = (uint64_t)seed; p.t0 = t0;
}

// the options of the exact and the bound form (S: vfm_elicit_solve_t or vfm_elicit_bound_t)
template <class S>
void solve_options(S& p, int64_t field, int64_t key_col, int64_t strategy, int64_t flags, int64_t reset, int64_t write,
                   int64_t lds_dim, double kl_weight, int64_t seed) {
  p.field = (int32_t)field; p.key_col = (int32_t)key_col; p.strategy = (int32_t)strategy; p.flags = (int32_t)flags;
  p.reset = (int32_t)reset; p.write = (int32_t)write; p.lds_dim = (int32_t)lds_dim; p.kl_weight = (float)kl_weight;
  p.seed = (uint64_t)seed;
}

int64_t elicit_workspace_bytes(int64_t P, int64_t n_ops, int64_t d, int64_t objective) {
  const int64_t b = vfm_elicit_workspace_bytes(P, n_ops, (int32_t)d, (int32_t)objective);
  TORCH_CHECK(b >= 0, "vfm_elicit_workspace_bytes: bad arguments");
  return b;
}

// the two-field form: its own rows (users, item ids), history and operands (the closed form's only)
void elicit(const Tensor& users, const Tensor& pool_ptr, const Tensor& pool_items, const Tensor& pool_y,
            const optional<Tensor>& hist_ptr, const optional<Tensor>& hist_items, const optional<Tensor>& hist_y,
            const optional<Tensor>& op_x, const optional<Tensor>& pool_op, const optional<Tensor>& hist_op,
            Tensor entity, Tensor bias, const Tensor& scalars, Tensor workspace, Tensor out_row, Tensor out_score,
            Tensor out_loss, const optional<Tensor>& out_theta, const optional<Tensor>& out_mean,
            const optional<Tensor>& out_var, int64_t n_rounds, int64_t strategy, int64_t objective, int64_t likelihood,
            int64_t flags, int64_t n_steps, int64_t n_samples, int64_t reset, int64_t write, int64_t lds_rows, double lr,
            double kl_weight, int64_t seed, int64_t t0) {
  vfm_elicit_t p;
  VFM_STRUCT_INIT(p);
  dev_tensor(users, at::kLong, "users"); dev_tensor(pool_ptr, at::kLong, "pool_ptr");
  dev_tensor(pool_items, at::kLong, "pool_items"); dev_tensor(pool_y, at::kFloat, "pool_y");
  p.U = users.numel(); p.P = pool_items.numel(); p.F = 2;
  TORCH_CHECK(pool_ptr.numel() == p.U + 1 && pool_y.numel() == p.P, "pool_ptr [U + 1], pool_y [P]");
  p.users = users.data_ptr<int64_t>(); p.pool_ptr = pool_ptr.data_ptr<int64_t>();
  p.pool_items = pool_items.data_ptr<int64_t>(); p.pool_y = pool_y.data_ptr<float>();
  fill_tables(p, entity, bias, scalars);
  fill_workspace(p, workspace);
  fill_session_outputs(p, n_rounds, out_row, out_score, out_loss, out_theta, out_mean, out_var);
  adam_options(p, strategy, objective, likelihood, flags, n_steps, n_samples, reset, write, lds_rows, lr, kl_weight, seed,
               t0);
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
  check(vfm_elicit_f32(&p, stream_of(users)), "vfm_elicit_f32");
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
  vfm_elicit_field_t p;
  VFM_STRUCT_INIT(p);
  fill_field_rows(p, entities, pool_ptr, pool_x, &pool_y, op_x, pool_op);
  fill_tables(p, entity, bias, scalars);
  fill_workspace(p, workspace);
  fill_session_outputs(p, n_rounds, out_row, out_score, out_loss, out_theta, out_mean, out_var);
  fill_field_history(p, hist_ptr, hist_x, hist_y, hist_op);
  p.field = (int32_t)field; p.key_col = (int32_t)key_col;
  adam_options(p, strategy, objective, likelihood, flags, n_steps, n_samples, reset, write, lds_rows, lr, kl_weight, seed,
               t0);
  c10::hip::HIPGuard guard(entities.get_device());
  check(vfm_elicit_field_f32(&p, stream_of(entities)), "vfm_elicit_field_f32");
}

int64_t elicit_solve_workspace_bytes(int64_t U, int64_t P, int64_t n_ops, int64_t d, int64_t lds_dim) {
  const int64_t b = vfm_elicit_solve_workspace_bytes(U, P, n_ops, (int32_t)d, (int32_t)lds_dim);
  TORCH_CHECK(b >= 0, "vfm_elicit_solve_workspace_bytes: bad arguments");
  return b;
}

// the exact field-form session: elicit_field's tensors, the exact fold-in's options in place of Adam's; prior: NULL, or
// the respondents' field prior [2, d + 1] (elicit_solve_prior)
void elicit_solve_call(const Tensor* prior, const Tensor& entities, const Tensor& pool_ptr, const Tensor& pool_x, const Tensor& pool_y,
                  const optional<Tensor>& hist_ptr, const optional<Tensor>& hist_x, const optional<Tensor>& hist_y,
                  const Tensor& op_x, const Tensor& pool_op, const optional<Tensor>& hist_op, Tensor entity, Tensor bias,
                  const Tensor& scalars, Tensor workspace, Tensor out_row, Tensor out_score, Tensor out_loss,
                  const optional<Tensor>& out_theta, const optional<Tensor>& out_mean, const optional<Tensor>& out_var,
                  int64_t field, int64_t key_col, int64_t n_rounds, int64_t strategy, int64_t flags, int64_t reset,
                  int64_t write, int64_t lds_dim, double kl_weight, int64_t seed) {
  vfm_elicit_solve_t p;
  VFM_STRUCT_INIT(p);
  fill_field_rows(p, entities, pool_ptr, pool_x, &pool_y, op_x, pool_op);
  fill_tables(p, entity, bias, scalars);
  fill_workspace(p, workspace);
  fill_session_outputs(p, n_rounds, out_row, out_score, out_loss, out_theta, out_mean, out_var);
  fill_field_history(p, hist_ptr, hist_x, hist_y, hist_op);
  solve_options(p, field, key_col, strategy, flags, reset, write, lds_dim, kl_weight, seed);
  c10::hip::HIPGuard guard(entities.get_device());
  if (prior) check(vfm_elicit_solve_prior_f32(&p, prior_of(*prior, p.d), stream_of(entities)), "vfm_elicit_solve_prior_f32");
  else check(vfm_elicit_solve_f32(&p, stream_of(entities)), "vfm_elicit_solve_f32");
}

#define VFM_SESSION_TENSORS                                                                                              \
  const Tensor &entities, const Tensor &pool_ptr, const Tensor &pool_x, const Tensor &pool_y,                            \
      const optional<Tensor>&hist_ptr, const optional<Tensor>&hist_x, const optional<Tensor>&hist_y, const Tensor &op_x, \
      const Tensor &pool_op, const optional<Tensor>&hist_op, Tensor entity, Tensor bias, const Tensor &scalars,          \
      Tensor workspace, Tensor out_row, Tensor out_score, Tensor out_loss, const optional<Tensor>&out_theta,             \
      const optional<Tensor>&out_mean, const optional<Tensor>&out_var
#define VFM_SESSION_TENSOR_NAMES                                                                                         \
  entities, pool_ptr, pool_x, pool_y, hist_ptr, hist_x, hist_y, op_x, pool_op, hist_op, entity, bias, scalars, workspace, \
      out_row, out_score, out_loss, out_theta, out_mean, out_var

void elicit_solve(VFM_SESSION_TENSORS, int64_t field, int64_t key_col, int64_t n_rounds, int64_t strategy, int64_t flags,
                  int64_t reset, int64_t write, int64_t lds_dim, double kl_weight, int64_t seed) {
  elicit_solve_call(nullptr, VFM_SESSION_TENSOR_NAMES, field, key_col, n_rounds, strategy, flags, reset, write, lds_dim,
                    kl_weight, seed);
}

void elicit_solve_prior(VFM_SESSION_TENSORS, const Tensor& prior, int64_t field, int64_t key_col, int64_t n_rounds,
                        int64_t strategy, int64_t flags, int64_t reset, int64_t write, int64_t lds_dim, double kl_weight,
                        int64_t seed) {
  elicit_solve_call(&prior, VFM_SESSION_TENSOR_NAMES, field, key_col, n_rounds, strategy, flags, reset, write, lds_dim,
                    kl_weight, seed);
}

int64_t elicit_bound_workspace_bytes(int64_t U, int64_t P, int64_t H, int64_t n_ops, int64_t d, int64_t n_rounds,
                                     int64_t lds_dim) {
  const int64_t b = vfm_elicit_bound_workspace_bytes(U, P, H, n_ops, (int32_t)d, (int32_t)n_rounds, (int32_t)lds_dim);
  TORCH_CHECK(b >= 0, "vfm_elicit_bound_workspace_bytes: bad arguments");
  return b;
}

// the bound field-form session ('class' models): elicit_solve's tensors and options, and the rounds of the bound per
// fold; prior: as elicit_solve_call's (elicit_bound_prior)
void elicit_bound_call(const Tensor* prior, const Tensor& entities, const Tensor& pool_ptr, const Tensor& pool_x, const Tensor& pool_y,
                  const optional<Tensor>& hist_ptr, const optional<Tensor>& hist_x, const optional<Tensor>& hist_y,
                  const Tensor& op_x, const Tensor& pool_op, const optional<Tensor>& hist_op, Tensor entity, Tensor bias,
                  const Tensor& scalars, Tensor workspace, Tensor out_row, Tensor out_score, Tensor out_loss,
                  const optional<Tensor>& out_theta, const optional<Tensor>& out_mean, const optional<Tensor>& out_var,
                  int64_t field, int64_t key_col, int64_t n_rounds, int64_t strategy, int64_t flags, int64_t reset,
                  int64_t write, int64_t lds_dim, double kl_weight, int64_t seed, int64_t n_iters) {
  vfm_elicit_bound_t p;
  VFM_STRUCT_INIT(p);
  fill_field_rows(p, entities, pool_ptr, pool_x, &pool_y, op_x, pool_op);
  fill_tables(p, entity, bias, scalars);
  fill_workspace(p, workspace);
  fill_session_outputs(p, n_rounds, out_row, out_score, out_loss, out_theta, out_mean, out_var);
  fill_field_history(p, hist_ptr, hist_x, hist_y, hist_op);
  solve_options(p, field, key_col, strategy, flags, reset, write, lds_dim, kl_weight, seed);
  TORCH_CHECK(n_iters >= 1 && n_iters <= INT32_MAX, "n_iters must be >= 1");
  p.n_iters = (int32_t)n_iters;
  c10::hip::HIPGuard guard(entities.get_device());
  if (prior) check(vfm_elicit_bound_prior_f32(&p, prior_of(*prior, p.d), stream_of(entities)), "vfm_elicit_bound_prior_f32");
  else check(vfm_elicit_bound_f32(&p, stream_of(entities)), "vfm_elicit_bound_f32");
}

void elicit_bound(VFM_SESSION_TENSORS, int64_t field, int64_t key_col, int64_t n_rounds, int64_t strategy, int64_t flags,
                  int64_t reset, int64_t write, int64_t lds_dim, double kl_weight, int64_t seed, int64_t n_iters) {
  elicit_bound_call(nullptr, VFM_SESSION_TENSOR_NAMES, field, key_col, n_rounds, strategy, flags, reset, write, lds_dim,
                    kl_weight, seed, n_iters);
}

void elicit_bound_prior(VFM_SESSION_TENSORS, const Tensor& prior, int64_t field, int64_t key_col, int64_t n_rounds,
                        int64_t strategy, int64_t flags, int64_t reset, int64_t write, int64_t lds_dim, double kl_weight,
                        int64_t seed, int64_t n_iters) {
  elicit_bound_call(&prior, VFM_SESSION_TENSOR_NAMES, field, key_col, n_rounds, strategy, flags, reset, write, lds_dim,
                    kl_weight, seed, n_iters);
}

int64_t elicit_implicit_workspace_bytes(int64_t U, int64_t P, int64_t n_ops, int64_t d, int64_t lds_dim) {
  const int64_t b = vfm_elicit_implicit_workspace_bytes(U, P, n_ops, (int32_t)d, (int32_t)lds_dim);
  TORCH_CHECK(b >= 0, "vfm_elicit_implicit_workspace_bytes: bad arguments");
  return b;
}

// the implicit field-form session (two-field 'reg' models): elicit_solve's tensors and options, the partner field's base
// block, its id range and the two weights; prior: as elicit_solve_call's (elicit_implicit_prior)
void elicit_implicit_call(const Tensor* prior, VFM_SESSION_TENSORS, const Tensor& base, int64_t field, int64_t key_col,
                          int64_t n_rounds, int64_t strategy, int64_t flags, int64_t reset, int64_t write, int64_t lds_dim,
                          double kl_weight, int64_t seed, int64_t lo, int64_t n, double w0, double w1) {
  vfm_elicit_solve_t p;
  VFM_STRUCT_INIT(p);
  fill_field_rows(p, entities, pool_ptr, pool_x, &pool_y, op_x, pool_op);
  fill_tables(p, entity, bias, scalars);
  fill_workspace(p, workspace);
  fill_session_outputs(p, n_rounds, out_row, out_score, out_loss, out_theta, out_mean, out_var);
  fill_field_history(p, hist_ptr, hist_x, hist_y, hist_op);
  solve_options(p, field, key_col, strategy, flags, reset, write, lds_dim, kl_weight, seed);
  dev_tensor(base, at::kDouble, "base");
  TORCH_CHECK(p.d >= 1 && p.d <= VFM_FOLDIN_MAX_D && base.numel() >= vfm_implicit_base_doubles(p.d),
              "base [vfm_implicit_base_doubles(d)]");
  vfm_elicit_implicit_t imp;
  imp.w0 = (float)w0; imp.w1 = (float)w1; imp.lo = lo; imp.n = n; imp.base = base.data_ptr<double>();
  c10::hip::HIPGuard guard(entities.get_device());
  check(vfm_elicit_implicit_f32(&p, &imp, prior ? prior_of(*prior, p.d) : nullptr, stream_of(entities)),
        "vfm_elicit_implicit_f32");
}

void elicit_implicit(VFM_SESSION_TENSORS, const Tensor& base, int64_t field, int64_t key_col, int64_t n_rounds,
                     int64_t strategy, int64_t flags, int64_t reset, int64_t write, int64_t lds_dim, double kl_weight,
                     int64_t seed, int64_t lo, int64_t n, double w0, double w1) {
  elicit_implicit_call(nullptr, VFM_SESSION_TENSOR_NAMES, base, field, key_col, n_rounds, strategy, flags, reset, write,
                       lds_dim, kl_weight, seed, lo, n, w0, w1);
}

void elicit_implicit_prior(VFM_SESSION_TENSORS, const Tensor& prior, const Tensor& base, int64_t field, int64_t key_col,
                           int64_t n_rounds, int64_t strategy, int64_t flags, int64_t reset, int64_t write,
                           int64_t lds_dim, double kl_weight, int64_t seed, int64_t lo, int64_t n, double w0, double w1) {
  elicit_implicit_call(&prior, VFM_SESSION_TENSOR_NAMES, base, field, key_col, n_rounds, strategy, flags, reset, write,
                       lds_dim, kl_weight, seed, lo, n, w0, w1);
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
  m.def("elicit_solve_prior(Tensor entities, Tensor pool_ptr, Tensor pool_x, Tensor pool_y, Tensor? hist_ptr, "
        "Tensor? hist_x, Tensor? hist_y, Tensor op_x, Tensor pool_op, Tensor? hist_op, Tensor(a!) entity_params, "
        "Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) out_row, Tensor(e!) out_score, "
        "Tensor(f!) out_loss, Tensor(g!)? out_theta, Tensor(h!)? out_mean, Tensor(i!)? out_var, Tensor prior, int field, "
        "int key_col, int n_rounds, int strategy, int flags, int reset, int write, int lds_dim, float kl_weight, "
        "int seed) -> ()",
        &elicit_solve_prior);
  m.def("elicit_bound_prior(Tensor entities, Tensor pool_ptr, Tensor pool_x, Tensor pool_y, Tensor? hist_ptr, "
        "Tensor? hist_x, Tensor? hist_y, Tensor op_x, Tensor pool_op, Tensor? hist_op, Tensor(a!) entity_params, "
        "Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) out_row, Tensor(e!) out_score, "
        "Tensor(f!) out_loss, Tensor(g!)? out_theta, Tensor(h!)? out_mean, Tensor(i!)? out_var, Tensor prior, int field, "
        "int key_col, int n_rounds, int strategy, int flags, int reset, int write, int lds_dim, float kl_weight, "
        "int seed, int n_iters) -> ()",
        &elicit_bound_prior);
  m.def("elicit_implicit_workspace_bytes(int U, int P, int n_ops, int d, int lds_dim) -> int",
        &elicit_implicit_workspace_bytes);
  m.def("elicit_implicit(Tensor entities, Tensor pool_ptr, Tensor pool_x, Tensor pool_y, Tensor? hist_ptr, Tensor? hist_x, "
        "Tensor? hist_y, Tensor op_x, Tensor pool_op, Tensor? hist_op, Tensor(a!) entity_params, "
        "Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) out_row, Tensor(e!) out_score, "
        "Tensor(f!) out_loss, Tensor(g!)? out_theta, Tensor(h!)? out_mean, Tensor(i!)? out_var, Tensor base, int field, "
        "int key_col, int n_rounds, int strategy, int flags, int reset, int write, int lds_dim, float kl_weight, "
        "int seed, int lo, int n, float w0, float w1) -> ()",
        &elicit_implicit);
  m.def("elicit_implicit_prior(Tensor entities, Tensor pool_ptr, Tensor pool_x, Tensor pool_y, Tensor? hist_ptr, "
        "Tensor? hist_x, Tensor? hist_y, Tensor op_x, Tensor pool_op, Tensor? hist_op, Tensor(a!) entity_params, "
        "Tensor(b!) bias_params, Tensor scalars, Tensor(c!) workspace, Tensor(d!) out_row, Tensor(e!) out_score, "
        "Tensor(f!) out_loss, Tensor(g!)? out_theta, Tensor(h!)? out_mean, Tensor(i!)? out_var, Tensor prior, Tensor base, "
        "int field, int key_col, int n_rounds, int strategy, int flags, int reset, int write, int lds_dim, "
        "float kl_weight, int seed, int lo, int n, float w0, float w1) -> ()",
        &elicit_implicit_prior);
}
