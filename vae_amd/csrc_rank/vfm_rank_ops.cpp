// vfm_rank_ops.cpp -- the TORCH_LIBRARY fragment over include/vfm_rank.h.  Its ops, all in torch.ops.vfm_hip:
//   moments    predictive_moments, field_moments, field_moments_post
//   top k      rank_items, rank_field, rank_field_post
//   held out   rank_heldout, rank_heldout_field, rank_heldout_field_post
//   workspace  rank_workspace_bytes, rank_field_workspace_bytes, rank_eval_workspace_bytes,
//              rank_eval_field_workspace_bytes
// Like vfm_torch_ops.cpp it only validates tensors, takes the current HIP stream of the tensors' device and forwards raw
// pointers; all arithmetic is in the HIP kernels.  An op is a sequence of the pieces below plus its own scalars.
#include "vfm_ops_common.hpp"

#include "vfm_rank.h"

namespace {

using namespace vfm_ops;

// ---- the pieces

// the tables and the workspace of a call (fill_tables, fill_workspace)
struct Model {
  int64_t T = 0, workspace_bytes = 0;
  int32_t d = 0;
  const float *entity_params = nullptr, *bias_params = nullptr, *scalars = nullptr;
  void* workspace = nullptr;
};

// a contiguous [rows, F] id matrix on the GPU: int64, or with `or_int32` either width
const Tensor& id_matrix(const Tensor& x, const char* name, bool or_int32) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2, name, " must be a contiguous [rows,F] GPU tensor");
  TORCH_CHECK(x.scalar_type() == at::kLong || (or_int32 && x.scalar_type() == at::kInt), name,
              or_int32 ? " must be int64 or int32" : " must be int64");
  return x;
}

int32_t id_bits(const Tensor& x) { return x.scalar_type() == at::kLong ? 64 : 32; }

// an optional int64 id list of n ids: NULL when it is not given
const int64_t* id_list(const optional<Tensor>& t, int64_t n, const char* name) {
  if (!given(t)) return nullptr;
  TORCH_CHECK(dev_tensor(*t, at::kLong, name).numel() == n, name, " must hold ", n, " ids");
  return t->data_ptr<int64_t>();
}

// a CSR over Q queries: ptr [Q + 1] and the items it cuts up (items NULL when there are none)
struct Csr {
  const int64_t *ptr = nullptr, *items = nullptr;
  int64_t n = 0;
};

Csr csr_of(const Tensor& ptr, const Tensor& items, int64_t Q, const char* ptr_name, const char* items_name) {
  TORCH_CHECK(dev_tensor(ptr, at::kLong, ptr_name).numel() == Q + 1, ptr_name, " needs one offset per query and one more");
  Csr c;
  c.ptr = ptr.data_ptr<int64_t>();
  c.n = dev_tensor(items, at::kLong, items_name).numel();
  c.items = c.n > 0 ? items.data_ptr<int64_t>() : nullptr;
  return c;
}

// the optional exclusion lists
Csr exclusions_of(const optional<Tensor>& ptr, const optional<Tensor>& items, int64_t Q) {
  if (!given(ptr)) return Csr();
  TORCH_CHECK(given(items), "excl_ptr without excl_items");
  return csr_of(*ptr, *items, Q, "excl_ptr", "excl_items");
}

// The supplied posteriors of the *_post ops: [rows, 2d + 2] fp32, one row per query
const float* post_rows(const Tensor& post, int64_t rows, const Model& m) {
  dev_tensor(post, at::kFloat, "post");
  TORCH_CHECK(post.dim() == 2 && post.size(0) == rows && post.size(1) == 2 * (int64_t)m.d + 2,
              "post must be [Q, 2d + 2], one row per query");
  return post.data_ptr<float>();
}

// the moments of n rows, the score optional
struct Moments {
  float *mean, *var, *score;
};

Moments moment_outputs(const Tensor& logit_mean, const Tensor& logit_var, const optional<Tensor>& score, int64_t n) {
  TORCH_CHECK(dev_tensor(logit_mean, at::kFloat, "logit_mean").numel() >= n &&
              dev_tensor(logit_var, at::kFloat, "logit_var").numel() >= n, "output sizes");
  Moments o{logit_mean.data_ptr<float>(), logit_var.data_ptr<float>(), nullptr};
  if (given(score)) {
    TORCH_CHECK(dev_tensor(*score, at::kFloat, "score").numel() >= n, "score too small");
    o.score = score->data_ptr<float>();
  }
  return o;
}

// the top k of Q queries: four [Q, k] outputs
struct TopK {
  int64_t* items;
  float *score, *mean, *var;
};

TopK topk_outputs(const Tensor& items, const Tensor& score, const Tensor& logit_mean, const Tensor& logit_var, int64_t n) {
  TORCH_CHECK(dev_tensor(items, at::kLong, "items").numel() >= n && dev_tensor(score, at::kFloat, "score").numel() >= n &&
              dev_tensor(logit_mean, at::kFloat, "logit_mean").numel() >= n &&
              dev_tensor(logit_var, at::kFloat, "logit_var").numel() >= n, "output sizes");
  return TopK{items.data_ptr<int64_t>(), score.data_ptr<float>(), logit_mean.data_ptr<float>(),
              logit_var.data_ptr<float>()};
}

// the held-out evaluation of n_pos positives of Q queries
struct Heldout {
  int64_t *rank, *rank_neg, *n_eligible, *n_neg;
};

Heldout heldout_outputs(const Tensor& rank, const Tensor& rank_neg, const Tensor& n_eligible, const Tensor& n_neg,
                        int64_t n_pos, int64_t Q) {
  TORCH_CHECK(dev_tensor(rank, at::kLong, "rank").numel() >= n_pos &&
              dev_tensor(rank_neg, at::kLong, "rank_neg").numel() >= n_pos &&
              dev_tensor(n_eligible, at::kLong, "n_eligible").numel() >= Q &&
              dev_tensor(n_neg, at::kLong, "n_neg").numel() >= Q, "output sizes");
  return Heldout{rank.data_ptr<int64_t>(), rank_neg.data_ptr<int64_t>(), n_eligible.data_ptr<int64_t>(),
                 n_neg.data_ptr<int64_t>()};
}

int64_t bytes_of(int64_t b, const char* what) {
  TORCH_CHECK(b >= 0, what, ": bad arguments");
  return b;
}

// ---- the two-field ops

void predictive_moments(const Tensor& x, const Tensor& entity, const Tensor& bias, const Tensor& scalars,
                        Tensor logit_mean, Tensor logit_var, const optional<Tensor>& score, int64_t flags,
                        int64_t strategy, int64_t seed) {
  const int64_t B = id_matrix(x, "x", true).size(0);
  Model m;
  fill_tables(m, entity, bias, scalars);
  const Moments o = moment_outputs(logit_mean, logit_var, score, B);
  c10::hip::HIPGuard guard(x.get_device());
  check(vfm_predictive_moments_f32(B, (int32_t)x.size(1), m.d, m.T, id_bits(x), (int32_t)flags, x.data_ptr(),
                                   m.entity_params, m.bias_params, m.scalars, (int32_t)strategy, (uint64_t)seed, o.mean,
                                   o.var, o.score, stream_of(x)),
        "vfm_predictive_moments_f32");
}

int64_t rank_workspace_bytes(int64_t U, int64_t n_cand, int64_t d, int64_t k, int64_t strategy, int64_t n_splits) {
  return bytes_of(vfm_rank_workspace_bytes(U, n_cand, (int32_t)d, (int32_t)k, (int32_t)strategy, (int32_t)n_splits),
                  "vfm_rank_workspace_bytes");
}

void rank_items(const Tensor& users, const optional<Tensor>& cand, int64_t n_cand, int64_t item_lo,
                const optional<Tensor>& excl_ptr, const optional<Tensor>& excl_items, const Tensor& entity,
                const Tensor& bias, const Tensor& scalars, Tensor workspace, Tensor items, Tensor score,
                Tensor logit_mean, Tensor logit_var, int64_t F, int64_t k, int64_t strategy, int64_t flags,
                int64_t seed, int64_t n_splits) {
  const int64_t U = dev_tensor(users, at::kLong, "users").numel();
  Model m;
  fill_tables(m, entity, bias, scalars);
  fill_workspace(m, workspace);
  const int64_t* cp = id_list(cand, n_cand, "cand");
  const Csr ex = exclusions_of(excl_ptr, excl_items, U);
  const TopK o = topk_outputs(items, score, logit_mean, logit_var, U * k);
  c10::hip::HIPGuard guard(users.get_device());
  check(vfm_rank_items_f32(U, users.data_ptr<int64_t>(), n_cand, cp, item_lo, m.T, (int32_t)F, m.d, (int32_t)k,
                           (int32_t)strategy, (int32_t)flags, (uint64_t)seed, (int32_t)n_splits, ex.ptr, ex.items, ex.n,
                           m.entity_params, m.bias_params, m.scalars, m.workspace, m.workspace_bytes, o.items, o.score,
                           o.mean, o.var, stream_of(users)),
        "vfm_rank_items_f32");
}

int64_t rank_eval_workspace_bytes(int64_t U, int64_t n_cand, int64_t n_pos, int64_t d, int64_t strategy,
                                  int64_t n_splits) {
  return bytes_of(vfm_rank_eval_workspace_bytes(U, n_cand, n_pos, (int32_t)d, (int32_t)strategy, (int32_t)n_splits),
                  "vfm_rank_eval_workspace_bytes");
}

void rank_heldout(const Tensor& users, const optional<Tensor>& cand, int64_t n_cand, int64_t item_lo,
                  const optional<Tensor>& excl_ptr, const optional<Tensor>& excl_items, const Tensor& pos_ptr,
                  const Tensor& pos_items, const Tensor& entity, const Tensor& bias, const Tensor& scalars,
                  Tensor workspace, Tensor rank, Tensor rank_neg, Tensor n_eligible, Tensor n_neg, int64_t F,
                  int64_t strategy, int64_t flags, int64_t seed, int64_t n_splits) {
  const int64_t U = dev_tensor(users, at::kLong, "users").numel();
  Model m;
  fill_tables(m, entity, bias, scalars);
  fill_workspace(m, workspace);
  const int64_t* cp = id_list(cand, n_cand, "cand");
  const Csr ex = exclusions_of(excl_ptr, excl_items, U);
  const Csr pos = csr_of(pos_ptr, pos_items, U, "pos_ptr", "pos_items");
  const Heldout o = heldout_outputs(rank, rank_neg, n_eligible, n_neg, pos.n, U);
  c10::hip::HIPGuard guard(users.get_device());
  check(vfm_rank_heldout_f32(U, users.data_ptr<int64_t>(), n_cand, cp, item_lo, m.T, (int32_t)F, m.d,
                             (int32_t)strategy, (int32_t)flags, (uint64_t)seed, (int32_t)n_splits, ex.ptr, ex.items,
                             ex.n, pos.ptr, pos.items, pos.n, m.entity_params, m.bias_params, m.scalars, m.workspace,
                             m.workspace_bytes, o.rank, o.rank_neg, o.n_eligible, o.n_neg, stream_of(users)),
        "vfm_rank_heldout_f32");
}

// ---- the field-form ops: each table form (post NULL) and its form under supplied posteriors share a body

void field_moments_any(const Tensor& x, int64_t field, const Tensor* post, int64_t post_field,
                       const optional<Tensor>& qkey, const Tensor& entity, const Tensor& bias, const Tensor& scalars,
                       Tensor logit_mean, Tensor logit_var, const optional<Tensor>& score, int64_t flags,
                       int64_t strategy, int64_t seed) {
  const int64_t B = id_matrix(x, "x", true).size(0);
  Model m;
  fill_tables(m, entity, bias, scalars);
  const Moments o = moment_outputs(logit_mean, logit_var, score, B);
  const int64_t* kp = id_list(qkey, B, "qkey");
  const float* pp = post ? post_rows(*post, B, m) : nullptr;
  const int32_t F = (int32_t)x.size(1);
  c10::hip::HIPGuard guard(x.get_device());
  if (post)
    check(vfm_field_moments_post_f32(B, F, m.d, m.T, id_bits(x), (int32_t)flags, x.data_ptr(), (int32_t)field,
                                     (int32_t)post_field, pp, m.entity_params, m.bias_params, m.scalars,
                                     (int32_t)strategy, (uint64_t)seed, kp, o.mean, o.var, o.score, stream_of(x)),
          "vfm_field_moments_post_f32");
  else
    check(vfm_field_moments_f32(B, F, m.d, m.T, id_bits(x), (int32_t)flags, x.data_ptr(), (int32_t)field,
                                m.entity_params, m.bias_params, m.scalars, (int32_t)strategy, (uint64_t)seed, kp, o.mean,
                                o.var, o.score, stream_of(x)),
          "vfm_field_moments_f32");
}

void field_moments(const Tensor& x, int64_t field, const optional<Tensor>& qkey, const Tensor& entity,
                   const Tensor& bias, const Tensor& scalars, Tensor logit_mean, Tensor logit_var,
                   const optional<Tensor>& score, int64_t flags, int64_t strategy, int64_t seed) {
  field_moments_any(x, field, nullptr, -1, qkey, entity, bias, scalars, logit_mean, logit_var, score, flags, strategy,
                    seed);
}

void field_moments_post(const Tensor& x, int64_t field, const Tensor& post, int64_t post_field,
                        const optional<Tensor>& qkey, const Tensor& entity, const Tensor& bias, const Tensor& scalars,
                        Tensor logit_mean, Tensor logit_var, const optional<Tensor>& score, int64_t flags,
                        int64_t strategy, int64_t seed) {
  field_moments_any(x, field, &post, post_field, qkey, entity, bias, scalars, logit_mean, logit_var, score, flags,
                    strategy, seed);
}

int64_t rank_field_workspace_bytes(int64_t Q, int64_t n_cand, int64_t F, int64_t d, int64_t k, int64_t strategy,
                                   int64_t n_splits) {
  return bytes_of(vfm_rank_field_workspace_bytes(Q, n_cand, (int32_t)F, (int32_t)d, (int32_t)k, (int32_t)strategy,
                                                 (int32_t)n_splits),
                  "vfm_rank_field_workspace_bytes");
}

void rank_field_any(const Tensor& ctx, int64_t field, const Tensor* post, int64_t post_field,
                    const optional<Tensor>& qkey, const optional<Tensor>& cand, int64_t n_cand, int64_t cand_lo,
                    const optional<Tensor>& excl_ptr, const optional<Tensor>& excl_items, const Tensor& entity,
                    const Tensor& bias, const Tensor& scalars, Tensor workspace, Tensor items, Tensor score,
                    Tensor logit_mean, Tensor logit_var, int64_t k, int64_t strategy, int64_t flags, int64_t seed,
                    int64_t n_splits) {
  const int64_t Q = id_matrix(ctx, "ctx", false).size(0);
  Model m;
  fill_tables(m, entity, bias, scalars);
  fill_workspace(m, workspace);
  const int64_t *kp = id_list(qkey, Q, "qkey"), *cp = id_list(cand, n_cand, "cand");
  const Csr ex = exclusions_of(excl_ptr, excl_items, Q);
  const TopK o = topk_outputs(items, score, logit_mean, logit_var, Q * k);
  const float* pp = post ? post_rows(*post, Q, m) : nullptr;
  const int32_t F = (int32_t)ctx.size(1);
  c10::hip::HIPGuard guard(ctx.get_device());
  if (post)
    check(vfm_rank_field_post_f32(Q, ctx.data_ptr<int64_t>(), (int32_t)field, (int32_t)post_field, pp, kp, n_cand, cp,
                                  cand_lo, m.T, F, m.d, (int32_t)k, (int32_t)strategy, (int32_t)flags, (uint64_t)seed,
                                  (int32_t)n_splits, ex.ptr, ex.items, ex.n, m.entity_params, m.bias_params, m.scalars,
                                  m.workspace, m.workspace_bytes, o.items, o.score, o.mean, o.var, stream_of(ctx)),
          "vfm_rank_field_post_f32");
  else
    check(vfm_rank_field_f32(Q, ctx.data_ptr<int64_t>(), (int32_t)field, kp, n_cand, cp, cand_lo, m.T, F, m.d,
                             (int32_t)k, (int32_t)strategy, (int32_t)flags, (uint64_t)seed, (int32_t)n_splits, ex.ptr,
                             ex.items, ex.n, m.entity_params, m.bias_params, m.scalars, m.workspace, m.workspace_bytes,
                             o.items, o.score, o.mean, o.var, stream_of(ctx)),
          "vfm_rank_field_f32");
}

void rank_field(const Tensor& ctx, int64_t field, const optional<Tensor>& qkey, const optional<Tensor>& cand,
                int64_t n_cand, int64_t cand_lo, const optional<Tensor>& excl_ptr, const optional<Tensor>& excl_items,
                const Tensor& entity, const Tensor& bias, const Tensor& scalars, Tensor workspace, Tensor items,
                Tensor score, Tensor logit_mean, Tensor logit_var, int64_t k, int64_t strategy, int64_t flags,
                int64_t seed, int64_t n_splits) {
  rank_field_any(ctx, field, nullptr, -1, qkey, cand, n_cand, cand_lo, excl_ptr, excl_items, entity, bias, scalars,
                 workspace, items, score, logit_mean, logit_var, k, strategy, flags, seed, n_splits);
}

void rank_field_post(const Tensor& ctx, int64_t field, const Tensor& post, int64_t post_field,
                     const optional<Tensor>& qkey, const optional<Tensor>& cand, int64_t n_cand, int64_t cand_lo,
                     const optional<Tensor>& excl_ptr, const optional<Tensor>& excl_items, const Tensor& entity,
                     const Tensor& bias, const Tensor& scalars, Tensor workspace, Tensor items, Tensor score,
                     Tensor logit_mean, Tensor logit_var, int64_t k, int64_t strategy, int64_t flags, int64_t seed,
                     int64_t n_splits) {
  rank_field_any(ctx, field, &post, post_field, qkey, cand, n_cand, cand_lo, excl_ptr, excl_items, entity, bias, scalars,
                 workspace, items, score, logit_mean, logit_var, k, strategy, flags, seed, n_splits);
}

int64_t rank_eval_field_workspace_bytes(int64_t Q, int64_t n_cand, int64_t n_pos, int64_t F, int64_t d, int64_t strategy,
                                        int64_t n_splits) {
  return bytes_of(vfm_rank_eval_field_workspace_bytes(Q, n_cand, n_pos, (int32_t)F, (int32_t)d, (int32_t)strategy,
                                                      (int32_t)n_splits),
                  "vfm_rank_eval_field_workspace_bytes");
}

void rank_heldout_field_any(const Tensor& ctx, int64_t field, const Tensor* post, int64_t post_field,
                            const optional<Tensor>& qkey, const optional<Tensor>& cand, int64_t n_cand, int64_t cand_lo,
                            const optional<Tensor>& excl_ptr, const optional<Tensor>& excl_items, const Tensor& pos_ptr,
                            const Tensor& pos_items, const Tensor& entity, const Tensor& bias, const Tensor& scalars,
                            Tensor workspace, Tensor rank, Tensor rank_neg, Tensor n_eligible, Tensor n_neg,
                            int64_t strategy, int64_t flags, int64_t seed, int64_t n_splits) {
  const int64_t Q = id_matrix(ctx, "ctx", false).size(0);
  Model m;
  fill_tables(m, entity, bias, scalars);
  fill_workspace(m, workspace);
  const int64_t *kp = id_list(qkey, Q, "qkey"), *cp = id_list(cand, n_cand, "cand");
  const Csr ex = exclusions_of(excl_ptr, excl_items, Q);
  const Csr pos = csr_of(pos_ptr, pos_items, Q, "pos_ptr", "pos_items");
  const Heldout o = heldout_outputs(rank, rank_neg, n_eligible, n_neg, pos.n, Q);
  const float* pp = post ? post_rows(*post, Q, m) : nullptr;
  const int32_t F = (int32_t)ctx.size(1);
  c10::hip::HIPGuard guard(ctx.get_device());
  if (post)
    check(vfm_rank_heldout_field_post_f32(Q, ctx.data_ptr<int64_t>(), (int32_t)field, (int32_t)post_field, pp, kp,
                                          n_cand, cp, cand_lo, m.T, F, m.d, (int32_t)strategy, (int32_t)flags,
                                          (uint64_t)seed, (int32_t)n_splits, ex.ptr, ex.items, ex.n, pos.ptr, pos.items,
                                          pos.n, m.entity_params, m.bias_params, m.scalars, m.workspace,
                                          m.workspace_bytes, o.rank, o.rank_neg, o.n_eligible, o.n_neg, stream_of(ctx)),
          "vfm_rank_heldout_field_post_f32");
  else
    check(vfm_rank_heldout_field_f32(Q, ctx.data_ptr<int64_t>(), (int32_t)field, kp, n_cand, cp, cand_lo, m.T, F, m.d,
                                     (int32_t)strategy, (int32_t)flags, (uint64_t)seed, (int32_t)n_splits, ex.ptr,
                                     ex.items, ex.n, pos.ptr, pos.items, pos.n, m.entity_params, m.bias_params,
                                     m.scalars, m.workspace, m.workspace_bytes, o.rank, o.rank_neg, o.n_eligible,
                                     o.n_neg, stream_of(ctx)),
          "vfm_rank_heldout_field_f32");
}

void rank_heldout_field(const Tensor& ctx, int64_t field, const optional<Tensor>& qkey, const optional<Tensor>& cand,
                        int64_t n_cand, int64_t cand_lo, const optional<Tensor>& excl_ptr,
                        const optional<Tensor>& excl_items, const Tensor& pos_ptr, const Tensor& pos_items,
                        const Tensor& entity, const Tensor& bias, const Tensor& scalars, Tensor workspace, Tensor rank,
                        Tensor rank_neg, Tensor n_eligible, Tensor n_neg, int64_t strategy, int64_t flags, int64_t seed,
                        int64_t n_splits) {
  rank_heldout_field_any(ctx, field, nullptr, -1, qkey, cand, n_cand, cand_lo, excl_ptr, excl_items, pos_ptr, pos_items,
                         entity, bias, scalars, workspace, rank, rank_neg, n_eligible, n_neg, strategy, flags, seed,
                         n_splits);
}

void rank_heldout_field_post(const Tensor& ctx, int64_t field, const Tensor& post, int64_t post_field,
                             const optional<Tensor>& qkey, const optional<Tensor>& cand, int64_t n_cand,
                             int64_t cand_lo, const optional<Tensor>& excl_ptr, const optional<Tensor>& excl_items,
                             const Tensor& pos_ptr, const Tensor& pos_items, const Tensor& entity, const Tensor& bias,
                             const Tensor& scalars, Tensor workspace, Tensor rank, Tensor rank_neg, Tensor n_eligible,
                             Tensor n_neg, int64_t strategy, int64_t flags, int64_t seed, int64_t n_splits) {
  rank_heldout_field_any(ctx, field, &post, post_field, qkey, cand, n_cand, cand_lo, excl_ptr, excl_items, pos_ptr,
                         pos_items, entity, bias, scalars, workspace, rank, rank_neg, n_eligible, n_neg, strategy, flags,
                         seed, n_splits);
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(vfm_hip, m) {
  m.def("predictive_moments(Tensor x, Tensor entity_params, Tensor bias_params, Tensor scalars, "
        "Tensor(a!) logit_mean, Tensor(b!) logit_var, Tensor(c!)? score=None, int flags=0, int strategy=0, "
        "int seed=0) -> ()",
        &predictive_moments);
  m.def("rank_workspace_bytes(int U, int n_cand, int d, int k, int strategy, int n_splits) -> int",
        &rank_workspace_bytes);
  m.def("rank_items(Tensor users, Tensor? cand, int n_cand, int item_lo, Tensor? excl_ptr, Tensor? excl_items, "
        "Tensor entity_params, Tensor bias_params, Tensor scalars, Tensor(a!) workspace, Tensor(b!) items, "
        "Tensor(c!) score, Tensor(d!) logit_mean, Tensor(e!) logit_var, int F, int k, int strategy, int flags, "
        "int seed, int n_splits) -> ()",
        &rank_items);
  m.def("rank_eval_workspace_bytes(int U, int n_cand, int n_pos, int d, int strategy, int n_splits) -> int",
        &rank_eval_workspace_bytes);
  m.def("rank_heldout(Tensor users, Tensor? cand, int n_cand, int item_lo, Tensor? excl_ptr, Tensor? excl_items, "
        "Tensor pos_ptr, Tensor pos_items, Tensor entity_params, Tensor bias_params, Tensor scalars, "
        "Tensor(a!) workspace, Tensor(b!) rank, Tensor(c!) rank_neg, Tensor(d!) n_eligible, Tensor(e!) n_neg, int F, "
        "int strategy, int flags, int seed, int n_splits) -> ()",
        &rank_heldout);
  m.def("field_moments(Tensor x, int field, Tensor? qkey, Tensor entity_params, Tensor bias_params, Tensor scalars, "
        "Tensor(a!) logit_mean, Tensor(b!) logit_var, Tensor(c!)? score=None, int flags=0, int strategy=0, "
        "int seed=0) -> ()",
        &field_moments);
  m.def("rank_field_workspace_bytes(int Q, int n_cand, int F, int d, int k, int strategy, int n_splits) -> int",
        &rank_field_workspace_bytes);
  m.def("rank_field(Tensor ctx, int field, Tensor? qkey, Tensor? cand, int n_cand, int cand_lo, Tensor? excl_ptr, "
        "Tensor? excl_items, Tensor entity_params, Tensor bias_params, Tensor scalars, Tensor(a!) workspace, "
        "Tensor(b!) items, Tensor(c!) score, Tensor(d!) logit_mean, Tensor(e!) logit_var, int k, int strategy, "
        "int flags, int seed, int n_splits) -> ()",
        &rank_field);
  m.def("rank_eval_field_workspace_bytes(int Q, int n_cand, int n_pos, int F, int d, int strategy, int n_splits) -> int",
        &rank_eval_field_workspace_bytes);
  m.def("rank_heldout_field(Tensor ctx, int field, Tensor? qkey, Tensor? cand, int n_cand, int cand_lo, "
        "Tensor? excl_ptr, Tensor? excl_items, Tensor pos_ptr, Tensor pos_items, Tensor entity_params, "
        "Tensor bias_params, Tensor scalars, Tensor(a!) workspace, Tensor(b!) rank, Tensor(c!) rank_neg, "
        "Tensor(d!) n_eligible, Tensor(e!) n_neg, int strategy, int flags, int seed, int n_splits) -> ()",
        &rank_heldout_field);
  m.def("field_moments_post(Tensor x, int field, Tensor post, int post_field, Tensor? qkey, Tensor entity_params, "
        "Tensor bias_params, Tensor scalars, Tensor(a!) logit_mean, Tensor(b!) logit_var, Tensor(c!)? score=None, "
        "int flags=0, int strategy=0, int seed=0) -> ()",
        &field_moments_post);
  m.def("rank_field_post(Tensor ctx, int field, Tensor post, int post_field, Tensor? qkey, Tensor? cand, int n_cand, "
        "int cand_lo, Tensor? excl_ptr, Tensor? excl_items, Tensor entity_params, Tensor bias_params, Tensor scalars, "
        "Tensor(a!) workspace, Tensor(b!) items, Tensor(c!) score, Tensor(d!) logit_mean, Tensor(e!) logit_var, int k, "
        "int strategy, int flags, int seed, int n_splits) -> ()",
        &rank_field_post);
  m.def("rank_heldout_field_post(Tensor ctx, int field, Tensor post, int post_field, Tensor? qkey, Tensor? cand, "
        "int n_cand, int cand_lo, Tensor? excl_ptr, Tensor? excl_items, Tensor pos_ptr, Tensor pos_items, "
        "Tensor entity_params, Tensor bias_params, Tensor scalars, Tensor(a!) workspace, Tensor(b!) rank, "
        "Tensor(c!) rank_neg, Tensor(d!) n_eligible, Tensor(e!) n_neg, int strategy, int flags, int seed, "
        "int n_splits) -> ()",
        &rank_heldout_field_post);
}
