// vfm_rank_ops.cpp -- torch.ops.vfm_hip.{predictive_moments, rank_items, rank_workspace_bytes, rank_heldout,
// rank_eval_workspace_bytes, field_moments, rank_field, rank_field_workspace_bytes, rank_heldout_field,
// rank_eval_field_workspace_bytes, field_moments_post, rank_field_post, rank_heldout_field_post}: the TORCH_LIBRARY fragment over include/vfm_rank.h.  Like vfm_torch_ops.cpp it only validates tensors, takes the current HIP stream
// of the tensors' device and forwards raw pointers; all arithmetic is in the HIP kernels.
#include "vfm_ops_common.hpp"

#include "vfm_rank.h"

namespace {

using namespace vfm_ops;

void tables(const Tensor& entity, const Tensor& bias, const Tensor& scalars) {
  dev_tensor(entity, at::kFloat, "entity_params"); dev_tensor(bias, at::kFloat, "bias_params");
  dev_tensor(scalars, at::kFloat, "scalars");
  TORCH_CHECK(entity.dim() == 2 && bias.dim() == 2 && bias.size(1) == 2 && bias.size(0) == entity.size(0) &&
              entity.size(1) % 2 == 0 && scalars.numel() >= 3, "table shapes");
}

void predictive_moments(const Tensor& x, const Tensor& entity, const Tensor& bias, const Tensor& scalars,
                        Tensor logit_mean, Tensor logit_var, const optional<Tensor>& score, int64_t flags,
                        int64_t strategy, int64_t seed) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2, "x must be a contiguous [B,F] GPU tensor");
  TORCH_CHECK(x.scalar_type() == at::kLong || x.scalar_type() == at::kInt, "x must be int64 or int32");
  tables(entity, bias, scalars);
  const int64_t B = x.size(0);
  dev_tensor(logit_mean, at::kFloat, "logit_mean"); dev_tensor(logit_var, at::kFloat, "logit_var");
  TORCH_CHECK(logit_mean.numel() >= B && logit_var.numel() >= B, "output sizes");
  float* sp = nullptr;
  if (score.has_value() && score->defined()) {
    TORCH_CHECK(dev_tensor(*score, at::kFloat, "score").numel() >= B, "score too small");
    sp = score->data_ptr<float>();
  }
  c10::hip::HIPGuard guard(x.get_device());
  check(vfm_predictive_moments_f32(B, (int32_t)x.size(1), (int32_t)(entity.size(1) / 2), entity.size(0),
                                   x.scalar_type() == at::kLong ? 64 : 32, (int32_t)flags, x.data_ptr(),
                                   entity.data_ptr<float>(), bias.data_ptr<float>(), scalars.data_ptr<float>(),
                                   (int32_t)strategy, (uint64_t)seed, logit_mean.data_ptr<float>(),
                                   logit_var.data_ptr<float>(), sp, stream_of(x)),
        "vfm_predictive_moments_f32");
}

int64_t rank_workspace_bytes(int64_t U, int64_t n_cand, int64_t d, int64_t k, int64_t strategy, int64_t n_splits) {
  const int64_t b = vfm_rank_workspace_bytes(U, n_cand, (int32_t)d, (int32_t)k, (int32_t)strategy, (int32_t)n_splits);
  TORCH_CHECK(b >= 0, "vfm_rank_workspace_bytes: bad arguments");
  return b;
}

void rank_items(const Tensor& users, const optional<Tensor>& cand, int64_t n_cand, int64_t item_lo,
                const optional<Tensor>& excl_ptr, const optional<Tensor>& excl_items, const Tensor& entity,
                const Tensor& bias, const Tensor& scalars, Tensor workspace, Tensor items, Tensor score,
                Tensor logit_mean, Tensor logit_var, int64_t F, int64_t k, int64_t strategy, int64_t flags,
                int64_t seed, int64_t n_splits) {
  dev_tensor(users, at::kLong, "users");
  tables(entity, bias, scalars);
  const int64_t U = users.numel();
  const int64_t* cp = nullptr;
  if (cand.has_value() && cand->defined()) {
    TORCH_CHECK(dev_tensor(*cand, at::kLong, "cand").numel() == n_cand, "cand must hold n_cand ids");
    cp = cand->data_ptr<int64_t>();
  }
  const int64_t *ep = nullptr, *ei = nullptr;
  int64_t n_excl = 0;
  if (excl_ptr.has_value() && excl_ptr->defined()) {
    TORCH_CHECK(dev_tensor(*excl_ptr, at::kLong, "excl_ptr").numel() == U + 1, "excl_ptr needs U + 1 offsets");
    TORCH_CHECK(excl_items.has_value() && excl_items->defined(), "excl_ptr without excl_items");
    ep = excl_ptr->data_ptr<int64_t>();
    n_excl = dev_tensor(*excl_items, at::kLong, "excl_items").numel();
    ei = n_excl > 0 ? excl_items->data_ptr<int64_t>() : nullptr;
  }
  dev_tensor(workspace, at::kByte, "workspace");
  dev_tensor(items, at::kLong, "items"); dev_tensor(score, at::kFloat, "score");
  dev_tensor(logit_mean, at::kFloat, "logit_mean"); dev_tensor(logit_var, at::kFloat, "logit_var");
  TORCH_CHECK(items.numel() >= U * k && score.numel() >= U * k && logit_mean.numel() >= U * k &&
              logit_var.numel() >= U * k, "output sizes");
  c10::hip::HIPGuard guard(users.get_device());
  check(vfm_rank_items_f32(U, users.data_ptr<int64_t>(), n_cand, cp, item_lo, entity.size(0), (int32_t)F,
                           (int32_t)(entity.size(1) / 2), (int32_t)k, (int32_t)strategy, (int32_t)flags,
                           (uint64_t)seed, (int32_t)n_splits, ep, ei, n_excl, entity.data_ptr<float>(),
                           bias.data_ptr<float>(), scalars.data_ptr<float>(), workspace.data_ptr(), workspace.numel(),
                           items.data_ptr<int64_t>(), score.data_ptr<float>(), logit_mean.data_ptr<float>(),
                           logit_var.data_ptr<float>(), stream_of(users)),
        "vfm_rank_items_f32");
}

int64_t rank_eval_workspace_bytes(int64_t U, int64_t n_cand, int64_t n_pos, int64_t d, int64_t strategy,
                                  int64_t n_splits) {
  const int64_t b = vfm_rank_eval_workspace_bytes(U, n_cand, n_pos, (int32_t)d, (int32_t)strategy, (int32_t)n_splits);
  TORCH_CHECK(b >= 0, "vfm_rank_eval_workspace_bytes: bad arguments");
  return b;
}

void rank_heldout(const Tensor& users, const optional<Tensor>& cand, int64_t n_cand, int64_t item_lo,
                  const optional<Tensor>& excl_ptr, const optional<Tensor>& excl_items, const Tensor& pos_ptr,
                  const Tensor& pos_items, const Tensor& entity, const Tensor& bias, const Tensor& scalars,
                  Tensor workspace, Tensor rank, Tensor rank_neg, Tensor n_eligible, Tensor n_neg, int64_t F,
                  int64_t strategy, int64_t flags, int64_t seed, int64_t n_splits) {
  dev_tensor(users, at::kLong, "users");
  tables(entity, bias, scalars);
  const int64_t U = users.numel();
  const int64_t* cp = nullptr;
  if (cand.has_value() && cand->defined()) {
    TORCH_CHECK(dev_tensor(*cand, at::kLong, "cand").numel() == n_cand, "cand must hold n_cand ids");
    cp = cand->data_ptr<int64_t>();
  }
  const int64_t *ep = nullptr, *ei = nullptr;
  int64_t n_excl = 0;
  if (excl_ptr.has_value() && excl_ptr->defined()) {
    TORCH_CHECK(dev_tensor(*excl_ptr, at::kLong, "excl_ptr").numel() == U + 1, "excl_ptr needs U + 1 offsets");
    TORCH_CHECK(excl_items.has_value() && excl_items->defined(), "excl_ptr without excl_items");
    ep = excl_ptr->data_ptr<int64_t>();
    n_excl = dev_tensor(*excl_items, at::kLong, "excl_items").numel();
    ei = n_excl > 0 ? excl_items->data_ptr<int64_t>() : nullptr;
  }
  TORCH_CHECK(dev_tensor(pos_ptr, at::kLong, "pos_ptr").numel() == U + 1, "pos_ptr needs U + 1 offsets");
  const int64_t n_pos = dev_tensor(pos_items, at::kLong, "pos_items").numel();
  dev_tensor(workspace, at::kByte, "workspace");
  dev_tensor(rank, at::kLong, "rank"); dev_tensor(rank_neg, at::kLong, "rank_neg");
  dev_tensor(n_eligible, at::kLong, "n_eligible"); dev_tensor(n_neg, at::kLong, "n_neg");
  TORCH_CHECK(rank.numel() >= n_pos && rank_neg.numel() >= n_pos && n_eligible.numel() >= U && n_neg.numel() >= U,
              "output sizes");
  c10::hip::HIPGuard guard(users.get_device());
  check(vfm_rank_heldout_f32(U, users.data_ptr<int64_t>(), n_cand, cp, item_lo, entity.size(0), (int32_t)F,
                             (int32_t)(entity.size(1) / 2), (int32_t)strategy, (int32_t)flags, (uint64_t)seed,
                             (int32_t)n_splits, ep, ei, n_excl, pos_ptr.data_ptr<int64_t>(),
                             n_pos > 0 ? pos_items.data_ptr<int64_t>() : nullptr, n_pos, entity.data_ptr<float>(),
                             bias.data_ptr<float>(), scalars.data_ptr<float>(), workspace.data_ptr(), workspace.numel(),
                             rank.data_ptr<int64_t>(), rank_neg.data_ptr<int64_t>(), n_eligible.data_ptr<int64_t>(),
                             n_neg.data_ptr<int64_t>(), stream_of(users)),
        "vfm_rank_heldout_f32");
}

// The supplied posteriors of the *_post ops: [rows, 2d + 2] fp32, one row per query
const float* post_rows(const Tensor& post, int64_t rows, const Tensor& entity) {
  dev_tensor(post, at::kFloat, "post");
  TORCH_CHECK(post.dim() == 2 && post.size(0) == rows && post.size(1) == entity.size(1) + 2,
              "post must be [Q, 2d + 2], one row per query");
  return post.data_ptr<float>();
}

// field_moments (post NULL) and field_moments_post
void field_moments_any(const Tensor& x, int64_t field, const Tensor* post, int64_t post_field,
                       const optional<Tensor>& qkey, const Tensor& entity, const Tensor& bias, const Tensor& scalars,
                       Tensor logit_mean, Tensor logit_var, const optional<Tensor>& score, int64_t flags,
                       int64_t strategy, int64_t seed) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2, "x must be a contiguous [B,F] GPU tensor");
  TORCH_CHECK(x.scalar_type() == at::kLong || x.scalar_type() == at::kInt, "x must be int64 or int32");
  tables(entity, bias, scalars);
  const int64_t B = x.size(0);
  dev_tensor(logit_mean, at::kFloat, "logit_mean"); dev_tensor(logit_var, at::kFloat, "logit_var");
  TORCH_CHECK(logit_mean.numel() >= B && logit_var.numel() >= B, "output sizes");
  float* sp = nullptr;
  if (score.has_value() && score->defined()) {
    TORCH_CHECK(dev_tensor(*score, at::kFloat, "score").numel() >= B, "score too small");
    sp = score->data_ptr<float>();
  }
  const int64_t* kp = nullptr;
  if (qkey.has_value() && qkey->defined()) {
    TORCH_CHECK(dev_tensor(*qkey, at::kLong, "qkey").numel() == B, "qkey must hold one key per row");
    kp = qkey->data_ptr<int64_t>();
  }
  const float* pp = post ? post_rows(*post, B, entity) : nullptr;
  c10::hip::HIPGuard guard(x.get_device());
  if (post)
    check(vfm_field_moments_post_f32(B, (int32_t)x.size(1), (int32_t)(entity.size(1) / 2), entity.size(0),
                                     x.scalar_type() == at::kLong ? 64 : 32, (int32_t)flags, x.data_ptr(),
                                     (int32_t)field, (int32_t)post_field, pp, entity.data_ptr<float>(),
                                     bias.data_ptr<float>(), scalars.data_ptr<float>(), (int32_t)strategy,
                                     (uint64_t)seed, kp, logit_mean.data_ptr<float>(), logit_var.data_ptr<float>(), sp,
                                     stream_of(x)),
          "vfm_field_moments_post_f32");
  else
    check(vfm_field_moments_f32(B, (int32_t)x.size(1), (int32_t)(entity.size(1) / 2), entity.size(0),
                                x.scalar_type() == at::kLong ? 64 : 32, (int32_t)flags, x.data_ptr(), (int32_t)field,
                                entity.data_ptr<float>(), bias.data_ptr<float>(), scalars.data_ptr<float>(),
                                (int32_t)strategy, (uint64_t)seed, kp, logit_mean.data_ptr<float>(),
                                logit_var.data_ptr<float>(), sp, stream_of(x)),
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
  const int64_t b = vfm_rank_field_workspace_bytes(Q, n_cand, (int32_t)F, (int32_t)d, (int32_t)k, (int32_t)strategy,
                                                   (int32_t)n_splits);
  TORCH_CHECK(b >= 0, "vfm_rank_field_workspace_bytes: bad arguments");
  return b;
}

// rank_field (post NULL) and rank_field_post
void rank_field_any(const Tensor& ctx, int64_t field, const Tensor* post, int64_t post_field,
                    const optional<Tensor>& qkey, const optional<Tensor>& cand, int64_t n_cand, int64_t cand_lo,
                    const optional<Tensor>& excl_ptr, const optional<Tensor>& excl_items, const Tensor& entity,
                    const Tensor& bias, const Tensor& scalars, Tensor workspace, Tensor items, Tensor score,
                    Tensor logit_mean, Tensor logit_var, int64_t k, int64_t strategy, int64_t flags, int64_t seed,
                    int64_t n_splits) {
  dev_tensor(ctx, at::kLong, "ctx");
  TORCH_CHECK(ctx.dim() == 2, "ctx must be [Q,F]");
  tables(entity, bias, scalars);
  const int64_t Q = ctx.size(0);
  const int64_t *kp = nullptr, *cp = nullptr;
  if (qkey.has_value() && qkey->defined()) {
    TORCH_CHECK(dev_tensor(*qkey, at::kLong, "qkey").numel() == Q, "qkey must hold one key per query");
    kp = qkey->data_ptr<int64_t>();
  }
  if (cand.has_value() && cand->defined()) {
    TORCH_CHECK(dev_tensor(*cand, at::kLong, "cand").numel() == n_cand, "cand must hold n_cand ids");
    cp = cand->data_ptr<int64_t>();
  }
  const int64_t *ep = nullptr, *ei = nullptr;
  int64_t n_excl = 0;
  if (excl_ptr.has_value() && excl_ptr->defined()) {
    TORCH_CHECK(dev_tensor(*excl_ptr, at::kLong, "excl_ptr").numel() == Q + 1, "excl_ptr needs Q + 1 offsets");
    TORCH_CHECK(excl_items.has_value() && excl_items->defined(), "excl_ptr without excl_items");
    ep = excl_ptr->data_ptr<int64_t>();
    n_excl = dev_tensor(*excl_items, at::kLong, "excl_items").numel();
    ei = n_excl > 0 ? excl_items->data_ptr<int64_t>() : nullptr;
  }
  dev_tensor(workspace, at::kByte, "workspace");
  dev_tensor(items, at::kLong, "items"); dev_tensor(score, at::kFloat, "score");
  dev_tensor(logit_mean, at::kFloat, "logit_mean"); dev_tensor(logit_var, at::kFloat, "logit_var");
  TORCH_CHECK(items.numel() >= Q * k && score.numel() >= Q * k && logit_mean.numel() >= Q * k &&
              logit_var.numel() >= Q * k, "output sizes");
  const float* pp = post ? post_rows(*post, Q, entity) : nullptr;
  c10::hip::HIPGuard guard(ctx.get_device());
  if (post)
    check(vfm_rank_field_post_f32(Q, ctx.data_ptr<int64_t>(), (int32_t)field, (int32_t)post_field, pp, kp, n_cand, cp,
                                  cand_lo, entity.size(0), (int32_t)ctx.size(1), (int32_t)(entity.size(1) / 2),
                                  (int32_t)k, (int32_t)strategy, (int32_t)flags, (uint64_t)seed, (int32_t)n_splits, ep,
                                  ei, n_excl, entity.data_ptr<float>(), bias.data_ptr<float>(),
                                  scalars.data_ptr<float>(), workspace.data_ptr(), workspace.numel(),
                                  items.data_ptr<int64_t>(), score.data_ptr<float>(), logit_mean.data_ptr<float>(),
                                  logit_var.data_ptr<float>(), stream_of(ctx)),
          "vfm_rank_field_post_f32");
  else
    check(vfm_rank_field_f32(Q, ctx.data_ptr<int64_t>(), (int32_t)field, kp, n_cand, cp, cand_lo, entity.size(0),
                             (int32_t)ctx.size(1), (int32_t)(entity.size(1) / 2), (int32_t)k, (int32_t)strategy,
                             (int32_t)flags, (uint64_t)seed, (int32_t)n_splits, ep, ei, n_excl,
                             entity.data_ptr<float>(), bias.data_ptr<float>(), scalars.data_ptr<float>(),
                             workspace.data_ptr(), workspace.numel(), items.data_ptr<int64_t>(),
                             score.data_ptr<float>(), logit_mean.data_ptr<float>(), logit_var.data_ptr<float>(),
                             stream_of(ctx)),
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
  const int64_t b = vfm_rank_eval_field_workspace_bytes(Q, n_cand, n_pos, (int32_t)F, (int32_t)d, (int32_t)strategy,
                                                        (int32_t)n_splits);
  TORCH_CHECK(b >= 0, "vfm_rank_eval_field_workspace_bytes: bad arguments");
  return b;
}

// rank_heldout_field (post NULL) and rank_heldout_field_post
void rank_heldout_field_any(const Tensor& ctx, int64_t field, const Tensor* post, int64_t post_field,
                            const optional<Tensor>& qkey, const optional<Tensor>& cand, int64_t n_cand, int64_t cand_lo,
                            const optional<Tensor>& excl_ptr, const optional<Tensor>& excl_items, const Tensor& pos_ptr,
                            const Tensor& pos_items, const Tensor& entity, const Tensor& bias, const Tensor& scalars,
                            Tensor workspace, Tensor rank, Tensor rank_neg, Tensor n_eligible, Tensor n_neg,
                            int64_t strategy, int64_t flags, int64_t seed, int64_t n_splits) {
  dev_tensor(ctx, at::kLong, "ctx");
  TORCH_CHECK(ctx.dim() == 2, "ctx must be [Q,F]");
  tables(entity, bias, scalars);
  const int64_t Q = ctx.size(0);
  const int64_t *kp = nullptr, *cp = nullptr;
  if (qkey.has_value() && qkey->defined()) {
    TORCH_CHECK(dev_tensor(*qkey, at::kLong, "qkey").numel() == Q, "qkey must hold one key per query");
    kp = qkey->data_ptr<int64_t>();
  }
  if (cand.has_value() && cand->defined()) {
    TORCH_CHECK(dev_tensor(*cand, at::kLong, "cand").numel() == n_cand, "cand must hold n_cand ids");
    cp = cand->data_ptr<int64_t>();
  }
  const int64_t *ep = nullptr, *ei = nullptr;
  int64_t n_excl = 0;
  if (excl_ptr.has_value() && excl_ptr->defined()) {
    TORCH_CHECK(dev_tensor(*excl_ptr, at::kLong, "excl_ptr").numel() == Q + 1, "excl_ptr needs Q + 1 offsets");
    TORCH_CHECK(excl_items.has_value() && excl_items->defined(), "excl_ptr without excl_items");
    ep = excl_ptr->data_ptr<int64_t>();
    n_excl = dev_tensor(*excl_items, at::kLong, "excl_items").numel();
    ei = n_excl > 0 ? excl_items->data_ptr<int64_t>() : nullptr;
  }
  TORCH_CHECK(dev_tensor(pos_ptr, at::kLong, "pos_ptr").numel() == Q + 1, "pos_ptr needs Q + 1 offsets");
  const int64_t n_pos = dev_tensor(pos_items, at::kLong, "pos_items").numel();
  dev_tensor(workspace, at::kByte, "workspace");
  dev_tensor(rank, at::kLong, "rank"); dev_tensor(rank_neg, at::kLong, "rank_neg");
  dev_tensor(n_eligible, at::kLong, "n_eligible"); dev_tensor(n_neg, at::kLong, "n_neg");
  TORCH_CHECK(rank.numel() >= n_pos && rank_neg.numel() >= n_pos && n_eligible.numel() >= Q && n_neg.numel() >= Q,
              "output sizes");
  const float* pp = post ? post_rows(*post, Q, entity) : nullptr;
  const int64_t* pi = n_pos > 0 ? pos_items.data_ptr<int64_t>() : nullptr;
  c10::hip::HIPGuard guard(ctx.get_device());
  if (post)
    check(vfm_rank_heldout_field_post_f32(Q, ctx.data_ptr<int64_t>(), (int32_t)field, (int32_t)post_field, pp, kp,
                                          n_cand, cp, cand_lo, entity.size(0), (int32_t)ctx.size(1),
                                          (int32_t)(entity.size(1) / 2), (int32_t)strategy, (int32_t)flags,
                                          (uint64_t)seed, (int32_t)n_splits, ep, ei, n_excl,
                                          pos_ptr.data_ptr<int64_t>(), pi, n_pos, entity.data_ptr<float>(),
                                          bias.data_ptr<float>(), scalars.data_ptr<float>(), workspace.data_ptr(),
                                          workspace.numel(), rank.data_ptr<int64_t>(), rank_neg.data_ptr<int64_t>(),
                                          n_eligible.data_ptr<int64_t>(), n_neg.data_ptr<int64_t>(), stream_of(ctx)),
          "vfm_rank_heldout_field_post_f32");
  else
    check(vfm_rank_heldout_field_f32(Q, ctx.data_ptr<int64_t>(), (int32_t)field, kp, n_cand, cp, cand_lo,
                                     entity.size(0), (int32_t)ctx.size(1), (int32_t)(entity.size(1) / 2),
                                     (int32_t)strategy, (int32_t)flags, (uint64_t)seed, (int32_t)n_splits, ep, ei,
                                     n_excl, pos_ptr.data_ptr<int64_t>(), pi, n_pos, entity.data_ptr<float>(),
                                     bias.data_ptr<float>(), scalars.data_ptr<float>(), workspace.data_ptr(),
                                     workspace.numel(), rank.data_ptr<int64_t>(), rank_neg.data_ptr<int64_t>(),
                                     n_eligible.data_ptr<int64_t>(), n_neg.data_ptr<int64_t>(), stream_of(ctx)),
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
