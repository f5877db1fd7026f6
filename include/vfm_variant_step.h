/*
 * vfm_variant_step.h -- C ABI of the fused training step of the ELBO variants of libvfm_hip.so (gfx950): the backward
 * of vfm_variant_bwd_f32 (vfm_hip.h) and torch.optim.Adam's dense update in one pass over the tables.
 *
 * The forward stays vfm_variant_fwd_f32.  From what it saved (state, grow, partials) one launch walks the inverted
 * index, a lane group per table row, forms the row's gradient in registers and updates (parameter, m, v) of that row
 * in place; the gradient of the tables is never written.  A row the batch does not touch takes its zero-gradient step
 * (dense Adam: m and v decay, the parameter moves).  The three scalars and the flat prior vector are read by every
 * workgroup, so their gradients are formed as in vfm_variant_bwd_f32 (workgroup 0 / one partial row per workgroup and
 * id group, summed in a fixed order for every d: no float atomics, the step is reproducible bit for bit) and a second,
 * small launch updates them.
 *
 * Update: torch.optim.Adam's single-tensor form, operation for operation as vfm_adam_f32 (IEEE sqrt and divisions):
 *   m' = m + (g - m)(1 - beta1);  v' = v beta2 + ((1 - beta2) g) g;
 *   p' = p + (-step_size m') / (sqrt(v') / sqrt(1 - beta2^t) + eps),  step_size = lr / (1 - beta1^t), t = adam_step.
 * The moments are stored plain (no scaled form, no lazy replay).
 *
 * Conventions: those of vfm_hip.h.  Every pointer is DEVICE memory owned by the caller; launch-only, no host
 * synchronisation; 0 on success, a negative VFM_E_* code or a positive hipError_t otherwise; arguments are checked
 * before any HIP call; vfm_last_error() describes the last failure on the calling thread.
 */
#ifndef VFM_VARIANT_STEP_H
#define VFM_VARIANT_STEP_H

#include <stdint.h>

#include "vfm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of scratch vfm_variant_step_f32 needs (16-byte aligned; contents need not be kept between calls): the positions
 * of the occurrences (used with values), the partial rows of the prior gradients, the gradients of the scalars.
 * Negative on bad arguments. */
int64_t vfm_variant_step_workspace_bytes(int64_t B, int32_t F, int32_t d);

/*
 * One Adam step of the variant objective `objective` (VFM_OBJ_SAMPLED / VFM_OBJ_CLOSED_FORM) from the state a
 * vfm_variant_fwd_f32 call with the SAME problem (seed and step included), objective, x, values, tables, scalars,
 * priors and eps tables left in state / grow / partials.  Shapes and meanings as in vfm_variant_bwd_f32:
 *   index       the batch's inverted index (vfm_build_index); a corrupted entry is clamped and counted in index->status
 *   values      [B,F] or NULL;  priors [2 + 2F + 2Fd] or NULL (then m_priors / v_priors are NULL too)
 *   eps_*       all three tables or none (none: Philox eps keyed by problem->seed / problem->step, as the forward's)
 *   grad_out    [1] the factor on the loss' gradient (1 for plain training)
 * Updated in place: entity_params [T,2d], bias_params [T,2], scalars [3], priors, and the moments m_X / v_X of the same
 * shapes.  F <= VFM_MAX_FIELDS, 1 <= d <= 1024 (d % 8 == 0: lane groups with eight coordinates per lane; any other d:
 * one coordinate per lane), both id widths, adam_step >= 1.
 */
int vfm_variant_step_f32(const vfm_problem_t* problem, int32_t objective, const vfm_index_t* index, void* workspace,
                         const void* x, const float* values, float* entity_params, float* bias_params,
                         const float* inv_occ, float* scalars, const double* W, float* priors, const float* eps_entity,
                         const float* eps_bias, const float* eps_global, const float* state, const float* grow,
                         const double* partials, const float* grad_out, float* m_entity, float* v_entity, float* m_bias,
                         float* v_bias, float* m_scalars, float* v_scalars, float* m_priors, float* v_priors, float lr,
                         float beta1, float beta2, float eps_adam, int64_t adam_step, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VFM_VARIANT_STEP_H */
