/*
 * vfm_bound_sweep.h -- C ABI of the split bound rounds of libvfm_hip.so (gfx950): the bound fold-in of vfm_bound.h for
 * entities with many rows, the hot path of a coordinate-ascent training sweep of a 'class' model (VFM.fit_bound).
 *
 * vfm_foldin_bound_f32 gives an entity to one workgroup however many rows it has, and every one of its n_iters rounds
 * walks all the entity's rows serially.  Here an entity's row list is cut in chunks, as in vfm_sweep.h, and each round's
 * primal system of vfm_bound.h,
 *   H theta = b,  H = sum_r w_r (u_r u_r^T + diag(0, A_r)) + kl I,
 *   b = sum_r ((y_r - 1/2) - w_r c_mean,r) u_r - (0, 1/2 sum_r w_r C_r),
 * is assembled by one workgroup per chunk.  Per call, on one stream:
 *   start     the fp64 iterate [E, 2 (d + 1)] = theta | sigma^2 of every entity: its fp32 row read through the link in
 *             fp64, or mu = 0, sigma^2 = 1 with `reset` (the start of vfm_foldin_bound_f32)
 *   and n_iters times
 *   assemble  a workgroup per chunk: w_r = tanh(xi_r / 2) / (2 xi_r) of the chunk's rows at the entity's iterate
 *             (xi_r^2 = (E f_r)^2 + Var f_r, clamped at 0; 1/4 - xi_r^2 / 48 below 1e-3), then, in fp64 and in row order,
 *             the chunk's share of the packed lower triangle of sum_r w_r u_r u_r^T and of sum_r w_r A_r,
 *             sum_r w_r (A_r + M_r^2) (coordinate 0: sum_r w_r), sum_r ((y_r - 1/2) - w_r c_mean,r) u_r and sum_r w_r C_r,
 *             into its slab of tri(d + 1) + 4 d + 3 doubles
 *   solve     a workgroup per entity adds its chunks' slabs in chunk order, adds kl and runs the Cholesky factorisation
 *             and the substitutions of vfm_foldin_solve_f32, the same code; theta and sigma^2 = kl / (kl + sum ..) go
 *             back to the fp64 iterate; after the last round the iterate is rounded to fp32 once and the table row is
 *             written as vfm_foldin_bound_f32 writes it
 *   then
 *   loss      B_e of vfm_bound.h at the written fp32 parameters with the per-row arithmetic of vfm_foldin_bound_f32's
 *             loss, a wave per chunk, the rows added in row order and the chunks' shares in chunk order, in fp64
 * The operands are those of vfm_foldin_bound_f32, from the same three prep kernels.  No atomics, no host
 * synchronisation, no cooperative launch and no grid-wide barrier: rounds are separated by kernel boundaries.  Every sum
 * has a fixed order that depends on the entity's own rows, the chunk length and d alone, so an entity's output bytes do
 * not depend on the other entities of the call, on the grid, on how the caller groups entities into calls or on where
 * the triangle lives.  They are not the bytes of vfm_foldin_bound_f32: the chunked sums associate differently.
 * The primal form is valid for any number of rows; the caller sends entities with more than d rows.
 *
 * Conventions: those of vfm_foldin.h.  The Bernoulli likelihood has no precision: scalars[0] is not read.
 */
#ifndef VFM_BOUND_SWEEP_H
#define VFM_BOUND_SWEEP_H

#include <stdint.h>

#include "vfm_foldin.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vfm_foldin_bound_split_t {
  int64_t E;          /* entities of the call                                                                    */
  int64_t R;          /* rows of y / row_op                                                                      */
  int64_t T;          /* table rows                                                                              */
  int64_t n_ops;      /* distinct frozen-partner tuples (row operands)                                           */
  int64_t n_chunks;   /* rows of the chunk table                                                                 */
  int32_t F, d;       /* fields (1 .. VFM_MAX_FIELDS), embedding size (1 .. VFM_FOLDIN_MAX_D)                     */
  int32_t col;        /* the folded column of op_x                                                               */
  int32_t flags;      /* 0 or VFM_FLAG_LINK_SOFTPLUS                                                             */
  int32_t lds_dim;    /* as in vfm_foldin_solve_t                                                                */
  float kl_weight;    /* > 0                                                                                     */
  int32_t n_iters;    /* rounds, >= 1                                                                            */
  int32_t reset;      /* 1: xi^(0) from the prior (mu = 0, sigma = 1) instead of the current rows                */
  const int64_t* entities;  /* [E] folded ids                                                                     */
  const int64_t* chunk_ptr; /* [E + 1] offsets of each entity's chunks in the chunk table, ascending              */
  const int64_t* chunks;    /* [n_chunks, 3] = (entity number in [0, E), first row, rows); an entity's chunks are  */
                            /* consecutive, in row order and do not overlap                                       */
  const float* y;           /* [R] in {0, 1}                                                                      */
  const int64_t* op_x;      /* [n_ops, F] one row of each partner tuple (the folded column is ignored)             */
  const int64_t* row_op;    /* [R] operand of each row                                                            */
  float* entity_params;     /* [T, 2d]: read; the rows of `entities` are written                                  */
  float* bias_params;       /* [T, 2]                                                                             */
  const float* scalars;     /* [3] (alpha is not read)                                                            */
  float* out_loss;          /* [E] B_e                                                                            */
  void* workspace;
  int64_t workspace_bytes;
} vfm_foldin_bound_split_t;

/* Workspace of vfm_foldin_bound_split_f32 in bytes, each part rounded up to 256: the operand block of
 * vfm_foldin_solve_f32, n_ops doubles of c_var, R doubles of row weights (a row's at its own index), n_heavy * 2 (d + 1)
 * doubles of iterate, n_chunks slabs of tri(d + 1) + 4 d + 3 doubles, n_chunks doubles of loss partials and, when a
 * (d + 1) x (d + 1) system does not stay in LDS, min(n_heavy, VFM_FOLDIN_SOLVE_SLABS) triangles.  VFM_E_INVALID on
 * negative arguments, d outside [1, VFM_FOLDIN_MAX_D], lds_dim < -1 or a size past 2^62. */
int64_t vfm_foldin_bound_split_workspace_bytes(int64_t n_chunks, int64_t n_heavy, int64_t R, int64_t n_ops, int32_t d,
                                               int32_t lds_dim);

/* Run n_iters rounds for every entity of p from its chunks and write its row.  An entity id outside [0, T) gets a NaN
 * loss and is not written; a partner id outside [0, T) or a row operand outside [0, n_ops) makes its rows' entities and
 * their losses NaN; a chunk is clamped to [0, R) and one whose entity number is outside [0, E) is skipped; an entity
 * without chunks gets the prior and loss 0.  E = 0: nothing is launched.  VFM_E_INVALID (nothing launched) for the range
 * checks of vfm_foldin_solve_split_f32 and vfm_foldin_bound_f32, n_iters < 1 and a short or misaligned (256 bytes)
 * workspace. */
int vfm_foldin_bound_split_f32(const vfm_foldin_bound_split_t* p, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VFM_BOUND_SWEEP_H */
