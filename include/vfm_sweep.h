/*
 * vfm_sweep.h -- C ABI of the split exact solve of libvfm_hip.so (gfx950): the exact fold-in of vfm_foldin.h for
 * entities with many rows, the hot path of a coordinate-ascent training sweep (VFM.fit_exact).
 *
 * vfm_foldin_solve_f32 gives an entity to one workgroup however many rows it has.  Here an entity's row list is cut in
 * chunks and the primal system of vfm_foldin.h,
 *   H theta = b,  H = prec (sum_r u_r u_r^T + diag(0, sum_r A_r)) + kl I,  b = prec (sum_r t_r u_r - (0, 1/2 sum_r C_r)),
 * is assembled by one workgroup per chunk:
 *   assemble  chunk c's share, in fp64 and in row order, of the packed lower triangle of sum_r u_r u_r^T and of
 *             sum_r A_r, sum_r (A_r + M_r^2), sum_r t_r u_r, sum_r C_r, into its slab of tri(d + 1) + 4 d + 3 doubles
 *   solve     one workgroup per entity adds its chunks' slabs in chunk order, adds kl, scales by prec and runs the
 *             Cholesky factorisation, the substitutions and the rounding of vfm_foldin_solve_f32, the same code; the
 *             fp32 row is written as that call writes it (the same links, the same inverse for softplus)
 *   loss      L_e at the written fp32 parameters with the per-row arithmetic of vfm_foldin_f32's final pass, a wave per
 *             chunk, the chunks' partials added in fp64 in chunk order
 * The operands are those of vfm_foldin_solve_f32, from the same two prep kernels.  No atomics, no host synchronisation;
 * every sum has a fixed order that depends on the entity's own rows, the chunk length and d alone, so an entity's
 * output bytes do not depend on the other entities of the call, on the grid or on how the caller groups entities into
 * calls.  The primal form is valid for any number of rows; the caller sends entities with more than d rows.
 *
 * Conventions: those of vfm_foldin.h.
 */
#ifndef VFM_SWEEP_H
#define VFM_SWEEP_H

#include <stdint.h>

#include "vfm_foldin.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vfm_foldin_split_t {
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
  const int64_t* entities;  /* [E] folded ids                                                                     */
  const int64_t* chunk_ptr; /* [E + 1] offsets of each entity's chunks in the chunk table, ascending              */
  const int64_t* chunks;    /* [n_chunks, 3] = (entity number in [0, E), first row, rows); an entity's chunks are  */
                            /* consecutive and in row order                                                       */
  const float* y;           /* [R]                                                                                */
  const int64_t* op_x;      /* [n_ops, F] one row of each partner tuple (the folded column is ignored)             */
  const int64_t* row_op;    /* [R] operand of each row                                                            */
  float* entity_params;     /* [T, 2d]: read; the rows of `entities` are written                                  */
  float* bias_params;       /* [T, 2]                                                                             */
  const float* scalars;     /* [3]                                                                                */
  float* out_loss;          /* [E] L_e                                                                            */
  void* workspace;
  int64_t workspace_bytes;
} vfm_foldin_split_t;

/* Workspace of vfm_foldin_solve_split_f32 in bytes: the operand block of vfm_foldin_solve_f32, n_chunks slabs of
 * tri(d + 1) + 4 d + 3 doubles, n_chunks doubles of loss partials and, when a (d + 1) x (d + 1) system does not stay in
 * LDS, min(n_heavy, VFM_FOLDIN_SOLVE_SLABS) triangles.  VFM_E_INVALID on negative arguments, d outside
 * [1, VFM_FOLDIN_MAX_D], lds_dim < -1 or a size past 2^62. */
int64_t vfm_foldin_split_workspace_bytes(int64_t n_chunks, int64_t n_heavy, int64_t n_ops, int32_t d, int32_t lds_dim);

/* Write the exact optimum of every entity of p from its chunks.  An entity id outside [0, T) gets a NaN loss and is not
 * written; a partner id outside [0, T) or a row operand outside [0, n_ops) makes its rows' entities NaN; a chunk is
 * clamped to [0, R) and one whose entity number is outside [0, E) is skipped; an entity without chunks gets the prior.
 * E = 0: nothing is launched.  VFM_E_INVALID (nothing launched) for the range checks of vfm_foldin_solve_f32, n_chunks
 * < 0 and a short or misaligned (256 bytes) workspace. */
int vfm_foldin_solve_split_f32(const vfm_foldin_split_t* p, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VFM_SWEEP_H */
