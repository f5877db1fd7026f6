/*
 * vfm_implicit.h -- C ABI of the implicit-feedback solves of libvfm_hip.so (gfx950): the exact fold-in of vfm_foldin.h
 * over EVERY (entity, partner) pair of a two-field 'reg' model, the hot path of VFM.fit_implicit.
 *
 * Every pair (e, j) of the folded field's entity e and the partner field's entity j is a row: an observed pair has its
 * target y and the weight w1, every other pair the target 0 and the weight w0 (w1 >= w0 > 0; Hu, Koren & Volinsky).  At
 * F = 2 a partner j is u_j = (1, M_j) with M_j = mu_j, A_j = sigma_j^2, C_j = 0, c_mean,j = m_0 + mu_w,j and
 * c_var,j = sigma_0^2 + sigma_w,j^2 (the operands of vfm_foldin.h).  The sums over all partners do not depend on e:
 *
 *   base      of the partner field's id range [lo, lo + n), vfm_implicit_base_f32, in fp64:
 *               T_B = sum_j u_j u_j^T (packed lower triangle)   SA_B = sum_j A_j   SB_B = sum_j (A_j + M_j^2), SB_B[0] = n
 *               tu_B = sum_j (-c_mean,j) u_j                    tt_B = sum_j (c_mean,j^2 + c_var,j)
 *             laid out [tri(d + 1) | SA [d + 1] | SB [d + 1] | tu [d + 1] | tt] (SA[0] = 0): vfm_implicit_base_doubles(d)
 *             doubles.  A workgroup per chunk of chunk_rows ids assembles its share in id order (the tile scheme of
 *             vfm_sweep.h's assembly), then the shares are added in chunk order.
 *   solve     vfm_foldin_solve_implicit_f32, a workgroup per entity, with dw = w1 - w0, prec = link(alpha), kl =
 *             kl_weight > 0, obs(e) the observed rows of e and n_e their number:
 *               H = kl I + prec [ w0 (T_B + diag(0, SA_B)) + dw sum_{r in obs(e)} (u_r u_r^T + diag(0, A_r)) ]
 *               b = prec [ w0 tu_B + sum_{r in obs(e)} (w1 y_r - dw c_mean,r) u_r ],   theta = H^-1 b
 *               sigma_w^2 = kl / (kl + prec (w0 n + dw n_e))
 *               sigma_k^2 = kl / (kl + prec (w0 SB_B,k + dw sum_obs (A_rk + M_rk^2)))
 *             always in the primal (d + 1) x (d + 1) form (the base has full rank), with the Cholesky factorisation, the
 *             substitutions and the rounding of vfm_foldin_solve_f32, the same code, and the row written as that call
 *             writes it.  An entity of the row-list form (chunk_ptr NULL) accumulates its observed rows inside its
 *             workgroup, a thread per triangle element, rows in order; an entity of the chunk form (chunk_ptr given) has
 *             its rows cut in chunks, a workgroup per chunk assembles the chunk's share and the entity's workgroup adds
 *             the shares in chunk order.  An entity without observed rows gets the base-only optimum.
 *   loss      L_e = sum over ALL partners j of w_ej [1/2 prec ((y_ej - E pred)^2 + Var pred) - 1/2 log prec + 1/2 log 2 pi]
 *             + kl KL(q_e || N(0, 1)) at the written fp32 parameters, from the assembled fp64 system: with theta and
 *             sigma the written values,
 *               L_e = 1/2 [prec tt' - 2 theta . b + (theta^T H theta - kl |theta|^2) + prec sum_c sigma_c^2 SB'_c]
 *                     + (w0 n + dw n_e) (1/2 log 2 pi - 1/2 log prec) + kl KL
 *               tt' = w0 tt_B + sum_obs (w1 (y_r - c_mean,r)^2 - w0 c_mean,r^2 + dw c_var,r)
 *             theta^T H theta = |L^T theta|^2 from the Cholesky factor: no second pass over the rows.
 *
 * No atomics, no host synchronisation; every sum has a fixed order that depends on the entity's observed rows, the
 * partner field's catalog, chunk_rows and d alone, so an entity's output bytes do not depend on the other entities of
 * the call, on the grid or on how the caller groups entities into calls.
 *
 * Conventions: those of vfm_foldin.h (device pointers, launch-only, caller-owned workspace, 0 / VFM_E_* / hipError_t,
 * every argument checked before any HIP call).
 */
#ifndef VFM_IMPLICIT_H
#define VFM_IMPLICIT_H

#include <stdint.h>

#include "vfm_foldin.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vfm_implicit_base_t {
  int64_t T;          /* table rows                                                                              */
  int64_t lo, n;      /* the field's id range [lo, lo + n) within [0, T), n >= 1                                 */
  int64_t chunk_rows; /* ids per chunk (>= 1)                                                                    */
  int32_t d;          /* embedding size (1 .. VFM_FOLDIN_MAX_D)                                                  */
  int32_t flags;      /* 0 or VFM_FLAG_LINK_SOFTPLUS                                                             */
  const float* entity_params; /* [T, 2d]                                                                         */
  const float* bias_params;   /* [T, 2]                                                                          */
  const float* scalars;       /* [3]                                                                             */
  double* out_base;           /* [vfm_implicit_base_doubles(d)]                                                  */
  void* workspace;
  int64_t workspace_bytes;
} vfm_implicit_base_t;

/* Doubles of a base block: tri(d + 1) + 3 (d + 1) + 1.  VFM_E_INVALID for d outside [1, VFM_FOLDIN_MAX_D]. */
int64_t vfm_implicit_base_doubles(int32_t d);

/* Workspace of vfm_implicit_base_f32 in bytes: ceil(n / chunk_rows) slabs of vfm_implicit_base_doubles(d) doubles.
 * VFM_E_INVALID for n < 1, chunk_rows < 1, d outside [1, VFM_FOLDIN_MAX_D] or a size past 2^62. */
int64_t vfm_implicit_base_workspace_bytes(int64_t n, int64_t chunk_rows, int32_t d);

/* Write the base block of p's id range.  VFM_E_INVALID (nothing launched) for T < 1, a range outside [0, T), n < 1,
 * chunk_rows < 1, d out of range, other flags, a null pointer and a short or misaligned (256 bytes) workspace. */
int vfm_implicit_base_f32(const vfm_implicit_base_t* p, void* stream);

typedef struct vfm_implicit_solve_t {
  int64_t E;          /* entities of the call                                                                    */
  int64_t R;          /* observed rows (of y / partner)                                                          */
  int64_t T;          /* table rows                                                                              */
  int64_t n_chunks;   /* rows of the chunk table (0 in the row-list form)                                        */
  int64_t lo, n;      /* the partner field's id range [lo, lo + n), the range of `base`                           */
  int32_t d;          /* embedding size (1 .. VFM_FOLDIN_MAX_D)                                                  */
  int32_t flags;      /* 0 or VFM_FLAG_LINK_SOFTPLUS                                                             */
  int32_t lds_dim;    /* as in vfm_foldin_solve_t                                                                */
  float kl_weight;    /* > 0                                                                                     */
  float w0, w1;       /* weight of an unobserved pair (> 0) and of an observed one (>= w0), finite               */
  const int64_t* entities;  /* [E] folded ids                                                                     */
  const int64_t* row_ptr;   /* row-list form: [E + 1] offsets of each entity's observed rows; else NULL            */
  const int64_t* chunk_ptr; /* chunk form: [E + 1] offsets of each entity's chunks in the chunk table; else NULL   */
  const int64_t* chunks;    /* chunk form: [n_chunks, 3] = (entity number in [0, E), first row, rows); an entity's */
                            /* chunks are consecutive, in row order and hold all its observed rows                */
  const float* y;           /* [R] targets of the observed rows                                                   */
  const int64_t* partner;   /* [R] partner id of each observed row, within [lo, lo + n); distinct per entity      */
  const double* base;       /* [vfm_implicit_base_doubles(d)] the partner field's base (vfm_implicit_base_f32)    */
  float* entity_params;     /* [T, 2d]: read; the rows of `entities` are written                                  */
  float* bias_params;       /* [T, 2]                                                                             */
  const float* scalars;     /* [3]                                                                                */
  float* out_loss;          /* [E] L_e                                                                            */
  void* workspace;
  int64_t workspace_bytes;
} vfm_implicit_solve_t;

/* Workspace of vfm_foldin_solve_implicit_f32 in bytes: n_chunks slabs of vfm_implicit_base_doubles(d) doubles and,
 * when a (d + 1) x (d + 1) system does not stay in LDS, min(E, VFM_FOLDIN_SOLVE_SLABS) triangles.  VFM_E_INVALID on
 * negative arguments, d outside [1, VFM_FOLDIN_MAX_D], lds_dim < -1 or a size past 2^62. */
int64_t vfm_implicit_solve_workspace_bytes(int64_t E, int64_t n_chunks, int32_t d, int32_t lds_dim);

/* Write the optimum of every entity of p.  An entity id outside [0, T) gets a NaN loss and is not written; a partner id
 * outside [lo, lo + n) makes the entity's means, factor scales and loss NaN (s_w, a function of the counts, stays
 * finite); a row list or a chunk is clamped to [0, R) and chunk_ptr to [0, n_chunks] (a chunk's entity number is not read).
 * E = 0: nothing is launched.  VFM_E_INVALID (nothing launched) for T < 1, d out of range, E < 0, R < 0, n_chunks < 0, a
 * range outside [0, T) or n < 1, other flags, lds_dim < -1, kl_weight <= 0 or not finite, w0 <= 0, w1 < w0 or not
 * finite, both or neither of row_ptr and chunk_ptr, a null pointer and a short or misaligned (256 bytes) workspace. */
int vfm_foldin_solve_implicit_f32(const vfm_implicit_solve_t* p, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VFM_IMPLICIT_H */
