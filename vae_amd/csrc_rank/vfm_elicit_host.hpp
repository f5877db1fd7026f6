// vfm_elicit_host.hpp -- the host side that vfm_elicit_f32 (vfm_elicit.hip) and vfm_elicit_field_f32
// (vfm_elicit_field.hip) share: the argument checks in the order they are reported, the fill of the kernel arguments
// both forms name alike, and the launch of the session kernel.  Included inside `namespace vfm { namespace {` of a
// unit, after vfm_foldin_body.hpp and the public header vfm_elicit.h.  The two kernels themselves are still two texts
// (k_elicit, k_elicit_field): sharing their body changed the code the compiler generates for them, and the session
// kernel slowed by about 1.5 % at d = 128, so that step is left for a change that can show equal code.
#pragma once

// ---------------------------------------------------------------------------------------------------------------------
// host side: what vfm_elicit_f32 and vfm_elicit_field_f32 share.  P: vfm_elicit_t or vfm_elicit_field_t, which name
// everything shared alike.
// ---------------------------------------------------------------------------------------------------------------------
inline int64_t flags_bytes(int64_t P) { return round_up(P > 0 ? P : 1, 256); }

// the struct's own header and size; the entry point's checks of F and its columns follow
template <class P>
int check_session_struct(const P* p, const char* null_msg, const char* size_msg) {
  if (!p) return fail(VFM_E_INVALID, null_msg);
  if (p->struct_size != (uint32_t)sizeof(P) || p->abi_version != (uint32_t)VFM_ABI_VERSION)
    return fail(VFM_E_INVALID, size_msg);
  if (p->T < 1) return fail(VFM_E_INVALID, "T < 1");
  return 0;
}

// the sizes and options, in the order they are reported.  ops_always: n_ops counts for both objectives (the field
// form's scores need the operands), else for the closed form only.
template <class P>
int check_session_options(const P* p, bool ops_always) {
  const bool bad_ops = p->n_ops < 0 || (p->P + p->H > 0 && p->n_ops < 1);
  if (p->d < 1 || p->d > VFM_FOLDIN_MAX_D) return fail(VFM_E_INVALID, "d out of range [1,512]");
  if (p->U < 0 || p->P < 0 || p->H < 0) return fail(VFM_E_INVALID, "U < 0, P < 0 or H < 0");
  if (p->n_rounds < 0 || p->n_rounds > VFM_ELICIT_MAX_ROUNDS) return fail(VFM_E_INVALID, "n_rounds out of range [0,4096]");
  if (p->strategy < VFM_RANK_TOP || p->strategy > VFM_RANK_RANDOM) return fail(VFM_E_INVALID, "unknown strategy");
  if (p->likelihood != VFM_LIK_NORMAL && p->likelihood != VFM_LIK_BERNOULLI)
    return fail(VFM_E_INVALID, "unknown likelihood");
  if (p->objective == VFM_OBJ_CLOSED_FORM) {
    if (p->likelihood != VFM_LIK_NORMAL) return fail(VFM_E_INVALID, "the closed form needs the Normal likelihood");
    if (!ops_always && bad_ops) return fail(VFM_E_INVALID, "n_ops out of range");
  } else if (p->objective == VFM_OBJ_SAMPLED) {
    if (p->n_samples < 1 || p->n_samples > VFM_FOLDIN_MAX_SAMPLES)
      return fail(VFM_E_INVALID, "n_samples out of range [1,4]");
  } else {
    return fail(VFM_E_INVALID, "unknown objective");
  }
  if (ops_always && bad_ops) return fail(VFM_E_INVALID, "n_ops out of range");
  if (p->flags & ~VFM_FLAG_LINK_SOFTPLUS) return fail(VFM_E_INVALID, "flags: only VFM_FLAG_LINK_SOFTPLUS is accepted");
  if (p->n_steps < 0) return fail(VFM_E_INVALID, "n_steps must be >= 0");
  if (p->t0 < 0 || p->t0 + (int64_t)(p->n_rounds + 1) * ((int64_t)p->n_steps + 1) >=
                       ((int64_t)1 << 60) / VFM_FOLDIN_MAX_SAMPLES)
    return fail(VFM_E_INVALID, "t0 out of range");
  if (!(p->lr >= 0.f) || !(p->kl_weight >= 0.f)) return fail(VFM_E_INVALID, "lr and kl_weight must be >= 0");
  if ((p->out_mean == nullptr) != (p->out_var == nullptr))
    return fail(VFM_E_INVALID, "out_mean and out_var: both or neither");
  return 0;
}

// the pointers both structs name alike (the entry point checks its ids and rows with them, in one message)
template <class P>
bool session_pointers_missing(const P* p) {
  return !p->pool_ptr || !p->entity_params || !p->bias_params || !p->scalars || (p->P > 0 && !p->pool_y) ||
         (p->H > 0 && (!p->hist_ptr || !p->hist_y)) || (p->n_rounds > 0 && (!p->out_row || !p->out_score || !p->out_loss));
}

template <class P>
int check_session_workspace(const P* p, int64_t ws, const char* small_msg) {
  if (ws < 0 || p->workspace_bytes < ws || !p->workspace) return fail(VFM_E_INVALID, small_msg);
  if (((uintptr_t)p->workspace) & 255) return fail(VFM_E_INVALID, "workspace must be 256-byte aligned");
  return 0;
}

// The fields of the kernel arguments that both forms name alike, from p; the asked flags are the head of the workspace.
// A: ElicitArgs or ElicitFieldArgs; the unit adds its ids, rows and operands.
template <class A, class P>
A session_args(const P* p, int F, int col) {
  A a = {};
  a.f = fill_fold_args(p->U, p->T, F, p->d, col, p->likelihood, p->objective == VFM_OBJ_CLOSED_FORM ? 1 : p->n_samples,
                       p->n_steps, p->reset ? 1 : 0, VFM_FOLDIN_FIT, p->lr, p->kl_weight, p->t0, p->seed,
                       p->entity_params, p->bias_params, p->scalars);
  a.U = p->U; a.P = p->P; a.H = p->H; a.Q = p->n_rounds; a.strat = p->strategy; a.write = p->write ? 1 : 0;
  a.seed = p->seed;
  a.pool_ptr = p->pool_ptr; a.pool_y = p->pool_y;
  a.hist_ptr = p->H > 0 ? p->hist_ptr : nullptr; a.hist_y = p->hist_y;
  a.pool_op = p->pool_op; a.hist_op = p->hist_op;
  a.out_row = p->out_row; a.out_score = p->out_score; a.out_loss = p->out_loss; a.out_theta = p->out_theta;
  a.out_mean = p->out_mean; a.out_var = p->out_var;
  a.asked = (uint8_t*)p->workspace;
  return a;
}

// One launch of the session kernel for shape sh.  theta_floats(DP): the floats of a group's LDS copy of theta next to
// its fold stage; kernel_of(IntC<W>, IntC<CPL>, IntC<LINK>, bool_constant<SAMPLED>): the unit's instance.
template <class Args, class ThetaFloats, class KernelOf>
void launch_session(const FShape& sh, bool sp, bool sampled, const Args& a, hipStream_t st, ThetaFloats&& theta_floats,
                    KernelOf&& kernel_of) {
  for_link(sp, [&](auto link) {
    for_shape(sh, [&](auto w, auto c) {
      constexpr int W = decltype(w)::value, DP = W * decltype(c)::value, GPB = FB / W;
      const size_t shm = (size_t)GPB * ((size_t)a.f.cap * (DP + 1) + theta_floats(DP)) * 4;
      const auto k = sampled ? kernel_of(w, c, link, std::true_type{}) : kernel_of(w, c, link, std::false_type{});
      hipLaunchKernelGGL(k, dim3((unsigned)((a.U + GPB - 1) / GPB)), dim3(FB), shm, st, a);
    });
  });
}
