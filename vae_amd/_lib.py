"""Loader for the C-ABI library `libvfm_hip.so` (include/vfm_hip.h).

The library is built in-tree by `vae_amd.build.build_all()` (hipcc, gfx950).  There is NO
fallback: if it is missing or does not load, every op of this package raises.
`import torch` must happen before the library is opened so that both resolve the same
HIP runtime (`libamdhip64.so.7`).
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (loads the HIP runtime the library binds to)

HERE = os.path.dirname(os.path.abspath(__file__))
# VFM_LIB_DIR: another build of the two libraries (the host-sanitizer build of vae_amd.build.build_sanitized)
LIB_DIR = os.environ.get("VFM_LIB_DIR") or HERE
LIB_PATH = os.path.join(LIB_DIR, "libvfm_hip.so")
OPS_PATH = os.path.join(LIB_DIR, "libvfm_torch_ops.so")

from . import _abi_gen as _gen      # GENERATED from include/vfm_hip.h (tools/gen_bindings.py): constants + struct mirrors

ABI_VERSION = _gen.VFM_ABI_VERSION
MAX_FWD_BLOCKS = _gen.VFM_MAX_FWD_BLOCKS
MAX_FIELDS = _gen.VFM_MAX_FIELDS
N_PARTIALS = _gen.VFM_N_PARTIALS
PARTIALS_LEN = _gen.VFM_PARTIALS_LEN
P_LL, P_KL, P_G, P_ALPHA, P_BADID = _gen.VFM_P_LL, _gen.VFM_P_KL, _gen.VFM_P_G, _gen.VFM_P_ALPHA, _gen.VFM_P_BADID
LIK_NORMAL, LIK_BERNOULLI = _gen.VFM_LIK_NORMAL, _gen.VFM_LIK_BERNOULLI
OBJ_SAMPLED, OBJ_CLOSED_FORM = _gen.VFM_OBJ_SAMPLED, _gen.VFM_OBJ_CLOSED_FORM

EXPORTS = (
    "vfm_abi_version", "vfm_last_error", "vfm_inv_occ_f32", "vfm_batch_norms",
    "vfm_elbo_fwd_f32", "vfm_elbo_finalize_f32", "vfm_elbo_bwd_f32", "vfm_philox_eps_f32",
    "vfm_adam_f32", "vfm_elbo_bwd_adam_f32", "vfm_elbo_bwd_acc_f32", "vfm_elbo_apply_adam_f32",
    "vfm_moments_rescale_f32", "vfm_index_workspace_bytes", "vfm_build_index", "vfm_heavy_list_for",
    "vfm_variant_fwd_f32", "vfm_variant_bwd_f32", "vfm_variant_workspace_elems", "vfm_adam_catchup_f32", "vfm_union_rows", "vfm_union_workspace_bytes",
    "vfm_sample_records_f32", "vfm_elbo_bwd_adam_pipe_f32", "vfm_elbo_bwd_adam_lookahead_f32",
    "vfm_step_consts", "vfm_dev_step_set", "vfm_wrec_build_f32", "vfm_elbo_apply_adam_rows_f32",
    "vfm_elbo_bwd_acc_rows_f32", "vfm_heavy_threshold", "vfm_rebuild_heavy",
)


class _Strict:
    """ctypes accepts ANY attribute name and silently keeps it as a Python attribute: a misspelt or missing field
    would leave the struct member 0 without an error."""

    def __setattr__(self, name, value):
        if name not in type(self)._names:
            raise AttributeError(f"{type(self).__name__} has no field {name!r}")
        super().__setattr__(name, value)


class Problem(_Strict, _gen.Problem):
    """`vfm_problem_t` (struct_size / abi_version are set by the generated __init__)."""


class Index(_Strict, _gen.Index):
    """`vfm_index_t`."""


class Pipe(_Strict, _gen.Pipe):
    """`vfm_pipe_t`."""


StepConsts, DevStep = _gen.StepConsts, _gen.DevStep

# ---- elicitation sessions (include/vfm_elicit.h): constants and the mirror of vfm_elicit_t, field for field
ELICIT_MAX_ROUNDS = 4096
# the exact field-form session (vfm_elicit_solve_f32) is declared in the same header
ELICIT_SOLVE_EXPORTS = ("vfm_elicit_solve_f32", "vfm_elicit_solve_workspace_bytes")
ELICIT_EXPORTS = ("vfm_elicit_f32", "vfm_elicit_workspace_bytes", "vfm_elicit_field_f32",
                  "vfm_elicit_field_workspace_bytes") + ELICIT_SOLVE_EXPORTS


# ---- the field-form ranking under supplied posteriors (include/vfm_rank.h: the *_post_f32 entry points)
RANK_POST_EXPORTS = ("vfm_field_moments_post_f32", "vfm_rank_field_post_f32", "vfm_rank_heldout_field_post_f32")


# ---- fused Adam step of the ELBO variants (include/vfm_variant_step.h)
VARIANT_STEP_EXPORTS = ("vfm_variant_step_f32", "vfm_variant_step_workspace_bytes")


def _fields(ctype, *names):
    return tuple((n, ctype) for n in names)


# ---- the fold-in solves: exact (include/vfm_foldin.h: vfm_foldin_solve_f32), split exact (include/vfm_sweep.h, the hot
# path of VFM.fit_exact), under a learnt field prior (include/vfm_prior.h: the same structs plus the prior pointer), bound
# for 'class' models (include/vfm_bound.h) and split bound (include/vfm_bound_sweep.h, the hot path of VFM.fit_bound), and
# the two bound forms under a learnt field prior (include/vfm_bound_prior.h: again the same structs plus the prior pointer)
FOLDIN_SOLVE_EXPORTS = ("vfm_foldin_solve_f32", "vfm_foldin_solve_workspace_bytes")
FOLDIN_SOLVE_LDS_DIM = 135
FOLDIN_SOLVE_SLABS = 256
SWEEP_EXPORTS = ("vfm_foldin_solve_split_f32", "vfm_foldin_split_workspace_bytes")
PRIOR_EXPORTS = ("vfm_foldin_solve_prior_f32", "vfm_foldin_solve_prior_workspace_bytes",
                 "vfm_foldin_solve_split_prior_f32", "vfm_foldin_split_prior_workspace_bytes")
BOUND_EXPORTS = ("vfm_foldin_bound_f32", "vfm_foldin_bound_workspace_bytes")
BOUND_SWEEP_EXPORTS = ("vfm_foldin_bound_split_f32", "vfm_foldin_bound_split_workspace_bytes")
BOUND_PRIOR_EXPORTS = ("vfm_foldin_bound_prior_f32", "vfm_foldin_bound_prior_workspace_bytes",
                       "vfm_foldin_bound_split_prior_f32", "vfm_foldin_bound_split_prior_workspace_bytes")

# the runs of fields that the four structs name alike; between them the row-list forms have objective and likelihood and
# a row_ptr, the chunk forms n_chunks and the chunk table, the bound forms n_iters and reset
_FOLD_COUNTS = _fields(C.c_int64, "E", "R", "T", "n_ops")
_FOLD_DIMS = _fields(C.c_int32, "F", "d", "col")
_FOLD_OPTIONS = _fields(C.c_int32, "flags", "lds_dim") + (("kl_weight", C.c_float),)
_FOLD_IDS = (("entities", C.c_void_p),)
_FOLD_TAIL = (_fields(C.c_void_p, "y", "op_x", "row_op", "entity_params", "bias_params", "scalars", "out_loss", "workspace")
              + (("workspace_bytes", C.c_int64),))
_FOLD_LIST_HEAD = _FOLD_COUNTS + _FOLD_DIMS + _fields(C.c_int32, "objective", "likelihood") + _FOLD_OPTIONS
_FOLD_CHUNK_HEAD = _FOLD_COUNTS + (("n_chunks", C.c_int64),) + _FOLD_DIMS + _FOLD_OPTIONS
_FOLD_LIST_ROWS = _FOLD_IDS + (("row_ptr", C.c_void_p),) + _FOLD_TAIL
_FOLD_CHUNK_ROWS = _FOLD_IDS + _fields(C.c_void_p, "chunk_ptr", "chunks") + _FOLD_TAIL


class FoldinSolve(_Strict, C.Structure):
    """`vfm_foldin_solve_t` (tests/test_foldin_exact_cpu.py checks the layout against gcc's)."""
    _fields_ = list(_FOLD_LIST_HEAD + _FOLD_LIST_ROWS)


class FoldinSplit(_Strict, C.Structure):
    """`vfm_foldin_split_t` (tests/test_fit_exact_cpu.py checks the layout against gcc's)."""
    _fields_ = list(_FOLD_CHUNK_HEAD + _FOLD_CHUNK_ROWS)


class FoldinBound(_Strict, C.Structure):
    """`vfm_foldin_bound_t` (tests/test_foldin_bound_cpu.py checks the layout against gcc's)."""
    _fields_ = list(_FOLD_LIST_HEAD + _fields(C.c_int32, "n_iters", "reset", "mode", "pad0") + _FOLD_LIST_ROWS)


class FoldinBoundSplit(_Strict, C.Structure):
    """`vfm_foldin_bound_split_t`: vfm_foldin_split_t's fields, n_iters and reset (tests/test_fit_bound_cpu.py checks the
    layout against gcc's)."""
    _fields_ = list(_FOLD_CHUNK_HEAD + _fields(C.c_int32, "n_iters", "reset") + _FOLD_CHUNK_ROWS)


# the family's prototypes: (entry point, struct, extra arguments, size function, its argument types)
_I64, _I32 = C.c_int64, C.c_int32
_SOLVE_SIZES, _SPLIT_SIZES = [_I64, _I64, _I32, _I32], [_I64, _I64, _I64, _I32, _I32]
_FOLD_PROTOTYPES = (
    ("vfm_foldin_solve_f32", FoldinSolve, [], "vfm_foldin_solve_workspace_bytes", _SOLVE_SIZES),
    ("vfm_foldin_solve_split_f32", FoldinSplit, [], "vfm_foldin_split_workspace_bytes", _SPLIT_SIZES),
    ("vfm_foldin_solve_prior_f32", FoldinSolve, [C.c_void_p], "vfm_foldin_solve_prior_workspace_bytes", _SOLVE_SIZES),
    ("vfm_foldin_solve_split_prior_f32", FoldinSplit, [C.c_void_p], "vfm_foldin_split_prior_workspace_bytes", _SPLIT_SIZES),
    ("vfm_foldin_bound_f32", FoldinBound, [], "vfm_foldin_bound_workspace_bytes", [_I64] + _SOLVE_SIZES),
    ("vfm_foldin_bound_split_f32", FoldinBoundSplit, [], "vfm_foldin_bound_split_workspace_bytes", [_I64] + _SPLIT_SIZES),
    ("vfm_foldin_bound_prior_f32", FoldinBound, [C.c_void_p], "vfm_foldin_bound_prior_workspace_bytes", [_I64] + _SOLVE_SIZES),
    ("vfm_foldin_bound_split_prior_f32", FoldinBoundSplit, [C.c_void_p], "vfm_foldin_bound_split_prior_workspace_bytes",
     [_I64] + _SPLIT_SIZES),
)


# ---- the implicit-feedback solves (include/vfm_implicit.h, the hot path of VFM.fit_implicit): a field's base block and
# the solve of every (entity, partner) pair that starts from it
IMPLICIT_EXPORTS = ("vfm_implicit_base_doubles", "vfm_implicit_base_workspace_bytes", "vfm_implicit_base_f32",
                    "vfm_implicit_solve_workspace_bytes", "vfm_foldin_solve_implicit_f32")
# ... under a learnt field prior (include/vfm_implicit_prior.h: the same struct plus the prior pointer)
IMPLICIT_PRIOR_EXPORTS = ("vfm_implicit_solve_prior_workspace_bytes", "vfm_foldin_solve_implicit_prior_f32")
# ... with a weight per observed row (include/vfm_implicit_weights.h: the same struct, the prior and the weights pointers)
IMPLICIT_WEIGHTS_EXPORTS = ("vfm_implicit_solve_weights_workspace_bytes", "vfm_foldin_solve_implicit_weights_f32")


class ImplicitBase(_Strict, C.Structure):
    """`vfm_implicit_base_t` (tests/test_fit_implicit_cpu.py checks the layout against gcc's)."""
    _fields_ = list(_fields(C.c_int64, "T", "lo", "n", "chunk_rows") + _fields(C.c_int32, "d", "flags")
                    + _fields(C.c_void_p, "entity_params", "bias_params", "scalars", "out_base", "workspace")
                    + (("workspace_bytes", C.c_int64),))


class ImplicitSolve(_Strict, C.Structure):
    """`vfm_implicit_solve_t` (tests/test_fit_implicit_cpu.py checks the layout against gcc's)."""
    _fields_ = list(_fields(C.c_int64, "E", "R", "T", "n_chunks", "lo", "n") + _fields(C.c_int32, "d", "flags", "lds_dim")
                    + _fields(C.c_float, "kl_weight", "w0", "w1")
                    + _fields(C.c_void_p, "entities", "row_ptr", "chunk_ptr", "chunks", "y", "partner", "base",
                              "entity_params", "bias_params", "scalars", "out_loss", "workspace")
                    + (("workspace_bytes", C.c_int64),))


# ---- the implicit field-form session (include/vfm_elicit_implicit.h): vfm_elicit_solve_t, the partner field's base
# block with its range and the two weights in a struct of their own, and the prior pointer (NULL: N(0, 1))
ELICIT_IMPLICIT_EXPORTS = ("vfm_elicit_implicit_f32", "vfm_elicit_implicit_workspace_bytes")


class ElicitImplicit(_Strict, C.Structure):
    """`vfm_elicit_implicit_t` (tests/test_elicit_implicit_cpu.py checks the layout against gcc's)."""
    _fields_ = list(_fields(C.c_float, "w0", "w1") + _fields(C.c_int64, "lo", "n") + (("base", C.c_void_p),))


# the bound field-form session (vfm_elicit_bound_f32) is declared in vfm_bound.h too
ELICIT_BOUND_EXPORTS = ("vfm_elicit_bound_f32", "vfm_elicit_bound_workspace_bytes")


# ---- the session structs: the runs of fields that every form names alike, and the stamp every one starts with
_STAMP = _fields(C.c_uint32, "struct_size", "abi_version")
_COUNTS = _fields(C.c_int64, "U", "P", "H", "T", "n_ops")
_FIELD_ROWS = _fields(C.c_void_p, "entities", "pool_ptr", "pool_x", "pool_y", "hist_ptr", "hist_x", "hist_y")
_OPERANDS = _fields(C.c_void_p, "op_x", "pool_op", "hist_op")
_TABLES_OUTPUTS = _fields(C.c_void_p, "entity_params", "bias_params", "scalars", "out_row", "out_score", "out_loss",
                          "out_theta", "out_mean", "out_var")
_WORKSPACE = (("workspace", C.c_void_p), ("workspace_bytes", C.c_int64))
_ADAM_TAIL = (_fields(C.c_int32, "objective", "likelihood", "flags", "n_steps", "n_samples", "reset", "write", "lds_rows")
              + _fields(C.c_float, "lr", "kl_weight") + (("seed", C.c_uint64), ("t0", C.c_int64)))
_SOLVE_HEAD = (_fields(C.c_int32, "F", "d", "field", "key_col", "n_rounds", "strategy", "flags", "reset", "write", "lds_dim")
               + (("kl_weight", C.c_float),))
_SEED = (("seed", C.c_uint64),)


class _Session(_Strict, C.Structure):
    """A session struct: struct_size and abi_version stamped as VFM_STRUCT_INIT does."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size, self.abi_version = C.sizeof(type(self)), ABI_VERSION


class Elicit(_Session):
    """`vfm_elicit_t` (tests/test_elicit_cpu.py checks the layout against gcc's)."""
    _fields_ = list(_STAMP + _COUNTS + _fields(C.c_int32, "F", "d", "n_rounds", "strategy") + _ADAM_TAIL
                    + _fields(C.c_void_p, "users", "pool_ptr", "pool_items", "pool_y", "hist_ptr", "hist_items", "hist_y")
                    + _OPERANDS + _TABLES_OUTPUTS + _WORKSPACE)


class ElicitField(_Session):
    """`vfm_elicit_field_t` (tests/test_elicit_field_cpu.py checks the layout against gcc's)."""
    _fields_ = list(_STAMP + _COUNTS + _fields(C.c_int32, "F", "d", "field", "key_col", "n_rounds", "strategy")
                    + _ADAM_TAIL + _FIELD_ROWS + _OPERANDS + _TABLES_OUTPUTS + _WORKSPACE)


class ElicitSolve(_Session):
    """`vfm_elicit_solve_t` (tests/test_elicit_exact_cpu.py checks the layout against gcc's)."""
    _fields_ = list(_STAMP + _COUNTS + _SOLVE_HEAD + _SEED + _FIELD_ROWS + _OPERANDS + _TABLES_OUTPUTS + _WORKSPACE)


class ElicitBound(_Session):
    """`vfm_elicit_bound_t`: vfm_elicit_solve_t's fields and n_iters (tests/test_elicit_bound_cpu.py checks the layout
    against gcc's)."""
    _fields_ = list(_STAMP + _COUNTS + _SOLVE_HEAD + (("n_iters", C.c_int32),) + _SEED + _FIELD_ROWS + _OPERANDS
                    + _TABLES_OUTPUTS + _WORKSPACE)


# ---- target-aware elicitation (include/vfm_design.h)
DESIGN_EXPORTS = ("vfm_design_workspace_bytes", "vfm_design_scores_f32", "vfm_design_elicit_f32")


class ElicitDesign(_Session):
    """`vfm_design_t` (tests/test_design_cpu.py checks the layout against gcc's)."""
    _fields_ = list(_STAMP + _COUNTS + (("n_targets", C.c_int64),)
                    + _fields(C.c_int32, "F", "d", "field", "n_rounds", "flags", "reset", "write", "lds_dim")
                    + (("kl_weight", C.c_float),) + _FIELD_ROWS + _fields(C.c_void_p, "tgt_ptr", "tgt_op") + _OPERANDS
                    + _TABLES_OUTPUTS + (("out_pool_score", C.c_void_p),) + _WORKSPACE)


# ---- the exact, bound and design sessions under a learnt field prior (include/vfm_elicit_prior.h: the same structs plus
# the prior pointer): (entry point, struct, size function, its argument types)
ELICIT_PRIOR_EXPORTS = ("vfm_elicit_solve_prior_f32", "vfm_elicit_solve_prior_workspace_bytes",
                        "vfm_elicit_bound_prior_f32", "vfm_elicit_bound_prior_workspace_bytes",
                        "vfm_design_scores_prior_f32", "vfm_design_elicit_prior_f32", "vfm_design_prior_workspace_bytes")
_ELICIT_PRIOR_PROTOTYPES = (
    ("vfm_elicit_solve_prior_f32", ElicitSolve, "vfm_elicit_solve_prior_workspace_bytes", [_I64, _I64, _I64, _I32, _I32]),
    ("vfm_elicit_bound_prior_f32", ElicitBound, "vfm_elicit_bound_prior_workspace_bytes",
     [_I64, _I64, _I64, _I64, _I32, _I32, _I32]),
    ("vfm_design_scores_prior_f32", ElicitDesign, "vfm_design_prior_workspace_bytes", [_I64, _I64, _I64, _I32, _I32]),
    ("vfm_design_elicit_prior_f32", ElicitDesign, "vfm_design_prior_workspace_bytes", [_I64, _I64, _I64, _I32, _I32]),
)


for _c in (Problem, Index, Pipe, Elicit, ElicitField, ElicitSolve, ElicitBound, ElicitDesign, FoldinSolve, FoldinSplit,
           FoldinBound, FoldinBoundSplit, ImplicitBase, ImplicitSolve, ElicitImplicit):
    _c._names = frozenset(n for n, _ in _c._fields_)


def heavy_list_for(n_occ: int, T: int) -> int:
    """Length above which an occurrence list is cut in work items: the library's rule (vfm_heavy_list_for)."""
    return int(load().vfm_heavy_list_for(int(n_occ), int(T)))


class VfmLibraryError(RuntimeError):
    pass


_lib = None


def load():
    """Open libvfm_hip.so (once) and declare the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VfmLibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  vae_amd has no CPU / PyTorch fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    PP = C.POINTER(Problem)
    lib.vfm_abi_version.restype = C.c_int
    lib.vfm_abi_version.argtypes = []
    lib.vfm_last_error.restype = C.c_char_p
    lib.vfm_last_error.argtypes = []
    lib.vfm_inv_occ_f32.argtypes = [vp, vp, i64, vp]
    lib.vfm_batch_norms.argtypes = [PP, vp, vp, vp, vp]
    lib.vfm_elbo_fwd_f32.argtypes = [PP] + [vp] * 15
    lib.vfm_elbo_finalize_f32.argtypes = [PP, vp, vp, vp, vp]
    lib.vfm_elbo_bwd_f32.argtypes = [PP] + [vp] * 17
    lib.vfm_philox_eps_f32.argtypes = [PP, vp, vp, vp, vp]
    lib.vfm_elbo_bwd_adam_f32.argtypes = ([PP] + [vp] * 18 +
                                          [C.c_float, C.c_float, C.c_float, C.c_float, i64, vp, vp])
    lib.vfm_adam_f32.argtypes = [vp, vp, vp, vp, i64, C.c_float, C.c_float, C.c_float, C.c_float,
                                 i64, vp]
    lib.vfm_elbo_bwd_acc_f32.argtypes = [PP] + [vp] * 7
    lib.vfm_elbo_apply_adam_f32.argtypes = ([PP] + [vp] * 16 +
                                            [C.c_float, C.c_float, C.c_float, C.c_float, i64, vp])
    lib.vfm_elbo_bwd_acc_rows_f32.argtypes = [PP, C.POINTER(Index), vp, i64] + [vp] * 6
    lib.vfm_elbo_apply_adam_rows_f32.argtypes = ([PP, vp, vp, vp, i64, i32] + [vp] * 11 +
                                                 [C.c_float, C.c_float, C.c_float, C.c_float, i64, vp])
    lib.vfm_moments_rescale_f32.argtypes = [vp, vp, i64, C.c_float, C.c_float, i64, i32, vp]
    lib.vfm_index_workspace_bytes.argtypes = [i64, i32, i64]
    lib.vfm_heavy_list_for.argtypes = [i64, i64]
    lib.vfm_build_index.argtypes = [i64, i32, i64, i32, vp, vp, vp, vp, i32, vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp]
    lib.vfm_rebuild_heavy.argtypes = [i64, vp, vp, i32, i32, vp, i64, vp, i64, vp, vp]
    lib.vfm_adam_catchup_f32.argtypes = [vp] * 8 + [i64, i64, i32, C.POINTER(C.c_float), i64, C.c_float, C.c_float, C.c_float,
                                         i64, i64, vp, vp]
    lib.vfm_step_consts.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float, i64, i32, C.POINTER(StepConsts)]
    lib.vfm_dev_step_set.argtypes = [vp, C.c_uint64, i64, vp]
    lib.vfm_wrec_build_f32.argtypes = [vp, vp, i64, vp, vp]
    lib.vfm_sample_records_f32.argtypes = [PP, vp, i64, vp, vp, vp, vp, vp, vp]
    lib.vfm_elbo_bwd_adam_pipe_f32.argtypes = ([PP, C.POINTER(Index), C.POINTER(Pipe)] + [vp] * 13 +
                                               [C.c_float, C.c_float, C.c_float, C.c_float, i64, vp, vp])
    lib.vfm_elbo_bwd_adam_lookahead_f32.argtypes = ([PP, C.POINTER(Index)] + [vp] * 14 +
                                                    [C.c_float, C.c_float, C.c_float, C.c_float, i64, vp, vp, vp, vp, vp])
    lib.vfm_variant_fwd_f32.argtypes = [PP, i32] + [vp] * 18
    lib.vfm_variant_bwd_f32.argtypes = [PP, i32, C.POINTER(Index)] + [vp] * 21
    lib.vfm_union_workspace_bytes.argtypes = [i64]
    lib.vfm_union_workspace_bytes.restype = i64
    lib.vfm_union_rows.argtypes = [i64] + [vp] * 7
    lib.vfm_variant_workspace_elems.argtypes = [i64, i32, i32]
    lib.vfm_variant_workspace_elems.restype = i64
    lib.vfm_elicit_f32.argtypes = [C.POINTER(Elicit), vp]
    lib.vfm_elicit_f32.restype = C.c_int
    lib.vfm_elicit_workspace_bytes.argtypes = [i64, i64, i32, i32]
    lib.vfm_elicit_workspace_bytes.restype = i64
    lib.vfm_elicit_field_f32.argtypes = [C.POINTER(ElicitField), vp]
    lib.vfm_elicit_field_f32.restype = C.c_int
    lib.vfm_elicit_field_workspace_bytes.argtypes = [i64, i64, i32, i32]
    lib.vfm_elicit_field_workspace_bytes.restype = i64
    lib.vfm_elicit_solve_f32.argtypes = [C.POINTER(ElicitSolve), vp]
    lib.vfm_elicit_solve_f32.restype = C.c_int
    lib.vfm_elicit_solve_workspace_bytes.argtypes = [i64, i64, i64, i32, i32]
    lib.vfm_elicit_solve_workspace_bytes.restype = i64
    lib.vfm_design_workspace_bytes.argtypes = [i64, i64, i64, i32, i32]
    lib.vfm_design_workspace_bytes.restype = i64
    for name in ("vfm_design_scores_f32", "vfm_design_elicit_f32"):
        getattr(lib, name).argtypes = [C.POINTER(ElicitDesign), vp]
        getattr(lib, name).restype = C.c_int
    for entry, struct, extra, size, size_args in _FOLD_PROTOTYPES:
        getattr(lib, entry).argtypes = [C.POINTER(struct)] + extra + [vp]
        getattr(lib, entry).restype = C.c_int
        getattr(lib, size).argtypes = size_args
        getattr(lib, size).restype = i64
    lib.vfm_implicit_base_doubles.argtypes = [i32]
    lib.vfm_implicit_base_workspace_bytes.argtypes = [i64, i64, i32]
    lib.vfm_implicit_solve_workspace_bytes.argtypes = [i64, i64, i32, i32]
    for name in ("vfm_implicit_base_doubles", "vfm_implicit_base_workspace_bytes", "vfm_implicit_solve_workspace_bytes"):
        getattr(lib, name).restype = i64
    lib.vfm_implicit_base_f32.argtypes = [C.POINTER(ImplicitBase), vp]
    lib.vfm_implicit_base_f32.restype = C.c_int
    lib.vfm_foldin_solve_implicit_f32.argtypes = [C.POINTER(ImplicitSolve), vp]
    lib.vfm_foldin_solve_implicit_f32.restype = C.c_int
    lib.vfm_implicit_solve_prior_workspace_bytes.argtypes = [i64, i64, i32, i32]
    lib.vfm_implicit_solve_prior_workspace_bytes.restype = i64
    lib.vfm_foldin_solve_implicit_prior_f32.argtypes = [C.POINTER(ImplicitSolve), vp, vp]
    lib.vfm_foldin_solve_implicit_prior_f32.restype = C.c_int
    lib.vfm_implicit_solve_weights_workspace_bytes.argtypes = [i64, i64, i32, i32]
    lib.vfm_implicit_solve_weights_workspace_bytes.restype = i64
    lib.vfm_foldin_solve_implicit_weights_f32.argtypes = [C.POINTER(ImplicitSolve), vp, vp, vp]
    lib.vfm_foldin_solve_implicit_weights_f32.restype = C.c_int
    lib.vfm_elicit_implicit_f32.argtypes = [C.POINTER(ElicitSolve), C.POINTER(ElicitImplicit), vp, vp]
    lib.vfm_elicit_implicit_f32.restype = C.c_int
    lib.vfm_elicit_implicit_workspace_bytes.argtypes = [i64, i64, i64, i32, i32]
    lib.vfm_elicit_implicit_workspace_bytes.restype = i64
    lib.vfm_elicit_bound_f32.argtypes = [C.POINTER(ElicitBound), vp]
    lib.vfm_elicit_bound_f32.restype = C.c_int
    lib.vfm_elicit_bound_workspace_bytes.argtypes = [i64, i64, i64, i64, i32, i32, i32]
    lib.vfm_elicit_bound_workspace_bytes.restype = i64
    for entry, struct, size, size_args in _ELICIT_PRIOR_PROTOTYPES:
        getattr(lib, entry).argtypes = [C.POINTER(struct), vp, vp]
        getattr(lib, entry).restype = C.c_int
        getattr(lib, size).argtypes = size_args
        getattr(lib, size).restype = i64
    u64 = C.c_uint64
    lib.vfm_field_moments_post_f32.argtypes = [i64, i32, i32, i64, i32, i32, vp, i32, i32, vp, vp, vp, vp, i32, u64,
                                               vp, vp, vp, vp, vp]
    lib.vfm_rank_field_post_f32.argtypes = ([i64, vp, i32, i32, vp, vp, i64, vp, i64, i64, i32, i32, i32, i32, i32, u64,
                                             i32, vp, vp, i64, vp, vp, vp, vp, i64] + [vp] * 5)
    lib.vfm_rank_heldout_field_post_f32.argtypes = ([i64, vp, i32, i32, vp, vp, i64, vp, i64, i64, i32, i32, i32, i32, u64,
                                                     i32, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, i64] + [vp] * 5)
    for name in RANK_POST_EXPORTS:
        getattr(lib, name).restype = C.c_int
    # problem, objective, index, workspace, x, values | entity, bias, inv_occ, scalars, W, priors | eps x3 | state, grow,
    # partials, grad_out | m / v of entity, bias, scalars, priors | lr, beta1, beta2, eps, adam_step, stream
    lib.vfm_variant_step_f32.argtypes = ([PP, i32, C.POINTER(Index)] + [vp] * 24 +
                                         [C.c_float, C.c_float, C.c_float, C.c_float, i64, vp])
    lib.vfm_variant_step_f32.restype = C.c_int
    lib.vfm_variant_step_workspace_bytes.argtypes = [i64, i32, i32]
    lib.vfm_variant_step_workspace_bytes.restype = i64
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name != "vfm_last_error":
            fn.restype = C.c_int
    for name in ("vfm_index_workspace_bytes", "vfm_union_workspace_bytes", "vfm_variant_workspace_elems"):
        getattr(lib, name).restype = i64
    if lib.vfm_abi_version() != ABI_VERSION:
        raise VfmLibraryError(f"ABI mismatch: library {lib.vfm_abi_version()}, package {ABI_VERSION}")
    _lib = lib
    return lib


_ops = None


def ops():
    """`torch.ops.vfm_hip` -- the TORCH_LIBRARY shim over the same C ABI (libvfm_torch_ops.so).
    The per-step calls (forward, finalize, backward, Adam) go through it."""
    global _ops
    if _ops is not None:
        return _ops
    load()
    if not os.path.exists(OPS_PATH):
        raise VfmLibraryError(f"{OPS_PATH} not found: run __graft_entry__.build()")
    torch.ops.load_library(OPS_PATH)
    if torch.ops.vfm_hip.abi_version() != ABI_VERSION:
        raise VfmLibraryError("ABI mismatch between libvfm_torch_ops.so and the package")
    _ops = torch.ops.vfm_hip
    return _ops


def check(rc, what):
    if rc != 0:
        msg = load().vfm_last_error().decode(errors="replace")
        raise VfmLibraryError(f"{what} failed (code {rc}): {msg}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def raw_stream(device) -> int:
    """The current HIP stream of `device` as an integer handle (torch.cuda.current_stream() builds a Python Stream object
    through three layers of device-index helpers: 4.5 us; a training step asked a dozen times)."""
    idx = device.index if getattr(device, "index", None) is not None else torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(idx)


def current_stream_ptr(device):
    return C.c_void_p(raw_stream(device))
