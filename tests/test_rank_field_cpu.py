"""CPU: the field form of the ranking (include/vfm_rank.h: vfm_field_moments_f32, vfm_rank_field_f32) -- its algebra
against a Monte-Carlo of the posterior, the argument checks of the three C entry points, the match_fields exclusion lists
and the Python argument errors."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from test_rank_cpu import _link, closed_form          # noqa: E402


def field_operands(ent, bia, scal, ctx, link="abs"):
    """fp64 operand decomposition of the contexts ctx [Q, F-1] (entity ids of the context columns):
    M, A, C [Q, d] and c_mean, c_var [Q], by the formulas of include/vfm_rank.h (two passes: C and Var P as written)."""
    ent, bia = np.asarray(ent, np.float64), np.asarray(bia, np.float64)
    d = ent.shape[1] // 2
    e, b = ent[ctx], bia[ctx]                                 # [Q, F-1, 2d], [Q, F-1, 2]
    mu, s2 = e[..., :d], _link(e[..., d:], link) ** 2
    M, A = mu.sum(1), s2.sum(1)
    Cq = 2 * (s2 * (M[:, None, :] - mu)).sum(1)
    EP = 0.5 * (M ** 2 - (mu ** 2).sum(1)).sum(1)
    VP = (0.5 * (A ** 2 - (s2 ** 2).sum(1)) + (s2 * (M[:, None, :] - mu) ** 2).sum(1)).sum(1)
    c_mean = float(scal[1]) + b[..., 0].sum(1) + EP
    c_var = float(_link(np.float64(scal[2]), link)) ** 2 + (_link(b[..., 1], link) ** 2).sum(1) + VP
    return M, A, Cq, c_mean, c_var


def field_form(ent, bia, scal, ctx, cand, link="abs"):
    """fp64 (mean, var, abs_mean, abs_var) [Q, C] of every (context, candidate) in the field form; abs_*: the sums of
    the absolute values of every term (products and constants) -- the scale of the fp32 rounding bound."""
    ent, bia = np.asarray(ent, np.float64), np.asarray(bia, np.float64)
    d = ent.shape[1] // 2
    M, A, Cq, c_mean, c_var = field_operands(ent, bia, scal, ctx, link)
    mu, s2 = ent[cand, :d], _link(ent[cand, d:], link) ** 2
    muw, sw2 = bia[cand, 0], _link(bia[cand, 1], link) ** 2
    mean = c_mean[:, None] + muw[None, :] + M @ mu.T
    var = c_var[:, None] + sw2[None, :] + A @ (mu ** 2).T + (A + M ** 2) @ s2.T + Cq @ mu.T
    abs_mean = np.abs(c_mean)[:, None] + np.abs(muw)[None, :] + np.abs(M) @ np.abs(mu).T
    abs_var = np.abs(c_var)[:, None] + sw2[None, :] + A @ (mu ** 2).T + (A + M ** 2) @ s2.T + np.abs(Cq) @ np.abs(mu).T
    return mean, var, abs_mean, abs_var


@pytest.mark.parametrize("link", ["abs", "softplus"])
@pytest.mark.parametrize("field", [0, 1, 2])
def test_field_form_matches_monte_carlo_and_the_general_closed_form(field, link):
    """F = 3, S = 200,000 posterior samples of pred: the sample mean and variance agree with the field form within 5
    standard errors of each estimator (computed from the samples); and the field form is the general closed form."""
    rng = np.random.default_rng(11 + field)
    F, d, n = 3, 4, 200_000
    T = 3 * F
    ent = rng.normal(size=(T, 2 * d)) * 0.7
    bia = rng.normal(size=(T, 2)) * 0.5
    scal = np.array([0.5, 0.3, -0.4])
    x = np.arange(F)[None, :] * 3 + rng.integers(0, 3, size=(1, F))
    ctx = np.delete(x, field, 1)
    mean, var, _, _ = field_form(ent, bia, scal, ctx, x[:, field], link)
    gm, gv = closed_form(ent, bia, scal, x, link)
    assert abs(mean[0, 0] - gm[0]) <= 1e-12 * (1 + abs(gm[0])) and abs(var[0, 0] - gv[0]) <= 1e-12 * (1 + gv[0])
    e, b = ent[x[0]], bia[x[0]]
    z = e[None, :, :d] + _link(e[None, :, d:], link) * rng.normal(size=(n, F, d))
    w = b[None, :, 0] + _link(b[None, :, 1], link) * rng.normal(size=(n, F))
    w0 = scal[1] + _link(np.float64(scal[2]), link) * rng.normal(size=n)
    sz = z.sum(1)
    pred = w0 + w.sum(1) + 0.5 * ((sz ** 2).sum(1) - (z ** 2).sum((1, 2)))
    mc_m, mc_v = pred.mean(), pred.var(ddof=1)
    assert abs(mc_m - mean[0, 0]) < 5 * math.sqrt(mc_v / n)
    m4 = ((pred - mc_m) ** 4).mean()
    assert abs(mc_v - var[0, 0]) < 5 * math.sqrt((m4 - mc_v ** 2) / n)


# ------------------------------------------------------------------------------------------------------- C ABI
def _lib():
    from vae_amd import _lib as L
    lib = L.load()
    i64, i32, vp, u64 = C.c_int64, C.c_int32, C.c_void_p, C.c_uint64
    lib.vfm_field_moments_f32.argtypes = [i64, i32, i32, i64, i32, i32, vp, i32, vp, vp, vp, i32, u64, vp, vp, vp, vp, vp]
    lib.vfm_field_moments_f32.restype = C.c_int
    lib.vfm_rank_field_workspace_bytes.argtypes = [i64, i64, i32, i32, i32, i32, i32]
    lib.vfm_rank_field_workspace_bytes.restype = i64
    lib.vfm_rank_field_f32.argtypes = ([i64, vp, i32, vp, i64, vp, i64, i64, i32, i32, i32, i32, i32, u64, i32, vp, vp, i64]
                                       + [vp] * 4 + [i64] + [vp] * 5)
    lib.vfm_rank_field_f32.restype = C.c_int
    return lib


FAKE = C.c_void_p(4096)          # a non-NULL pointer the library must never dereference: every call below fails its checks


def _rank(lib, F=3, field=1, k=10, ctx=FAKE, ent=FAKE, out=FAKE, ws=FAKE, ws_bytes=1 << 40, strategy=0, flags=0,
          n_splits=0, n_cand=100, cand_lo=10, d=16, n_excl=0):
    return lib.vfm_rank_field_f32(8, ctx, field, None, n_cand, None, cand_lo, 200, F, d, k, strategy, flags, 0, n_splits,
                                  None, None, n_excl, ent, FAKE, FAKE, ws, ws_bytes, out, FAKE, FAKE, FAKE, None)


def test_rank_field_rejects_bad_arguments_without_a_gpu():
    from vae_amd._lib import load
    lib = _lib()
    err = load().vfm_last_error
    E = -1
    assert _rank(lib, F=1) == E and b"F out of range" in err()
    assert _rank(lib, F=65) == E
    assert _rank(lib, field=-1) == E and b"field" in err()
    assert _rank(lib, field=3) == E
    assert _rank(lib, k=0) == E and b"k out of range" in err()
    assert _rank(lib, k=129) == E
    assert _rank(lib, strategy=4) == E and _rank(lib, strategy=-1) == E
    assert _rank(lib, flags=2) == E and b"flags" in err()
    assert _rank(lib, n_splits=65) == E and _rank(lib, n_splits=-1) == E
    assert _rank(lib, d=0) == E and _rank(lib, d=4097) == E
    assert _rank(lib, n_cand=-1) == E
    assert _rank(lib, cand_lo=150) == E and b"candidate range" in err()
    assert _rank(lib, n_excl=5) == E
    assert _rank(lib, ctx=None) == E and b"null" in err()
    assert _rank(lib, ent=None) == E and _rank(lib, out=None) == E and _rank(lib, ws=None) == E
    assert _rank(lib, ws_bytes=16) == E and b"workspace too small" in err()
    assert _rank(lib, ws=C.c_void_p(4097)) == E and b"aligned" in err()


def test_rank_field_workspace_bytes_checks_its_arguments():
    lib = _lib()
    wb = lib.vfm_rank_field_workspace_bytes
    for bad in ((-1, 100, 3, 16, 10, 0, 0), (8, -1, 3, 16, 10, 0, 0), (8, 1 << 31, 3, 16, 10, 0, 0),
                (8, 100, 1, 16, 10, 0, 0), (8, 100, 65, 16, 10, 0, 0), (8, 100, 3, 0, 10, 0, 0),
                (8, 100, 3, 4097, 10, 0, 0), (8, 100, 3, 16, 0, 0, 0), (8, 100, 3, 16, 129, 0, 0),
                (8, 100, 3, 16, 10, 4, 0), (8, 100, 3, 16, 10, 0, 65), (8, 100, 3, 16, 10, 0, -1)):
        assert wb(*bad) < 0, bad
    top = wb(8, 100, 3, 16, 10, 0, 0)
    assert top > 0 and top % 256 == 0
    # both operand parts are packed for every strategy (K = d + 3d, padded to 16 each); no candidate block for random
    assert wb(8, 100, 3, 16, 10, 1, 0) == top and wb(8, 100, 3, 16, 10, 2, 0) == top
    assert wb(8, 100, 3, 16, 10, 3, 0) < top
    assert top >= (256 + 128) * (16 + 48) * 4
    assert wb(8, 100, 3, 16, 10, 0, 64) > wb(8, 100, 3, 16, 10, 0, 1)


def test_field_moments_rejects_bad_arguments_without_a_gpu():
    lib = _lib()

    def call(F=3, field=1, x=FAKE, out=FAKE, id_bits=64, strategy=0, B=4, flags=0, d=8):
        return lib.vfm_field_moments_f32(B, F, d, 100, id_bits, flags, x, field, FAKE, FAKE, FAKE, strategy, 0, None, out,
                                         FAKE, None, None)
    assert call(x=None) == -1 and call(out=None) == -1
    assert call(F=1, field=0) == -1 and call(F=65) == -1
    assert call(field=3) == -1 and call(field=-1) == -1
    assert call(id_bits=16) == -1
    assert call(strategy=7) == -1 and call(flags=4) == -1 and call(d=0) == -1
    assert call(B=-1) == -1
    assert call(B=0, x=None) == 0                 # nothing to do: no launch


# ------------------------------------------------------------------------------------------------------- exclusions
@pytest.mark.parametrize("field,match", [(1, (0, 2)), (1, (0,)), (1, (2,)), (1, ()), (0, (1, 2)), (2, (0,))])
def test_match_fields_exclusion_csr_against_brute_force(field, match):
    from vae_amd.rank import field_exclusion_csr
    rng = np.random.default_rng(5 + field)
    sizes = [6, 9, 3]
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    T = int(sum(sizes))
    ex = (rng.integers(0, sizes, size=(400, 3)) + off).astype(np.int64)
    ctx = (rng.integers(0, sizes, size=(40, 3)) + off).astype(np.int64)
    ctx[:, field] = 0
    ctx = np.unique(ctx, axis=0)[rng.permutation(len(np.unique(ctx, axis=0)))]       # distinct, any order
    ptr, items = field_exclusion_csr(torch.tensor(ctx), torch.tensor(ex), field, list(match), T)
    ptr, items = ptr.tolist(), items.tolist()
    assert len(ptr) == len(ctx) + 1 and ptr[0] == 0 and ptr[-1] == len(items)
    for q, c in enumerate(ctx):
        want = sorted({int(r[field]) for r in ex if all(r[f] == c[f] for f in match)})
        assert items[ptr[q]:ptr[q + 1]] == want, (q, c)


def test_exclusion_csr_with_no_rows_and_with_no_matching_row():
    from vae_amd.rank import field_exclusion_csr
    ctx = torch.tensor([[0, 0, 7], [1, 0, 8]])
    ptr, items = field_exclusion_csr(ctx, torch.zeros(0, 3, dtype=torch.int64), 1, [0, 2], 10)
    assert ptr.tolist() == [0, 0, 0] and items.numel() == 0
    ptr, items = field_exclusion_csr(ctx, torch.tensor([[1, 4, 7], [0, 5, 8], [1, 3, 8]]), 1, [0, 2], 10)
    assert ptr.tolist() == [0, 0, 1] and items.tolist() == [3]


# ------------------------------------------------------------------------------------------------------- Python
def test_rank_field_argument_errors_need_no_gpu():
    from vae_amd.model import VFM
    from vae_amd._lib import VfmLibraryError
    m = VFM(field_sizes=[5, 6, 3], embedding_size=4, device="cpu")            # ids: [0,5) [5,11) [11,14)
    ctx = torch.tensor([[0, 0, 11], [1, 0, 12]])
    for kw in (dict(field=3), dict(field=-1), dict(field=True), dict(field=1, k=0), dict(field=1, k=129),
               dict(field=1, strategy="best"), dict(field=1, strategy="mean"), dict(field=1, n_splits=65),
               dict(field=1, candidates=[4]), dict(field=1, candidates=[11]), dict(field=1, candidates=[5, 5]),
               dict(field=1, key_field=1), dict(field=1, key_field=3), dict(field=1, match_fields=(1,)),
               dict(field=1, match_fields=(0, 5)), dict(field=1, exclude=torch.tensor([[0, 5]])),
               dict(field=1, exclude=torch.tensor([[0, 0, 11]])), dict(field=1, exclude=torch.tensor([[5, 5, 11]])),
               dict(field=1, exclude=torch.tensor([[0, 5, 14]]))):
        with pytest.raises(ValueError):
            m.rank_field(ctx, **kw)
    for bad in (torch.tensor([[0, 0]]), torch.tensor([[5, 0, 11]]), torch.tensor([[0, 0, 6]]), torch.tensor([[0, 0, 14]]),
                torch.tensor([[-1, 0, 11]]), torch.tensor([[0.5, 0, 11]])):
        with pytest.raises(ValueError):
            m.rank_field(bad, field=1)
    with pytest.raises(ValueError):
        m.field_moments(torch.tensor([[0, 5]]), field=1)
    with pytest.raises(ValueError):
        m.field_moments(torch.tensor([[0, 5, 11]]), field=1, strategy="mean")
    with pytest.raises(ValueError):
        VFM(field_sizes=[5], embedding_size=4, device="cpu").rank_field(torch.tensor([[0]]), field=0)
    # valid arguments on a CPU model: no fallback, a loud error
    with pytest.raises(VfmLibraryError):
        m.rank_field(ctx, field=1, k=2, exclude=torch.tensor([[0, 5, 11]]), match_fields=(0,))
    with pytest.raises(VfmLibraryError):
        m.field_moments(torch.tensor([[0, 5, 11]]), field=1)

