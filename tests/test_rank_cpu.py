"""CPU: the closed-form predictive moments of preference elicitation (include/vfm_rank.h) against a Monte-Carlo of the
posterior, the argument checks of the two C entry points, and the exclusion-list plumbing."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _link(s, link):
    return np.abs(s) if link == "abs" else np.logaddexp(0.0, s)


def closed_form(ent, bia, scal, x, link="abs"):
    """fp64 logit mean / variance of rows x [B, F] under the mean-field posterior (a_f ~ N(m_f, s_f^2) independent):
    E = m0 + sum_f mu_w,f + sum_k sum_{f<g} m_f m_g
    Var = s0^2 + sum_f s_w,f^2 + sum_k [sum_{f<g} s_f^2 s_g^2 + sum_f s_f^2 (sum_{g!=f} m_g)^2]."""
    ent, bia = np.asarray(ent, np.float64), np.asarray(bia, np.float64)
    d = ent.shape[1] // 2
    m0, s0 = float(scal[1]), float(_link(np.float64(scal[2]), link))
    e = ent[np.asarray(x)]                                   # [B, F, 2d]
    b = bia[np.asarray(x)]                                   # [B, F, 2]
    m, s2 = e[..., :d], _link(e[..., d:], link) ** 2
    sw2 = _link(b[..., 1], link) ** 2
    sm = m.sum(1)                                            # [B, d]
    mean = m0 + b[..., 0].sum(1) + 0.5 * (sm ** 2 - (m ** 2).sum(1)).sum(1)
    quad = 0.5 * (s2.sum(1) ** 2 - (s2 ** 2).sum(1)).sum(1)
    lin = (s2 * (sm[:, None, :] - m) ** 2).sum((1, 2))
    var = s0 ** 2 + sw2.sum(1) + quad + lin
    return mean, var


@pytest.mark.parametrize("F", [2, 4])
@pytest.mark.parametrize("link", ["abs", "softplus"])
def test_closed_form_matches_monte_carlo(F, link):
    rng = np.random.default_rng(7 + F)
    d, T, n = 3, 3 * F, 200_000
    ent = rng.normal(size=(T, 2 * d)) * 0.7
    bia = rng.normal(size=(T, 2)) * 0.5
    scal = np.array([0.5, 0.3, -0.4])
    x = np.arange(F)[None, :] * 3 + rng.integers(0, 3, size=(1, F))
    mean, var = closed_form(ent, bia, scal, x, link)
    e, b = ent[x[0]], bia[x[0]]
    z = e[None, :, :d] + _link(e[None, :, d:], link) * rng.normal(size=(n, F, d))
    w = b[None, :, 0] + _link(b[None, :, 1], link) * rng.normal(size=(n, F))
    w0 = scal[1] + _link(np.float64(scal[2]), link) * rng.normal(size=n)
    sz = z.sum(1)
    pred = w0 + w.sum(1) + 0.5 * ((sz ** 2).sum(1) - (z ** 2).sum((1, 2)))
    mc_m, mc_v = pred.mean(), pred.var(ddof=1)
    assert abs(mc_m - mean[0]) < 5 * math.sqrt(var[0] / n)
    m4 = ((pred - mc_m) ** 4).mean()
    assert abs(mc_v - var[0]) < 5 * math.sqrt((m4 - mc_v ** 2) / n)


def _lib():
    from vae_amd import _lib as L
    lib = L.load()
    i64, i32, vp = C.c_int64, C.c_int32, C.c_void_p
    lib.vfm_predictive_moments_f32.argtypes = [i64, i32, i32, i64, i32, i32, vp, vp, vp, vp, i32, C.c_uint64, vp, vp, vp, vp]
    lib.vfm_predictive_moments_f32.restype = C.c_int
    lib.vfm_rank_items_f32.argtypes = ([i64, vp, i64, vp, i64, i64, i32, i32, i32, i32, i32, C.c_uint64, i32, vp, vp, i64]
                                       + [vp] * 4 + [i64] + [vp] * 5)
    lib.vfm_rank_items_f32.restype = C.c_int
    lib.vfm_rank_workspace_bytes.argtypes = [i64, i64, i32, i32, i32, i32]
    lib.vfm_rank_workspace_bytes.restype = i64
    return lib


FAKE = C.c_void_p(4096)          # a non-NULL pointer the library must never dereference: every call below fails its checks


def _rank(lib, k=10, F=2, users=FAKE, ent=FAKE, out=FAKE, ws=FAKE, strategy=0, n_splits=0):
    return lib.vfm_rank_items_f32(8, users, 100, None, 10, 200, F, 16, k, strategy, 0, 0, n_splits, None, None, 0,
                                  ent, FAKE, FAKE, ws, 1 << 30, out, FAKE, FAKE, FAKE, None)


def test_rank_items_rejects_bad_arguments_without_a_gpu():
    from vae_amd._lib import load
    lib = _lib()
    E = -1
    assert _rank(lib, k=0) == E and b"k out of range" in load().vfm_last_error()
    assert _rank(lib, k=129) == E
    assert _rank(lib, F=3) == E and b"F == 2" in load().vfm_last_error()
    assert _rank(lib, users=None) == E and b"null" in load().vfm_last_error()
    assert _rank(lib, ent=None) == E
    assert _rank(lib, out=None) == E
    assert _rank(lib, ws=None) == E
    assert _rank(lib, strategy=4) == E
    assert _rank(lib, n_splits=65) == E
    assert lib.vfm_rank_workspace_bytes(8, 100, 16, 0, 0, 0) == E
    assert lib.vfm_rank_workspace_bytes(8, 100, 16, 129, 0, 0) == E
    assert lib.vfm_rank_workspace_bytes(8, 100, 16, 10, 0, 0) > 0
    # a workspace smaller than the library asks for
    assert lib.vfm_rank_items_f32(8, FAKE, 100, None, 10, 200, 2, 16, 10, 0, 0, 0, 0, None, None, 0, FAKE, FAKE, FAKE,
                                  FAKE, 16, FAKE, FAKE, FAKE, FAKE, None) == E
    assert b"workspace" in load().vfm_last_error()


def test_predictive_moments_rejects_bad_arguments_without_a_gpu():
    lib = _lib()

    def call(F=2, x=FAKE, out=FAKE, id_bits=64, strategy=0, B=4):
        return lib.vfm_predictive_moments_f32(B, F, 8, 100, id_bits, 0, x, FAKE, FAKE, FAKE, strategy, 0, out, FAKE,
                                              None, None)
    assert call(x=None) == -1
    assert call(out=None) == -1
    assert call(F=0) == -1 and call(F=65) == -1
    assert call(id_bits=16) == -1
    assert call(F=3, strategy=3) == -1            # the random score keys on (user, item): two fields
    assert call(strategy=7) == -1
    assert call(B=0, x=None) == 0                 # nothing to do: no launch


def test_cpu_model_rank_ops_fail_loudly():
    from vae_amd.model import VFM
    from vae_amd._lib import VfmLibraryError
    m = VFM(5, 5, 4, device="cpu")
    with pytest.raises(VfmLibraryError):
        m.rank_items([0, 1], k=2)
    with pytest.raises(VfmLibraryError):
        m.predictive_moments(torch.tensor([[0, 5]]))
    with pytest.raises(VfmLibraryError):
        m.select_next_questions(torch.tensor([[0, 5]]))


def test_exclusion_csr_groups_sorts_and_drops_duplicates():
    from vae_amd.rank import exclusion_csr
    users = torch.tensor([7, 2, 5])
    ex = torch.tensor([[2, 30], [7, 12], [2, 11], [9, 10], [2, 30], [7, 40], [2, 20]])
    ptr, items = exclusion_csr(users, ex, 50)
    assert ptr.tolist() == [0, 2, 5, 5]
    assert items.tolist() == [12, 40, 11, 20, 30]
