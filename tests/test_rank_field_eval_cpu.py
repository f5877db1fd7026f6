"""CPU: the field form of the held-out ranking evaluation -- the positives' grouping (vae_amd.rank.field_positive_csr)
against a brute-force dict grouping, the argument checks of the two C entry points (include/vfm_rank.h:
vfm_rank_heldout_field_f32, vfm_rank_eval_field_workspace_bytes) with pointers that are never dereferenced, and the
Python argument errors of VFM.rank_heldout_field / VFM.evaluate_ranking_field."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


# ---------------------------------------------------------------------------------------------------- field_positive_csr
def _brute_groups(rows, field):
    groups = {}
    for r in rows.tolist():
        c = list(r)
        item, c[field] = c[field], 0
        groups.setdefault(tuple(c), set()).add(item)
    ctxs = sorted(groups)                                  # (torch.unique(dim=0): rows in lexicographic order)
    ptr, items = [0], []
    for c in ctxs:
        items += sorted(groups[c])
        ptr.append(len(items))
    return np.array(ctxs, np.int64).reshape(len(ctxs), rows.shape[1]), np.array(ptr, np.int64), np.array(items, np.int64)


@pytest.mark.parametrize("F", [3, 5])
def test_field_positive_csr_matches_a_dict_grouping(F):
    from vae_amd.rank import field_positive_csr
    rng = np.random.default_rng(F)
    sizes = [7] * F
    for field in range(F):
        sz = list(sizes)
        sz[field] = 40
        off = np.concatenate([[0], np.cumsum(sz)])
        T = int(off[-1])
        ctx = rng.integers(0, np.array(sz)[None, :], size=(12, F)) + off[None, :-1]       # few contexts: many repeats
        rows = ctx[rng.integers(0, 12, 300)]
        rows[:, field] = off[field] + rng.integers(0, 40, 300)
        rows = np.concatenate([rows, rows[:25]])                                          # duplicate rows
        rows = rows[rng.permutation(len(rows))].astype(np.int64)                          # contexts in scrambled order
        uq, ptr, items = field_positive_csr(torch.tensor(rows), field, T)
        wc, wp, wi = _brute_groups(rows, field)
        assert uq.dtype == ptr.dtype == items.dtype == torch.int64
        np.testing.assert_array_equal(uq.numpy(), wc)
        np.testing.assert_array_equal(ptr.numpy(), wp)
        np.testing.assert_array_equal(items.numpy(), wi)
        assert (uq[:, field] == 0).all() and items.numel() < len(rows)
        # the same context given with different values in the ignored column is one query
        one = np.repeat(rows[:1], 3, 0)
        one[:, field] = off[field] + np.array([5, 2, 5])
        uq, ptr, items = field_positive_csr(torch.tensor(one), field, T)
        assert uq.shape == (1, F) and ptr.tolist() == [0, 2] and items.tolist() == [off[field] + 2, off[field] + 5]
        uq, ptr, items = field_positive_csr(torch.zeros(0, F, dtype=torch.int64), field, T)
        assert uq.shape == (0, F) and ptr.tolist() == [0] and items.numel() == 0


# ---------------------------------------------------------------------------------------------------- the C entries
def _lib():
    from vae_amd import _lib as L
    lib = L.load()
    i64, i32, vp = C.c_int64, C.c_int32, C.c_void_p
    lib.vfm_rank_heldout_field_f32.argtypes = ([i64, vp, i32, vp, i64, vp, i64, i64, i32, i32, i32, i32, C.c_uint64, i32,
                                                vp, vp, i64, vp, vp, i64] + [vp] * 4 + [i64] + [vp] * 5)
    lib.vfm_rank_heldout_field_f32.restype = C.c_int
    lib.vfm_rank_eval_field_workspace_bytes.argtypes = [i64, i64, i64, i32, i32, i32, i32]
    lib.vfm_rank_eval_field_workspace_bytes.restype = i64
    return lib


FAKE = C.c_void_p(4096)          # a non-NULL pointer the library must never dereference: every call below fails its checks


def _heldout(lib, Q=8, ctx=FAKE, field=1, qkey=None, n_cand=100, cand=None, cand_lo=10, T=200, F=3, d=16, strategy=0,
             flags=0, n_splits=0, excl_ptr=None, excl_items=None, n_excl=0, pos_ptr=FAKE, pos_items=FAKE, n_pos=20,
             ent=FAKE, bias=FAKE, scal=FAKE, ws=FAKE, ws_bytes=1 << 30, rank=FAKE, rank_neg=FAKE, n_el=FAKE, n_neg=FAKE):
    return lib.vfm_rank_heldout_field_f32(Q, ctx, field, qkey, n_cand, cand, cand_lo, T, F, d, strategy, flags, 0,
                                          n_splits, excl_ptr, excl_items, n_excl, pos_ptr, pos_items, n_pos, ent, bias,
                                          scal, ws, ws_bytes, rank, rank_neg, n_el, n_neg, None)


def test_rank_heldout_field_rejects_bad_arguments_without_a_gpu():
    from vae_amd._lib import load
    lib = _lib()
    E = -1
    err = load().vfm_last_error
    assert _heldout(lib, F=1) == E and b"F out of range" in err()
    assert _heldout(lib, F=65) == E and b"F out of range" in err()
    assert _heldout(lib, field=-1) == E and b"field out of range" in err()
    assert _heldout(lib, field=3) == E and b"field out of range" in err()
    for name in ("ctx", "pos_ptr", "ent", "bias", "scal", "ws", "rank", "rank_neg", "n_el", "n_neg"):
        assert _heldout(lib, **{name: None}) == E and b"null" in err(), name
    assert _heldout(lib, pos_items=None) == E and b"pos_items" in err()
    assert _heldout(lib, excl_ptr=FAKE, excl_items=None, n_excl=5) == E and b"exclusion" in err()
    assert _heldout(lib, excl_ptr=None, excl_items=FAKE, n_excl=5) == E and b"exclusion" in err()
    assert _heldout(lib, strategy=4) == E and b"strategy" in err()
    assert _heldout(lib, n_splits=-1) == E and _heldout(lib, n_splits=65) == E and b"n_splits" in err()
    assert _heldout(lib, n_pos=-1) == E and b"n_pos" in err()
    assert _heldout(lib, n_cand=1 << 31) == E and b"n_cand" in err()
    assert _heldout(lib, cand_lo=150) == E and b"candidate range" in err()
    assert _heldout(lib, cand_lo=-1) == E and b"candidate range" in err()
    assert _heldout(lib, d=0) == E and _heldout(lib, flags=8) == E and _heldout(lib, Q=-1) == E
    assert _heldout(lib, ws_bytes=16) == E and b"workspace too small" in err()
    assert _heldout(lib, ws=C.c_void_p(4096 + 8)) == E and b"aligned" in err()
    # the two-field entry keeps its refusal
    lib.vfm_rank_heldout_f32.argtypes = ([C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64]
                                         + [C.c_int32] * 4 + [C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                                              C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4
                                         + [C.c_int64] + [C.c_void_p] * 5)
    assert lib.vfm_rank_heldout_f32(8, FAKE, 100, None, 10, 200, 3, 16, 0, 0, 0, 0, None, None, 0, FAKE, FAKE, 20, FAKE,
                                    FAKE, FAKE, FAKE, 1 << 30, FAKE, FAKE, FAKE, FAKE, None) == E and b"F == 2" in err()


def test_rank_heldout_field_with_no_query_launches_nothing():
    lib = _lib()
    # every pointer NULL: Q == 0 returns before anything is read or launched (no GPU on this path)
    assert _heldout(lib, Q=0, ctx=None, pos_ptr=None, pos_items=None, n_pos=0, ent=None, bias=None, scal=None, ws=None,
                    ws_bytes=0, rank=None, rank_neg=None, n_el=None, n_neg=None) == 0


def test_rank_eval_field_workspace_bytes():
    lib = _lib()
    E = -1
    w = lib.vfm_rank_eval_field_workspace_bytes
    assert w(8, 100, 20, 3, 16, 0, 0) > 0
    assert w(0, 0, 0, 2, 1, 3, 0) >= 0
    for bad in ((-1, 100, 20, 3, 16, 0, 0), (8, -1, 20, 3, 16, 0, 0), (8, 1 << 31, 20, 3, 16, 0, 0),
                (8, 100, -1, 3, 16, 0, 0), (8, 100, 20, 1, 16, 0, 0), (8, 100, 20, 65, 16, 0, 0),
                (8, 100, 20, 3, 0, 0, 0), (8, 100, 20, 3, 4097, 0, 0), (8, 100, 20, 3, 16, 4, 0),
                (8, 100, 20, 3, 16, -1, 0), (8, 100, 20, 3, 16, 0, -1), (8, 100, 20, 3, 16, 0, 65)):
        assert w(*bad) == E, bad
    # the field operands plus O(S (Q + n_pos)): the split count and the positives grow it, never Q x n_cand
    w1 = w(8192, 26744, 115_000, 3, 128, 0, 1)
    w8 = w(8192, 26744, 115_000, 3, 128, 0, 8)
    wp = w(8192, 26744, 230_000, 3, 128, 0, 1)
    assert 0 < w1 < w8 and w1 < wp
    assert w8 < 8192 * 26744 * 4 // 8 and wp < 8192 * 26744 * 4 // 8
    # the entry accepts exactly that size: one byte less is refused, before any pointer is read
    need = w(8, 100, 20, 3, 16, 0, 0)
    assert _heldout(lib, ws_bytes=need - 1) == E


# ---------------------------------------------------------------------------------------------------- Python arguments
def _cpu_model(output="reg"):
    from vae_amd.model import VFM
    return VFM(field_sizes=[5, 6, 3], embedding_size=4, output=output, device="cpu")      # ranges [0,5) [5,11) [11,14)


def test_python_argument_errors_need_no_gpu():
    m = _cpu_model()
    good = torch.tensor([[0, 5, 11], [1, 6, 12]])
    y = torch.tensor([5.0, 5.0])

    def both(match, pos=good, **kw):
        with pytest.raises(ValueError, match=match):
            m.rank_heldout_field(pos, 1, **kw)
        kw.pop("strategy", None), kw.pop("key_field", None)
        if kw or pos is not good:
            with pytest.raises(ValueError, match=match):
                m.evaluate_ranking_field(pos, y[:len(pos)], 1, **kw)

    both("ranked field's range", pos=torch.tensor([[5, 5, 11], [1, 6, 12]]))       # a context id that is a candidate id
    both("column 1 must lie", pos=torch.tensor([[0, 4, 11], [1, 6, 12]]))          # column `field` outside its range
    both("column 1 must lie", pos=torch.tensor([[0, 11, 11], [1, 6, 12]]))
    both("context ids must lie", pos=torch.tensor([[0, 5, 14], [1, 6, 12]]))
    both(r"must be \[R, 3\]|must be \[B, 3\]", pos=torch.tensor([[0, 5], [1, 6]]))
    both("match_fields", match_fields=(1,))
    both("match_fields", match_fields=(0, 3))
    both("ineligible", ineligible="skip")
    both("exclude", exclude=torch.tensor([[0, 4, 11]]))
    both("candidate ids", candidates=[4, 5])
    both("duplicate candidates", candidates=[5, 5])
    for bad_key in (1, 3, True):
        with pytest.raises(ValueError, match="key_field"):
            m.rank_heldout_field(good, 1, key_field=bad_key)
    with pytest.raises(ValueError, match="'mean'"):
        m.rank_heldout_field(good, 1, strategy="mean")                               # 'mean' needs a 'class' model
    with pytest.raises(ValueError, match="strategy must be"):
        m.rank_heldout_field(good, 1, strategy="best")
    for n_splits in (-1, 65):
        with pytest.raises(ValueError, match="n_splits"):
            m.rank_heldout_field(good, 1, n_splits=n_splits)
    for field in (-1, 3, True, 1.0):
        with pytest.raises(ValueError, match="field must be"):
            m.rank_heldout_field(good, field)
        with pytest.raises(ValueError, match="field must be"):
            m.evaluate_ranking_field(good, y, field)
    for ks in ((0,), (10, -1), ()):
        with pytest.raises(ValueError, match="ks"):
            m.evaluate_ranking_field(good, y, 1, ks=ks)
    with pytest.raises(ValueError, match="one y_test value per row"):
        m.evaluate_ranking_field(good, y[:1], 1)


def test_cpu_model_field_eval_fails_loudly():
    from vae_amd._lib import VfmLibraryError
    for output in ("reg", "class"):
        m = _cpu_model(output)
        with pytest.raises(VfmLibraryError):
            m.rank_heldout_field(torch.tensor([[0, 5, 11]]), 1)
        with pytest.raises(VfmLibraryError):
            m.evaluate_ranking_field(torch.tensor([[0, 5, 11], [1, 6, 12]]), torch.tensor([5.0, 1.0]), 1)
    # the two-field methods are unchanged: rank_heldout checks the device first, evaluate_ranking refuses F != 2 first
    with pytest.raises(VfmLibraryError):
        _cpu_model().rank_heldout(torch.tensor([[0, 5]]))
    with pytest.raises(ValueError, match="two-field"):
        _cpu_model().evaluate_ranking(torch.tensor([[0, 5]]), torch.tensor([5.0]))
