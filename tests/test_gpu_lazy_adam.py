"""GPU: lazy EXACT dense Adam (vfm_adam_catchup_f32 + the touched-rows fused step) against the dense fused step:
the trajectory must be the dense one BIT FOR BIT -- parameters, moments, losses -- over several moment periods,
with changing learning rates, predictions in the middle, checkpoints, and a mode switch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _setup(lazy, n_samples=1, F=3, d=16, T_sizes=(900, 700, 400), B=48, nb=12):
    from vae_amd.model import VFM
    from vae_amd.data import synthetic_triples
    torch.manual_seed(3)
    m = VFM(field_sizes=list(T_sizes)[:F], embedding_size=d, device="cuda", rng_seed=11, n_samples=n_samples)
    m.lazy_adam = lazy
    m.pipeline = False
    X, y = synthetic_triples(list(T_sizes)[:F], nb * B, seed=4, device="cuda")
    m.set_training_data(X, nb_train=nb * B)
    plans = [m.plan(X[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) for i in range(nb)]
    return m, plans, X


# d = 300 / 512: k_bwd <64, 2, 4> with 75 of 128 chunks filled / full (vfm_abi.hip pick_shape)
@pytest.mark.parametrize("F,d", [(3, 16), (2, 128), (2, 5), (2, 300), (2, 512)])
def test_lazy_adam_is_bitwise_the_dense_trajectory(F, d):
    dense, plans_d, X = _setup(False, F=F, d=d)
    lazy, plans_l, _ = _setup(True, F=F, d=d)
    assert plans_l[0].touched_ids().numel() < 0.2 * lazy.T          # a sparse-touch regime
    n_steps = 300                                                     # > 2 moment periods of 128 steps
    for s in range(n_steps):
        lr = 0.05 if s % 7 else 0.02                                  # the learning rate may change from step to step
        ld, _ = dense.train_step(plans_d[s % len(plans_d)], lr=lr)
        ll, _ = lazy.train_step(plans_l[s % len(plans_l)], lr=lr)
        if s % 50 == 17:
            assert torch.equal(ld, ll), s                             # losses see only up-to-date rows
        if s == 140:                                                  # predictions in the middle of a period
            pd_, pl_ = dense.predict(X[:200]), lazy.predict(X[:200])
            assert torch.equal(pd_["y_pred"], pl_["y_pred"])
    assert lazy._lazy_dirty                                           # rows are lagging right now ...
    lazy.sync_lazy()                                                  # ... until they are replayed
    assert torch.equal(dense._flat, lazy._flat)
    assert torch.equal(dense._adam_m, lazy._adam_m) and torch.equal(dense._adam_v, lazy._adam_v)
    assert dense._adam_t == lazy._adam_t == n_steps


def test_lazy_adam_checkpoint_mode_switch_and_auto():
    dense, plans_d, X = _setup(False)
    lazy, plans_l, _ = _setup("auto")
    lazy.lazy_threshold, lazy.lazy_min_params = 0.5, 0
    for s in range(40):
        dense.train_step(plans_d[s % 12], lr=0.03)
        lazy.train_step(plans_l[s % 12], lr=0.03)
    assert lazy._lazy_last is not None                                # "auto" chose the lazy step here
    sd = lazy.training_state_dict()                                   # (replays the lagging rows first)
    assert np.array_equal(sd["model"]["entity_params.weight"].numpy(), dense.entity_params.weight.detach().cpu().numpy())
    lazy.lazy_adam = False                                            # dense steps after lazy ones
    for s in range(40, 60):
        dense.train_step(plans_d[s % 12], lr=0.03)
        lazy.train_step(plans_l[s % 12], lr=0.03)
    assert not lazy._lazy_dirty and torch.equal(dense._flat, lazy._flat)
    lazy.lazy_adam = True                                             # and back
    for s in range(60, 150):
        dense.train_step(plans_d[s % 12], lr=0.03)
        lazy.train_step(plans_l[s % 12], lr=0.03, fused=(s % 10 != 3))      # an unfused step in between
    # the dense run took fused steps throughout; the unfused steps use the plain-moment Adam kernel (IEEE sqrt / div,
    # not bitwise the scaled form), so this part is compared with a tolerance -- the bitwise claim is for the
    # fused step (test above).  What it checks: no step is replayed twice or dropped across the switches.
    lazy.sync_lazy()
    rel = (dense._flat - lazy._flat).abs().max() / dense._flat.abs().max()
    assert rel < 1e-3
    # resume from the checkpoint taken at step 40 reproduces the dense run from there
    fresh, plans_f, _ = _setup(True)
    fresh.load_training_state_dict(sd)
    ref, plans_r, _ = _setup(False)
    ref.load_training_state_dict(sd)
    for s in range(40, 80):
        ref.train_step(plans_r[s % 12], lr=0.03)
        fresh.train_step(plans_f[s % 12], lr=0.03)
    fresh.sync_lazy()
    assert torch.equal(ref._flat, fresh._flat)


def test_catchup_argument_checks():
    import ctypes as C
    from vae_amd import _lib
    lib = _lib.load()
    lr = (C.c_float * 1)(0.1)
    assert lib.vfm_adam_catchup_f32(None, None, None, None, None, None, None, None, 0, 10, 8, lr, 1, 0.9, 0.999, 1e-8, 1, 1, None, None) == -1


@pytest.mark.parametrize("listed", [True, False])
# d = 300 / 512: k_bwd <64, 2, 4> with 75 of 128 chunks filled / full (vfm_abi.hip pick_shape)
@pytest.mark.parametrize("B,F,d", [(48, 3, 16), (700, 2, 128), (48, 2, 5), (700, 2, 300), (700, 2, 512)])
def test_lookahead_lazy_adam_is_bitwise_the_dense_trajectory(B, F, d, listed):
    """The look-ahead form (train_step(plan, next_plan=...): the fused step visits only the rows of this batch and of
    the next) against the dense fused step: bitwise over 300 steps with changing learning rates, an un-announced
    batch in between (its rows are caught up by the separate pass), predictions, and two moment-period boundaries."""
    dense, plans_d, X = _setup(False, F=F, d=d, B=B)
    la, plans_l, _ = _setup(False, F=F, d=d, B=B)
    dense.lookahead = False
    dense.pipeline = la.pipeline = False
    la.lookahead_list = listed                            # rows as a list per pair of plans / classified by the kernel
    n = len(plans_l)
    f = plans_l[0].U / la.T
    assert (1 - f) ** 2 >= la.lookahead_min_skip
    order = list(range(300))
    order[100] = 7                                        # step 100 does not take the batch step 99 announced
    for s in range(300):
        lr = 0.05 if s % 7 else 0.02
        i, j = order[s] % n, order[s + 1] % n if s + 1 < 300 else 0
        ld, _ = dense.train_step(plans_d[i], lr=lr)
        ll, _ = la.train_step(plans_l[i], lr=lr, next_plan=plans_l[j])
        assert la._lazy_kind in ("la", None)
        if s % 50 == 17:
            assert torch.equal(ld, ll), s
        if s == 140:
            assert torch.equal(dense.predict(X[:200])["y_pred"], la.predict(X[:200])["y_pred"])
    assert la._lazy_dirty
    la.sync_lazy()
    assert torch.equal(dense._flat, la._flat)
    assert torch.equal(dense._adam_m, la._adam_m) and torch.equal(dense._adam_v, la._adam_v)


@pytest.mark.parametrize("form", ["lookahead_list", "lookahead_scan", "lazy_list"])
def test_lazy_forms_with_heavy_lists_are_bitwise_the_dense_trajectory(form):
    """The same on a batch shape with LONG occurrence lists (40 items in 600 rows: every item's list is cut in work
    items and pre-reduced by k_heavy; short ones are summed inside k_bwd, long ones by k_heavy_sum) next to a sparse
    user column: the heavy path and the lazy forms together, bit for bit the dense trajectory over 150 steps."""
    sizes, B, nb = (3000, 40), 600, 6
    dense, plans_d, X = _setup(False, F=2, d=32, T_sizes=sizes, B=B, nb=nb)
    lz, plans_l, _ = _setup(form == "lazy_list", F=2, d=32, T_sizes=sizes, B=B, nb=nb)
    dense.lookahead = False
    lz.lookahead = form != "lazy_list"
    lz.lookahead_list = form == "lookahead_list"
    assert plans_l[0].heavy is not None and plans_l[0].U < 0.4 * lz.T
    for s in range(150):
        lr = 0.05 if s % 5 else 0.03
        ld, _ = dense.train_step(plans_d[s % nb], lr=lr)
        ll, _ = lz.train_step(plans_l[s % nb], lr=lr, next_plan=plans_l[(s + 1) % nb])
        if s % 40 == 7:
            assert torch.equal(ld, ll), s
    assert lz._lazy_dirty and lz._lazy_kind == ("list" if form == "lazy_list" else "la")
    lz.sync_lazy()
    assert torch.equal(dense._flat, lz._flat)
    assert torch.equal(dense._adam_m, lz._adam_m) and torch.equal(dense._adam_v, lz._adam_v)


# ---- hand-placed lists: what the sparse synthetic batches above do not hold at d = 128
SIZES = (200, 100)          # T = 300 table rows: users 0..199, items 200..299
B, NB, STEPS = 400, 6, 140  # six batches in turn; 140 steps cross the moment-period boundary at step 128
ONCE, TWICE, RARE = 0, 1, 2            # users: a list of length 1, of length 2 (batch 1); in batch 0 only (replay gap 4)
HEAVY, HEAVIER = 200, 201              # items of batch 1: 12 rows (2 work items of 8), 80 rows (10 > VFM_HEAVY_DIRECT)
HEAVY_MIN, HEAVY_DIRECT = 8, 8         # include/vfm_hip.h; a table this small cuts its lists in work items of 8


def _batches(device):
    """Six batches of B rows over T = 300.  Batch b draws from the 60 % of the users and of the items with (id + b) % 5 >= 2,
    so a step has rows in both batches, rows in the next batch only and rows in neither; the special ids are placed by hand."""
    g = torch.Generator().manual_seed(33)
    special_u, special_i = (ONCE, TWICE, RARE), (HEAVY, HEAVIER)
    xs = []
    for b in range(NB):
        users = torch.tensor([u for u in range(SIZES[0]) if (u + b) % 5 >= 2 and u not in special_u])
        items = torch.tensor([i for i in range(SIZES[0], sum(SIZES)) if (i + b) % 5 >= 2 and i not in special_i])
        x = torch.stack([users[torch.randint(0, len(users), (B,), generator=g)],
                         items[torch.randint(0, len(items), (B,), generator=g)]], 1)
        if b == 0:
            x[7, 0] = RARE
            x[250, 0] = RARE
        if b == 1:
            x[5, 0] = ONCE
            x[40, 0] = TWICE
            x[399, 0] = TWICE
            x[100:112, 1] = HEAVY
            x[200:280, 1] = HEAVIER
        xs.append(x)
    X = torch.cat(xs).to(device)
    y = torch.randint(1, 6, (NB * B,), generator=g).to(torch.float32).to(device)
    return X, y


def _check_shape_of_data(X):
    """What the cases are there for, checked on the data itself."""
    T = sum(SIZES)
    cnt = [torch.bincount(X[b * B:(b + 1) * B].reshape(-1), minlength=T) for b in range(NB)]
    assert cnt[1][ONCE] == 1 and cnt[1][TWICE] == 2
    assert HEAVY_MIN < cnt[1][HEAVY] <= HEAVY_MIN * HEAVY_DIRECT and cnt[1][HEAVIER] > HEAVY_MIN * HEAVY_DIRECT
    assert cnt[0][RARE] > 0 and all(cnt[b][RARE] == 0 for b in range(1, NB))      # replays NB - 2 = 4 steps when batch 0 is next
    for b in range(NB):
        cur, nxt = cnt[b] > 0, cnt[(b + 1) % NB] > 0
        assert (cur & nxt).any() and (cur & ~nxt).any() and (~cur & nxt).any() and (~cur & ~nxt).any()


def _run_placed(X, y, attrs):
    from vae_amd.model import VFM
    torch.manual_seed(4)
    m = VFM(field_sizes=list(SIZES), embedding_size=128, device="cuda", rng_seed=6)
    m.pipeline = False
    for k_, v_ in attrs.items():
        setattr(m, k_, v_)
    m.set_training_data(X, nb_train=NB * B)
    plans = [m.plan(X[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) for i in range(NB)]
    losses = []
    for s in range(STEPS):
        nxt = {"next_plan": plans[(s + 1) % NB]} if m.lookahead else {}
        losses.append(m.train_step(plans[s % NB], lr=0.03 if s % 5 else 0.01, **nxt)[0].clone())
    for pl in plans:
        pl.check_status()
    if m.lookahead:
        assert m._lazy_dirty and (m._lazy_last < STEPS - 2).any()      # rows do lag at the end: the look-ahead form ran
        m.sync_lazy()
    out = {"loss": torch.stack(losses), "flat": m._flat.clone(), "m": m._adam_m.clone(), "v": m._adam_v.clone()}
    assert not torch.isnan(out["flat"]).any()
    return out


@pytest.mark.parametrize("listed", [True, False], ids=["listed", "scan"])
def test_lookahead_on_hand_placed_lists_is_bitwise_the_dense_trajectory(listed, monkeypatch):
    """d = 128, T = 300 under B = 400: losses, parameters and both moments BIT FOR BIT over 140 steps, the look-ahead step
    against the dense one on the same plans -- lists of length 1 and 2, a pre-reduced list added in the kernel and one added
    by k_heavy_sum, rows in both batches / the next only / neither, a row that replays four steps."""
    monkeypatch.setenv("VFM_BWD_SMALL", "0")      # the period-end / dense steps of this small table through k_bwd as well
    X, y = _batches("cuda")
    _check_shape_of_data(X)
    la = _run_placed(X, y, dict(lookahead=True, lookahead_list=listed))
    dense = _run_placed(X, y, dict(lookahead=False))
    for k_ in dense:
        assert torch.equal(la[k_], dense[k_]), k_
