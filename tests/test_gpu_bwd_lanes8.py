"""k_bwd<16, 2, 4, ..., ADJ> (VFM_BWD_LANES8=1 at d = 128: a lane owns 8 adjacent coordinates and makes one Philox call,
four table rows per wave) against the 32-lane shape of the table: the same step bit for bit.  At every other d the switch
leaves the shape where it was."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

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


def _run(d, sizes, X, y, lanes8, attrs, monkeypatch, steps=STEPS):
    from vae_amd.model import VFM
    monkeypatch.setenv("VFM_BWD_LANES8", lanes8)
    monkeypatch.setenv("VFM_BWD_SMALL", "0")      # the period-end / dense steps of these small tables through k_bwd as well
    torch.manual_seed(4)
    m = VFM(field_sizes=list(sizes), embedding_size=d, device="cuda", rng_seed=6)
    m.pipeline = False
    for k_, v_ in attrs.items():
        setattr(m, k_, v_)
    nb = X.shape[0] // B
    m.set_training_data(X, nb_train=nb * B)
    plans = [m.plan(X[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) for i in range(nb)]
    losses = []
    for s in range(steps):
        nxt = {"next_plan": plans[(s + 1) % nb]} if m.lookahead else {}
        losses.append(m.train_step(plans[s % nb], lr=0.03 if s % 5 else 0.01, **nxt)[0].clone())
    for pl in plans:
        pl.check_status()
    out = {"loss": torch.stack(losses)}
    if m.lookahead:      # the lagging state first: which step every row is at, and the rows as they are
        assert m._lazy_dirty
        out.update(last_step=m._lazy_last.clone(), flat_lag=m._flat.clone(), m_lag=m._adam_m.clone(), v_lag=m._adam_v.clone())
        m.sync_lazy()
    out.update(flat=m._flat.clone(), m=m._adam_m.clone(), v=m._adam_v.clone())
    assert not torch.isnan(out["flat"]).any()
    return out


def _assert_bitwise(a, b):
    assert a.keys() == b.keys()
    for k_ in a:
        assert torch.equal(a[k_], b[k_]), k_


@pytest.mark.parametrize("attrs", [
    dict(lookahead=True, lookahead_list=True),      # the rows of the two batches as a list
    dict(lookahead=True, lookahead_list=False),     # the kernel classifies all T rows: skipped rows
    dict(lookahead=False),                          # the dense fused step, every row every step
], ids=["listed", "scan", "dense"])
def test_lanes8_is_bitwise_the_table_shape_at_d128(attrs, monkeypatch):
    """Losses, parameters, both moments and last_step BIT FOR BIT over 140 steps, switch on against off: lists of length
    1 and 2, a pre-reduced list added in the kernel and one added by k_heavy_sum, rows in both batches / the next only /
    neither, a row that replays four steps."""
    X, y = _batches("cuda")
    _check_shape_of_data(X)
    on = _run(128, SIZES, X, y, "1", attrs, monkeypatch)
    off = _run(128, SIZES, X, y, "0", attrs, monkeypatch)
    if attrs["lookahead"]:
        assert (on["last_step"] < STEPS - 2).any()      # rows do lag at the end: the look-ahead form ran
    _assert_bitwise(on, off)


@pytest.mark.parametrize("d", [24, 136])
def test_switch_leaves_other_sizes_alone(d, monkeypatch):
    """d = 24 (8 lanes per row) and d = 136 (64 lanes, past the 32-lane bucket): bitwise the step without the switch."""
    X, y = _batches("cuda")
    attrs = dict(lookahead=True, lookahead_list=True)
    _assert_bitwise(_run(d, SIZES, X, y, "1", attrs, monkeypatch), _run(d, SIZES, X, y, "0", attrs, monkeypatch))


_K_BWD = re.compile(r"k_bwd(?:<|ILi)(\d+)(?:, |ELi)(\d+)(?:, |ELi)(\d+)")


@pytest.mark.parametrize("d,lanes8,shape", [(128, "1", (16, 2, 4)), (128, "0", (32, 1, 4)), (24, "1", (8, 1, 4)),
                                            (136, "1", (64, 1, 4))])
def test_which_instance_runs(d, lanes8, shape, monkeypatch):
    """The (lanes per row, chunks per lane, vector width) of the k_bwd instances a few look-ahead steps launch, from the
    kernel names: (16, 2, 4) at d = 128 with the switch, the table's shape otherwise."""
    from torch.profiler import ProfilerActivity, profile
    X, y = _batches("cuda")
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        _run(d, SIZES, X, y, lanes8, dict(lookahead=True, lookahead_list=True), monkeypatch, steps=4)
        torch.cuda.synchronize()
    seen = {tuple(int(v) for v in m_.groups()) for ev in prof.events() for m_ in [_K_BWD.search(ev.name)] if m_}
    assert seen == {shape}, seen
