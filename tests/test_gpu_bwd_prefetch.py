"""k_bwd<PF> (VFM_BWD_PREFETCH=1: each row's index fetched one row ahead, under the previous row's epilogue) against the
row-serial k_bwd: the same step bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sizes,d,B,kw", [
    ((3000, 900), 128, 1999, dict(lookahead=True, lookahead_list=True)),    # d = 128: two lane groups per wave; odd list
    ((3000, 900), 128, 1999, dict(lookahead=True, lookahead_list=False)),   # the kernel classifies every row: skipped rows
    ((3000, 900), 32, 1500, dict(lookahead=False)),                          # the dense fused step
    ((5000, 40), 64, 6000, dict(lookahead=True, lookahead_list=True, zipf=1.1)),   # heavy lists (k_heavy, filtered launches)
    ((700, 500), 5, 333, dict(lookahead=True, lookahead_list=True)),       # d = 5: four lanes per entity, a partial chunk
])
def test_prefetch_form_is_bitwise_the_row_serial_form(sizes, d, B, kw, monkeypatch):
    """Losses, parameters and both moments BIT FOR BIT over 140 steps (across the moment-period boundary at step 128), four
    batches in turn with the look-ahead plan announced (rows in neither batch wait and later replay: la_gap > 0)."""
    from vae_amd.model import VFM
    from vae_amd.data import synthetic_triples
    attrs = dict(kw)
    zipf = attrs.pop("zipf", 0.0)
    X, y = synthetic_triples(list(sizes), 4 * B, seed=21, device="cuda", zipf=zipf)
    runs = []
    for pf in ("1", "0"):
        monkeypatch.setenv("VFM_BWD_PREFETCH", pf)
        torch.manual_seed(4)
        m = VFM(field_sizes=list(sizes), embedding_size=d, device="cuda", rng_seed=6)
        m.pipeline = False
        for k_, v_ in attrs.items():
            setattr(m, k_, v_)
        m.set_training_data(X, nb_train=4 * B)
        plans = [m.plan(X[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) for i in range(4)]
        losses = []
        for s in range(140):
            nxt = {"next_plan": plans[(s + 1) % 4]} if m.lookahead else {}
            losses.append(m.train_step(plans[s % 4], lr=0.03 if s % 5 else 0.01, **nxt)[0].clone())
        for pl in plans:
            pl.check_status()
        if m.lookahead:
            m.sync_lazy()
        runs.append((m, torch.stack(losses)))
    (a, la), (b, lb) = runs
    assert torch.equal(la, lb)
    assert torch.equal(a._flat, b._flat) and torch.equal(a._adam_m, b._adam_m) and torch.equal(a._adam_v, b._adam_v)
    assert not torch.isnan(a._flat).any()
