"""CPU: the restatement behind tests/test_gpu_adam_state.py holds on its own -- the fp32 transcriptions of both branches of
adam_update stay inside the derived bounds when the gradient is off by the FULL granted tolerance, the planted states of
the GPU cases leave at most 2 % of a tensor out of the update assertion, and the host's per-step constants
(vfm_step_consts: pure host arithmetic) are the fp64 formulas at every position of the moment period."""
import ctypes as C
import math

import numpy as np
import pytest

import adam_restatement as R

STEPS = [2, 57, 127, 128, 129, 300, 1000]


def _tensor(rng, kind):
    """A gradient of one tensor kind with rows outside the batch (exact zeros) and the fresh rows among both."""
    shape = {"entity": (400, 24), "bias": (400, 2), "scalars": (3,)}[kind]
    g = rng.standard_normal(shape) * 0.3
    p = (rng.standard_normal(shape) * 0.5).astype(np.float32)
    if kind == "scalars":
        return g, p, None, None
    touched = rng.random(shape[0]) < 0.55
    g[~touched] = 0.0
    return g, p, touched, R.fresh_rows(rng, touched)


@pytest.mark.parametrize("t", STEPS)
def test_fp32_transcriptions_stay_inside_the_bounds_with_the_full_gradient_tolerance(t):
    rng = np.random.default_rng(t)
    for kind in ("entity", "bias", "scalars"):
        g64, p, touched, fresh = _tensor(rng, kind)
        G = float(np.abs(g64).max())
        tol_g = R.TOL_TABLE if kind != "scalars" else np.array([3e-3, 1e-3, 2e-4])     # (per entry, as the scalars' bound is)
        # the kernel's gradient: off by the whole granted error, either sign; exact zero where the row has no gradient
        g32 = (g64 + np.asarray(tol_g) * G * rng.choice([-1.0, 1.0], g64.shape) * (g64 != 0)).astype(np.float32)
        m, v = R.plant_state(rng, g64, t, fresh)
        p_ref, m_ref, v_ref = R.step_fp64(p, g64, m, v, t)
        ok = R.asserted(G, g64, v_ref, fresh)
        assert 1.0 - ok.mean() <= R.MAX_EXCLUDED
        for form in ("plain", "scaled"):
            scaled = form == "scaled"
            ms, vs = R.to_stored(m, v, t - 1, scaled)
            fn = R.step_fp32_scaled if scaled else R.step_fp32_plain
            p_got, ms2, vs2 = fn(p, g32, ms, vs, t)
            m_got, v_got = R.to_plain(ms2, vs2, t, scaled)
            dm, dv, du = R.bounds(G, tol_g, p, m_ref, v_ref, t, k=((t - 1) % R.PERIOD + 1) if scaled else 0)
            rm = (np.abs(m_got - m_ref) / dm).max()
            rv = (np.abs(v_got - v_ref) / dv).max()
            ru = (np.abs((p_got.astype(np.float64) - p) - (p_ref - p)) / du)[ok].max()
            print("t=%d %s %s: worst value / bound  m' %.3f  v' %.3f  update %.3f" % (t, kind, form, rm, rv, ru))
            assert rm <= 1 and rv <= 1 and ru <= 1, (kind, form, rm, rv, ru)
            if touched is not None:
                out = ~touched
                if scaled and t % R.PERIOD:            # the stored moments of a row without gradient do not change
                    assert np.array_equal(ms2[out], ms[out]) and np.array_equal(vs2[out], vs[out])
                assert np.array_equal(p_got[fresh & out], p[fresh & out])
            # the bounds are not slack by orders: a dropped bias correction / swapped betas are errors of order one
            bad_p = p - (R.LR / (1 - R.B1 ** t)) * m_ref / (np.sqrt(v_ref) + R.EPS)      # sqrt(bc2) dropped
            if t <= 300:
                assert (np.abs((bad_p - p) - (p_ref - p)) / du)[ok].max() > 10


def test_replay_restatement_and_its_bound():
    """replay_fp64 with one lag per row == step_fp64 with zero gradient, step after step; the fp32 replay of the scaled form
    stays inside replay_bound over a 126-step lag."""
    rng = np.random.default_rng(5)
    g = rng.standard_normal((50, 6))
    p = (rng.standard_normal((50, 6)) * 0.5).astype(np.float32)
    m, v = R.plant_state(rng, g, 2)
    t_from = rng.integers(1, 127, 50)
    p1, m1, v1, moved, n = R.replay_fp64(p, m, v, t_from, 127)
    for row in (0, 17, 49):
        q, a, b = p[row].astype(np.float64), m[row].astype(np.float64), v[row].astype(np.float64)
        for s in range(int(t_from[row]) + 1, 128):
            q, a, b = R.step_fp64(q, np.zeros(6), a, b, s)
        assert np.allclose(q, p1[row], rtol=0, atol=1e-13) and np.allclose(a, m1[row]) and np.allclose(b, v1[row])
    # fp32 replay from step 1 (stored = plain / b^1), the kernels' operation order
    p1, _, _, moved, n = R.replay_fp64(p, m, v, 1, 127)
    ms, vs = R.to_stored(m, v, 1, True)
    q, r = p.copy(), np.sqrt(vs)
    for s in range(2, 128):
        c = R.scaled_consts(s)
        q = R._fma(-c["a1"] * ms, np.float32(1) / R._fma(r, c["q2"], np.float32(R.EPS)), q)
    ratio = (np.abs(q - p1) / R.replay_bound(p, moved, n)).max()
    print("replay of 126 steps: worst value / bound %.3f" % ratio)
    assert ratio <= 1


def test_planted_states_of_the_gpu_cases_leave_at_most_two_percent_out():
    """Pure numpy: the problems of tests/test_gpu_adam_state.py, a synthetic gradient on the batch's rows, the planted state
    and the fp64 step -- what falls out of the update assertion are the fresh rows alone, within the cap; and every
    problem has at least 30 % of its rows in the batch and 30 % outside."""
    from test_gpu_adam_state import build_problem, problems_of_gpu_cases
    from test_gpu_lazy_forms import problems_of_lazy_forms
    for name, kw in problems_of_gpu_cases() + [(name, kw) for name, kw, _ in problems_of_lazy_forms()]:
        pb = build_problem(**kw)
        touched, T, d = pb["touched"], pb["spec"].T, pb["spec"].d
        assert T >= 200 and 0.3 <= touched.mean() <= 0.7, (name, T, touched.mean())
        rng = np.random.default_rng(T)
        fresh = R.fresh_rows(rng, touched)
        for width in (2 * min(d, 64), 2):
            g = rng.standard_normal((T, width)) * touched[:, None]
            m, v = R.plant_state(rng, g, 57, fresh)
            _, _, v_ref = R.step_fp64(np.zeros_like(g), g, m, v, 57)
            ok = R.asserted(float(np.abs(g).max()), g, v_ref, fresh)
            assert 1.0 - ok.mean() <= R.MAX_EXCLUDED, (name, 1.0 - ok.mean())
            assert np.array_equal(~ok.all(axis=1), fresh), name          # (only the fresh rows)


def test_lookahead_problems_of_the_gpu_cases_meet_their_preconditions():
    """Pure numpy: every look-ahead problem of tests/test_gpu_lazy_forms.py, with the next batch _case will draw for it, has
    >= 30 % of its rows in this batch and >= 30 % outside, >= 20 rows only the next batch holds and >= 20 rows in neither
    (asserted by _lookahead_lag itself), and the fresh rows -- all a record check can lose -- within the 2 % cap."""
    from test_gpu_adam_state import build_problem
    from test_gpu_lazy_forms import lookahead_split, problems_of_lazy_forms
    n = 0
    for name, kw, steps in problems_of_lazy_forms():
        if not steps:
            continue
        pb = build_problem(**kw)
        touched, T = pb["touched"], pb["spec"].T
        assert 0.3 <= touched.mean() <= 0.7, (name, touched.mean())
        assert 4.0 / T <= R.MAX_EXCLUDED, (name, T)
        for t in steps:
            nxt = lookahead_split(pb, t)
            assert nxt["x"].shape == pb["x"].shape and (nxt["mask"] & ~touched).sum() >= 20, name
            assert (~nxt["mask"] & ~touched).sum() >= 20, name
            n += 1
    assert n >= 28


def _consts(lr, t, scaled):
    from vae_amd import _lib
    c = _lib.StepConsts()
    assert _lib.load().vfm_step_consts(lr, 0.9, 0.999, 1e-8, t, int(scaled), C.byref(c)) == 0
    return c


@pytest.mark.parametrize("scaled", [False, True])
def test_step_consts_are_the_fp64_formulas_at_every_period_position(scaled):
    """vfm_step_consts over steps 1..400 and 10^6: step_size, bc2_sqrt, a1, q2, c1, c2, s1, s2 each within one fp32 rounding
    of the fp64 formula (a1, q2 are formed from the ROUNDED step_size / bc2_sqrt: two roundings), k = (t-1) mod 128 + 1,
    store_true exactly at the multiples of 128 (scaled form only)."""
    lr, b1, b2 = R.LR, R.B1, R.B2
    u = 2.0 ** -24
    for t in list(range(1, 401)) + [10 ** 6]:
        c = _consts(lr, t, scaled)
        k = (t - 1) % 128 + 1
        assert c.k == k and c.scaled == int(scaled)
        assert c.store_true == int(scaled and t % 128 == 0)
        step, sb = lr / (1 - b1 ** t), math.sqrt(1 - b2 ** t)
        s1, s2 = (b1 ** k, b2 ** k) if scaled else (1.0, 1.0)
        want = {"step_size": (step, 1), "bc2_sqrt": (sb, 1), "s1": (s1, 1), "s2": (s2, 1), "c1": ((1 - b1) / s1, 1),
                "c2": ((1 - b2) / s2, 1), "a1": (step * s1, 2), "q2": (math.sqrt(s2) / sb, 2)}
        for name, (w, n) in want.items():
            got = float(getattr(c, name))
            assert abs(got - w) <= n * 1.0001 * u * abs(w), (t, name, got, w)
        # ... and bitwise the restatement the GPU tests fill the look-ahead table with
        if scaled:
            r = R.scaled_consts(t, lr)
            for name in ("a1", "q2", "c1", "c2", "s1", "s2", "step_size", "bc2_sqrt"):
                assert abs(float(getattr(c, name)) - float(r[name])) <= R.ulp32(r[name]), (t, name)
