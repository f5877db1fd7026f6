"""CPU half of tests/test_gpu_variant_scale.py: the problems it builds do drive every capped loop of the objective-variant
kernels round more than once.  The caps are read out of the csrc text, so a changed cap fails here instead of quietly ending
the coverage; the launch arithmetic is the restatement the GPU file sizes its problems with."""
import os
import re

import numpy as np
import pytest

import test_gpu_variant_scale as S
from golden_util import ROOT

CSRC = os.path.join(ROOT, "vae_amd", "csrc")


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_caps_in_the_sources_are_the_restated_ones():
    v8, v, args = _text("vfm_variants8.hpp"), _text("vfm_variants.hip"), _text("vfm_args.hpp")
    assert [int(m) for m in re.findall(r"constexpr\s+int\s+VAR_BWD_BLOCKS\s*=\s*(\d+)\s*;", v8)] == [S.CAP]
    assert [int(m) for m in re.findall(r"constexpr\s+int\s+VAR_PSUM_CH\s*=\s*(\d+)\s*;", v8)] == [S.VAR_PSUM_CH]
    assert [int(m) for m in re.findall(r"constexpr\s+int\s+BLOCK\s*=\s*(\d+)\s*;", args)] == [S.BLOCK]
    # the forward of both families and the scalar backward cap nb with a literal; the lane-group backward with VAR_BWD_BLOCKS
    caps = re.findall(r"if\s*\(nb\s*>\s*(\w+)\)\s*nb\s*=\s*(\w+)\s*;", v)
    assert sorted(caps) == sorted([(str(S.CAP),) * 2] * 3 + [("VAR_BWD_BLOCKS",) * 2]), caps
    assert len(re.findall(r"int64_t\s+nb\s*=\s*\(a\.[BT]\s*\+\s*GPB\s*-\s*1\)\s*/\s*GPB\s*;", v)) == 2
    assert len(re.findall(r"int64_t\s+nb\s*=\s*\(p->[BT]\s*\+\s*BLOCK\s*/\s*64\s*-\s*1\)\s*/\s*\(BLOCK\s*/\s*64\)\s*;", v)) == 2
    # epb: the same two lines on the host and in the kernel
    assert len(re.findall(r"epb\s*=\s*\(epb\s*\+\s*GPB\s*-\s*1\)\s*/\s*GPB\s*\*\s*GPB\s*;", v + v8)) == 2
    assert "(a.T + nb - 1) / nb" in v and "(a.T + gridDim.x - 1) / gridDim.x" in v8
    # k_positions: 4096 workgroups of 256 threads, both call sites
    assert [int(m) for m in re.findall(r"if\s*\(nbp\s*>\s*(\d+)\)\s*nbp\s*=\s*\1\s*;", v)] == [S.POS_THREADS // 256] * 2
    assert len(re.findall(r"k_positions,\s*dim3\(\(unsigned\)nbp\),\s*dim3\(256\)", v)) == 2
    # the eight-rows-in-flight loop and the rows per chunk
    assert "b + 7 <= be" in v8 and "(b1 - b0 + VAR_PSUM_CH) / VAR_PSUM_CH" in v8
    # lane-group shapes: the instantiated list is what var_shape yields over d = 8 .. 1024
    shapes = re.search(r"#define\s+VFM_FOR_VAR_SHAPES\(X\)(.*)", v).group(1)
    inst = {(int(a), int(b)) for a, b in re.findall(r"X\((\d+),\s*(\d+)\)", shapes)}
    assert inst == {S.var_shape(d) for d in range(8, 1025, 8)}
    assert "while (l < D8 && l < 64) l <<= 1;" in v and "(p->d & 7) == 0" in v


def test_case_list_covers_what_it_claims():
    lane = [c for c in S.CASES if S.family(c.d) == "lane"]
    scalar = [c for c in S.CASES if S.family(c.d) == "scalar"]
    assert {c.d for c in lane} == {8, 64, 136, 512, 1024} and {c.d for c in scalar} == {20, 300}
    assert {S.var_shape(c.d) for c in lane} == {(1, 1), (8, 1), (32, 1), (64, 1), (64, 2)}
    for d in (8, 64, 136, 512, 20, 300):
        assert {c.objective for c in S.CASES if c.d == d} == {"sampled", "closed_form"}
    assert [c.objective for c in S.CASES if c.d == 1024] == ["sampled"]
    for cf in (False, True):
        for hv in (False, True):
            assert len({c.d for c in lane if (c.objective == "closed_form") == cf and c.values == hv}) >= 2, (cf, hv)
    for pri in (False, True):
        assert len({c.d for c in lane if c.priors == pri}) >= 2
    for fam in (lane, scalar):
        assert {c.id32 for c in fam} == {False, True}
        assert any(c.priors for c in fam) and any(c.values for c in fam)
    assert all(c.values for c in S.CASES if c.d == 8)
    assert any(c.output == "class" for c in S.CASES) and all(c.output == "reg" for c in S.CASES if c.objective == "closed_form")
    for d in (8, 64, 136, 512, 20, 300):                     # the id width alternates within every d
        assert {c.id32 for c in S.CASES if c.d == d} == {False, True}
    assert S.EXCLUDED_SHARE <= 0.01


def test_chunked_oracle_is_the_oracle():
    """oracle_eval's row chunks add up to one call of oracle.variant_elbo on the whole batch (loss, pred, every gradient)."""
    import torch
    from oracle import vfm_oracle as O
    g = np.random.default_rng(3)
    case = S.ScaleCase(16, "sampled", True, True, False)
    B, sizes, d, F = 57, (9, 3, 11), 16, 3
    T = sum(sizes)
    x, _ = S.make_batch(g, sizes, B)
    pb = dict(case=case, B=B, T=T, F=F, d=d, sizes=sizes, hi=np.cumsum(sizes), gn=np.array(sizes, np.float64), x=x,
              y=g.integers(1, 6, B).astype(np.float32), nb_occ=np.bincount(x.reshape(-1), minlength=T) + 1,
              P={"alpha": np.array([0.7], np.float32), "global_bias_mean": np.array([0.2], np.float32),
                 "global_bias_scale": np.array([-0.8], np.float32),
                 "bias_params": g.standard_normal((T, 2)).astype(np.float32),
                 "entity_params": (0.5 * g.standard_normal((T, 2 * d))).astype(np.float32)},
              pri=np.concatenate([[0.1, -1.2], 0.3 * g.standard_normal(F), g.uniform(0.6, 1.5, F), 0.3 * g.standard_normal(F * d),
                                  g.uniform(0.6, 1.5, F * d) * g.choice([-1, 1], F * d)]).astype(np.float32),
              vals=g.uniform(0.3, 2.0, (B, F)).astype(np.float32), nb_train=7 * B)
    eps = (g.standard_normal(1), g.standard_normal(T), g.standard_normal((T, d)))
    got = S.oracle_eval(pb, eps, chunk_elems=10 * F * d)              # six chunks, the last ragged
    leaf = lambda a_: torch.tensor(np.asarray(a_, np.float64), requires_grad=True)
    Pt, flat = {k: leaf(v) for k, v in pb["P"].items()}, leaf(pb["pri"])
    r = O.variant_elbo(Pt, x, pb["y"], pb["nb_occ"], pb["hi"], pb["gn"], pb["nb_train"], "sampled",
                       priors=S.split_priors(flat, F, d), values=pb["vals"], eps=eps, output="reg")
    r["pred"].retain_grad()
    r["loss"].backward()
    close = lambda a_, b_: np.allclose(a_, b_, rtol=1e-12, atol=1e-12)
    assert close(got["loss"], r["loss"].item()) and close(got["pred"], r["pred"].detach().numpy())
    assert close(got["g_row"], r["pred"].grad.numpy())
    assert close(got["g_entity"], Pt["entity_params"].grad.numpy()) and close(got["g_bias"], Pt["bias_params"].grad.numpy())
    assert close(got["g_scalars"], [Pt[k].grad.numpy()[0] for k in ("alpha", "global_bias_mean", "global_bias_scale")])
    assert close(got["g_priors"], flat.grad.numpy())
    # the fp64 terms behind the summation bounds add up to those gradients
    tot, ab = S.prior_terms(pb)
    assert np.all(np.abs(tot - got["g_priors"]) <= 1e-12 * ab + 1e-14)
    ab_sc = S.scalar_terms(pb, got, float(eps[0][0]))
    assert np.all(ab_sc >= np.abs(got["g_scalars"]) * (1 - 1e-12))


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.id)
def test_problem_drives_every_loop_round_again(case):
    pb = S.build_problem(case)
    d, B, T, F, sizes, x = pb["d"], pb["B"], pb["T"], pb["F"], pb["sizes"], pb["x"]
    u = S.unit_of(d)
    assert u == {8: 256, 64: 32, 136: 8, 512: 4, 1024: 4, 20: 4, 300: 4}[d]
    assert B == 2 * S.CAP * u + u + 3 and T >= B and F == (2 if d in (8, 1024) else 3)
    if d == 8:
        assert T > S.POS_THREADS and case.values              # k_positions strides too
    # passes
    assert S.fwd_blocks(B, u) == S.CAP and S.fwd_rows(B, u) == (2, 3)
    assert S.bwd_blocks(T, u) == S.CAP
    assert S.bwd_entities(d, T) == (2, 3)
    # groups
    assert sum(sizes) == T and len(sizes) == F
    assert len([n for n in sizes if n > 3]) == 2 and (F == 2 or sizes[1] == 3)
    if S.family(d) == "lane":                                  # (the scalar pair has no entity ranges and no partial rows)
        epb = S.bwd_epb(T, u)
        assert epb == 3 * u
        spans = S.group_spans(d, T, sizes)
        big = [s for s, n in zip(spans, sizes) if n > 3]
        assert all(S.span_ok(b1 - b0 + 1) for b0, b1 in big), spans
        assert all((b1 - b0 + S.VAR_PSUM_CH) // S.VAR_PSUM_CH >= 8 for b0, b1 in big)    # `per`: the unrolled loop runs
        assert all(int(h) % epb != 0 for h in pb["hi"][:-1])
        if F == 3:
            assert spans[1][0] == spans[1][1] == spans[0][1] == spans[2][0]               # one workgroup, three partial rows
    # ids: every column inside its group, int32 holds them
    lo = np.concatenate([[0], pb["hi"][:-1]])
    assert ((x >= lo) & (x < pb["hi"])).all() and T < 2 ** 31
    # lists: 0, 1, 2 and several hundred inside one workgroup's range; odd and even lengths for the two-in-flight walk
    n_wg, odd_seen, even_seen = S.list_classes(d, T, x)
    assert n_wg >= 1 and odd_seen and even_seen
    cnt = np.bincount(x.reshape(-1), minlength=T)
    assert (cnt == 0).sum() > 0 and cnt.max() >= 200
    # half of every large column sits on the Zipf tail's entities (local id = 0 mod 7): a uniform column would put 1/7
    # there; 1/14 + 1/2 less the ranks past size / 7, which wrap (P(rank >= 386) = 0.14 for the smallest group here)
    for f, (l, n) in enumerate(zip(lo, sizes)):
        if n > 3:
            share = ((x[:, f] - l) % 7 == 0).mean()
            assert 0.45 <= share <= 0.60, (f, share)
    # oracle: finite on the whole batch (draws of the same law stand in for the Philox ones); nothing is left out
    g = np.random.default_rng(1)
    eps = None
    if case.objective == "sampled":
        eps = (g.standard_normal(1), g.standard_normal(T), g.standard_normal((T, d), dtype=np.float32))
    ref = S.oracle_eval(pb, eps, grads=False)
    assert np.isfinite(ref["loss"]) and np.isfinite(ref["pred"]).all() and ref["pred"].shape == (B,)
    assert np.abs(ref["pred"]).max() < 100.0                   # the scale the tolerances are relative to stays O(10)
    assert S.EXCLUDED_SHARE <= 0.01
    if case.priors:
        tot, ab = S.prior_terms(pb)
        assert np.isfinite(tot).all() and np.isfinite(ab).all() and (ab > 0).all()
        assert S.n_chain_priors(d, T, sizes) == {8: 327, 64: 103, 136: 79, 512: 75, 1024: 75, 20: 8195, 300: 8195}[d]
    assert S.n_chain_scalars() == 12
