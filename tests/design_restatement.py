"""numpy fp64 restatement of target-aware elicitation (include/vfm_design.h) and the cases of its GPU tests.

  operands          M, A [n, d] of context rows in fp64 (solve_reference.operands64: k_foldin_solve_prep's sums)
  walk_S, walk_W    the two sums, in the kernel's orders
  scores            the score of every candidate, from the bias term on in k order, fp64 (round with np.float32)
  session           one respondent's whole session: score, choose (on the fp32 scores, ties to the lower position),
                    fold in with solve_fp64; also the gap between the two best scores of every round
  objective_after   sigma_w^2 + sum_k W_k sigma_k^2 from solve_fp64's scales: what the score predicts the drop of
  CASES, build      the GPU cases, CPU tensors only; build() reseeds until every round of every respondent has a gap
                    of at least 2^-20 of the best between the two best scores (exact duplicates of a context excepted)

numpy does not contract a * b + c; the device forms S with phase A's fused a_rk.  The difference is a few units of
2^-53 relative, far inside the fp32 rounding the GPU tests allow and the 2^-20 gap the cases keep."""
import functools

import numpy as np
import torch

import solve_reference as SR
from test_foldin_exact_cpu import solve_fp64

GAP = 2.0 ** -20


def operands(ent, bia, scal, xr, field, link):
    M, A, _, _ = SR.operands64(ent, bia, scal, np.asarray(xr), field, link)
    return M, A


def prec_kl(scal, link, kl_weight):
    return float(SR._link64(SR._np(scal, np.float32)[0], link)), SR.f32(kl_weight)


def walk_S(M, A):
    S = np.zeros(M.shape[1])
    for r in range(M.shape[0]):
        S = S + (A[r] + M[r] * M[r])
    return S


def walk_W(M, A):
    nt = M.shape[0]
    s = np.zeros(M.shape[1])
    for j in range(nt):
        s = s + (A[j] + M[j] * M[j])
    return (1.0 / nt) * s if nt else s


def v(kl, prec, S):
    return kl / (kl + prec * S)


def scores(S, W, n, Mq, Aq, kl, prec):
    """[P] fp64: the score of each candidate row (Mq, Aq [P, d])."""
    acc = np.full(Mq.shape[0], v(kl, prec, float(n)) - v(kl, prec, float(n) + 1.0))
    vS = v(kl, prec, S)
    for k in range(Mq.shape[1]):
        a = Aq[:, k] + Mq[:, k] * Mq[:, k]
        acc = acc + W[k] * (vS[k] - v(kl, prec, S[k] + a))
    return acc


def _sigma2(sol, link):
    s = np.concatenate([sol["s_w"].numpy().reshape(1), sol["s"].numpy().reshape(-1)])
    return SR._link64(s, link) ** 2


def objective_after(ent, bia, scal, xr, yr, field, link, kl_weight, W):
    """sigma_w^2 + sum_k W_k sigma_k^2 at the exact optimum over the rows xr (the prior for no rows)."""
    if len(xr) == 0:
        return 1.0 + float(W.sum())
    sol = solve_fp64(ent, bia, scal, torch.as_tensor(xr), torch.as_tensor(yr), field, link, SR.f32(kl_weight))
    s2 = _sigma2(sol, link)
    return float(s2[0] + (W * s2[1:]).sum())


def session(ent, bia, scal, pool_x, pool_y, hist_x, hist_y, tgt_x, field, link, kl_weight, Q):
    """One respondent (every row of pool_x / hist_x / tgt_x is its own; tgt_x None: the pool).  Returns dict(rows [Q]
    pool positions or -1, score [Q] fp64 (NaN), theta [Q] of (mu_w, mu, s_w, s) fp64 or None, gaps [Q] = (best - second
    best among the rows of another context) / best, inf when there is no second)."""
    pool_x, hist_x = np.asarray(pool_x), np.asarray(hist_x)
    prec, kl = prec_kl(scal, link, kl_weight)
    Mp, Ap = operands(ent, bia, scal, pool_x, field, link)
    Mh, Ah = operands(ent, bia, scal, hist_x, field, link)
    Mt, At = (Mp, Ap) if tgt_x is None else operands(ent, bia, scal, np.asarray(tgt_x), field, link)
    W = walk_W(Mt, At)
    ctx = np.delete(pool_x, field, 1)
    asked, rows, sc_out, thetas, gaps = [], [], [], [], []
    for q in range(Q):
        Mr = np.concatenate([Mh, Mp[asked]]) if asked else Mh
        Ar = np.concatenate([Ah, Ap[asked]]) if asked else Ah
        n = Mr.shape[0]
        sc = scores(walk_S(Mr, Ar), W, n, Mp, Ap, kl, prec)
        left = [p for p in range(pool_x.shape[0]) if p not in asked and not np.isnan(sc[p])]
        if not left:
            rows.append(-1); sc_out.append(float("nan")); thetas.append(thetas[-1] if thetas else None)
            gaps.append(float("inf"))
            continue
        s32 = sc.astype(np.float32)
        best = max(left, key=lambda p: (s32[p], -p))
        others = [sc[p] for p in left if not (ctx[p] == ctx[best]).all()]
        # (no targets: W = 0 and every score is the bias term alone, equal bits on the device too: position decides)
        gaps.append((sc[best] - max(others)) / sc[best] if others and W.any() else float("inf"))
        asked.append(best)
        rows.append(best); sc_out.append(float(sc[best]))
        xr = np.concatenate([hist_x, pool_x[asked]])
        yr = np.concatenate([np.asarray(hist_y, np.float32), np.asarray(pool_y, np.float32)[asked]])
        sol = solve_fp64(ent, bia, scal, torch.as_tensor(xr), torch.as_tensor(yr), field, link, SR.f32(kl_weight))
        thetas.append(dict(mu_w=float(sol["mu_w"][0]), mu=sol["mu"][0].numpy(), s_w=float(sol["s_w"][0]),
                           s=sol["s"][0].numpy()))
    return dict(rows=rows, score=sc_out, theta=thetas, gaps=gaps, W=W)


# ---------------------------------------------------------------------------------------------------------------------
# the GPU cases (CPU tensors)
# ---------------------------------------------------------------------------------------------------------------------
# name: field sizes, field, link, d, pool rows per respondent (cycled), history rows (cycled), respondents, targets
# ("pool": None; "given": a list per respondent, empty for the first), rounds, lds_dim, kl_weight
CASES = {
    "d5_abs": dict(sizes=(40, 90, 4), field=0, link="abs", d=5, pools=[1, 9, 40, 3], hists=[0, 4, 11], n_resp=5,
                   targets="pool", Q=6, lds_dim=-1, klw=0.8, dup=True),
    "d20_softplus": dict(sizes=(40, 90), field=1, link="softplus", d=20, pools=[17, 30, 1], hists=[6, 0, 25], n_resp=4,
                         targets="given", Q=4, lds_dim=-1, klw=1.0),
    "d128_abs": dict(sizes=(12, 400, 3), field=0, link="abs", d=128, pools=[300, 20], hists=[60, 0], n_resp=3,
                     targets="given", Q=4, lds_dim=-1, klw=0.8),
    "d128_softplus": dict(sizes=(12, 200), field=0, link="softplus", d=128, pools=[30, 5], hists=[0], n_resp=3,
                          targets="pool", Q=3, lds_dim=-1, klw=1.0),
    "d200_slab": dict(sizes=(6, 500), field=0, link="abs", d=200, pools=[12, 40], hists=[205, 140, 0], n_resp=3,
                      targets="given", Q=3, lds_dim=-1, klw=2.0),
    "d5_past_cap": dict(sizes=(300, 60, 5), field=0, link="softplus", d=5, pools=[3, 5, 2], hists=[2, 0, 7], n_resp=261,
                        targets="pool", Q=3, lds_dim=0, klw=0.75),
}


def _rows(g, sizes, lo, field, e, n, distinct=True):
    cols = [f for f in range(len(sizes)) if f != field]
    n_ctx = int(np.prod([sizes[f] for f in cols]))
    pick = torch.randperm(n_ctx, generator=g)[:n] if distinct else torch.randint(0, n_ctx, (n,), generator=g)
    rows = torch.zeros(n, len(sizes), dtype=torch.int64)
    rows[:, field] = e
    for f in reversed(cols):                                 # mixed radix: a distinct number is a distinct context
        rows[:, f] = lo[f] + pick % sizes[f]
        pick = pick // sizes[f]
    return rows


def generate(name, seed):
    """The case `name` drawn with `seed`: dict(spec.., ent, bia, scal, pool, y_pool, hist_x, hist_y, targets or None,
    ents [U] ascending) -- shuffled pool, history and targets, CPU tensors."""
    c = dict(CASES[name])
    sizes, field, d = c["sizes"], c["field"], c["d"]
    given = c["targets"] == "given"
    ent, bia, scal = SR.tables(sizes, d, seed)
    g = torch.Generator().manual_seed(seed + 1)
    lo = [sum(sizes[:f]) for f in range(len(sizes))]
    resp = lo[field] + torch.randperm(sizes[field], generator=g)[:c["n_resp"]]
    pool, hist, tgt = [], [], []
    for i, e in enumerate(resp.tolist()):
        n, h = c["pools"][i % len(c["pools"])], c["hists"][i % len(c["hists"])]
        rows = _rows(g, sizes, lo, field, e, n + h)
        p = rows[:n].clone()
        if c.get("dup") and n >= 9:
            p[n - 1] = p[2]                                  # an exact duplicate of a context: equal bits, position decides
        pool.append(p)
        hist.append(rows[n:])
        if given and i > 0:
            tgt.append(_rows(g, sizes, lo, field, e, 7 + i, distinct=False))
    pool, hist = torch.cat(pool), torch.cat(hist)
    pool = pool[torch.randperm(pool.shape[0], generator=g)]
    hist = hist[torch.randperm(hist.shape[0], generator=g)]
    c.update(ent=ent, bia=bia, scal=scal, pool=pool, y_pool=torch.randn(pool.shape[0], generator=g) + 1.0, hist_x=hist,
             hist_y=torch.randn(hist.shape[0], generator=g) + 1.0, targets=None, seed=seed,
             ents=torch.sort(resp).values)
    if given:
        t = torch.cat(tgt)
        c["targets"] = t[torch.randperm(t.shape[0], generator=g)]
    return c


def restate(c):
    """{entity id: session(..)} of a generated case."""
    f = c["field"]
    out = {}
    for e in c["ents"].tolist():
        pm, hm = c["pool"][:, f] == e, c["hist_x"][:, f] == e
        tx = None if c["targets"] is None else c["targets"][c["targets"][:, f] == e].numpy()
        out[e] = session(c["ent"], c["bia"], c["scal"], c["pool"][pm].numpy(), c["y_pool"][pm].numpy(),
                         c["hist_x"][hm].numpy(), c["hist_y"][hm].numpy(), tx, f, c["link"], c["klw"], c["Q"])
        out[e]["pool_index"] = torch.nonzero(pm).reshape(-1)
    return out


def min_gap(ref):
    return min(min(r["gaps"]) for r in ref.values())


@functools.lru_cache(maxsize=None)
def build(name):
    """(case, restatement): the first seed from the case's base on whose every round of every respondent keeps GAP."""
    base = 1000 * (1 + sorted(CASES).index(name))
    for seed in range(base, base + 50):
        c = generate(name, seed)
        ref = restate(c)
        if min_gap(ref) >= GAP:
            return c, ref
    raise AssertionError(f"no seed in [{base}, {base + 50}) keeps the gap for {name}")
