"""The fp64 reference of the fused variant step (include/vfm_variant_step.h), shared by tests/test_variant_step_cpu.py and
tests/test_gpu_variant_step.py.  TEST INFRASTRUCTURE ONLY (numpy + torch on the CPU; no vae_amd import).

Reference: the gradients of oracle.vfm_oracle.variant_elbo by autograd (fp64), then adam_restatement.step_fp64 from a
PLANTED state (m, v, t) per tensor -- entity table, bias table, scalars[3], flat priors.  One teacher-forced step has no
trajectory amplification, so (m', v', p' - p) are held entry by entry against adam_restatement.bounds(G, tol_g, ..., k=0)
where adam_restatement.asserted says, with at most MAX_EXCLUDED of a tensor left out.

tol_g is what tests/test_gpu_objectives.py::test_variants_vs_oracle grants the variant gradients, in golden_util.rel_err's
measure (error over the tensor's largest entry): 5e-4 both tables, 1e-3 the priors; the scalars in its absolute-plus-
magnitude form 5e-4 |want| + 2e-4 (sum |pred| nb_train / B + 1), divided by G to enter `bounds` per entry.

C_U.  The step's update is k_adam's operation sequence (fp32(step_size), step_size m', IEEE sqrt, fp32(bc2_sqrt), the
division by it, + eps, the last division: 7 roundings of half an ulp), the count adam_restatement's docstring gives for the
plain form; C_U = 8 covers it and is used unchanged.  C_M = C_V = 2 (plain moments) likewise.

t = 1 is run from a planted state as well (moments planted as for t = 2): the kernel is teacher-forced, and from m = v = 0
no update entry would be asserted (v' = (1 - B2) g^2 < (0.1 G)^2)."""
import dataclasses
import math

import numpy as np
import torch

import adam_restatement as R
from oracle import vfm_oracle as O

f4, f8 = np.float32, np.float64
TOL_TABLE, TOL_PRIOR = 5e-4, 1e-3
TENSORS = ("entity", "bias", "scalars", "priors")


@dataclasses.dataclass(frozen=True)
class StepCase:
    d: int
    F: int
    B: int
    t: int
    objective: str           # "sampled" / "closed_form"
    priors: bool
    values: bool
    output: str = "reg"      # "reg" Normal / "class" Bernoulli
    id32: bool = False
    eps_table: bool = False

    @property
    def id(self):
        return "d%d-F%d-B%d-t%d-%s-%s%s-%s-%s-%s" % (self.d, self.F, self.B, self.t, self.objective, "pri" if self.priors else "n01",
                                                     "-val" if self.values else "", self.output, "i32" if self.id32 else "i64",
                                                     "table" if self.eps_table else "philox")


# the smallest cases that reach each code path: general family d = 2, 5, 20 (+ 70, 130, 300: two, four and sixteen
# coordinates per lane), lane-group family d = 8, 16, 136, 520; every listed d with priors on at least once
CASES = [
    StepCase(2, 2, 500, 1, "closed_form", True, False),
    StepCase(2, 3, 33, 57, "sampled", False, True, "class", True, True),
    StepCase(5, 1, 500, 2, "closed_form", True, True, "reg", True),
    StepCase(5, 5, 1, 1000, "sampled", True, False),
    StepCase(20, 3, 500, 57, "sampled", True, True, "class", False, True),
    StepCase(20, 2, 33, 2, "closed_form", False, False, "reg", True),
    StepCase(8, 2, 500, 1000, "sampled", True, True, "reg", True),
    StepCase(8, 5, 33, 1, "closed_form", False, True),
    StepCase(16, 3, 500, 2, "closed_form", True, False),
    StepCase(16, 1, 33, 57, "closed_form", False, False, "reg", True),
    StepCase(136, 2, 500, 57, "sampled", True, False, "class", False, True),
    StepCase(136, 3, 1, 1, "closed_form", True, True, "reg", True),
    StepCase(520, 2, 33, 1000, "closed_form", True, True),
    StepCase(520, 5, 500, 2, "sampled", False, False, "reg", True),
    StepCase(70, 2, 500, 57, "sampled", True, True),
    StepCase(130, 3, 33, 57, "sampled", False, True),
    StepCase(300, 2, 33, 2, "closed_form", True, False, "reg", True),
]


def split_priors(flat, G, d):
    return {"global": (flat[0], flat[1]), "bias": (flat[2:2 + G], flat[2 + G:2 + 2 * G]),
            "entity": (flat[2 + 2 * G:2 + 2 * G + G * d], flat[2 + 2 * G + G * d:])}


def build_problem(case, seed=0):
    """Tables of >= 200 rows with rows outside the batch in every group (a group holds at least B / 2 ids), ids inside
    their groups, parameters of the sizes test_variants_vs_oracle draws."""
    g = np.random.default_rng(4000 + 97 * seed + 13 * case.d + case.F + 7 * case.B + case.t)
    F, d, B = case.F, case.d, case.B
    lo = max(-(-200 // F), B // 2)
    sizes = [int(g.integers(lo, lo + 40)) for _ in range(F)]
    T = sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    x = np.stack([off[f] + g.integers(0, sizes[f], B) for f in range(F)], 1).astype(np.int64)
    y = (g.integers(1, 6, B) if case.output == "reg" else g.integers(0, 2, B)).astype(f4)
    nb_occ = np.bincount(x.reshape(-1), minlength=T) + g.integers(1, 4, T)
    se = 0.5 * min(1.0, math.sqrt(64.0 / d))
    P = {"alpha": np.array([g.uniform(0.3, 1.5)], f4), "global_bias_mean": np.array([g.normal()], f4),
         "global_bias_scale": np.array([g.uniform(0.3, 1.2) * g.choice([-1, 1])], f4),
         "bias_params": (0.6 * g.standard_normal((T, 2))).astype(f4),
         "entity_params": (se * g.standard_normal((T, 2 * d))).astype(f4)}
    pri = None
    if case.priors:
        G = F
        pri = np.concatenate([[g.normal() * 0.3, g.uniform(0.6, 1.5) * g.choice([-1, 1])], 0.3 * g.standard_normal(G),
                              g.uniform(0.6, 1.5, G) * g.choice([-1, 1], G), se * 0.6 * g.standard_normal(G * d),
                              g.uniform(0.6, 1.5, G * d) * g.choice([-1, 1], G * d)]).astype(f4)
    vals = g.uniform(0.3, 2.0, (B, F)).astype(f4) if case.values else None
    return dict(case=case, B=B, T=T, F=F, d=d, sizes=sizes, hi=np.cumsum(sizes), gn=np.array(sizes, f8), x=x, y=y, nb_occ=nb_occ,
                P=P, pri=pri, vals=vals, nb_train=7 * B, seed=int(g.integers(0, 2 ** 31)), step=int(g.integers(0, 10 ** 6)),
                rng=np.random.default_rng(77 + seed))


def oracle_grads(pb, eps, pri=None):
    """fp64 autograd gradients of oracle.variant_elbo: dict(entity, bias, scalars, priors | None) + pred, loss.
    eps: (eps0[1], eps_w[T], eps_v[T,d]) or None (closed form).  pri: prior vector to evaluate at (default pb['pri'])."""
    case, F, d = pb["case"], pb["F"], pb["d"]
    leaf = lambda a_: torch.tensor(np.asarray(a_, f8), requires_grad=True)
    Pt = {k: leaf(v) for k, v in pb["P"].items()}
    pri = pb["pri"] if pri is None else pri
    flat = leaf(pri) if case.priors else None
    r = O.variant_elbo(Pt, pb["x"], pb["y"], pb["nb_occ"], pb["hi"], pb["gn"], pb["nb_train"], case.objective,
                       priors=split_priors(flat, F, d) if case.priors else None, values=pb["vals"],
                       eps=None if eps is None else tuple(np.asarray(e, f8) for e in eps), output=case.output)
    r["loss"].backward()
    return {"entity": Pt["entity_params"].grad.numpy(), "bias": Pt["bias_params"].grad.numpy(),
            "scalars": np.array([0.0 if Pt[k].grad is None else Pt[k].grad.numpy()[0]
                                 for k in ("alpha", "global_bias_mean", "global_bias_scale")]),
            "priors": flat.grad.numpy() if case.priors else None, "pred": r["pred"].detach().numpy(), "loss": float(r["loss"].detach())}


def params_of(pb):
    P = pb["P"]
    return {"entity": P["entity_params"], "bias": P["bias_params"],
            "scalars": np.concatenate([P["alpha"], P["global_bias_mean"], P["global_bias_scale"]]).astype(f4), "priors": pb["pri"]}


def tolerances(pb, ref):
    """tol_g per tensor (a number, or one per entry for the scalars), as `bounds` takes it."""
    G_sc = float(np.abs(ref["scalars"]).max())
    mag = float(np.abs(ref["pred"]).sum()) * pb["nb_train"] / max(pb["B"], 1) + 1.0
    return {"entity": TOL_TABLE, "bias": TOL_TABLE, "scalars": (5e-4 * np.abs(ref["scalars"]) + 2e-4 * mag) / G_sc,
            "priors": TOL_PRIOR}


def fresh_mask(rng, touched):
    """adam_restatement.fresh_rows; a batch that touches fewer than two rows (B = 1, F = 1) plants what it can."""
    touched = np.asarray(touched, bool)
    if touched.sum() >= 2:
        return R.fresh_rows(rng, touched)
    fresh = np.zeros(touched.size, bool)
    fresh[np.flatnonzero(touched)] = True
    fresh[rng.choice(np.flatnonzero(~touched), 2, replace=False)] = True
    return fresh


def plant(pb, ref):
    """{tensor: (m, v, fresh mask | None)} planted for the step pb['case'].t (fp32)."""
    rng, t = pb["rng"], max(pb["case"].t, 2)
    touched = np.bincount(pb["x"].reshape(-1), minlength=pb["T"]) > 0
    fresh = fresh_mask(rng, touched)
    out = {}
    for name in TENSORS:
        if ref[name] is None:
            out[name] = None
            continue
        fr = fresh if name in ("entity", "bias") else None
        m, v = R.plant_state(rng, ref[name], t, fr)
        out[name] = (m, v, fr)
    return out


def reference_step(pb, ref, planted, lr=R.LR):
    """{tensor: (p', m', v')} in fp64."""
    P, t = params_of(pb), pb["case"].t
    return {n: (None if ref[n] is None else R.step_fp64(P[n], ref[n], planted[n][0], planted[n][1], t, lr)) for n in TENSORS}


def compare(pb, ref, planted, want, got, lr=R.LR):
    """got: {tensor: (p', m', v')} as the code under test left them.  Returns the list of (tensor, quantity, worst error /
    bound, share of entries left out) and the list of failures among them."""
    P, t, tol = params_of(pb), pb["case"].t, tolerances(pb, ref)
    rows, bad = [], []
    for n in TENSORS:
        if ref[n] is None:
            continue
        g64 = np.asarray(ref[n], f8)
        G = float(np.abs(g64).max())
        p0 = np.asarray(P[n], f8)
        pw, mw, vw = want[n]
        pg, mg, vg = (np.asarray(a, f8) for a in got[n])
        dm, dv, du = R.bounds(G, tol[n], p0, mw, vw, t, lr, k=0)
        ok = R.asserted(G, g64, vw, planted[n][2])
        left = 1.0 - float(ok.mean())
        for q, err, bound, mask in (("m'", np.abs(mg - mw), dm, None), ("v'", np.abs(vg - vw), dv, None),
                                    ("update", np.abs((pg - p0) - (pw - p0)), du, ok)):
            if mask is not None:
                err, bound = err[mask], np.broadcast_to(bound, mask.shape)[mask]
            finite = bool(np.isfinite(err).all())
            worst = float(np.max(err / np.maximum(bound, 1e-300))) if err.size and finite else (0.0 if finite else np.inf)
            rows.append((n, q, worst, left if mask is not None else 0.0))
            if not worst <= 1.0 or (mask is not None and left > R.MAX_EXCLUDED):
                bad.append(rows[-1])
        if not (np.isfinite(pg).all() and np.isfinite(mg).all() and np.isfinite(vg).all()):
            bad.append((n, "finite", np.inf, 0.0))
    return rows, bad
