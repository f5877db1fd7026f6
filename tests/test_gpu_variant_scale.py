"""GPU: the objective-variant kernels (csrc/vfm_variants8.hpp, csrc/vfm_variants.hip) PAST their grid caps, against fp64.

Every other variant test runs the kernels' arithmetic at one batch row / one table row per lane group; production runs the
grid-stride loop around it (ML-20M shape: three or four rows per lane group).  Each case here is one variant_forward +
variant_backward with Philox eps at the smallest B and T at which every capped loop goes round two full passes and a
ragged third, compared with oracle.vfm_oracle.variant_elbo (fp64 autograd, evaluated in row chunks and summed) fed with the
same eps (ops.philox_eps): loss, pred, both table gradients, the three scalar gradients, the prior gradients.  The
oracle is the only reference; the scalar pair is never the reference of the lane-group kernels.

Shapes (restated launch arithmetic: var_shape, unit_of, fwd_blocks, bwd_blocks, bwd_epb; tests/test_variant_scale_cpu.py
checks them against the csrc text).  cap = 2048 workgroups, unit = lane groups (or waves) per workgroup,
B = T = 2 cap unit + unit + 3:
  d     kernels            unit   B = T       F
  8     lane group (1,1)   256    1,048,835   2   (T > 1,048,576: k_positions strides too; always with values)
  64    lane group (8,1)    32      131,107   3
  136   lane group (32,1)    8       32,779   3   (17 of 32 lanes filled)
  512   lane group (64,1)    4       16,391   3
  1024  lane group (64,2)    4       16,391   2   (sampled only: the fp64 oracle's memory)
  20, 300  scalar pair       4       16,391   3
Forward: nb = cap, every lane group (wave) owns 2 or 3 rows -- the id cursor, the two-ahead prefetch, the `last` clamp and
reset() cross rows; k_var_finalize sums 2048 slots.  Backward, lane groups: epb = 3 unit (ceil(T / cap) rounded up to the
unit), so 1366 workgroups own 3 entities per lane group and the last a ragged 2-or-3; the scalar pair's waves own 2 or 3
entities.  Groups (group_sizes): F = 3 -> (s0, 3, rest) with s0 about T / 6 (0.13 T would span 178 of the 1366 ACTIVE
workgroups, fewer than the 225 at which k_var_priors_part's eight-rows-in-flight loop first runs); both large groups span
>= 225 workgroups, neither span a multiple of 8 (hence of VAR_PSUM_CH), no boundary on a multiple of epb, the 3-entity group
inside one workgroup's range (that workgroup writes three partial rows).  F = 2 -> (s0, rest).
Batches (make_batch): even rows draw each column uniformly over its group, odd rows from a Zipf(1.3) tail whose rank r lands
on entity 7 r mod size -- hot entities lie seven apart with cold ones in between, so one workgroup's range holds lists of
length 0, 1, 2 and of several hundred (asserted on the data, list_classes).  Entities the batch does not touch must come
back as exact zero rows.

Tolerances.  Per-row and per-entity quantities and the loss keep what test_variants_vs_oracle grants, independent of B and
T: loss 1e-4, pred 2e-4, table gradients 5e-4 of the largest entry (the table gradients also on the cold rows alone --
lists of length <= 2 -- and per id group, since one hot row's entry would otherwise set the scale for a million cold ones).
Scalar and prior gradients are fp32 sums of up to 10^6 cancelling terms and are bounded as a summation error,
    |got - want| <= rel |want| + gamma sum|terms|,   rel = 5e-4 (scalars), 1e-3 (priors),   gamma = n_chain 2^-24,
sum|terms| from the oracle's own terms (scalars: dloss/dpred_r = pred.grad of the oracle's graph; priors: the per-entity
KL-gradient terms in fp64, whose sum is checked against the autograd gradient to 1e-9), n_chain the longest chain of
dependent fp32 additions a term passes through, counted in the code:
  scalars, both families     rows per lane group or wave (3, tot[] += in the row loop) + block_sum: 6 shuffle levels + 3 adds
                             over the 4 waves = 12; the workgroup slots are fp64 from there on (k_var_finalize)
  priors, lane groups        entities per lane group and segment (epb / GPB = 3, acc_* +=) + GPB (the serial LDS sum over q)
                             + rows per chunk of k_var_priors_part (per = (span + 31) / 32 of the widest group: <= 36; the
                             eight accumulators and their tree are shorter than the serial count) + VAR_PSUM_CH (32,
                             k_var_priors_sum):  d = 8: 327, 64: 103, 136: 79, 512, 1024: 75
  priors, scalar pair        entities per wave (3) + one atomicAdd per contributing wave in arbitrary order (8192) = 8195
Nothing is fitted to what the kernels return, and no entry of any gradient is left out (EXCLUDED_SHARE = 0; F >= 2).

Wrong kernels this file catches and the suite before it passes (there nrows = 1, epb = GPB, one chunk row per group, and
every id is 64 bits wide).  Mutations 1, 2, 4, 5 and 6 were each built and run once against the nine lane-group cases on an
MI355X; "trips" names the first assertion of the test that fails (the checks run in the order loss, pred, table gradients,
scalars, priors) and the error / bound the test printed, smallest to largest over the failing cases:
  1. `ri += stride` replaced by `ri += GPB` (id cursor of k_var_fwd8): the second row of a lane group is read at r0 + GPB,
     another workgroup's row, while rc writes r0 + stride.  Fails all 9 cases: trips `loss` (1.4 .. 56), and `pred` stands
     at 4979 .. 7593 times its bound in every case, with g_bias (34 .. 441) and g_m0 behind it.
  2. reset() dropped at a row change: S, M2, S2, R and klrow of the first row leak into the second.  Fails all 9 cases:
     trips `loss` (4961 .. 54177); `pred` at 5985 .. 57740 times its bound, the table and scalar gradients wrong as well.
  3. the `last` clamp one row early: the prefetches past the stream re-read a row that is not the last; nothing wrong is
     computed unless an id there is bad (tot[4]) -- caught only through the loss turning NaN on a planted bad id; NOT
     caught here (the clamp target is never consumed), and not run.
  4. acc_mp / acc_sp / acc_mw / acc_sw not zeroed at a segment change (hoisted out of the while loop): the workgroup that
     holds a group boundary writes group g's sums into group g + 1's partial row as well.  Fails the 6 cases with priors
     (loss, pred, table and scalar gradients stay inside their bounds): trips `g_prior w` (1322 .. 45169) in the four
     F = 3 cases -- the 3-entity group's terms drown in a large group's partial sum -- and `g_prior v mean` in the two
     F = 2 cases (d = 8: 3.0, d = 1024: 225); `g_prior v scale` up to 8e5.
  5. epb rounded up to GPB on the device only (the host's rounding removed): k_var_priors_part looks for a group's partial
     rows in workgroups that did not write them.  Fails the 6 cases with priors: trips `g_prior w`, NaN in every case
     (rows of the scratch that no workgroup wrote); `g_prior v mean` and `v scale` NaN as well.
  6. the unrolled chunk loop of k_var_priors_part starting at b + 8: the first eight partial rows of every chunk are
     dropped.  Fails the 6 cases with priors: trips `g_prior w` (969 .. 996); `g_prior v mean` 981 .. 3158, `v scale`
     980 .. 996.
  7. id_shift = 3 whatever the width: int32 ids are read at twice the offset, x[2 pos] for x[pos] -- pred of every int32
     lane-group case from the first row on.  Its reads of the second half of the stream lie past the end of x, so it is
     not to be run.
The cases without priors pass under 4, 5 and 6, as they must: the mutated code does not run for them.

Measured on an MI355X, worst error / bound over the cases of a family (the test prints every figure as `SCALE <case>
<quantity> error/bound <ratio>` before it asserts; "sum part" = against gamma sum|terms| alone, without rel |want|):
  quantity                        lane groups   scalar pair
  loss                            0.0011        0.0004
  pred                            0.0015        0.0011
  g_entity  all / cold / group    0.0103  0.0002  0.0539      0.0008  0.0001  0.0400
  g_bias    all / cold / group    0.0072  0.0001  0.0163      0.0032  0.0002  0.0037
  g_alpha, g_m0, g_s0             0.0002  0.0004  0.0004      0.0001  0.0001  0.0003
  g_prior global   (sum part)     0.0004  (0.0126)            0.0000  (0.0001)
  g_prior w        (sum part)     0.0005  (0.0437)            0.0004  (0.0010)
  g_prior v mean   (sum part)     0.0077  (0.0678)            0.0019  (0.0049)
  g_prior v scale  (sum part)     0.0166  (0.1552)            0.0023  (0.0071)
All 13 cases pass in 16 s (4 s the largest, d = 8); the counted summation bound alone would hold with a factor 6 to spare.
"""
import dataclasses
import functools
import math
import os

import numpy as np
import pytest
import torch

from golden_util import rel_err

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------- launch arithmetic, restated (numpy only)
CAP = 2048                  # workgroups: the forward's cap and VAR_BWD_BLOCKS (and the scalar pair's two caps)
BLOCK = 256
VAR_PSUM_CH = 32
POS_THREADS = 4096 * 256    # k_positions' grid
MIN_SPAN = 225              # workgroups a group must span for per >= 8 in k_var_priors_part
U24 = 2.0 ** -24
EXCLUDED_SHARE = 0.0        # share of a gradient's entries left out of a comparison (the cap is 1 %)
LOSS_TOL, PRED_TOL, TABLE_TOL, SCALAR_REL, PRIOR_REL = 1e-4, 2e-4, 5e-4, 5e-4, 1e-3      # test_variants_vs_oracle


def var_shape(d):
    """(LPE, CPL) of vfm_variants.hip's var_shape."""
    D8, lpe = d >> 3, 1
    while lpe < D8 and lpe < 64:
        lpe <<= 1
    return lpe, (D8 + lpe - 1) // lpe


def family(d):
    return "lane" if d % 8 == 0 else "scalar"


def unit_of(d):
    """Lane groups (d % 8 == 0) or waves per workgroup."""
    return BLOCK // var_shape(d)[0] if family(d) == "lane" else BLOCK // 64


def fwd_blocks(B, unit):
    return max(1, min(CAP, (B + unit - 1) // unit))


def fwd_rows(B, unit):
    """(fewest, most) rows of a lane group / wave in the forward."""
    stride = fwd_blocks(B, unit) * unit
    return B // stride, (B - 1) // stride + 1


def bwd_blocks(T, unit):
    return min(CAP, (T + unit - 1) // unit)


def bwd_epb(T, unit):
    """Entities per workgroup of k_var_bwd8 (host and device round the same way)."""
    nb = bwd_blocks(T, unit)
    epb = (T + nb - 1) // nb
    return (epb + unit - 1) // unit * unit


def bwd_entities(d, T):
    """(fewest, most) entities of a lane group / wave that has any, in the backward."""
    u = unit_of(d)
    if family(d) == "scalar":
        nw = bwd_blocks(T, u) * u
        return T // nw, (T - 1) // nw + 1
    epb = bwd_epb(T, u)
    last = T - (T - 1) // epb * epb                     # the ragged last workgroup
    return min(epb // u, last // u), epb // u


def group_spans(d, T, sizes):
    """Workgroups [b0, b1] of k_var_bwd8 whose entity range meets each group (k_var_priors_part's b0, b1)."""
    epb = bwd_epb(T, unit_of(d))
    hi = np.cumsum(sizes)
    lo = np.concatenate([[0], hi[:-1]])
    return [(int(l // epb), int((h - 1) // epb)) for l, h in zip(lo, hi)]


def span_ok(n):
    return n >= MIN_SPAN and n % 8 != 0 and n % VAR_PSUM_CH != 0


def sizes_of(d):
    u = unit_of(d)
    n = 2 * CAP * u + u + 3
    return n, n                                          # B, T


def group_sizes(d, T, F):
    """(s0, 3, rest) or (s0, rest): see the module docstring."""
    epb = bwd_epb(T, unit_of(d))
    nwg = (T + epb - 1) // epb
    b0 = next(b for b in range(MIN_SPAN + 1, nwg) if span_ok(b + 1) and span_ok(nwg - b))
    s0 = b0 * epb + max(1, epb // 2 - 2)                 # inside workgroup b0's range, room for the 3-entity group
    return (s0, 3, T - s0 - 3) if F == 3 else (s0, T - s0)


def n_chain_scalars():
    return 3 + 6 + 3


def n_chain_priors(d, T, sizes):
    if family(d) == "scalar":
        return 3 + CAP * (BLOCK // 64)
    u = unit_of(d)
    per = max((b1 - b0 + VAR_PSUM_CH) // VAR_PSUM_CH for b0, b1 in group_spans(d, T, sizes))
    return bwd_epb(T, u) // u + u + per + VAR_PSUM_CH


# ------------------------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass(frozen=True)
class ScaleCase:
    d: int
    objective: str
    priors: bool
    values: bool
    id32: bool
    output: str = "reg"

    @property
    def F(self):
        return 2 if self.d in (8, 1024) else 3

    @property
    def id(self):
        return "d%d-%s-%s%s%s-%s" % (self.d, self.objective, "pri" if self.priors else "n01", "-val" if self.values else "",
                                     "-i32" if self.id32 else "-i64", self.output)


# each <CF, HASV> instance of the lane-group kernels and both PRI values at two or more d; the id width alternates
CASES = [
    ScaleCase(8, "sampled", True, True, True), ScaleCase(8, "closed_form", False, True, False),
    ScaleCase(64, "sampled", False, False, False, "class"), ScaleCase(64, "closed_form", True, True, True),
    ScaleCase(136, "sampled", True, True, True), ScaleCase(136, "closed_form", True, False, False),
    ScaleCase(512, "sampled", True, False, False, "class"), ScaleCase(512, "closed_form", False, False, True),
    ScaleCase(1024, "sampled", True, True, True),
    ScaleCase(20, "sampled", True, True, True, "class"), ScaleCase(20, "closed_form", False, False, False),
    ScaleCase(300, "sampled", False, False, False), ScaleCase(300, "closed_form", True, True, True),
]


def make_batch(g, sizes, B):
    """x [B,F]: even rows uniform over each column's group, odd rows from a Zipf tail (rank r -> entity 7 r mod size)."""
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    odd = (np.arange(B) & 1).astype(bool)
    cols = []
    for f, n in enumerate(sizes):
        uni = g.integers(0, n, B)
        hot = (np.minimum(g.zipf(1.3, B) - 1, 1 << 40) * 7) % n
        cols.append(off[f] + np.where(odd, hot, uni))
    return np.stack(cols, 1).astype(np.int64), odd


def list_classes(d, T, x):
    """Workgroup ranges (epb consecutive entities) that hold occurrence lists of length 0, 1, 2 and >= 200 at once, and
    whether odd and even lengths above 2 occur: (number of such ranges, odd seen, even seen)."""
    epb = bwd_epb(T, unit_of(d))
    cnt = np.bincount(x.reshape(-1), minlength=T)
    nwg = T // epb                                       # full ranges only
    c = cnt[:nwg * epb].reshape(nwg, epb)
    both = (c == 0).any(1) & (c == 1).any(1) & (c == 2).any(1) & (c >= 200).any(1)
    long_ = cnt[cnt > 2]
    return int(both.sum()), bool((long_ % 2 == 1).any()), bool((long_ % 2 == 0).any())


@functools.lru_cache(maxsize=1)
def build_problem(case):
    """Everything of a case that needs no GPU (numpy)."""
    d, F = case.d, case.F
    B, T = sizes_of(d)
    sizes = group_sizes(d, T, F)
    g = np.random.default_rng(9000 + 31 * d + (case.objective == "closed_form"))
    x, odd = make_batch(g, sizes, B)
    y = (g.integers(1, 6, B) if case.output == "reg" else g.integers(0, 2, B)).astype(np.float32)
    nb_occ = np.bincount(x.reshape(-1), minlength=T) + g.integers(1, 4, T)
    se = 0.5 * min(1.0, math.sqrt(64.0 / d))             # keeps pred O(1..10) at every d (an unsaturated Bernoulli)
    P = {"alpha": np.array([g.uniform(0.3, 1.5)], np.float32), "global_bias_mean": np.array([g.normal()], np.float32),
         "global_bias_scale": np.array([g.uniform(0.3, 1.2) * g.choice([-1, 1])], np.float32),
         "bias_params": (0.6 * g.standard_normal((T, 2))).astype(np.float32),
         "entity_params": (se * g.standard_normal((T, 2 * d))).astype(np.float32)}
    G = F
    pri = None
    if case.priors:
        pri = np.concatenate([[g.normal() * 0.3, g.uniform(0.6, 1.5) * g.choice([-1, 1])], 0.3 * g.standard_normal(G),
                              g.uniform(0.6, 1.5, G) * g.choice([-1, 1], G), se * 0.6 * g.standard_normal(G * d),
                              g.uniform(0.6, 1.5, G * d) * g.choice([-1, 1], G * d)]).astype(np.float32)
    vals = g.uniform(0.3, 2.0, (B, F)).astype(np.float32) if case.values else None
    return dict(case=case, B=B, T=T, F=F, d=d, sizes=sizes, hi=np.cumsum(sizes), gn=np.array(sizes, np.float64), x=x, y=y,
                odd=odd, nb_occ=nb_occ, P=P, pri=pri, vals=vals, nb_train=7 * B, seed=int(g.integers(0, 2 ** 31)),
                step=int(g.integers(0, 10 ** 6)))


# ----------------------------------------------------------------------------------------------------------------- oracle
def split_priors(flat, G, d):
    return {"global": (flat[0], flat[1]), "bias": (flat[2:2 + G], flat[2 + G:2 + 2 * G]),
            "entity": (flat[2 + 2 * G:2 + 2 * G + G * d], flat[2 + 2 * G + G * d:])}


def oracle_eval(pb, eps, grads=True, chunk_elems=1 << 22):
    """oracle.vfm_oracle.variant_elbo over the whole batch, evaluated in row chunks and summed.  A chunk is the oracle's own
    call on those rows with nb_train scaled by the chunk's share of B (its nll uses nb_train / rows) and group_n by the
    chunk's share of each column normaliser W (its KL weights use group_n / W of the rows it sees); kl0 is counted once.
    eps: (eps0[1], eps_w[T], eps_v[T,d]) or None (closed form).  Returns loss, pred, and with grads: the gradient of every
    parameter, of the flat priors, and dloss/dpred (g_row)."""
    from oracle import vfm_oracle as O
    case, B, F, d, x, y, nb_occ = pb["case"], pb["B"], pb["F"], pb["d"], pb["x"], pb["y"], pb["nb_occ"]
    leaf = lambda a_: torch.tensor(np.asarray(a_, np.float64), requires_grad=grads)
    Pt = {k: leaf(v) for k, v in pb["P"].items()}
    flat = leaf(pb["pri"]) if case.priors else None
    prt = split_priors(flat, F, d) if case.priors else None
    eps_t = tuple(torch.as_tensor(np.asarray(e, np.float64)) for e in eps) if eps is not None else None
    W_full = (1.0 / nb_occ[x].astype(np.float64)).sum(0)
    rows = max(1, chunk_elems // (F * d))
    loss, pred, g_row = 0.0, [], []
    with torch.set_grad_enabled(grads):
        for lo in range(0, B, rows):
            hi = min(B, lo + rows)
            xc = x[lo:hi]
            Wc = (1.0 / nb_occ[xc].astype(np.float64)).sum(0)
            r = O.variant_elbo(Pt, xc, y[lo:hi], nb_occ, pb["hi"], pb["gn"] * Wc / W_full, pb["nb_train"] * (hi - lo) / B,
                               case.objective, priors=prt, values=None if pb["vals"] is None else pb["vals"][lo:hi],
                               eps=eps_t, output=case.output)
            part = r["loss"] if lo == 0 else r["loss"] - r["kl0"]
            if grads:
                r["pred"].retain_grad()
                part.backward()
                g_row.append(r["pred"].grad.numpy())
            loss += float(part.detach())
            pred.append(r["pred"].detach().numpy())
    out = {"loss": loss, "pred": np.concatenate(pred)}
    if grads:
        out["g_row"] = np.concatenate(g_row)
        out["g_entity"], out["g_bias"] = Pt["entity_params"].grad.numpy(), Pt["bias_params"].grad.numpy()
        out["g_scalars"] = np.array([0.0 if Pt[k].grad is None else Pt[k].grad.numpy()[0]      # (alpha: unused by Bernoulli)
                                     for k in ("alpha", "global_bias_mean", "global_bias_scale")])
        out["g_priors"] = flat.grad.numpy() if case.priors else None
    return out


def prior_terms(pb):
    """The per-entity terms of the prior gradients in fp64 (the KL gradients of oracle.variant_elbo's `kl`, weighted by
    group_n / W * count / nb_occ), summed and abs-summed per group, in the layout of the flat prior vector."""
    F, d, T, x, nb_occ, P, pri = pb["F"], pb["d"], pb["T"], pb["x"], pb["nb_occ"], pb["P"], pb["pri"].astype(np.float64)
    G = F
    W = (1.0 / nb_occ[x].astype(np.float64)).sum(0)
    cnt = np.bincount(x.reshape(-1), minlength=T).astype(np.float64)
    tot, ab = np.zeros(pri.size), np.zeros(pri.size)
    pv = 2 + 2 * G

    def pair(mu, sg, pm, ps_raw, c):
        ps, dm = np.abs(ps_raw), mu - pm
        return c * (-dm / ps ** 2), c * np.sign(ps_raw) * (1.0 / ps - (sg ** 2 + dm ** 2) / ps ** 3)

    lo = 0
    for g_, hi in enumerate(pb["hi"]):
        c = pb["gn"][g_] / W[g_] * cnt[lo:hi] / nb_occ[lo:hi]
        bia, ent = P["bias_params"][lo:hi].astype(np.float64), P["entity_params"][lo:hi].astype(np.float64)
        tm, ts = pair(bia[:, 0], np.abs(bia[:, 1]), pri[2 + g_], pri[2 + G + g_], c)
        tot[2 + g_], ab[2 + g_], tot[2 + G + g_], ab[2 + G + g_] = tm.sum(), np.abs(tm).sum(), ts.sum(), np.abs(ts).sum()
        sm, ss = slice(pv + g_ * d, pv + (g_ + 1) * d), slice(pv + G * d + g_ * d, pv + G * d + (g_ + 1) * d)
        tm, ts = pair(ent[:, :d], np.abs(ent[:, d:]), pri[sm], pri[ss], c[:, None])
        tot[sm], ab[sm], tot[ss], ab[ss] = tm.sum(0), np.abs(tm).sum(0), ts.sum(0), np.abs(ts).sum(0)
        lo = hi
    m0, sg0 = float(P["global_bias_mean"][0]), abs(float(P["global_bias_scale"][0]))
    tm, ts = pair(m0, sg0, pri[0], pri[1], 1.0)
    ps = abs(pri[1])
    tot[0], ab[0], tot[1], ab[1] = tm, abs(tm), ts, 1.0 / ps + (sg0 ** 2 + (m0 - pri[0]) ** 2) / ps ** 3
    return tot, ab


def scalar_terms(pb, ref, e0):
    """sum|terms| of the three scalar gradients (alpha, m0, s0) from the oracle's dloss/dpred_r and its own totals."""
    case, P, B = pb["case"], pb["P"], pb["B"]
    alpha, s0 = float(P["alpha"][0]), float(P["global_bias_scale"][0])
    a, s = abs(alpha), pb["nb_train"] / B
    g, want = ref["g_row"], ref["g_scalars"]
    cf = case.objective == "closed_form"
    # alpha: sign(alpha) s (sum_r at_r - B / (2a)) with at_r >= 0, so sum|terms| = s sum at_r + s B / (2a)
    ab_a = (np.sign(alpha) * want[0] + s * B / a) if case.output == "reg" else 0.0
    # m0: sum_r g_r + dKL0/dm0
    ab_m = np.abs(g).sum() + abs(want[1] - g.sum())
    # s0: sign(s0) (e0 sum_r g_r [sampled] + 2 h sg0 B [closed form] + dKL0/dsg0)
    lead = (0.0 if cf else e0 * g.sum()) + (s * a * abs(s0) * B if cf else 0.0)
    ab_s = (0.0 if cf else abs(e0) * np.abs(g).sum()) + (s * a * abs(s0) * B if cf else 0.0) + abs(np.sign(s0) * want[2] - lead)
    return np.array([ab_a, ab_m, ab_s])


# --------------------------------------------------------------------------------------------------------------- the test
def _ratio(err, bound):
    return float(np.max(err / np.maximum(bound, 1e-300)))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_variant_kernels_past_their_grid_caps(case):
    from vae_amd import ops, _lib
    from vae_amd.variants import variant_forward, variant_backward, priors_len
    dev = torch.device("cuda:0")
    assert os.environ.get("VFM_VARIANT_SCALAR", "0") == "0", "d % 8 == 0 would go through the scalar pair (use_var8)"
    pb = build_problem(case)
    B, T, F, d, x, P = pb["B"], pb["T"], pb["F"], pb["d"], pb["x"], pb["P"]
    n_wg, odd_seen, even_seen = list_classes(d, T, x)
    assert n_wg >= 1 and odd_seen and even_seen, (n_wg, odd_seen, even_seen)
    spec = ops.Spec(T=T, F=F, d=d, group_hi=tuple(int(v) for v in pb["hi"]), group_n=tuple(pb["gn"]), nb_train=pb["nb_train"],
                    likelihood=_lib.LIK_NORMAL if case.output == "reg" else _lib.LIK_BERNOULLI)
    ent, bia = torch.tensor(P["entity_params"], device=dev), torch.tensor(P["bias_params"], device=dev)
    scal = torch.tensor(np.concatenate([P["alpha"], P["global_bias_mean"], P["global_bias_scale"]]), device=dev)
    inv_occ = ops.inv_occ_from_counts(torch.tensor(pb["nb_occ"], device=dev))
    x_t = torch.tensor(x, device=dev).to(torch.int32 if case.id32 else torch.int64).contiguous()
    plan = ops.BatchPlan(spec, x_t, torch.tensor(pb["y"], device=dev), inv_occ)
    assert plan.id_bits == (32 if case.id32 else 64)
    pri = torch.tensor(pb["pri"], device=dev) if case.priors else None
    assert pri is None or pri.numel() == priors_len(F, d)
    v_t = torch.tensor(pb["vals"], device=dev) if case.values else None
    one = torch.ones(1, device=dev)

    def run():
        st_ = variant_forward(plan, case.objective, ent, bia, scal, inv_occ, priors=pri, values=v_t, seed=pb["seed"],
                              step=pb["step"])
        return st_, variant_backward(plan, st_, ent, bia, scal, inv_occ, one)

    st, grads = run()
    g_ent, g_bias, g_sc, g_pr = grads
    ee, eb, eg = (t.cpu().numpy() for t in ops.philox_eps(spec, seed=pb["seed"], step=pb["step"], device=dev))
    ref = oracle_eval(pb, (eg, eb, ee) if case.objective == "sampled" else None)
    assert np.isfinite(ref["loss"]) and np.isfinite(ref["pred"]).all()

    checks = []                                                      # (name, error / bound)
    checks.append(("loss", abs(st["loss3"][0].item() - ref["loss"]) / abs(ref["loss"]) / LOSS_TOL))
    checks.append(("pred", rel_err(st["pred"].cpu().numpy(), ref["pred"]) / PRED_TOL))
    cnt = np.bincount(x.reshape(-1), minlength=T)
    cold = (cnt >= 1) & (cnt <= 2)
    ge, gb = g_ent.cpu().numpy(), g_bias.cpu().numpy()
    for name, got, want in (("g_entity", ge, ref["g_entity"]), ("g_bias", gb, ref["g_bias"])):
        checks.append((name, rel_err(got, want) / TABLE_TOL))
        checks.append((name + " cold rows", rel_err(got[cold], want[cold]) / TABLE_TOL))
        lo = 0
        for g_, hi in enumerate(pb["hi"]):
            checks.append(("%s group %d" % (name, g_), rel_err(got[lo:hi], want[lo:hi]) / TABLE_TOL))
            lo = hi
    gam_s = n_chain_scalars() * U24
    ab = scalar_terms(pb, ref, float(eg[0]))
    err = np.abs(g_sc.cpu().numpy().astype(np.float64) - ref["g_scalars"])
    bound = SCALAR_REL * np.abs(ref["g_scalars"]) + gam_s * ab
    for i, name in enumerate(("g_alpha", "g_m0", "g_s0")):
        checks.append((name, 0.0 if err[i] == 0.0 else err[i] / bound[i]))
    if case.priors:
        tot, pab = prior_terms(pb)
        want = ref["g_priors"]
        assert np.all(np.abs(tot - want) <= 1e-9 * pab + 1e-12), "the fp64 terms do not add up to the oracle's gradient"
        gam_p = n_chain_priors(d, T, pb["sizes"]) * U24
        err = np.abs(g_pr.cpu().numpy().astype(np.float64) - want)
        bound = PRIOR_REL * np.abs(want) + gam_p * pab
        pv = 2 + 2 * F
        for name, sl in (("g_prior global", slice(0, 2)), ("g_prior w", slice(2, pv)), ("g_prior v mean", slice(pv, pv + F * d)),
                         ("g_prior v scale", slice(pv + F * d, None))):
            checks.append((name, _ratio(err[sl], bound[sl])))
            checks.append((name + " (sum part alone)", _ratio(err[sl], gam_p * pab[sl])))
    for name, r in checks:
        print("SCALE %-28s %-30s error/bound %.4f" % (case.id, name, r))
    for name, r in checks:
        if not name.endswith("(sum part alone)"):                    # (a figure for the table; the assertion is the full bound)
            assert r <= 1.0, (case.id, name, r)

    # untouched entities: exact zero rows
    untouched = cnt == 0
    assert untouched.sum() > 0
    assert not ge[untouched].any() and not gb[untouched].any()

    # prediction-only launch on a plan without y: same kernel, seed and step -> the same bits
    plan0 = ops.BatchPlan(spec, x_t, None, None)
    p0 = variant_forward(plan0, case.objective, ent, bia, scal, None, priors=pri, values=v_t, seed=pb["seed"], step=pb["step"],
                         train=False)
    assert p0["loss3"] is None and torch.equal(p0["pred"], st["pred"])

    # the lane-group kernels' gradients do not depend on the scheduling (more than one chunk row per group here)
    if family(d) == "lane" and case.priors:
        _, again = run()
        for a_, b_, name in zip(grads, again, ("entity", "bias", "scalars", "priors")):
            assert torch.equal(a_, b_), name
