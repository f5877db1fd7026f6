"""Field-form ranking (VFM.rank_field, include/vfm_rank.h) against its yardsticks.

Shapes: "ml20m" -- 8,192 (user, format) contexts x all 26,744 items, F = 3, d = 128, k = 10, every context with an
exclusion list of ML-20M's size (about 116, as tools/rank_bench.py draws them); "criteo" -- F = 32, d = 256, 8,192
contexts of 31 entities x a 26,744-entity field, no exclusions.
One JSON line per (shape, strategy), appended to profiles/rank_field_bench.jsonl with --record:
  ms            rank_field at the op (workspace and exclusion CSR made once, outside the loop), HIP-event median
  prep_share    the share of the two operand kernels (k_field_ctx_prep, k_field_cand_prep) in the call's kernel time,
                from a kernel trace of one call (torch.profiler); null if no trace could be taken
  torch_ms      the torch fp32 composition in the same process: query operands, mm, masking, topk
  rank_items_ms rank_items on a two-field model of the same Q, catalog and d (ml20m shape only): the yardstick."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.rank_bench import timed          # noqa: E402


def prep_share(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        tot = prep = 0.0
        for e in prof.key_averages():
            t = float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))
            tot += t
            if "k_field_ctx_prep" in e.key or "k_field_cand_prep" in e.key:
                prep += t
        return round(prep / tot, 4) if tot > 0 else None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml20m,criteo")
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--strategies", default="top,variance,mean,random")
    ap.add_argument("--record", action="store_true", help="append to profiles/rank_field_bench.jsonl")
    args = ap.parse_args()
    from vae_amd import _lib, rank
    from vae_amd.model import VFM
    dev = torch.device("cuda")
    o = _lib.ops()
    Q, k, M = args.queries, args.k, 26_744
    f32 = dict(dtype=torch.float32, device=dev)
    out = [torch.empty(Q, k, dtype=torch.int64, device=dev)] + [torch.empty(Q, k, **f32) for _ in range(3)]
    for shape in args.shapes.split(","):
        torch.manual_seed(0)
        g = torch.Generator(device=dev).manual_seed(1)
        if shape == "ml20m":
            sizes, d, field = [138_493, M, 4], 128, 1
        else:
            sizes, d, field = [M] + [1000] * 31, 256, 0
        F = len(sizes)
        m = VFM(field_sizes=sizes, embedding_size=d, output="class", device=dev)
        with torch.no_grad():
            m._flat.mul_(0.3 if shape == "ml20m" else 0.1)
        off = [sum(sizes[:f]) for f in range(F)]
        lo = off[field]
        ctx = torch.stack([off[f] + torch.randint(0, sizes[f], (Q,), device=dev, generator=g) for f in range(F)], 1)
        ctx[:, field] = 0
        ctx = torch.unique(ctx, dim=0)
        Qn = ctx.shape[0]
        ptr = ex_items = None
        if shape == "ml20m":
            lens = (torch.rand(Qn, device=dev, generator=g).log() * (-(116 - 16))).long() + 16
            ex = torch.repeat_interleave(ctx, lens, 0)
            ex[:, field] = lo + torch.randint(0, M, (ex.shape[0],), device=dev, generator=g)
            ptr, ex_items = rank.field_exclusion_csr(ctx, ex, field, [f for f in range(F) if f != field], m.T)
            mask_rows = torch.repeat_interleave(torch.arange(Qn, device=dev), ptr[1:] - ptr[:-1])
            mask_cols = ex_items - lo
        ent, bia, scal = m._views(m._flat)
        qkey = ctx[:, 1 if field == 0 else 0].contiguous()
        cols = [f for f in range(F) if f != field]
        for strategy in args.strategies.split(","):
            code = rank.STRATEGIES[strategy]
            ws = torch.empty(o.rank_field_workspace_bytes(Qn, M, F, d, k, code, 0), dtype=torch.uint8, device=dev)
            outs = [t[:Qn] for t in out]

            def run():
                o.rank_field(ctx, field, qkey, None, M, lo, ptr, ex_items, ent, bia, scal, ws, *outs, k, code, 0, 7, 0)
            ms, ms_min = timed(run, args.warmup, args.reps)
            rec = {"shape": shape, "strategy": strategy, "queries": Qn, "catalog": M, "F": F, "d": d, "k": k,
                   "excluded": 0 if ex_items is None else int(ex_items.numel()), "ms": round(ms, 4),
                   "ms_min": round(ms_min, 4), "prep_share": prep_share(run)}
            mu, s2 = ent[:, :d], ent[:, d:].abs() ** 2
            mu_c, s2_c = mu[lo:lo + M], s2[lo:lo + M]

            def comp():
                e, b = ent[ctx[:, cols]], bia[ctx[:, cols]]                     # [Q, F-1, 2d]: the gather is part of it
                mq, sq = e[..., :d], e[..., d:].abs() ** 2
                Mq, Aq = mq.sum(1), sq.sum(1)
                if strategy == "random":
                    S = torch.rand(Qn, M, device=dev)
                else:
                    if strategy in ("top", "mean"):
                        cm = scal[1] + b[..., 0].sum(1) + 0.5 * (Mq ** 2 - (mq ** 2).sum(1)).sum(1)
                        Sm = torch.addmm(cm[:, None] + bia[lo:lo + M, 0][None, :], Mq, mu_c.T)
                    if strategy in ("variance", "mean"):
                        dm = Mq[:, None, :] - mq
                        cv = (scal[2] ** 2 + (b[..., 1] ** 2).sum(1)
                              + (0.5 * (Aq ** 2 - (sq ** 2).sum(1)) + (sq * dm ** 2).sum(1)).sum(1))
                        A3 = torch.cat([Aq, Aq + Mq ** 2, 2 * (sq * dm).sum(1)], 1)
                        B3 = torch.cat([mu_c ** 2, s2_c, mu_c], 1)
                        Sv = torch.addmm(cv[:, None] + (bia[lo:lo + M, 1] ** 2)[None, :], A3, B3.T)
                    S = Sm if strategy == "top" else Sv if strategy == "variance" else \
                        -Sm.abs() / torch.sqrt(1 + math.pi / 8 * Sv)
                if ex_items is not None:
                    S[mask_rows, mask_cols] = -float("inf")
                return torch.topk(S, k, dim=1)
            tms, _ = timed(comp, args.warmup, args.reps)
            rec.update({"torch_ms": round(tms, 4), "speedup_vs_torch": round(tms / ms, 2)})
            if shape == "ml20m":
                users = torch.unique(ctx[:, 0])
                m2 = VFM(sizes[0], M, d, output="class", device=dev)
                e2, b2, s2f = m2._views(m2._flat)
                ws2 = torch.empty(o.rank_workspace_bytes(users.numel(), M, d, k, code, 0), dtype=torch.uint8, device=dev)
                U = users.numel()
                p2, x2 = rank.exclusion_csr(users, torch.stack([ex[:, 0], ex[:, 1]], 1), m2.T)
                outs2 = [t[:U] for t in out]

                def run2():
                    o.rank_items(users, None, M, sizes[0], p2, x2, e2, b2, s2f, ws2, *outs2, 2, k, code, 0, 7, 0)
                rms, _ = timed(run2, args.warmup, args.reps)
                rec.update({"rank_items_ms": round(rms, 4), "rank_items_users": U, "vs_rank_items": round(ms / rms, 2)})
                del m2, ws2
            print(json.dumps(rec), flush=True)
            if args.record:
                with open(os.path.join(ROOT, "profiles", "rank_field_bench.jsonl"), "a") as f:
                    f.write(json.dumps(rec) + "\n")
        del m


if __name__ == "__main__":
    main()
