"""Fused top-k ranking (include/vfm_rank.h) at the ML-20M shape against the torch fp32 composition.

One JSON line per strategy: 8,192 users, all 26,744 items, d = 128, k = 10, every user with an exclusion list of
ML-20M's size (train ratings per user: 80 % of 20,000,263 over 138,493 users, about 116; drawn geometric, at least 16).
Times are HIP-event medians over `--reps` launches after `--warmup` launches; the ranking is timed at the op (the
workspace and the exclusion CSR made once, outside the loop), the composition as mm + bias terms + masking + topk.
Effective TF/s = 2 U M K / time, K = d (top), 2d (variance), 3d (mean); random runs no GEMM."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=8192)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--strategies", default="top,variance,mean,random")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    from vae_amd import _lib, ops, rank
    from vae_amd.model import VFM
    N, M, d, U, k = 138_493, 26_744, args.d, args.users, args.k
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m = VFM(N, M, d, output="class", device=dev)
    with torch.no_grad():
        m._flat.mul_(0.3)
    g = torch.Generator(device=dev).manual_seed(1)
    users = torch.randperm(N, device=dev, generator=g)[:U].sort().values
    lens = (torch.rand(U, device=dev, generator=g).log() * (-(116 - 16))).long() + 16        # geometric-like, mean ~116
    ex_u = torch.repeat_interleave(users, lens)
    ex_i = N + torch.randint(0, M, (ex_u.numel(),), device=dev, generator=g)
    ptr, ex_items = rank.exclusion_csr(users, torch.stack([ex_u, ex_i], 1), m.T)
    ent, bia, scal = m._views(m._flat)
    o = _lib.ops()
    f32 = dict(dtype=torch.float32, device=dev)
    out = [torch.empty(U, k, dtype=torch.int64, device=dev)] + [torch.empty(U, k, **f32) for _ in range(3)]
    mask_rows = torch.repeat_interleave(torch.arange(U, device=dev), ptr[1:] - ptr[:-1])
    mask_cols = ex_items - N
    for strategy in args.strategies.split(","):
        code = rank.STRATEGIES[strategy]
        ws = torch.empty(o.rank_workspace_bytes(U, M, d, k, code, 0), dtype=torch.uint8, device=dev)

        def run():
            o.rank_items(users, None, M, N, ptr, ex_items, ent, bia, scal, ws, *out, 2, k, code, 0, 7, 0)
        ms, ms_min = timed(run, args.warmup, args.reps)
        K = {"top": d, "variance": 2 * d, "mean": 3 * d, "random": 0}[strategy]
        tf = 2.0 * U * M * K / (ms * 1e-3) / 1e12 if K else None
        rec = {"strategy": strategy, "users": U, "items": M, "d": d, "k": k, "excluded": int(ex_items.numel()),
               "ms": round(ms, 4), "ms_min": round(ms_min, 4), "tflops": None if tf is None else round(tf, 2)}
        if not args.no_torch:
            mu, sg = ent[:, :d], ent[:, d:].abs()
            mu_u, mu_i, sg_u, sg_i = mu[users], mu[N:], sg[users], sg[N:]
            cu, ci = (scal[1] + bia[users, 0])[:, None], bia[N:, 0][None, :]
            vu, vi = (scal[2].abs() ** 2 + bia[users, 1] ** 2)[:, None], (bia[N:, 1] ** 2)[None, :]
            A2, B2 = torch.cat([mu_u ** 2, sg_u ** 2], 1), torch.cat([sg_i ** 2, mu_i ** 2 + sg_i ** 2], 1)

            def comp():
                if strategy == "random":
                    S = torch.rand(U, M, device=dev)
                else:
                    if strategy in ("top", "mean"):
                        Sm = torch.addmm(cu + ci, mu_u, mu_i.T)
                    if strategy in ("variance", "mean"):
                        Sv = torch.addmm(vu + vi, A2, B2.T)
                    S = Sm if strategy == "top" else Sv if strategy == "variance" else \
                        -Sm.abs() / torch.sqrt(1 + math.pi / 8 * Sv)
                S[mask_rows, mask_cols] = -float("inf")
                return torch.topk(S, k, dim=1)
            tms, tms_min = timed(comp, args.warmup, args.reps)
            rec.update({"torch_ms": round(tms, 4), "torch_tflops": None if not K else round(2.0 * U * M * K / (tms * 1e-3) / 1e12, 2),
                        "speedup": round(tms / ms, 2)})
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
