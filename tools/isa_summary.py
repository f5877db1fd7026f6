#!/usr/bin/env python3
"""Instruction-class counts of named kernel instances from the gfx950 ISA hipcc emits (`--offload-device-only -S`):
the evidence behind "hand-written CDNA4, no scratch, counted waits" without asking the reader to recompile.
usage: tools/isa_summary.py [--only SUBSTRING] [--every SUBSTRING] > profiles/rNN_isa_summary.txt   (cross-compiles; no GPU
needed; ~3 minutes; --only keeps the entries whose translation unit or instance name holds SUBSTRING; --every adds one line
(registers, scratch, LDS, waves per SIMD) for EVERY kernel instance of the listed units whose path holds SUBSTRING)"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vae_amd", "csrc")
# (translation unit, extra flags, substring of the demangled instance, what it is)
WANT = [
    ("vfm_fwd2.hip", [], "k_fwd2<16, true, 0, 1, true, 0, true>", "cfg3 forward (d = 128, Philox, training, int64 ids, |.| link, packed records)"),
    ("vfm_fwd2.hip", [], "k_fwd2<4, false, 0, 1, true, 0, true>", "cfg2 forward (d = 20)"),
    ("vfm_fwdg.hip", [], "k_fwdg<32, true, 0, 1, true, 0, true>", "cfg5 forward (F = 32, d = 256: fields split over lane groups)"),
    ("vfm_bwd.hip", ["-ffp-contract=on", "-DVFM_BWD_PART=1"], "k_bwd<32, 1, 4, 0, 1, 0, 0, false, false, true>", "cfg3 fused backward + dense Adam, look-ahead form"),
    ("vfm_bwd.hip", ["-ffp-contract=on", "-DVFM_BWD_PART=1"], "k_bwd<64, 1, 4, 0, 1, 0, 0, false, false, true>", "cfg5 fused backward + dense Adam, look-ahead form"),
    ("vfm_bwd.hip", ["-ffp-contract=on", "-DVFM_BWD_PART=1"], "k_bwd<32, 1, 4, 0, 1, 0, 0, false, true, true>", "pipelined step's backward in the look-ahead form (data-file-order batches; the rows exchange)"),
    ("vfm_bwd.hip", ["-ffp-contract=on", "-DVFM_BWD_PART=1"], "k_bwd_small<8, 0>", "cfg2 one-launch backward + dense Adam (a wave per table row)"),
    ("vfm_bwd.hip", ["-ffp-contract=on", "-DVFM_BWD_PART=1"], "k_bwd_small<32, 0>", "the same at d = 128"),
    ("vfm_bwd.hip", ["-ffp-contract=on", "-DVFM_BWD_PART=1"], "k_bwd<32, 1, 4, 0, 1, 2, 0, false, false, false>", "multi-rank apply stage (epilogue + Adam from the summed statistics)"),
    ("vfm_abi.hip", ["-ffp-contract=on"], "k_heavy<32, 1, 4>", "pre-reduction of the long lists' work items (eight occurrences in flight, the next eight's row numbers fetched under them)"),
    ("vfm_index.hip", [], "k_index_keys", "index build: ids -> keys, first digit counts, batch normalisers"),
    ("vfm_index.hip", [], "k_radix_scatter<true>", "index build: last radix pass (writes occ_rows / occ_other)"),
    ("vfm_index.hip", [], "k_index_count<true>", "index build: occ_ptr by LDS-staged lower bounds + per-chunk counts (256-thread workgroups)"),
    ("vfm_index.hip", [], "k_index_write<false>", "index build: heavy lists, work items, touched list, totals, W"),
    # field-form elicitation sessions (a path relative to csrc/; --only elicit_field prints these alone)
    ("../csrc_rank/vfm_elicit_field.hip", ["-ffp-contract=on"], "k_elicit_field<8, 1, 0, false>", "field-form session, d <= 8, closed form, |.|"),
    ("../csrc_rank/vfm_elicit_field.hip", ["-ffp-contract=on"], "k_elicit_field<64, 2, 0, false>", "field-form session, d = 128 (the benchmark shape), closed form, |.|"),
    ("../csrc_rank/vfm_elicit_field.hip", ["-ffp-contract=on"], "k_elicit_field<64, 2, 1, true>", "field-form session, d = 128, sampled, softplus"),
    ("../csrc_rank/vfm_elicit_field.hip", ["-ffp-contract=on"], "k_elicit_field<64, 8, 0, false>", "field-form session, d = 512, closed form, |.|"),
    ("../csrc_rank/vfm_elicit_field.hip", ["-ffp-contract=on"], "k_elicit_field<64, 8, 1, true>", "field-form session, d = 512, sampled, softplus"),
    ("../csrc_rank/vfm_elicit_field.hip", ["-ffp-contract=on"], "k_elicit_ctx_prep", "field-form session: the score's operand pass (a wave per context)"),
    # the two-field session and the fold-in at the same shapes: the three kernels restate one another and are compared instance by instance
    ("../csrc_rank/vfm_elicit.hip", ["-ffp-contract=on"], "k_elicit<8, 1, 0, false>", "two-field session, d <= 8, closed form, |.|"),
    ("../csrc_rank/vfm_elicit.hip", ["-ffp-contract=on"], "k_elicit<64, 2, 0, false>", "two-field session, d = 128, closed form, |.|"),
    ("../csrc_rank/vfm_elicit.hip", ["-ffp-contract=on"], "k_elicit<64, 2, 1, true>", "two-field session, d = 128, sampled, softplus"),
    ("../csrc_rank/vfm_elicit.hip", ["-ffp-contract=on"], "k_elicit<64, 8, 0, false>", "two-field session, d = 512, closed form, |.|"),
    ("../csrc_rank/vfm_elicit.hip", ["-ffp-contract=on"], "k_elicit<64, 8, 1, true>", "two-field session, d = 512, sampled, softplus"),
    ("../csrc_rank/vfm_foldin.hip", ["-ffp-contract=on"], "k_foldin<8, 1, 0, false>", "fold-in, d <= 8, closed form, |.|"),
    ("../csrc_rank/vfm_foldin.hip", ["-ffp-contract=on"], "k_foldin<64, 2, 0, false>", "fold-in, d = 128, closed form, |.|"),
    ("../csrc_rank/vfm_foldin.hip", ["-ffp-contract=on"], "k_foldin<64, 2, 1, true>", "fold-in, d = 128, sampled, softplus"),
    ("../csrc_rank/vfm_foldin.hip", ["-ffp-contract=on"], "k_foldin<64, 8, 0, false>", "fold-in, d = 512, closed form, |.|"),
    ("../csrc_rank/vfm_foldin.hip", ["-ffp-contract=on"], "k_foldin<64, 8, 1, true>", "fold-in, d = 512, sampled, softplus"),
    # the exact sessions: two kernels, one session loop (csrc_rank/vfm_elicit_exact_body.hpp), compared instance by instance
    # (--only elicit_solve --every elicit_solve, and the same for elicit_design: profiles/exact_session_isa*.txt)
    ("../csrc_rank/vfm_elicit_solve.hip", ["-ffp-contract=on"], "k_elicit_solve<8, 1, 0>", "exact session, moment scores, d <= 8, |.|"),
    ("../csrc_rank/vfm_elicit_solve.hip", ["-ffp-contract=on"], "k_elicit_solve<64, 2, 0>", "exact session, moment scores, d = 128 (the benchmark shape), |.|"),
    ("../csrc_rank/vfm_elicit_solve.hip", ["-ffp-contract=on"], "k_elicit_solve<64, 2, 1>", "exact session, moment scores, d = 128, softplus"),
    ("../csrc_rank/vfm_elicit_solve.hip", ["-ffp-contract=on"], "k_elicit_solve<64, 8, 0>", "exact session, moment scores, d = 512, |.|"),
    ("../csrc_rank/vfm_elicit_design.hip", ["-ffp-contract=on"], "k_elicit_design<8, 1, 0>", "exact session, target-aware score, d <= 8, |.|"),
    ("../csrc_rank/vfm_elicit_design.hip", ["-ffp-contract=on"], "k_elicit_design<64, 2, 0>", "exact session, target-aware score, d = 128 (the benchmark shape), |.|"),
    ("../csrc_rank/vfm_elicit_design.hip", ["-ffp-contract=on"], "k_elicit_design<64, 2, 1>", "exact session, target-aware score, d = 128, softplus"),
    ("../csrc_rank/vfm_elicit_design.hip", ["-ffp-contract=on"], "k_elicit_design<64, 8, 0>", "exact session, target-aware score, d = 512, |.|"),
    # the bound session: the same session loop with the bound fold-in's body as the fold of a round
    # (--only elicit_bound --every elicit_bound: profiles/bound_session_isa.txt)
    ("../csrc_rank/vfm_elicit_bound.hip", ["-ffp-contract=on"], "k_elicit_bound<8, 1, 0>", "bound session ('class'), moment scores, d <= 8 (the questionnaire's shape), |.|"),
    ("../csrc_rank/vfm_elicit_bound.hip", ["-ffp-contract=on"], "k_elicit_bound<64, 2, 0>", "bound session, moment scores, d = 128 (the benchmark shape), |.|"),
    ("../csrc_rank/vfm_elicit_bound.hip", ["-ffp-contract=on"], "k_elicit_bound<64, 2, 1>", "bound session, moment scores, d = 128, softplus"),
    ("../csrc_rank/vfm_elicit_bound.hip", ["-ffp-contract=on"], "k_elicit_bound<64, 8, 0>", "bound session, moment scores, d = 512, |.|"),
    # the split bound rounds beside the split exact solve's assembly they are modelled on
    # (--only _split --every _split: profiles/bound_split_isa.txt)
    ("../csrc_rank/vfm_foldin_split.hip", ["-ffp-contract=on"], "k_split_assemble", "split exact solve: a chunk's share of the system (4 x 4 fp64 register tiles)"),
    ("../csrc_rank/vfm_foldin_bound_split.hip", ["-ffp-contract=on"], "k_bsplit_assemble", "split bound rounds: a chunk's weights and its weighted share of the system"),
    ("../csrc_rank/vfm_foldin_bound_split.hip", ["-ffp-contract=on"], "k_bsplit_solve<0>", "split bound rounds: a round's solve of one entity, |.|"),
    ("../csrc_rank/vfm_foldin_bound_split.hip", ["-ffp-contract=on"], "k_bsplit_loss<64, 2, 0>", "split bound rounds: a chunk's share of B_e, d = 128, |.|"),
    # fused Adam step of the ELBO variants (--only variant_step prints these alone; --every variant_step adds one line per instance)
    ("../csrc_var/vfm_variant_step.hip", ["-ffp-contract=on"], "k_vstep<8, 16, 1, true, false, true>", "variant step, d = 128 (the benchmark shape), closed form, learnable priors"),
    ("../csrc_var/vfm_variant_step.hip", ["-ffp-contract=on"], "k_vstep<8, 16, 1, false, true, false>", "variant step, d = 128, sampled objective, feature values, N(0,1) priors"),
    ("../csrc_var/vfm_variant_step.hip", ["-ffp-contract=on"], "k_vstep<8, 64, 2, true, true, true>", "variant step, d = 1024 (two blocks of 8 per lane), closed form, values, priors"),
    ("../csrc_var/vfm_variant_step.hip", ["-ffp-contract=on"], "k_vstep<1, 4, 1, true, false, true>", "variant step, d = 2 (VFMClosedForm's default: one coordinate per lane), closed form, priors"),
    ("../csrc_var/vfm_variant_step.hip", ["-ffp-contract=on"], "k_vstep<1, 64, 16, true, true, true>", "variant step, d % 8 != 0 up to 1024 (sixteen coordinates per lane), closed form, values, priors"),
    ("../csrc_var/vfm_variant_step.hip", ["-ffp-contract=on"], "k_vstep_small", "variant step: partial rows of the prior gradients summed in order + Adam on priors and scalars"),
    ("../csrc_var/vfm_variant_step.hip", ["-ffp-contract=on"], "k_vstep_positions", "variant step: positions of the occurrences (with feature values)"),
]
CLASSES = ["global_load_dwordx4", "global_load_dwordx2", "global_load_dword", "global_store_dwordx4", "global_store_dwordx2",
           "global_store_dword", "ds_read_b128", "ds_write_b128", "ds_read", "ds_write", "s_barrier", "v_pk_fma_f32", "v_pk_mul_f32",
           "v_pk_add_f32", "v_fma_f32", "v_mad_u64_u32", "v_log_f32", "v_sqrt_f32", "v_rcp_f32", "v_sin_f32", "v_cos_f32", "v_exp_f32",
           "v_mov_b32_dpp", "v_add_f32_dpp", "v_permlane", "scratch_", "buffer_", "global_atomic"]


def main():
    hipcc = os.environ.get("HIPCC", "hipcc")
    cache = {}
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
    for tu, extra, inst, what in WANT:
        if only not in tu and only not in inst:
            continue
        if (tu, tuple(extra)) not in cache:
            out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
            subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                            "-DVFM_LINK=0", "--offload-device-only", "-S", os.path.join(CSRC, tu), "-o", out] + extra, check=True,
                           stderr=subprocess.DEVNULL)
            txt = open(out).read()
            os.unlink(out)
            labels = re.findall(r"\n(_Z[^\s:]+):", txt)
            dem = subprocess.run(["c++filt"] + labels, capture_output=True, text=True).stdout.strip().split("\n")
            cache[(tu, tuple(extra))] = (txt, dict(zip(dem, labels)))
        txt, names = cache[(tu, tuple(extra))]
        hit = [(d, l) for d, l in names.items() if inst in d]
        if not hit:
            print(f"## {inst}: not found in {tu}\n")
            continue
        d, label = hit[0]
        body = txt[txt.index("\n" + label + ":"):]
        end = body.index(".Lfunc_end")                    # (a kernel may hold several s_endpgm: early exits)
        meta = body[end: end + 6000]
        body = body[:end]
        ins = [l.strip() for l in body.split("\n") if l.strip() and not l.strip().startswith((".", ";", "//", "_Z")) and not l.strip().endswith(":")]
        ops = collections.Counter(i.split()[0] for i in ins)
        print(f"## {inst}\n{what}   ({tu})")
        g = lambda k: (re.search(r"; " + k + r": (\d+)", meta) or [None, "?"])[1]
        print(f"instructions {len(ins)}; vgprs {g('NumVgprs')}, "
              f"scratch {g('ScratchSize')} bytes/lane, LDS {g('LDSByteSize')} bytes, occupancy {g('Occupancy')} waves/SIMD")
        for c in CLASSES:
            n = sum(v for k, v in ops.items() if k.startswith(c)) if c.endswith("_") or c in ("ds_read", "ds_write", "v_permlane", "global_atomic") else \
                sum(v for k, v in ops.items() if k == c or k.startswith(c + "_e"))
            if n:
                print(f"  {c:<22}{n}")
        waits = collections.Counter(i for i in ins if i.startswith("s_waitcnt"))
        vm = {k: v for k, v in waits.items() if "vmcnt" in k}
        print("  s_waitcnt vmcnt:", ", ".join(f"{k.split('vmcnt')[1].split()[0]}x{v}" for k, v in sorted(vm.items())),
              "  (vmcnt(0) = wait for every load in flight)")
        print()
    every = sys.argv[sys.argv.index("--every") + 1] if "--every" in sys.argv else None
    if every:
        for (tu, extra), (txt, names) in cache.items():
            if every not in tu:
                continue
            print(f"## every kernel instance of {tu}: vgprs / scratch bytes per lane / LDS bytes / waves per SIMD")
            worst = 0
            for d, label in sorted(names.items()):
                body = txt[txt.index("\n" + label + ":"):]
                meta = body[body.index(".Lfunc_end"):][:6000]
                g = lambda k: (re.search(r"; " + k + r": (\d+)", meta) or [None, "?"])[1]
                if g("NumVgprs") == "?":
                    continue                          # (a device function, not a kernel)
                worst = max(worst, int(g("ScratchSize")))
                print(f"  {d.replace('(anonymous namespace)::', '').split('(')[0]:<62} {g('NumVgprs'):>4} {g('ScratchSize'):>4} {g('LDSByteSize'):>6} {g('Occupancy'):>3}")
            print(f"largest scratch of any instance: {worst} bytes\n")


if __name__ == "__main__":
    main()
