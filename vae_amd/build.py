"""In-tree build of the native libraries (hipcc cross-compiles gfx950 without a GPU)."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def sources_digest() -> str:
    """sha1 over the kernel sources (csrc/*.hip, *.hpp, *.cpp + include/vfm_hip.h), in name order: ties measured
    figures (profiles/latest_traffic.json) to the code they were measured on."""
    import hashlib
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "csrc")
    files = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".hpp", ".cpp")))
    files.append(os.path.join(os.path.dirname(here), "include", "vfm_hip.h"))
    h = hashlib.sha1()
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()


def _stale(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


# translation units of libvfm_hip.so: (source, object suffix, extra flags).  The row kernels are
# compiled once per link function (vfm-torch.py:125-126: |.| and softplus).
# -ffp-contract=on (a*b+c fuses only inside one source expression) for the units holding the update arithmetic: under
# hipcc's default ("fast": fusion across statements, decided after inlining) two template instances of k_bwd rounded
# the same source differently in the last bit, and the lazy / look-ahead step forms are specified as BITWISE the dense one.
_EXACT = ["-ffp-contract=" + os.environ.get("VFM_FP_CONTRACT", "on")]      # (the variable: A/B builds only)
# The softplus link (the reference's own dead assignment, vfm-torch.py:125) is served by the GENERAL kernels only (k_fwd,
# k_bwd); the specialised forward kernels and the record step are built for |.| (:126, the assignment in effect).  vfm_bwd.hip
# is compiled in two parts per link (VFM_BWD_PART: gradient / statistics forms, fused-Adam forms) so that no single unit
# dominates the wall time of a clean build.
_UNITS = [("vfm_abi.hip", "", _EXACT), ("vfm_index.hip", "", []), ("vfm_variants.hip", "", []),
          ("vfm_fwd.hip", "_abs", ["-DVFM_LINK=0"]), ("vfm_fwd.hip", "_softplus", ["-DVFM_LINK=1"]),
          ("vfm_fwd2.hip", "_abs", ["-DVFM_LINK=0"]), ("vfm_fwd2m.hip", "_abs", ["-DVFM_LINK=0"]),
          ("vfm_fwdg.hip", "_abs", ["-DVFM_LINK=0"]),
          ("vfm_bwd.hip", "0_abs", ["-DVFM_LINK=0", "-DVFM_BWD_PART=0"] + _EXACT),
          ("vfm_bwd.hip", "1_abs", ["-DVFM_LINK=0", "-DVFM_BWD_PART=1"] + _EXACT),
          ("vfm_bwd.hip", "0_softplus", ["-DVFM_LINK=1", "-DVFM_BWD_PART=0"] + _EXACT),
          ("vfm_bwd.hip", "1_softplus", ["-DVFM_LINK=1", "-DVFM_BWD_PART=1"] + _EXACT),
          # preference elicitation (include/vfm_rank.h): kept out of csrc/ so that sources_digest() -- the training
          # kernels the committed traffic profile was measured on -- does not move with it.  Contraction off: the explicit
          # fmaf chains of the pair moments are the MFMA chains of the ranking kernel, bit for bit.
          ("csrc_rank/vfm_rank.hip", "", ["-ffp-contract=off"]),
          # held-out ranking evaluation: the same score tiles (csrc_rank/vfm_rank_tile.hpp), hence the same flag
          ("csrc_rank/vfm_rank_eval.hip", "", ["-ffp-contract=off"]),
          # field-form ranking (any number of fields): operands of its own for the same tiles and scan, the same flag
          ("csrc_rank/vfm_rank_field.hip", "", ["-ffp-contract=off"]),
          # fold-in (include/vfm_foldin.h): outside csrc/ for the same reason; it includes csrc/'s Philox stream and link
          # helpers, so its draws and links are those of the training kernels.  csrc_rank/vfm_foldin_body.hpp holds the
          # per-entity body and the host helpers (shape dispatch, FoldArgs fill, prep launch) of this unit and the next three
          ("csrc_rank/vfm_foldin.hip", "", _EXACT),
          # exact fold-in (vfm_foldin_solve_f32): the same prep and, for the loss, the same final pass (vfm_foldin_body.hpp),
          # hence the same flag
          ("csrc_rank/vfm_foldin_solve.hip", "", _EXACT),
          # elicitation sessions (include/vfm_elicit.h): the fold-in's body (csrc_rank/vfm_foldin_body.hpp) and the pair
          # scores of vfm_rank_tile.hpp in one kernel; the host side it shares with the field form is
          # csrc_rank/vfm_elicit_host.hpp.  The fold-in's flag: its body is defined under contraction `on`; the pair
          # functions pin `off` with a pragma of their own, so the scores stay those of vfm_rank.hip bit for bit
          ("csrc_rank/vfm_elicit.hip", "", _EXACT),
          # the field form of the sessions (any number of fields): the same body with the field-form scores of
          # csrc_rank/vfm_field_ctx.hpp, which pin `off` themselves; a unit of its own so that the two compile side by side
          ("csrc_rank/vfm_elicit_field.hip", "", _EXACT),
          # the exact field-form session (vfm_elicit_solve_f32): the session loop and host path of
          # csrc_rank/vfm_elicit_exact_body.hpp with the field form's scores (csrc_rank/vfm_elicit_field_score.hpp); the
          # loop runs the exact fold-in's body (csrc_rank/vfm_foldin_solve_body.hpp), hence its flag.  This unit and the
          # next, and vfm_elicit_bound.hip below, each hold their session under a field prior as well
          # (include/vfm_elicit_prior.h: the PRIOR = true instantiation beside the parent's, one host path for both)
          ("csrc_rank/vfm_elicit_solve.hip", "", _EXACT),
          # target-aware elicitation (include/vfm_design.h): the same session loop and host path with the score of
          # csrc_rank/vfm_design_score.hpp, which pins its own contraction expression by expression; the same flag, and a
          # unit of its own so that the two compile side by side
          ("csrc_rank/vfm_elicit_design.hip", "", _EXACT),
          # fused Adam step of the ELBO variants (include/vfm_variant_step.h): outside csrc/ for the same reason.  It
          # restates the backward of vfm_variants.hip and holds update arithmetic, hence the flag of the Adam units
          ("csrc_var/vfm_variant_step.hip", "", _EXACT),
          # split exact solve (include/vfm_sweep.h): the exact fold-in's prep, factorisation and rounding
          # (csrc_rank/vfm_foldin_solve_body.hpp) with a chunk-parallel assembly in front, hence its flag
          ("csrc_rank/vfm_foldin_split.hip", "", _EXACT),
          # bound fold-in (include/vfm_bound.h): the exact fold-in's preps, factorisation and rounding
          # (csrc_rank/vfm_foldin_solve_body.hpp) under weights of the Jaakkola-Jordan bound, and the fold-in's fp32 row
          # moments (csrc_rank/vfm_foldin_body.hpp) for the loss, hence their flag
          ("csrc_rank/vfm_foldin_bound.hip", "", _EXACT),
          # bound elicitation session (include/vfm_bound.h: vfm_elicit_bound_f32): the exact sessions' loop and host path
          # (csrc_rank/vfm_elicit_exact_body.hpp) with the bound fold-in's body (csrc_rank/vfm_foldin_bound_body.hpp) as
          # the fold of a round, hence their flag
          ("csrc_rank/vfm_elicit_bound.hip", "", _EXACT),
          # split bound rounds (include/vfm_bound_sweep.h): the bound fold-in's preps and weights with the split solve's
          # chunk-parallel assembly in front of the same factorisation and rounding, hence their flag
          ("csrc_rank/vfm_foldin_bound_split.hip", "", _EXACT),
          # implicit-feedback solves (include/vfm_implicit.h): the split solve's tile assembly over a field's whole
          # catalog and the exact fold-in's factorisation and rounding (csrc_rank/vfm_foldin_solve_body.hpp), hence its
          # flag; the unit holds the solve under a field prior (include/vfm_implicit_prior.h) and with a weight per
          # observed row (include/vfm_implicit_weights.h) as well
          ("csrc_rank/vfm_implicit.hip", "", _EXACT),
          # implicit elicitation session (include/vfm_elicit_implicit.h): the exact sessions' loop and host path
          # (csrc_rank/vfm_elicit_exact_body.hpp) with the implicit solve's per-entity body
          # (csrc_rank/vfm_implicit_body.hpp) as the fold of a round, hence their flag; the unit holds the session under a
          # field prior as well
          ("csrc_rank/vfm_elicit_implicit.hip", "", _EXACT)]
RANK_DIR = os.path.join(HERE, "csrc_rank")
VAR_DIR = os.path.join(HERE, "csrc_var")
# the public headers beside include/vfm_hip.h (vfm_foldin_ops.cpp holds the ops of foldin, sweep, bound_sweep, prior,
# bound_prior, implicit, implicit_prior, implicit_weights and vfm_bound.h's fold-in; vfm_elicit_ops.cpp holds vfm_bound.h's session, the
# session of elicit_implicit and, with vfm_design_ops.cpp, the ops of elicit_prior)
PUBLIC_HDRS = tuple(os.path.join(ROOT, "include", f"vfm_{n}.h")
                    for n in ("rank", "foldin", "elicit", "design", "variant_step", "sweep", "bound", "bound_sweep", "prior",
                              "bound_prior", "elicit_prior", "implicit", "implicit_prior", "implicit_weights", "elicit_implicit"))
# the TORCH_LIBRARY fragments linked into the shim beside csrc/vfm_torch_ops.cpp, and the header they share: host C++
# only, so it is no source of libvfm_hip.so.  One file per family
OPS_SOURCES = tuple(os.path.join(RANK_DIR, f"vfm_{n}_ops.cpp") for n in ("rank", "foldin", "elicit", "design"))
OPS_HDR = os.path.join(RANK_DIR, "vfm_ops_common.hpp")


def _unit_path(src):
    """A unit named by a bare file name lives in csrc/, one with a directory part relative to the package."""
    return os.path.join(HERE, src) if "/" in src else os.path.join(HERE, "csrc", src)


def _unit_obj(objdir, src, suffix):
    return os.path.join(objdir, os.path.splitext(os.path.basename(src))[0] + suffix + ".o")


def _rank_sources():
    """What libvfm_hip.so is built from outside csrc/: the public headers and every .hip / .hpp of csrc_rank/ and
    csrc_var/ but the shim's own header."""
    return ([*PUBLIC_HDRS] +
            [f for d in (RANK_DIR, VAR_DIR) for f in sorted(os.path.join(d, n) for n in os.listdir(d))
             if f.endswith((".hip", ".hpp")) and f != OPS_HDR])


def build_hip_library(force=False, verbose=False):
    """libvfm_hip.so: kernels + C ABI (include/vfm_hip.h), gfx950 only.  The translation units are
    compiled in parallel (hipcc -c) and linked into one shared object."""
    csrc = os.path.join(HERE, "csrc")
    hdr = os.path.join(ROOT, "include", "vfm_hip.h")
    parts = [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.endswith((".hpp", ".hip"))] + _rank_sources()
    out = os.path.join(HERE, "libvfm_hip.so")
    if not force and not _stale(out, [hdr, os.path.abspath(__file__)] + parts):      # (this file holds the compile flags)
        return out
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    common = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-fvisibility-inlines-hidden",
              "-I" + os.path.join(ROOT, "include"), "-I" + csrc]
    jobs, objs = [], []
    shared = [hdr, *PUBLIC_HDRS, os.path.abspath(__file__)] + [f for f in parts if f.endswith(".hpp")]      # what every unit depends on
    for src, suffix, extra in _UNITS:
        obj = _unit_obj(objdir, src, suffix)
        objs.append(obj)
        if not force and not _stale(obj, shared + [_unit_path(src)]):
            continue                      # (a change to one .hip recompiles that unit only)
        cmd = common + extra + ["-c", _unit_path(src), "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        jobs.append((cmd, subprocess.Popen(cmd)))
    for cmd, pr in jobs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    n_inst = 0                            # kernel instances in the library (host-side launch stubs of the objects)
    for obj in objs:
        try:
            n_inst += subprocess.run(["nm", "-C", obj], capture_output=True, text=True).stdout.count("__device_stub__")
        except OSError:
            pass
    print(f"libvfm_hip.so: {len(jobs)} of {len(objs)} translation units compiled, {n_inst} kernel instances", file=sys.stderr)
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    return out


def build_torch_ops(force=False, verbose=False):
    """libvfm_torch_ops.so: TORCH_LIBRARY shim `torch.ops.vfm_hip.*` over the C ABI (host C++ only); the ranking and
    fold-in, session and design ops are TORCH_LIBRARY_FRAGMENTs of their own sources (OPS_SOURCES, over OPS_HDR) linked
    into the same shim."""
    import torch
    src = os.path.join(HERE, "csrc", "vfm_torch_ops.cpp")
    hdr = os.path.join(ROOT, "include", "vfm_hip.h")
    out = os.path.join(HERE, "libvfm_torch_ops.so")
    lib = os.path.join(HERE, "libvfm_hip.so")
    if not force and not _stale(out, [src, hdr, lib, OPS_HDR, *OPS_SOURCES, *PUBLIC_HDRS]):
        return out
    ti = os.path.dirname(torch.__file__)
    rocm = os.environ.get("ROCM_HOME", "/opt/rocm")
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-DUSE_ROCM",
           "-D_GLIBCXX_USE_CXX11_ABI=%d" % int(torch._C._GLIBCXX_USE_CXX11_ABI),
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ti, "include"),
           "-I" + os.path.join(ti, "include", "torch", "csrc", "api", "include"),
           "-I" + os.path.join(rocm, "include"), "-o", out, src, *OPS_SOURCES,
           "-L" + os.path.join(ti, "lib"), "-ltorch", "-ltorch_cpu", "-lc10", "-lc10_hip", "-ltorch_hip",
           "-L" + HERE, "-lvfm_hip", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath," + os.path.join(ti, "lib")]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    return out


def sanitizer_runtime():
    """ROCm clang's shared ASan runtime (LD_PRELOAD it into an uninstrumented python to load the sanitized libraries)."""
    out = subprocess.run([HIPCC, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    return out if os.path.isabs(out) and os.path.exists(out) else None


def build_sanitized(force=False, verbose=False):
    """The HOST side of both libraries under AddressSanitizer + UndefinedBehaviorSanitizer (`-Xarch_host
    -fsanitize=address,undefined`: the device code objects are the ordinary ones -- GPU sanitizers are not available on
    this pool), into vae_amd/build/san/.  What it covers: the argument checks, struct handling, host-side tables and
    launch set-up of csrc/vfm_abi.hip / vfm_index.hip / vfm_variants.hip and the TORCH_LIBRARY shim.  Load it with
    VFM_LIB_DIR=<returned dir> and LD_PRELOAD=sanitizer_runtime() (tests/test_sanitized_host.py does)."""
    import torch
    csrc = os.path.join(HERE, "csrc")
    outdir = os.path.join(HERE, "build", "san")
    os.makedirs(outdir, exist_ok=True)
    stamp = os.path.join(outdir, "digest.txt")
    import hashlib
    digest = sources_digest() + hashlib.sha1(b"".join(open(f, "rb").read() for f in _rank_sources() + [OPS_HDR, *OPS_SOURCES])).hexdigest()
    out = os.path.join(outdir, "libvfm_hip.so")
    out_ops = os.path.join(outdir, "libvfm_torch_ops.so")
    if (not force and os.path.exists(out) and os.path.exists(out_ops) and os.path.exists(stamp)
            and open(stamp).read().strip() == digest):
        return outdir
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_device", "-O0"]     # (device code: never run from here)
    common = [HIPCC, "-O1", "-g", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-fvisibility-inlines-hidden",
              "-I" + os.path.join(ROOT, "include"), "-I" + csrc] + san
    jobs, objs = [], []
    for src, suffix, extra in _UNITS:
        obj = _unit_obj(outdir, src, suffix)
        cmd = common + extra + ["-c", _unit_path(src), "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        jobs.append((cmd, subprocess.Popen(cmd)))
        objs.append(obj)
    for cmd, pr in jobs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-fsanitize=address,undefined", "-shared-libsan",
                    "-o", out] + objs, check=True)
    ti = os.path.dirname(torch.__file__)
    rocm = os.environ.get("ROCM_HOME", "/opt/rocm")
    clangxx = os.path.join(rocm, "lib", "llvm", "bin", "clang++")
    cmd = [clangxx, "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-fsanitize=address,undefined", "-shared-libsan",
           "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-fno-sanitize=vptr",
           "-mllvm", "-asan-globals=0",    # (libstdc++'s merged string literals trip the globals check: "not properly aligned")
           "-D__HIP_PLATFORM_AMD__", "-DUSE_ROCM",
           "-D_GLIBCXX_USE_CXX11_ABI=%d" % int(torch._C._GLIBCXX_USE_CXX11_ABI),
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ti, "include"),
           "-I" + os.path.join(ti, "include", "torch", "csrc", "api", "include"),
           "-I" + os.path.join(rocm, "include"), "-o", out_ops, os.path.join(csrc, "vfm_torch_ops.cpp"), *OPS_SOURCES,
           "-L" + os.path.join(ti, "lib"), "-ltorch", "-ltorch_cpu", "-lc10", "-lc10_hip", "-ltorch_hip",
           "-L" + outdir, "-lvfm_hip", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath," + os.path.join(ti, "lib")]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    # the native example: compiled (not run: it needs a GPU) under the same sanitizers -- its host code is UB-checked
    # by the compiler's diagnostics at least
    subprocess.run([HIPCC, "-O1", "-g", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include")] + san +
                   ["-c", os.path.join(ROOT, "examples", "c_abi_step.cpp"), "-o", os.path.join(outdir, "c_abi_step.o")], check=True)
    open(stamp, "w").write(digest)
    return outdir


def build_all(force=False, verbose=False):
    return [build_hip_library(force, verbose), build_torch_ops(force, verbose)]


if __name__ == "__main__":
    print(build_all(force="--force" in sys.argv, verbose=True))
