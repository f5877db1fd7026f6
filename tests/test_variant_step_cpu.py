"""CPU: the fused variant step (include/vfm_variant_step.h) -- the header's symbols are exported and bound, bad arguments
are refused before any launch, the case list of the GPU test covers what it claims, and the GPU test's fp64 reference
(tests/variant_step_reference.py) CAN fail: a step whose gradient is off by the whole granted tolerance stays inside the
bounds, three wrong steps fall outside."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import adam_restatement as R
import variant_step_reference as V
from golden_util import ROOT

HDR = os.path.join(ROOT, "include", "vfm_variant_step.h")
SRC = os.path.join(ROOT, "vae_amd", "csrc_var", "vfm_variant_step.hip")


def test_header_symbols_are_exported_and_bound():
    from vae_amd import _lib
    text = open(HDR).read()
    declared = sorted(set(re.findall(r"\b(vfm_variant_step\w*)\s*\(", text)))
    assert declared == sorted(_lib.VARIANT_STEP_EXPORTS) and len(declared) == 2
    lib = _lib.load()
    for n in declared:
        assert hasattr(lib, n), n
    assert len(lib.vfm_variant_step_f32.argtypes) == 33
    w = lib.vfm_variant_step_workspace_bytes
    assert w(100, 2, 8) > 0 and w(100, 2, 8) % 16 == 0 and w(0, 1, 1) > 0
    assert w(100, 2, 0) < 0 and w(100, 2, 1025) < 0 and w(100, 0, 8) < 0 and w(-1, 2, 8) < 0


def _args(_lib, **over):
    """A complete argument list with non-NULL dummy pointers (never dereferenced: every case below fails the host checks)."""
    p = _lib.Problem()
    p.B, p.B_global, p.T, p.nb_train, p.F, p.d, p.likelihood, p.id_bits, p.n_samples = 10, 10, 50, 70, 2, 8, _lib.LIK_NORMAL, 64, 1
    p.group_hi[0], p.group_hi[1], p.group_n[0], p.group_n[1] = 25, 50, 25.0, 25.0
    ix = _lib.Index()
    ix.occ_ptr, ix.occ_rows, ix.status = 256, 256, 256
    names = ["workspace", "x", "values", "entity", "bias", "inv_occ", "scalars", "W", "priors", "eps_e", "eps_b", "eps_g", "state",
             "grow", "partials", "grad_out", "m_entity", "v_entity", "m_bias", "v_bias", "m_scalars", "v_scalars", "m_priors",
             "v_priors"]
    ptrs = {n: C.c_void_p(256) for n in names}
    for n in ("values", "eps_e", "eps_b", "eps_g"):
        ptrs[n] = None
    a = dict(problem=p, objective=_lib.OBJ_CLOSED_FORM, index=ix, lr=0.01, b1=0.9, b2=0.999, eps=1e-8, adam_step=1, **ptrs)
    a.update(over)
    return a, names


def _call(lib, a, names):
    return lib.vfm_variant_step_f32(C.byref(a["problem"]) if a["problem"] is not None else None, a["objective"],
                                    C.byref(a["index"]) if a["index"] is not None else None, *[a[n] for n in names],
                                    a["lr"], a["b1"], a["b2"], a["eps"], a["adam_step"], None)


def test_bad_arguments_are_refused_before_any_launch():
    from vae_amd import _lib
    lib = _lib.load()
    INV = _lib._gen.VFM_E_INVALID

    def refused(needle, **over):
        a, names = _args(_lib, **over)
        rc = _call(lib, a, names)
        msg = lib.vfm_last_error()
        assert rc == INV and needle in msg, (over.keys(), rc, msg)

    refused(b"problem is NULL", problem=None)
    for name in ("entity", "bias", "scalars", "m_entity", "v_entity", "m_bias", "v_bias", "m_scalars", "v_scalars", "workspace",
                 "state", "partials", "grad_out", "x", "inv_occ", "W"):
        refused(b"NULL pointer", **{name: None})
    refused(b"NULL pointer", index=None)
    refused(b"go with priors", m_priors=None)
    refused(b"go with priors", priors=None)
    refused(b"all three eps tables", eps_e=C.c_void_p(256))
    refused(b"unknown objective", objective=7)
    refused(b"adam_step", adam_step=0)
    refused(b"adam_step", adam_step=-3)
    refused(b"16-byte aligned", workspace=C.c_void_p(260))
    for d in (0, 1025, -8):
        a, names = _args(_lib)
        a["problem"].d = d
        assert _call(lib, a, names) == INV and b"d out of range" in lib.vfm_last_error(), d
    a, names = _args(_lib)
    a["problem"].struct_size -= 8
    assert _call(lib, a, names) == INV and b"struct_size" in lib.vfm_last_error()
    a, names = _args(_lib)
    a["index"].struct_size += 8
    assert _call(lib, a, names) == INV and b"vfm_index_t" in lib.vfm_last_error()
    a, names = _args(_lib)
    a["problem"].F = _lib.MAX_FIELDS + 1
    assert _call(lib, a, names) == INV and b"bad problem" in lib.vfm_last_error()


def test_source_holds_the_caps_the_gpu_test_reads():
    import test_gpu_variant_step as G
    cap, shapes = G.read_launch_arithmetic()
    assert cap == 2048
    assert G.unit_of(8, shapes) == 256 and G.unit_of(5, shapes) == 16 and G.unit_of(2, shapes) == 64
    assert G.unit_of(136, shapes) == 8 and G.unit_of(520, shapes) == 4 and G.unit_of(20, shapes) == 4
    text = open(SRC).read()
    assert "if (nb > VSTEP_BLOCKS) nb = VSTEP_BLOCKS;" in text and "(p->T + GPB - 1) / GPB" in text
    assert len(re.findall(r"epb\s*=\s*\(epb\s*\+\s*GPB\s*-\s*1\)\s*/\s*GPB\s*\*\s*GPB\s*;", text)) == 2      # host and kernel
    assert "atomicAdd(a.status" in text and len(re.findall(r"atomicAdd\(", text)) == 2      # the clamp counters, nothing else


def test_case_list_covers_what_it_claims():
    cs = V.CASES
    assert {c.d for c in cs} >= {2, 5, 20, 8, 16, 136, 520}
    for d in (2, 5, 20, 8, 16, 136, 520):
        assert any(c.priors for c in cs if c.d == d), d
    assert {c.F for c in cs} == {1, 2, 3, 5} and all(c.objective == "closed_form" for c in cs if c.F == 1)
    assert {c.B for c in cs} == {1, 33, 500} and {c.t for c in cs} == {1, 2, 57, 1000}
    for fam in (lambda c: c.d % 8 == 0, lambda c: c.d % 8 != 0):
        f = [c for c in cs if fam(c)]
        assert {c.objective for c in f} == {"sampled", "closed_form"} and {c.priors for c in f} == {False, True}
        assert {c.values for c in f} == {False, True} and {c.id32 for c in f} == {False, True}
        assert {c.output for c in f} == {"reg", "class"} and {c.eps_table for c in f} == {False, True}
    assert all(c.output == "reg" for c in cs if c.objective == "closed_form")
    assert all(not c.eps_table for c in cs if c.objective == "closed_form")


@pytest.mark.parametrize("case", [V.StepCase(5, 2, 33, 57, "closed_form", True, True), V.StepCase(8, 3, 33, 2, "sampled", True, False),
                                  V.StepCase(2, 2, 33, 1, "closed_form", True, False)], ids=lambda c: c.id)
def test_reference_accepts_the_granted_error_and_rejects_wrong_steps(case):
    pb = V.build_problem(case)
    g = np.random.default_rng(5)
    T, d = pb["T"], pb["d"]
    eps = (g.standard_normal(1), g.standard_normal(T), g.standard_normal((T, d))) if case.objective == "sampled" else None
    ref = V.oracle_grads(pb, eps)
    planted = V.plant(pb, ref)
    want = V.reference_step(pb, ref, planted)
    P, tol, t = V.params_of(pb), V.tolerances(pb, ref), case.t
    touched = np.bincount(pb["x"].reshape(-1), minlength=T) > 0
    assert (~touched).sum() >= 2 and T >= 200

    def fp32_step(grads, step=R.step_fp32_plain, **kw):
        return {n: (None if ref[n] is None else step(P[n], grads[n], planted[n][0], planted[n][1], t, **kw)) for n in V.TENSORS}

    # 1. the gradient off by the whole granted tolerance, the update in fp32: inside
    pert = {}
    for n in V.TENSORS:
        if ref[n] is None:
            pert[n] = None
            continue
        G = np.abs(ref[n]).max()
        pert[n] = ref[n] + np.asarray(tol[n]) * G * g.choice([-1.0, 1.0], ref[n].shape)
    rows, bad = V.compare(pb, ref, planted, want, fp32_step(pert))
    assert not bad, bad
    assert max(r[2] for r in rows) > 0.5          # (the perturbation fills the bound: the check is not slack)

    # 2. rows outside the batch skipped (their zero-gradient step not taken)
    got = fp32_step(ref)
    for n in ("entity", "bias"):
        p_, m_, v_ = (np.array(a) for a in got[n])
        p_[~touched], m_[~touched], v_[~touched] = P[n][~touched], planted[n][0][~touched], planted[n][1][~touched]
        got[n] = (p_, m_, v_)
    _, bad = V.compare(pb, ref, planted, want, got)
    assert {(b[0], b[1]) for b in bad} >= {("entity", "m'"), ("entity", "v'"), ("entity", "update"), ("bias", "m'"), ("bias", "update")}

    # 3. sqrt(bc2) dropped from the denominator
    def no_bc2(p, g_, m, v, t_):
        p, g_, m, v = (np.asarray(a, np.float32) for a in (p, g_, m, v))
        m2 = m + (g_ - m) * np.float32(1 - R.B1)
        v2 = v * np.float32(R.B2) + (np.float32(1 - R.B2) * g_) * g_
        return p + (-np.float32(R.LR / (1.0 - R.B1 ** t_)) * m2) / (np.sqrt(v2) + np.float32(R.EPS)), m2, v2
    _, bad = V.compare(pb, ref, planted, want, fp32_step(ref, step=no_bc2))
    assert {(b[0], b[1]) for b in bad} >= {(n, "update") for n in V.TENSORS}

    # 4. prior gradients taken at the previous step's priors (the table kernel reading priors the small launch already moved)
    stale = (pb["pri"].astype(np.float64) + R.LR * g.choice([-1.0, 1.0], pb["pri"].shape)).astype(np.float32)
    ref_stale = V.oracle_grads(pb, eps, pri=stale)
    got = fp32_step({**ref, "priors": ref_stale["priors"]})
    _, bad = V.compare(pb, ref, planted, want, got)
    assert ("priors", "m'") in {(b[0], b[1]) for b in bad}
    assert all(b[0] == "priors" for b in bad)
