"""CPU half of tests/test_gpu_arith.py: the device harness builds and exports its entry points (and stays out of the
shipped library), and every case list meets the precondition its function states -- so that a failure on the GPU can
only mean a wrong kernel."""
import os
import subprocess

import pytest

import arith_cases as C
from helpers import ROOT

HARNESS = os.path.join(ROOT, "tests", "cpp", "libdevice_arith.so")
ENTRY_POINTS = ("da_fr", "da_fq30", "da_fr30", "da_g1", "da_wave")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_harness_builds_and_exports(built):
    assert os.path.exists(HARNESS)
    syms = _exports(HARNESS)
    assert all(f in syms for f in ENTRY_POINTS)
    shipped = _exports(os.path.join(ROOT, "typlonk_amd", "libtyplonk_hip.so"))
    assert not any(f in shipped for f in ENTRY_POINTS), "the test harness is linked into the shipped library"


def _check(name, pre, cases):
    n = C.distinct(cases)
    assert n >= C.min_distinct(name), f"{name}: only {n} distinct cases"
    bad = [i for i, c in enumerate(cases) if not pre(*c)]
    assert not bad, f"{name}: cases {bad[:5]} break the precondition"


@pytest.mark.parametrize("name", list(C.FR_OPS))
def test_fr_cases(name):
    _, make, pre, _ = C.FR_OPS[name]
    _check(name, pre, make())


@pytest.mark.parametrize("name", list(C.FQ_OPS))
def test_fq30_cases(name):
    _, make, pre = C.FQ_OPS[name]
    cases = make()
    _check(name, pre, cases)
    if name in ("fq30_mul", "fq30_sqr"):
        # all-ones limbs for both operands: the contract a * b < 2^780 still holds and every fused column is at its maximum
        assert (C.FQ_R - 1,) * (1 if name == "fq30_sqr" else 2) in cases


@pytest.mark.parametrize("name", list(C.FR30_OPS))
def test_fr30_cases(name):
    _, make, pre = C.FR30_OPS[name]
    _check(name, pre, make())


@pytest.mark.parametrize("name", list(C.G1_OPS))
def test_g1_cases(name):
    _check(name, lambda a, b, f: C.g1_pre(name, a, b, f), C.g1_cases(name))


@pytest.mark.parametrize("name", list(C.WAVE_OPS))
def test_wave_cases(name):
    """whole wavefronts for the butterflies of msm_common.hpp: every lane within the XYZZ invariants and on the curve, the
    four-lane step's operands identical on lanes l and l ^ 1, and the kinds of wave the checks are about really there"""
    cases = C.wave_cases(name)
    n = len({repr((param, wave)) for _, param, wave in cases})
    assert n >= C.wave_min_distinct(name), f"{name}: only {n} distinct waves"
    bad = [label for label, param, wave in cases if not C.wave_pre(name, param, wave)]
    assert not bad, f"{name}: waves {bad[:5]} break the precondition"
    assert {param for _, param, _ in cases} == set(C.WAVE_PARAMS[name])
    for param in C.WAVE_PARAMS[name]:
        mine = [(label, wave) for label, p, wave in cases if p == param]
        tops = [wave for label, wave in mine if label.endswith("top lift")]
        assert len(tops) * 2 + (name != "butterfly_reduce") == len(mine)   # (one wave mixes both identity encodings)
        # the largest lift: X, Y, ZZ, ZZZ of every point within one p of the invariants' limits (the identity: ZZ = 0 or p)
        assert all(C.X_MAX - c[0] <= C.P and C.Y_MAX - c[1] <= C.P and C.Z_MAX - c[2] <= C.P and C.Z_MAX - c[3] <= C.P
                   for wave in tops for c in wave if c[2] % C.P)
        if name == "butterfly_reduce":
            continue
        # partner lanes: the same point in two representations, in identical words, opposite, and both identity encodings
        pm = param
        kinds = set()
        for _, wave in mine:
            pts = [C.xyzz_point(c) for c in wave]
            for i in range(C.WAVE):
                a, b = wave[i], wave[i ^ pm]
                if pts[i] is None and pts[i ^ pm] is None:
                    kinds.add("identities" if a[2] == b[2] else "identities, two encodings")
                elif pts[i] is not None and pts[i] == pts[i ^ pm]:
                    kinds.add("equal words" if a == b else "equal, two representations")
                elif pts[i] is not None and pts[i ^ pm] == C.O.g1_neg(pts[i]):
                    kinds.add("opposite")
        assert kinds == {"identities", "identities, two encodings", "equal words", "equal, two representations", "opposite"}
        # a wave with exactly one exceptional pair, for each kind
        for kind in ("equal", "opposite", "identity"):
            for where in ("first", "last", "middle"):
                wave = next(w for label, w in mine if label == f"one {kind} pair, {where}")
                pts = [C.xyzz_point(c) for c in wave]
                exc = [i for i in range(C.WAVE) if pts[i] is None or pts[i ^ pm] is None or pts[i][0] == pts[i ^ pm][0]]
                assert len(exc) == (2 if name == "butterfly_add" else 4), (kind, where, exc)


def test_fr30_cases_reach_the_limits():
    """the lazy limb forms at their contract limits are in the lists: limbs 0..7 = 2^30 + 3 with limb 8 = 2^29 - 1 into
    fr30_mul and fr30_reduce_lazy, and fr30_reduce_lazy at both sides of every 0x73ee multiple it is given"""
    mul = C.FR30_OPS["fr30_mul"][1]()
    assert any(a == C.fr30_lazy_max() for a, _ in mul) and (C.fr30_lazy_max(), C.fr30_lazy_max()) in mul
    red = [c[0] for c in C.FR30_OPS["fr30_reduce_lazy"][1]()]
    assert C.fr30_lazy_max() in red
    tops = {a[8] for a in red}
    assert all({k * 0x73EE - 1, k * 0x73EE} <= tops for k in range(1, 9))


def test_fr30_sub_subtrahend_limit():
    """fr30_sub's bias (fr30_bias) lends 2^31 down from limb 8, so limb 8 of the result is x_8 + N8 - 2 - y_8 before the
    carry step: the subtrahend's top limb may not exceed x_8 + N8 - 2.  With x = 0 that excludes y = 2^12 r - 1 in every
    lazy limb form (limbs 0..7 <= 2^30 + 3 cannot carry what a top limb N8 - 2 leaves over), although it is < 2^12 r.
    The NTT never comes near: its subtrahends are sums of at most 2^10 values < 2r, or products < 2r, so below 2^11 r.
    The case lists hold the true limit, and y = 2^12 r - 1 with x_8 = 2."""
    assert C.val([C.LAZY] * 8 + [C.N8 - 2]) < (1 << 12) * C.R - 1
    assert C.limbs((1 << 12) * C.R - 1, 9)[8] == C.N8
    pre = C.FR30_OPS["fr30_sub"][2]
    assert not pre([0] * 9, C.fr30_exact((1 << 12) * C.R - 1))
    cases = C.FR30_OPS["fr30_sub"][1]()
    assert ([0] * 9, [C.LAZY] * 8 + [C.N8 - 2]) in cases
    assert (C.fr30_exact(2 << 240), C.fr30_exact((1 << 12) * C.R - 1)) in cases


def test_fq30_mul_representable_limit():
    """fq30_mul's columns are bounded for a * b < 2^780 (tools/fq30_fused_bounds.py), but its result p + a * b / 2^390 fits
    13 limbs only for a * b < (2^390 - p) 2^390: the all-ones operands lie between the two and come back as REDC(a b)
    without its top bit (fq30.hpp states both limits).  The library's operands are < 8p: a * b < 2^767."""
    top = (C.FQ_R - 1) ** 2
    assert top < C.FQ_R ** 2 and top >= C.FQ_MUL_MAX
    assert C.redc(top) >= C.FQ_R
    assert (8 * C.P) ** 2 < C.FQ_MUL_MAX
