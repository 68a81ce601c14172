"""The candidate loop's FP64 primitives (csrc/pp_math.h, the SpeedController wrappers of
csrc/pp_device.h, the turn functions of csrc/pp_k_frame.h) against exact references, through
ppamd.math_eval (k_math calls the functions themselves). Each primitive's written accuracy claim is
held on the corpora of tests/math_cases.py: bit for bit against the host's IEEE operations where the
claim is exactness, in ulps of the mpmath value where it is an ulp bound, and by bounds derived
from the operations for the output frame's approximations. Every figure is printed before it is
asserted (tools/math_census.py records them in profiles/math_primitives.json)."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest
from mpmath import mp, mpf

import math_cases as mc
import oracle_lib
from oracle_lib import ppamd

REPO = oracle_lib.REPO
gpu = pytest.mark.gpu


def ev(kind, *arrays):
    """math_eval over numpy inputs -> tuple of numpy outputs"""
    import torch
    dev = torch.device("cuda", 0)
    out = ppamd.math_eval(kind, *[torch.from_numpy(mc.f64(a)).to(dev) for a in arrays], device=0)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def fig(name, **figures):
    print("MATHFIG " + json.dumps({"test": name, **{k: (float(v) if np.ndim(v) == 0 else [float(x) for x in v])
                                                    for k, v in figures.items()}}))


def assert_same(got, ref, *inputs):
    ok = mc.same_bits(got, ref)
    bad = np.flatnonzero(~ok)
    assert ok.all(), (len(bad), [(tuple(float(a[i]).hex() for a in inputs), float(got[i]).hex(), float(ref[i]).hex())
                                 for i in bad[:4]])


def worst(err, *inputs):
    i = int(np.nanargmax(err))
    return [float(a[i]) for a in inputs]


def not_rn_share(got, rn):
    return float((~mc.same_bits(got, rn)).mean())


# ---- exact -------------------------------------------------------------------------------------------
@gpu
def test_sqrt_rd_exact():
    c = mc.sqrt_rd_cases()
    d, rd, dok = ev("sqrt_rd", c["q"])
    assert_same(d, c["d"], c["q"])
    assert_same(dok, c["dok"].astype(np.float64), c["q"])
    slow = ~c["dok"]
    assert_same(rd[slow], c["rd"][slow], c["q"][slow])
    # (recorded, not bounded: rd = 2 h on the fast path, in ulps of 1 / d)
    with np.errstate(all="ignore"):
        rel = np.abs(rd[c["dok"]] * c["d"][c["dok"]] - 1.0) / 2.0 ** -53
    fig("sqrt_rd", n=len(d), rd_fast_path_max_rel_2m53=rel.max())


@gpu
def test_div_rcp_with_rounded_reciprocal_is_the_ieee_quotient():
    """div_rcp(n, d, RN(1 / d)) == n / d on every input: operands at and around 2^+-900, quotients
    that overflow, are subnormal or underflow, zeros, non-finite operands."""
    c = mc.div_rcp_cases()
    (q,) = ev("div_rcp", c["n"], c["d"], c["r"])
    (one,) = ev("div_rcp", [2.0 ** 900], [2.0 ** -900], [2.0 ** 900])
    fig("div_rcp", n=len(q), differ=int((~mc.same_bits(q, c["q"])).sum()), overflow_case=one[0])
    assert one[0] == np.inf
    assert_same(q, c["q"], c["n"], c["d"])


@gpu
def test_div50_exact():
    c = mc.div50_cases()
    (q,) = ev("div50", c["v"])
    assert_same(q, c["q"], c["v"])
    c = mc.div50_nc_cases()
    (q,) = ev("div50_nc", c["v"])
    assert_same(q, c["q"], c["v"])


@gpu
def test_div_rcp_nc_with_rounded_reciprocal():
    """the unchecked form on its documented domain: the IEEE quotient, up to the sign of a zero one"""
    c = mc.div_rcp_nc_cases()
    (q,) = ev("div_rcp_nc", c["n"], c["d"], c["r"])
    nz = c["n"] != 0
    assert_same(q[nz], c["q"][nz], c["n"][nz], c["d"][nz])
    assert (q[~nz] == 0).all()


@gpu
def test_fmod_2pi_exact():
    c = mc.fmod_cases()
    (r,) = ev("fmod_2pi", c["a"])
    assert_same(r, c["r"], c["a"])
    c = mc.fmod_small_cases()
    (r,) = ev("fmod_2pi_small", c["a"])
    assert_same(r, c["r"], c["a"])


@gpu
def test_atan2_unit_equals_atan2_fast():
    c = mc.atan2_cases()
    (u,) = ev("atan2_unit", c["y"], c["x"])
    (f,) = ev("atan2_fast", c["y"], c["x"])
    assert_same(u, f, c["y"], c["x"])


@gpu
def test_atan2_special_values():
    c = mc.atan2_special_cases()
    for kind in ("atan2_pp", "atan2_fast"):
        (r,) = ev(kind, c["y"], c["x"])
        assert_same(r, c["r"], c["y"], c["x"])


@gpu
def test_sincos_nolarge_equals_sincos():
    """sincos_pp<false> is sincos_pp<true> wherever sincos_pp reduces the argument itself (high word
    of |x| <= 0x413921fb: every |x| <= kMediumMax and on to ~2^20 pi/2), and NaN beyond"""
    c = mc.sincos_cases()
    s1, c1 = ev("sincos", c["x"])
    s0, c0 = ev("sincos_nolarge", c["x"])
    m = c["medium"]
    assert (np.abs(c["x"][~m & c["finite"]]) > mc.K_MEDIUM_MAX).all()
    assert_same(s0[m], s1[m], c["x"][m])
    assert_same(c0[m], c1[m], c["x"][m])
    assert np.isnan(s0[~m]).all() and np.isnan(c0[~m]).all()


@gpu
def test_turn_sincos_nolarge_equals_turn_sincos():
    c = mc.turn_sincos_cases()
    s1, c1 = ev("turn_sincos", c["x"])
    s0, c0 = ev("turn_sincos_nolarge", c["x"])
    assert_same(s0, s1, c["x"])
    assert_same(c0, c1, c["x"])


@gpu
def test_speed_in_range_is_its_definition():
    c = mc.speed_in_range_cases()
    (r,) = ev("speed_in_range", c["x"])
    assert_same(r, c["r"], c["x"])


def _sc_in(c, speed=False):
    d = np.stack([c["shift"], c["k"]] + ([c["speed"]] if speed else []))
    return c["start"], c["target"], c["ttime"], d


def _one_of(got, cands):
    ok = np.zeros(len(got), bool)
    for v in cands:
        ok |= mc.same_bits(got, v)
    return ok


@gpu
def test_sc_get_speed():
    """sc_get_speed is the host's expression bit for bit. sc_get_speed_r<true/false>: the target
    past the ramp; inside it start + q' with the quotient q' within one ulp of sc_get_speed's
    q = (target - start) t / ttime — held exactly: the result is RN(start + q') for q' one of q's
    two neighbours or q itself (the sum is computed by the same one addition)."""
    c = mc.sc_cases()
    (s,) = ev("sc_speed", *_sc_in(c))
    assert_same(s, c["speed_ref"], c["start"], c["target"], c["ttime"], c["shift"], c["k"])
    with np.errstate(all="ignore"):
        cands = [np.where(c["past"], c["target"], c["start"] + q) for q in (c["q"], mc.up(c["q"], 1), mc.up(c["q"], -1))]
    for kind in ("sc_speed_r", "sc_speed_r_nc"):
        (g,) = ev(kind, *_sc_in(c))
        ok = _one_of(g, cands)
        zero_q = ~c["past"] & (c["q"] == 0)
        fig(kind, n=len(g), not_equal_share=not_rn_share(g, c["speed_ref"]))
        assert_same(g[c["past"]], c["target"][c["past"]])
        if kind == "sc_speed_r":
            assert_same(g[zero_q], c["speed_ref"][zero_q])
        assert ok.all(), [(c["start"][i], c["target"][i], c["ttime"][i], c["shift"][i], c["k"][i], g[i], c["speed_ref"][i])
                          for i in np.flatnonzero(~ok)[:4]]


@gpu
def test_sc_override():
    """sc_override is the host's expression bit for bit; the _r forms leave shift untouched, bit for
    bit, when t > ttime or |target - start| < kEps (target == start included: r is infinite or NaN
    there) and otherwise give t - mt' with mt' within one ulp of mt, held as in test_sc_get_speed."""
    c = mc.sc_cases()
    (s,) = ev("sc_override", *_sc_in(c, True))
    assert_same(s, c["shift_ref"], c["start"], c["target"], c["ttime"], c["shift"], c["k"], c["speed"])
    keep = c["keep"]
    with np.errstate(all="ignore"):
        cands = [np.where(keep, c["shift"], c["t"] - m) for m in (c["mt"], mc.up(c["mt"], 1), mc.up(c["mt"], -1))]
    for kind in ("sc_override_r", "sc_override_r_nc"):
        (g,) = ev(kind, *_sc_in(c, True))
        assert_same(g[keep], c["shift"][keep], c["start"][keep], c["target"][keep], c["ttime"][keep])
        ok = _one_of(g, cands)
        fig(kind, n=len(g), changed=int((~keep).sum()), not_equal_share=not_rn_share(g, c["shift_ref"]))
        assert ok.all(), [(c["start"][i], c["target"][i], c["ttime"][i], c["k"][i], c["speed"][i], g[i], c["shift_ref"][i])
                          for i in np.flatnonzero(~ok)[:4]]


@gpu
def test_turn_angle_checked_is_the_ieee_expression():
    c = mc.turn_angle_cases()
    (r,) = ev("turn_angle", c["nc"], c["speed"], c["adiff"])
    assert_same(r, c["rot"], c["nc"], c["speed"], c["adiff"])


# ---- within one ulp of the exact value ------------------------------------------------------------------
@gpu
def test_rcp_nr_one_ulp():
    c = mc.rcp_cases()
    (r,) = ev("rcp_nr", c["d"])
    e = mc.ulp_errs(r, c["exact"])
    fig("rcp_nr", n=len(e), max_ulp=e.max(), at=worst(e, c["d"]), not_rn_share=not_rn_share(r, mc.hostdiv(1.0, c["d"])))
    assert e.max() <= 1.0


@gpu
def test_div_rcp_auto_one_ulp():
    c = mc.div_auto_cases()
    (q,) = ev("div_rcp_auto", c["n"], c["d"])
    e = mc.ulp_errs(q, c["exact"])
    fig("div_rcp_auto", n=len(e), max_ulp=e.max(), at=worst(e, c["n"], c["d"]), not_rn_share=not_rn_share(q, c["q"]))
    assert e.max() <= 1.0
    c = mc.div_nc_auto_cases()
    (q,) = ev("div_rcp_nc_auto", c["n"], c["d"])
    nz = c["n"] != 0
    e = mc.ulp_errs(q, c["exact"])
    fig("div_rcp_nc_auto", n=len(e), max_ulp=e.max(), at=worst(e, c["n"], c["d"]), not_rn_share=not_rn_share(q[nz], c["q"][nz]))
    assert e.max() <= 1.0
    assert (np.isfinite(q[nz]) & (q[nz] != 0)).all()       # every exact quotient of the domain is a normal double


@gpu
def test_div_rcp_with_reciprocal_ulps_off():
    """r one and two ulps from RN(1 / d): still within one ulp of the exact quotient"""
    o = mc.div_off_cases()
    for kind, c in (("div_rcp", o["checked"]), ("div_rcp_nc", o["nc"])):
        (q,) = ev(kind, c["n"], c["d"], c["r"])
        e = mc.ulp_errs(q, c["exact"])
        nz = c["n"] != 0
        fig(kind + "_r_off", n=len(e), max_ulp=e.max(), at=worst(e, c["n"], c["d"], c["r"]),
            not_rn_share=not_rn_share(q[nz], mc.hostdiv(c["n"], c["d"])[nz]))
        assert e.max() <= 1.0


@gpu
def test_div_rcp_n_and_d_one_ulp():
    """n / sqrt(q) after sqrt_rd(q), as the step divides. div_rcp_n: within one ulp of
    n / RN(sqrt(q)) wherever dok, the IEEE quotient where not, for |n| outside [2^-900, 2^900] and
    for n = +-0. div_rcp_d (no check of n): within one ulp on its documented domain (the numerator
    a component of the step times dstep: math_cases.div_sqrt_d_cases), the IEEE quotient where not
    dok."""
    c = mc.div_sqrt_cases()
    dok = c["dok"]
    ex = [e for e in c["exact"] if e is not None]
    (q,) = ev("div_rcp_n", c["n"], c["q"])
    e = mc.ulp_errs(q[dok], ex)
    fig("div_rcp_n", n=int(dok.sum()), max_ulp=e.max(), at=worst(e, c["n"][dok], c["q"][dok]),
        not_rn_share=not_rn_share(q[dok], c["ieee"][dok]))
    assert e.max() <= 1.0
    assert_same(q[~dok], c["ieee"][~dok], c["n"][~dok], c["q"][~dok])
    an = np.abs(c["n"])
    out = dok & ((an < 2.0 ** -900) | (an > 2.0 ** 900))
    assert out.sum() > 10 and (dok & (an == 0)).sum() > 2
    assert_same(q[out], c["ieee"][out], c["n"][out], c["q"][out])
    (q,) = ev("div_rcp_d", c["n"], c["q"])
    assert_same(q[~dok], c["ieee"][~dok], c["n"][~dok], c["q"][~dok])
    c = mc.div_sqrt_d_cases()
    (q,) = ev("div_rcp_d", c["n"], c["q"])
    e = mc.ulp_errs(q, c["exact"])
    fig("div_rcp_d", n=len(e), max_ulp=e.max(), at=worst(e, c["n"], c["q"]), not_rn_share=not_rn_share(q, c["ieee"]))
    assert e.max() <= 1.0 and np.isfinite(q).all()


@gpu
def test_asin_small_one_ulp():
    c = mc.asin_cases()
    (r,) = ev("asin_small", c["s"])
    e = mc.ulp_errs(r, c["exact"])
    fig("asin_small", n=len(e), max_ulp=e.max(), at=worst(e, c["s"]))
    assert e.max() <= 1.0


@gpu
def test_turn_branch_seam():
    """At |cr| = kStepSinMax the step turn changes from asin_small(cr) to atan2_unit(cr, dt): the two
    agree within one ulp of the angle there (dt = RN(sqrt(1 - cr^2)) from mpmath)"""
    c = mc.seam_cases()
    (a,) = ev("asin_small", c["cr"])
    (u,) = ev("atan2_unit", c["cr"], c["dt"])
    with mp.workprec(mc.PREC):
        e = np.array([abs(float(p) - float(q)) / float(mc.ulp_of(x)) for p, q, x in zip(a, u, c["exact"])])
    fig("seam", n=len(e), max_ulp=e.max(), at=worst(e, c["cr"], c["dt"]))
    assert e.max() <= 1.0


@functools.lru_cache(None)
def _atan2_errors():
    c = mc.atan2_cases()
    nz, rp = c["nonzero"], c["pp_reached"]
    (f,) = ev("atan2_fast", c["y"], c["x"])
    (p,) = ev("atan2_pp", c["y"], c["x"])
    ex = [e for e, k in zip(c["exact"], nz) if k]
    ef, ep = mc.ulp_errs(f[nz], ex), mc.ulp_errs(p[nz], ex)
    epr = ep[rp[nz]]
    fig("atan2_fast", n=len(ef), max_ulp=ef.max(), at=worst(ef, c["y"][nz], c["x"][nz]))
    fig("atan2_pp", n=len(epr), max_ulp=epr.max(), at=worst(epr, c["y"][rp], c["x"][rp]),
        unreached_n=len(ep), unreached_max_ulp=ep.max(), unreached_at=worst(ep, c["y"][nz], c["x"][nz]))
    right = c["x"][nz] > 0
    fig("atan2_fast.x>0", n=int(right.sum()), max_ulp=ef[right].max())
    return c, ef, epr


@gpu
def test_atan2_pp_one_ulp_on_exponent_gaps():
    """atan2_pp (fdlibm's form: it divides first) serves the planner only for zero or non-finite
    arguments (test_atan2_special_values: atan2_fast sends every finite nonzero pair through
    atan2_core). It is held to 1 ulp on the pairs with exponent gaps beyond 60, where it returns a
    rounded constant or the rounded quotient; on the other finite pairs its atan of the already
    rounded |y / x| reaches 1.23 ulp (measured, printed here, reached by no caller)."""
    c, _, epr = _atan2_errors()
    assert c["pp_reached"].sum() > 500
    assert epr.max() < 1.0


@gpu
def test_atan2_fast_one_ulp():
    """atan2_fast (and atan2_unit, bit-identical) within 1 ulp on every finite nonzero pair, exponent
    gaps of 59..62 included. (fdlibm's form, which this replaced, measured 1.178 ulp here: rounded
    3 |x|, 3 |y|, denominator and quotient, and a second rounding in the quadrant step.)"""
    _, ef, _ = _atan2_errors()
    assert ef.max() < 1.0


@gpu
def test_sincos_pp_one_ulp():
    """sincos_pp's own reduction (|x| up to high word 0x413921fb, which covers kMediumMax): < 1 ulp.
    Beyond it the device library's code: NaN for inf and NaN, within 1e-15 absolute otherwise (loose
    on purpose: it catches a dead branch, not library rounding)."""
    c = mc.sincos_cases()
    s, co = ev("sincos", c["x"])
    m = c["medium"]
    for name, got, ref in (("sin", s, c["sin"]), ("cos", co, c["cos"])):
        e = mc.ulp_errs(got[m], [r for r, k in zip(ref, m) if k])
        fig("sincos_pp." + name, n=len(e), max_ulp=e.max(), at=worst(e, c["x"][m]))
        assert e.max() < 1.0
        big = ~m & c["finite"]
        with mp.workprec(mc.PREC):
            ab = np.array([abs(float(mpf(float(g)) - r)) for g, r in zip(got[big], [r for r, k in zip(ref, big) if k])])
        fig("sincos_pp.large." + name, n=len(ab), max_abs=ab.max(), at=worst(ab, c["x"][big]))
        assert ab.max() <= 1e-15
        assert np.isnan(got[~c["finite"]]).all()


# ---- output-frame approximations ----------------------------------------------------------------------
@functools.lru_cache(None)
def _turn_sincos_errors():
    c = mc.turn_sincos_cases()
    s, co = ev("turn_sincos", c["x"])
    d = c["direct"]
    out = {}
    for name, got, ref in (("sin", s, c["sin"]), ("cos", co, c["cos"])):
        with mp.workprec(mc.PREC):
            ab = np.array([abs(float(mpf(float(g)) - r)) for g, r in zip(got, ref)])
        e = mc.ulp_errs(got[d], [r for r, k in zip(ref, d) if k])
        fig("turn_sincos." + name, n=len(ab), max_abs=ab.max(), at=worst(ab, c["x"]), direct_max_ulp=e.max(),
            direct_at=worst(e, c["x"][d]))
        out[name] = (ab.max(), e.max())
    return c, out


@gpu
def test_turn_sincos_bounds():
    """turn_sincos (no decision reads it): within 1e-15 + 2^-52 absolute of sin and cos up to
    kMediumMax (the two-part reduction's stated argument error plus the kernels' rounding), sin
    within 1 ulp on [-pi/4, pi/4] (cos: test_turn_sincos_cos_one_ulp); beyond kMediumMax
    turn_sincos<true> is sincos_pp<true>."""
    c, e = _turn_sincos_errors()
    assert e["sin"][0] <= 1e-15 + 2.0 ** -52 and e["cos"][0] <= 1e-15 + 2.0 ** -52
    assert e["sin"][1] <= 1.0
    bs, bc = ev("turn_sincos", c["beyond"])
    ps, pc = ev("sincos", c["beyond"])
    assert_same(bs, ps, c["beyond"])
    assert_same(bc, pc, c["beyond"])
    f = c["beyond_finite"]
    assert np.isnan(bs[~f]).all() and np.isnan(bc[~f]).all()
    with mp.workprec(mc.PREC):
        ab = max(abs(float(mpf(float(g)) - r)) for got, ref in ((bs, c["beyond_sin"]), (bc, c["beyond_cos"]))
                 for g, r, k in zip(got, ref, f) if k)
    assert ab <= 1e-15


@gpu
def test_turn_sincos_cos_one_ulp():
    """turn_sincos's cos within 1 ulp on [-pi/4, pi/4]: the rounding error of 1 - z/2 joins the small
    term, as in fdlibm's kernel (the fused form without it measured 1.191 ulp at
    x = 0.7592440901963402)."""
    _, e = _turn_sincos_errors()
    assert e["cos"][1] <= 1.0


@gpu
def test_sincos_small_bounds():
    """|x| <= 0.0709: sin within 1.3e-16 (the neglected x^9 / 9!) plus half an ulp, cos within 1e-18
    (the neglected x^10 / 10!) plus half an ulp"""
    c = mc.sincos_small_cases()
    s, co = ev("sincos_small", c["x"])
    with mp.workprec(mc.PREC):
        es = np.array([float(abs(mpf(float(g)) - r) - mc.ulp_of(r) / 2) for g, r in zip(s, c["sin"])])
        ec = np.array([float(abs(mpf(float(g)) - r) - mc.ulp_of(r) / 2) for g, r in zip(co, c["cos"])])
    fig("sincos_small", n=len(es), sin_max_over_half_ulp=es.max(), sin_at=worst(es, c["x"]),
        cos_max_over_half_ulp=ec.max(), cos_at=worst(ec, c["x"]))
    assert es.max() <= 1.3e-16
    assert ec.max() <= 1e-18


@gpu
def test_turn_angle_by_reciprocal_bounds():
    """turn_angle<false> and turn_angle_fast compute rot = +-nad - adiff with nad = RN(RN(nc c) r),
    c = RN(0.02), r ~ 1 / speed, against the exact nad* = nc / (speed 50). Relative errors, each
    factor (1 + e): c's representation |e| <= 2^-53; the product nc c, 2^-53; the product with r,
    2^-53; and r itself:
      turn_angle<false>: r = rcp_nr(speed), within one ulp of 1 / speed (test_rcp_nr_one_ulp), i.e.
        |e| <= 2^-52: |nad - nad*| <= 2.5 * 2^-52 (1 + 2^-50) |nad*|;
      turn_angle_fast: r = r0 + r0 RN(1 - speed r0) by two fmas from r0 = v_rcp_f64(speed), whose
        documented accuracy is 2^29 ulp, |speed r0 - 1| <= 2^-23: speed r - 1 = -e0^2 + e0 d (1 - e0)
        then the fma's rounding, |e| <= 2^-46 + 1.001 * 2^-53; with the three 2^-53 above
        |nad - nad*| <= 2^-46 (1 + 2^-5) |nad*|.
    The sign flip is exact and the final subtraction rounds once: half an ulp at |rot*| + that bound.
    (No product here is subnormal: nc is 0 or >= 2^-60, |speed| in [2^-113, 2^21].)"""
    c = mc.turn_angle_rcp_cases()
    for kind, rel in (("turn_angle_nolarge", 2.5 * 2.0 ** -52 * (1 + 2.0 ** -50)), ("turn_angle_fast", 2.0 ** -46 * (1 + 2.0 ** -5))):
        (r,) = ev(kind, c["nc"], c["speed"], c["adiff"])
        with mp.workprec(mc.PREC):
            bound = [abs(n) * rel for n in c["nad"]]
            bound = [b + mc.ulp_of(abs(x) + b) / 2 for b, x in zip(bound, c["rot"])]
            ratio = np.array([float(abs(mpf(float(g)) - x) / b) for g, x, b in zip(r, c["rot"], bound)])
        fig(kind, n=len(ratio), max_error_over_bound=ratio.max(), at=worst(ratio, c["nc"], c["speed"], c["adiff"]))
        assert np.isfinite(r).all() and ratio.max() <= 1.0


# ---- launch shape, arguments, the stand-alone checker ---------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_launch_shape_writes_n_elements_only(n):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(n)
    x = rng.uniform(0.1, 4.0, n)
    sentinel = -12345.678
    for kind, ins in (("sqrt_rd", [x]), ("sincos", [x]), ("atan2_fast", [x, x[::-1].copy()]),
                      ("sc_override_r", [x, x + 1.0, x, np.stack([0 * x, 1 + 0 * x, x])])):
        k, nin, nout = ppamd.MATH_KINDS[kind]
        t = [torch.from_numpy(mc.f64(a)).to(dev) for a in ins]
        outs = [torch.full((n + 64,), sentinel, dtype=torch.float64, device=dev) for _ in range(nout)]
        p = [a.data_ptr() for a in t] + [None] * (4 - nin)
        o = [a.data_ptr() for a in outs] + [None] * (3 - nout)
        assert ppamd.lib.pp_math_eval(k, *p, *o, n, 0, None) == 0
        torch.cuda.synchronize()
        want = ev(kind, *ins)
        for g, w in zip(outs, want):
            g = g.cpu().numpy()
            assert (g[n:] == sentinel).all(), kind
            assert mc.same_bits(g[:n], w).all(), kind


def test_argument_errors():
    """a bad kind, a missing array, a negative n, a bad device: PP_ERR_ARG before any HIP call (the
    pointers are never read: any non-null value stands for an array); n = 0: PP_OK"""
    f = ppamd.lib.pp_math_eval
    P = 0x1000
    kinds = ppamd.MATH_KINDS
    assert len(kinds) == 31 and sorted(v[0] for v in kinds.values()) == list(range(31))
    assert f(-1, P, P, P, P, P, P, P, 4, 0, None) == -1
    assert f(31, P, P, P, P, P, P, P, 4, 0, None) == -1
    for name, (k, nin, nout) in kinds.items():
        for miss in range(nin):
            a = [P if j != miss else None for j in range(4)]
            assert f(k, *a, P, P, P, 4, 0, None) == -1, (name, miss)
        for miss in range(nout):
            o = [P if j != miss else None for j in range(3)]
            assert f(k, P, P, P, P, *o, 4, 0, None) == -1, (name, miss)
        assert f(k, P, P, P, P, P, P, P, -1, 0, None) == -1
        assert f(k, P, P, P, P, P, P, P, 4, -1, None) == -1 and f(k, P, P, P, P, P, P, P, 4, 9999, None) == -1
        assert f(k, None, None, None, None, None, None, None, 0, 0, None) == 0
    with pytest.raises(ValueError):
        ppamd.math_eval("atan2_pp", np.zeros(3))
    with pytest.raises(KeyError):
        ppamd.math_eval("nope", np.zeros(3))


@gpu
def test_standalone_atan2_checker(tmp_path):
    """tools/atan2_check.hip (atan2_unit against atan2_fast over its own, larger corpus), compiled
    here and run once with its random sections cut to 2^16 inputs each"""
    exe = str(tmp_path / "pp_atan2_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17",
                    "-I" + os.path.join(REPO, "carnd-path-planning-project_amd", "csrc"),
                    os.path.join(REPO, "tools", "atan2_check.hip"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, "65536"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " 0 differ" in r.stdout
