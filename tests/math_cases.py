"""Inputs and references for the candidate loop's FP64 primitives (csrc/pp_math.h and its wrappers in
pp_device.h / pp_k_frame.h; ppamd.math_eval). One seeded generator per kind: it returns the inputs
and, beside them, the reference values. Exact claims are referred to the host's IEEE operations
(`/`, np.sqrt, np.fmod, math.atan2 for the Annex-F values: the correctly rounded results), ulp
claims to mpmath at 240 bits, with errors in ulps of the true value (ulp_err). No GPU needed:
tests/test_math_cases.py checks this module, tests/test_math_primitives.py and tools/math_census.py
run the corpora through the kernels. A kind's domain is what its generator returns; nothing is
dropped after seeing a kernel's output."""
import functools
import math

import numpy as np
from mpmath import mp, mpf

PREC = 240
K_STEP_SIN_MAX = 0.0708               # ppm::kStepSinMax
K_MEDIUM_MAX = 823549.6               # ppm::kMediumMax (< 2^19 pi/2): turn_sincos's two-part reduction up to it
SEAM_HI = 0x413921FB                  # sincos_pp's own reduction: high word of |x| <= this (|x| <~ 2^20 pi/2)
K_EPS = 1e-5                          # ppd::kEps
TWO_PI = 2 * 3.14159265358979323846   # fmod_2pi's y
PIO4 = 0.78539816339744828            # turn_sincos's direct range
PIO2 = math.pi / 2
DBL_MAX = np.finfo(np.float64).max
F = np.float64


def f64(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def up(x, k=1):
    """x moved k ulps towards +inf (k < 0: towards -inf)"""
    x = f64(x).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def up1(x, k=1):
    """up() of one number, as a float"""
    return float(up(x, k).ravel()[0])


def neighbours(x, k=1):
    """x with its k neighbours on both sides"""
    x = f64(np.atleast_1d(x))
    return np.concatenate([up(x, j) for j in range(-k, k + 1)])


def hiword(x):
    return (f64(x).view(np.uint64) >> np.uint64(32)).astype(np.int64) & 0x7FFFFFFF


def same_bits(a, b):
    """elementwise: bit for bit (signed zeros count), NaN matches NaN"""
    a, b = f64(a), f64(b)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def member(corpus, *vals):
    """every val is an element of corpus, bit for bit (NaN: any NaN)"""
    bits = set(f64(corpus).view(np.uint64).tolist())
    has_nan = bool(np.isnan(corpus).any())
    return all((has_nan if v != v else int(F(v).view(np.uint64)) in bits) for v in vals)


def ulp_of(exact):
    """the ulp of the double grid at the real number `exact` (mpf): 2^(e - 52) for 2^e <= |exact| <
    2^(e + 1), 2^-1074 below 2^-1022"""
    if exact == 0:
        return mpf(2) ** -1074
    e = mp.frexp(abs(exact))[1] - 1       # frexp: m in [0.5, 1), |exact| = m 2^(e + 1)
    return mpf(2) ** (max(e, -1022) - 52)


def ulp_err(got, exact):
    """|got - exact| in ulps of the true value `exact` (mpf). A true value that rounds to infinity
    (>= DBL_MAX + half an ulp) asks for that infinity: error 0 then, inf otherwise; a non-finite
    `got` elsewhere is an infinite error."""
    with mp.workprec(PREC):
        got = float(got)
        if abs(exact) >= mpf(2) ** 1024 - mpf(2) ** 970:
            return 0.0 if got == math.copysign(math.inf, float(mp.sign(exact))) else math.inf
        if not math.isfinite(got):
            return math.inf
        return float(abs(mpf(got) - exact) / ulp_of(exact))


def ulp_errs(got, exact):
    """ulp_err over an array and a list of mpf"""
    got = f64(got).ravel()
    assert len(got) == len(exact)
    return np.array([ulp_err(g, e) for g, e in zip(got, exact)])


def mp_map(fn, *arrays):
    """[fn(mpf(a_i), ...)] at PREC bits"""
    with mp.workprec(PREC):
        return [fn(*(mpf(float(v)) for v in row)) for row in zip(*(f64(a).ravel() for a in arrays))]


def rand_mant(rng, n):
    return 1.0 + rng.random(n)


def wide(rng, n, elo, ehi, signed=True):
    """random significands times 2^e, e uniform in [elo, ehi)"""
    v = np.ldexp(rand_mant(rng, n), rng.integers(elo, ehi, n).astype(np.int32))
    return v * rng.choice([-1.0, 1.0], n) if signed else v


def hostdiv(n, d):
    with np.errstate(all="ignore"):
        return f64(n) / f64(d)


# ---- sqrt_rd -----------------------------------------------------------------------------------
@functools.lru_cache(None)
def sqrt_rd_cases():
    rng = np.random.default_rng(101)
    edges = np.concatenate([neighbours([2.0 ** -900, 2.0 ** 900], 2),
                            [0.0, -0.0, 5e-324, 2.0 ** -1050, 2.0 ** -1022, np.inf, np.nan, -1.0, -np.inf, DBL_MAX,
                             1.0, 2.0, 4.0]])
    k = rng.integers(1, 2 ** 26, 4000).astype(np.float64)
    squares = np.concatenate([k * k, (k * k)[:1000] * 4.0 ** rng.integers(-200, 200, 1000)])
    m = (rng.integers(2 ** 25, 2 ** 26, 4000) * 2 + 1).astype(object)        # odd, 27 bits
    msq = f64([float(int(v) * int(v)) for v in m])
    odd = neighbours(msq, 1)
    binades = np.ldexp(rand_mant(rng, 1801), np.arange(-900, 901, dtype=np.int32))
    bulk = np.concatenate([wide(rng, 60000, -905, 905, signed=False), rng.uniform(0, 4, 20000) ** 2,
                           wide(rng, 2000, -1074, 1024, signed=False)])
    q = f64(np.concatenate([edges, squares, odd, binades, bulk]))
    with np.errstate(all="ignore"):
        d = np.sqrt(q)
        rd = 1.0 / d
    dok = (q >= 2.0 ** -900) & (q <= 2.0 ** 900)
    return {"q": q, "d": d, "rd": rd, "dok": dok, "odd27_squares": msq, "perfect": k * k}


# ---- div_rcp with a given r ----------------------------------------------------------------------
def _div_edges():
    e9 = neighbours([2.0 ** -900, 2.0 ** 900], 2)
    e9 = np.concatenate([e9, -e9])
    ne, de = np.meshgrid(e9, e9)
    n = [ne.ravel(), ]
    d = [de.ravel(), ]
    # overflowing quotients
    n.append(f64([2.0 ** 900, 2.0 ** 600, 1.5 * 2.0 ** 800, -2.0 ** 900, 1.9 * 2.0 ** 899, 2.0 ** 512, 1.75 * 2.0 ** 124]))
    d.append(f64([2.0 ** -900, 2.0 ** -600, 2.0 ** -300, 2.0 ** -900, -1.1 * 2.0 ** -899, 2.0 ** -512, 1.25 * 2.0 ** -900]))
    # subnormal quotients, and quotients that underflow to zero
    n.append(f64([1.3 * 2.0 ** -900, 1.3 * 2.0 ** -900, -1.7 * 2.0 ** -880, 3 * 2.0 ** -900, 1.1 * 2.0 ** -600,
                  2.0 ** -900, 1.5 * 2.0 ** -900, -2.0 ** -850, 1.2 * 2.0 ** -521, 1.2 * 2.0 ** -800]))
    d.append(f64([1.7 * 2.0 ** 150, 1.7 * 2.0 ** 130, 1.9 * 2.0 ** 170, 2.0 ** 174, 1.3 * 2.0 ** 450,
                  2.0 ** 900, 1.1 * 2.0 ** 200, 2.0 ** 800, 1.9 * 2.0 ** 520, 1.9 * 2.0 ** 221]))
    # subnormal quotients exactly halfway between two doubles: n = (2 j + 1) 2^-1075 d for a d of
    # few significant bits (the product is exact)
    m = f64([1.0 + 2.0 ** -20, 1.5 + 2.0 ** -30, 1.25 + 2.0 ** -40, 1.0 + 2.0 ** -10])
    for j in (1, 3, 5, 7):
        n.append((2 * j + 1) * m * 2.0 ** -875)
        d.append(m * 2.0 ** 200)
    # zero numerators, 50 with 0.02, non-finite and zero operands
    sp = f64([0.0, -0.0, 1.0, -1.0, 50.0, 22.2, np.inf, -np.inf, np.nan, 5e-324, 2.0 ** -1022, DBL_MAX, 2.0 ** 900])
    a, b = np.meshgrid(sp, sp)
    n.append(a.ravel())
    d.append(b.ravel())
    return np.concatenate(n), np.concatenate(d)


@functools.lru_cache(None)
def div_rcp_cases():
    """(n, d, r = RN(1 / d)) over the whole double range; reference: the host's n / d"""
    rng = np.random.default_rng(102)
    ne, de = _div_edges()
    v50 = np.concatenate([rng.uniform(-30, 30, 20000), wide(rng, 5000, -1074, 1024)])
    n = np.concatenate([ne, v50, wide(rng, 60000, -950, 950), rng.uniform(-100, 100, 30000),
                        wide(rng, 30000, -1074, 1024), wide(rng, 20000, 400, 900), wide(rng, 20000, -900, -500)])
    d = np.concatenate([de, np.full(len(v50), 50.0), wide(rng, 60000, -950, 950), rng.uniform(-100, 100, 30000),
                        wide(rng, 30000, -1074, 1024), wide(rng, 20000, -900, -100), wide(rng, 20000, 100, 900)])
    n, d = f64(n), f64(d)
    return {"n": n, "d": d, "r": hostdiv(1.0, d), "q": hostdiv(n, d), "edges": (ne, de)}


@functools.lru_cache(None)
def div50_cases():
    rng = np.random.default_rng(103)
    sp = f64([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.0 ** -1022, DBL_MAX, -DBL_MAX, 50.0, 22.2])
    e9 = neighbours([2.0 ** -900, 2.0 ** 900], 2)
    v = f64(np.concatenate([sp, e9, -e9, rng.uniform(-30, 30, 60000), wide(rng, 60000, -1074, 1024),
                            50.0 * wide(rng, 4000, -1074, -1010)]))
    return {"v": v, "q": hostdiv(v, 50.0)}


def nc_speed_values(rng, n):
    """+0 and magnitudes in [2^-113, 2^21]: the speeds of a walk k_prep admits (speed_in_range)"""
    v = np.concatenate([wide(rng, n, -113, 21), rng.uniform(-30, 30, n)])
    v[np.abs(v) < 2.0 ** -113] = 0.0
    v = np.abs(v) * np.where(v == 0, 1.0, np.sign(v))
    corners = f64([0.0, 2.0 ** -113, -2.0 ** -113, 2.0 ** 21, -2.0 ** 21, up1(2.0 ** -113), up1(2.0 ** 21, -1)])
    return f64(np.concatenate([corners, v]))


@functools.lru_cache(None)
def div50_nc_cases():
    v = nc_speed_values(np.random.default_rng(104), 60000)
    return {"v": v, "q": hostdiv(v, 50.0)}


NC_D = (2.0 ** -113, 2.0 ** 21)
NC_N = (2.0 ** -400, 2.0 ** 400)


def _nc_operands(rng, m):
    """|d| in [2^-113, 2^21], |n| in [2^-400, 2^400] or n = +0, the four corners (all signs) first"""
    cn, cd = np.meshgrid(f64([NC_N[0], NC_N[1], -NC_N[0], -NC_N[1]]), f64([NC_D[0], NC_D[1], -NC_D[0], -NC_D[1]]))
    n = np.concatenate([cn.ravel(), np.zeros(16), wide(rng, m, -400, 400), rng.uniform(-100, 100, m)])
    d = np.concatenate([cd.ravel(), wide(rng, 16, -113, 21), wide(rng, m, -113, 21), rng.uniform(-30, 30, m)])
    d[np.abs(d) < NC_D[0]] = 1.0
    n[(np.abs(n) < NC_N[0]) & (n != 0)] = 1.0
    n[n == 0] = 0.0
    return f64(n), f64(d)


@functools.lru_cache(None)
def div_rcp_nc_cases():
    """(n, d, r = RN(1 / d)) on the unchecked variants' documented domain; reference: n / d"""
    n, d = _nc_operands(np.random.default_rng(105), 60000)
    return {"n": n, "d": d, "r": hostdiv(1.0, d), "q": hostdiv(n, d)}


@functools.lru_cache(None)
def div_off_cases():
    """r one and two ulps off RN(1 / d), both sides, on the checked domain (a) and the unchecked
    one (b); reference: the exact quotient"""
    rng = np.random.default_rng(106)
    out = {}
    for key in ("checked", "nc"):
        if key == "checked":
            ne, de = _div_edges()
            fin = np.isfinite(ne) & np.isfinite(de) & (de != 0) & (np.abs(de) >= 2.0 ** -1020) & (np.abs(de) <= 2.0 ** 1020)
            n = np.concatenate([ne[fin], wide(rng, 3000, -950, 950), rng.uniform(-100, 100, 3000)])
            d = np.concatenate([de[fin], wide(rng, 3000, -950, 950), rng.uniform(-100, 100, 3000)])
        else:
            n, d = _nc_operands(rng, 3000)
        r0 = hostdiv(1.0, d)
        ns, ds, rs, off = [], [], [], []
        for k in (-2, -1, 1, 2):
            ns.append(n); ds.append(d); rs.append(up(r0, k)); off.append(np.full(len(n), k))
        n, d, r = map(np.concatenate, (ns, ds, rs))
        out[key] = {"n": n, "d": d, "r": r, "off": np.concatenate(off), "exact": mp_map(lambda a, b: a / b, n, d)}
    return out


@functools.lru_cache(None)
def div_auto_cases():
    """(n, d) for r = rcp_nr(d) inside: finite operands, d normal; reference: the exact quotient"""
    rng = np.random.default_rng(107)
    ne, de = _div_edges()
    fin = np.isfinite(ne) & np.isfinite(de) & (np.abs(de) >= 2.0 ** -1022)
    n = np.concatenate([ne[fin], wide(rng, 12000, -950, 950), rng.uniform(-100, 100, 12000), wide(rng, 6000, -1022, 1023)])
    d = np.concatenate([de[fin], wide(rng, 12000, -950, 950), rng.uniform(-100, 100, 12000), wide(rng, 6000, -1022, 1023)])
    n, d = f64(n), f64(d)
    return {"n": n, "d": d, "q": hostdiv(n, d), "exact": mp_map(lambda a, b: a / b, n, d)}


@functools.lru_cache(None)
def div_nc_auto_cases():
    n, d = _nc_operands(np.random.default_rng(108), 18000)
    return {"n": n, "d": d, "q": hostdiv(n, d), "exact": mp_map(lambda a, b: a / b, n, d)}


@functools.lru_cache(None)
def rcp_cases():
    """finite normal d"""
    rng = np.random.default_rng(109)
    e = f64([2.0 ** -1022, DBL_MAX, 1.0, 50.0, 3.0, 2.0 ** 1023, 2.0 ** 1022, up1(2.0 ** 1022), up1(1.0, -1),
             up1(2.0, -1), 2.0 ** -113, 2.0 ** 21])
    d = f64(np.concatenate([e, -e, wide(rng, 16000, -1022, 1024), rng.uniform(-30, 30, 12000),
                            np.ldexp(2.0 - rng.integers(1, 64, 2000) * 2.0 ** -52, rng.integers(-100, 100, 2000).astype(np.int32))]))
    return {"d": d, "exact": mp_map(lambda a: 1 / a, d)}


@functools.lru_cache(None)
def div_sqrt_cases():
    """(n, q) for div_rcp_n / div_rcp_d after sqrt_rd(q), as run_candidate's step divides its step
    vector by its length; reference: the exact n / RN(sqrt(q))"""
    rng = np.random.default_rng(110)
    eq = np.concatenate([neighbours([2.0 ** -900, 2.0 ** 900], 1), [0.0, np.inf, 5e-324, 1.0, 0.19 ** 2]])
    en = f64([0.0, -0.0, 1.0, -0.19, 2.0 ** -900, up1(2.0 ** -900, -1), 2.0 ** 900, up1(2.0 ** 900), 2.0 ** -450, 1e-160])
    a, b = np.meshgrid(en, eq)
    st = rng.uniform(0.0, 0.6, 12000)                         # ordinary steps: metres per 0.02 s
    th = rng.uniform(-np.pi, np.pi, 12000)
    n = np.concatenate([a.ravel(), st * np.cos(th) * st, wide(rng, 8000, -450, 450), wide(rng, 6000, -905, 905)])
    q = np.concatenate([b.ravel(), st * st, wide(rng, 8000, -900, 900, signed=False), wide(rng, 6000, -905, 905, signed=False)])
    n, q = f64(n), f64(q)
    with np.errstate(all="ignore"):
        d = np.sqrt(q)
    dok = (q >= 2.0 ** -900) & (q <= 2.0 ** 900)
    exact = [e if k else None for e, k in zip(mp_map(lambda a, b: a / b if b != 0 else mpf(0), n, np.where(dok, d, 1.0)), dok)]
    return {"n": n, "q": q, "d": d, "dok": dok, "ieee": hostdiv(n, d), "exact": exact}


@functools.lru_cache(None)
def div_sqrt_d_cases():
    """div_rcp_d's documented domain (k_cand<false>): the numerator is a component of the step vector
    times dstep and the divisor the vector's length d = sqrt(q), q in [2^-900, 2^900], so
    n = +-c d dstep with a direction cosine c (0, or 2^-60 .. 1) and dstep +0 or in [2^-119, 2^15]"""
    rng = np.random.default_rng(123)
    m = 24000
    q = np.concatenate([wide(rng, m // 2, -900, 900, signed=False), rng.uniform(0.0, 0.6, m // 2) ** 2,
                        [2.0 ** -900, 2.0 ** 900, up1(2.0 ** 900, -1), up1(2.0 ** -900)]])
    q = np.maximum(q, 2.0 ** -900)
    k = len(q)
    c = np.where(rng.random(k) < 0.5, rng.uniform(0, 1, k), np.ldexp(rand_mant(rng, k), rng.integers(-60, 0, k).astype(np.int32)) / 2)
    c[:8] = [0.0, 1.0, 2.0 ** -60, 1.0, 0.5, 1.0, 0.0, 2.0 ** -60]
    ds = np.where(rng.random(k) < 0.5, rng.uniform(0, 0.6, k), np.ldexp(rand_mant(rng, k), rng.integers(-119, 15, k).astype(np.int32)))
    ds[:8] = [1.0, 2.0 ** -119, 2.0 ** 15, 2.0 ** 15, 0.0, 0.44, 2.0 ** 15, 2.0 ** -119]
    ds = np.minimum(ds, 2.0 ** 15)
    d = np.sqrt(q)
    n = f64(c * d * ds * rng.choice([-1.0, 1.0], k))
    n[n == 0] = 0.0
    return {"n": n, "q": f64(q), "d": d, "ieee": hostdiv(n, d), "exact": mp_map(lambda a, b: a / b, n, d)}


# ---- fmod -----------------------------------------------------------------------------------------
@functools.lru_cache(None)
def fmod_cases():
    rng = np.random.default_rng(111)
    y = TWO_PI
    seams = neighbours(f64([k * y for k in range(4)]), 3)
    big = wide(rng, 62, 990, 1000)
    a = f64(np.concatenate([seams, -seams, [0.0, -0.0, 1e300, -1e300, np.inf, -np.inf, np.nan, 5e-324, -5e-324],
                            big, rng.uniform(-30, 30, 60000), rng.uniform(-1e6, 1e6, 30000), wide(rng, 20000, -60, 60)]))
    with np.errstate(all="ignore"):
        return {"a": a, "r": np.fmod(a, y), "big": np.concatenate([big, [1e300, -1e300]])}


@functools.lru_cache(None)
def fmod_small_cases():
    """[0, 3 (2 pi)) and NaN"""
    rng = np.random.default_rng(112)
    y = TWO_PI
    top = up1(3.0 * y, -1)                 # 3 y is a double: the largest argument is the one below it
    a = np.concatenate([neighbours(f64([y, 2 * y]), 3), [0.0, 5e-324, top, up1(top, -1), np.nan, 3 * np.pi],
                        rng.uniform(0, 3 * y, 60000)])
    a = f64(a[~(a >= 3.0 * y)])
    return {"a": a, "r": np.fmod(a, y), "top": top}


# ---- asin_small and the seam to atan2_unit --------------------------------------------------------
@functools.lru_cache(None)
def asin_cases():
    rng = np.random.default_rng(113)
    m = K_STEP_SIN_MAX
    near = np.concatenate([up(m, -j) for j in range(0, 600)])
    s = np.concatenate([[0.0, -0.0, m, -m, 2.0 ** -27, up1(2.0 ** -27, -1), 5e-324, 2.0 ** -1022],
                        near, -near, rng.uniform(m - 1e-6, m, 2000), rng.uniform(-m, -m + 1e-6, 2000),
                        rng.uniform(-m, m, 10000), wide(rng, 4000, -60, -5), wide(rng, 2000, -1000, -27)])
    s = f64(s[np.abs(s) <= m])
    return {"s": s, "exact": mp_map(mp.asin, s)}


@functools.lru_cache(None)
def seam_cases():
    """cr within a few ulps of +-kStepSinMax (and a little around it), dt = RN(sqrt(1 - cr^2))"""
    rng = np.random.default_rng(114)
    m = K_STEP_SIN_MAX
    cr = np.concatenate([neighbours(m, 8), rng.uniform(m - 1e-4, m + 1e-4, 400)])
    cr = f64(np.concatenate([cr, -cr]))
    with mp.workprec(PREC):
        dt = f64([float(mp.sqrt(1 - mpf(float(c)) ** 2)) for c in cr])
    return {"cr": cr, "dt": dt, "exact": mp_map(mp.asin, cr)}


# ---- atan2 ------------------------------------------------------------------------------------------
ATAN_EDGES = (7.0 / 16, 11.0 / 16, 19.0 / 16, 39.0 / 16)


@functools.lru_cache(None)
def atan2_cases():
    """tools/atan2_check.hip's corpus cut to ~40,000 finite pairs, not both zero (atan2_unit's
    domain; zeros on one side included), plus exponent gaps of 59..62. Reference: mpmath."""
    rng = np.random.default_rng(115)
    sp = f64([0.0, 1.0, 2.0 ** -61, 2.0 ** -70, 5e-324, 1e-300, 2.0 ** -1022, 7.0 / 16, 11.0 / 16, 19.0 / 16, 39.0 / 16,
              0.5, np.nextafter(7.0 / 16, 0.0), np.nextafter(11.0 / 16, 1.0), 1e300])
    sp = np.concatenate([sp, -sp])
    a, b = np.meshgrid(sp, sp)
    ys, xs = [a.ravel()], [b.ravel()]
    t = rng.uniform(-np.pi, np.pi, 12000)                      # unit vectors over every direction
    ys.append(np.sin(t)); xs.append(np.cos(t))
    ys.append(wide(rng, 12000, -80, 80)); xs.append(wide(rng, 12000, -4, 4))
    x = rng.uniform(0.25, 1.25, 8000)                          # ratios within four ulps of the interval edges
    y = x * rng.choice(ATAN_EDGES, 8000)
    k = rng.integers(-4, 5, 8000)
    for j in range(1, 5):
        y = np.where(k >= j, np.nextafter(y, 10.0), np.where(k <= -j, np.nextafter(y, 0.0), y))
    ys.append(y * rng.choice([-1.0, 1.0], 8000)); xs.append(x * rng.choice([-1.0, 1.0], 8000))
    for r in ATAN_EDGES:                                        # the exact ratios at x = 1 and their neighbours
        ys.append(neighbours(r, 4)); xs.append(np.ones(9))
    for gap in (59, 60, 61, 62):                                # exponent gaps, both ways, every sign
        g = wide(rng, 300, -3, 3)
        ys.append(g * 2.0 ** gap); xs.append(wide(rng, 300, -3, 3))
        ys.append(wide(rng, 300, -3, 3)); xs.append(g * 2.0 ** gap)
    y, x = f64(np.concatenate(ys)), f64(np.concatenate(xs))
    keep = ~((y == 0) & (x == 0))
    y, x = y[keep], x[keep]
    nz = (y != 0) & (x != 0)
    # exponent gaps beyond 60 as atan2_pp tests them (on the high words): its short cuts
    k = (hiword(y) - hiword(x)) >> 20
    return {"y": y, "x": x, "nonzero": nz, "pp_reached": nz & ((k > 60) | (k < -60)), "exact": mp_map(mp.atan2, y, x)}


@functools.lru_cache(None)
def atan2_special_cases():
    """The Annex-F table with signed zeros; reference: math.atan2"""
    sp = f64([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 5e-324, -5e-324, 1e300, -1e300])
    a, b = np.meshgrid(sp, sp)
    y, x = a.ravel(), b.ravel()
    sel = (y == 0) | (x == 0) | ~np.isfinite(y) | ~np.isfinite(x)
    y, x = f64(y[sel]), f64(x[sel])
    return {"y": y, "x": x, "r": f64([math.atan2(p, q) for p, q in zip(y, x)])}


# ---- sin / cos ----------------------------------------------------------------------------------------
def _kpio2(k):
    """RN(k pi / 2)"""
    with mp.workprec(PREC):
        return f64([float(int(j) * mp.pi / 2) for j in k])


@functools.lru_cache(None)
def sincos_cases():
    rng = np.random.default_rng(116)
    ks = np.unique(np.concatenate([np.arange(1, 4097), rng.integers(4097, 2 ** 19, 3000), 2 ** 19 - np.arange(0, 64),
                                   2 ** np.arange(1, 21), rng.integers(2 ** 19, 2 ** 20, 1500), 2 ** 20 - np.arange(1, 32)]))
    kp = _kpio2(ks)
    seam = f64(np.array([(SEAM_HI << 32), (SEAM_HI << 32) | 0x33333333, (SEAM_HI << 32) | 0xFFFFFFFF,
                         ((SEAM_HI + 1) << 32), ((SEAM_HI + 1) << 32) | 1, ((SEAM_HI - 1) << 32) | 0xFFFFFFFF],
                        dtype=np.uint64).view(np.float64))
    beyond = np.concatenate([[1647100.0, 1e7, 1e10, 1e22, 2.0 ** 500, 1e300, DBL_MAX],
                             wide(rng, 200, 21, 1024, signed=False)])
    x = np.concatenate([[0.0, -0.0, PIO4, up1(PIO4), up1(PIO4, -1), 2.0 ** -27, up1(2.0 ** -27, -1), 5e-324,
                         K_MEDIUM_MAX, up1(K_MEDIUM_MAX), np.inf, -np.inf, np.nan],
                        rng.uniform(-PIO4, PIO4, 6000), wide(rng, 1000, -1000, -27),
                        kp, -kp[::3], up(kp[::5]), up(kp[::7], -1), seam, -seam, beyond, -beyond,
                        rng.uniform(-K_MEDIUM_MAX, K_MEDIUM_MAX, 5000), rng.uniform(-2 * K_MEDIUM_MAX, 2 * K_MEDIUM_MAX, 2000),
                        rng.uniform(-100, 100, 5000)])
    x = f64(x)
    medium = hiword(x) <= SEAM_HI
    fin = np.isfinite(x)
    xs = np.where(fin, x, 0.0)
    return {"x": x, "medium": medium, "finite": fin, "kpio2": kp, "ks": ks, "seam": seam,
            "sin": mp_map(mp.sin, xs), "cos": mp_map(mp.cos, xs)}


@functools.lru_cache(None)
def turn_sincos_cases():
    """up to kMediumMax (both instantiations), and `beyond` it (turn_sincos<true> only)"""
    rng = np.random.default_rng(117)
    ks = np.unique(np.concatenate([np.arange(1, 1025), rng.integers(1025, 2 ** 19, 1500), 2 ** 19 - np.arange(1, 16)]))
    kp = _kpio2(ks)
    x = np.concatenate([[0.0, -0.0, 5e-324, K_MEDIUM_MAX, -K_MEDIUM_MAX], neighbours(PIO4, 3), -neighbours(PIO4, 3),
                        rng.uniform(-PIO4, PIO4, 6000), wide(rng, 500, -1000, -20),
                        kp, up(kp, 2), up(kp, -2), kp + 1e-9, kp - 1e-9, -(kp + 1e-5), kp[::2] - 1e-5,
                        rng.uniform(-K_MEDIUM_MAX, K_MEDIUM_MAX, 4000), rng.uniform(-10, 10, 4000)])
    x = f64(x[np.abs(x) <= K_MEDIUM_MAX])
    beyond = f64(np.concatenate([[up1(K_MEDIUM_MAX), 823550.0, 1e6, -1e6, 1e10, 1e22, 1e300, np.inf, np.nan],
                                 wide(rng, 100, 20, 1024)]))
    bfin = np.isfinite(beyond)
    bs = np.where(bfin, beyond, 0.0)
    return {"x": x, "direct": np.abs(x) <= PIO4, "sin": mp_map(mp.sin, x), "cos": mp_map(mp.cos, x),
            "beyond": beyond, "beyond_finite": bfin, "beyond_sin": mp_map(mp.sin, bs), "beyond_cos": mp_map(mp.cos, bs),
            "kpio2": kp}


SMALL_MAX = 0.0709


@functools.lru_cache(None)
def sincos_small_cases():
    rng = np.random.default_rng(118)
    x = np.concatenate([[0.0, -0.0, SMALL_MAX, -SMALL_MAX, up1(SMALL_MAX, -1), 5e-324, 2.0 ** -27],
                        rng.uniform(-SMALL_MAX, SMALL_MAX, 8000), rng.uniform(SMALL_MAX - 1e-5, SMALL_MAX, 1000),
                        wide(rng, 1000, -60, -4)])
    x = f64(x[np.abs(x) <= SMALL_MAX])
    return {"x": x, "sin": mp_map(mp.sin, x), "cos": mp_map(mp.cos, x)}


# ---- the turn angle -----------------------------------------------------------------------------------
def _turn_operands(rng, m, zero_speed):
    nc = np.concatenate([[0.0, 8.0, 2.0 ** -60, 16.0], np.ldexp(rand_mant(rng, m), rng.integers(-60, 4, m).astype(np.int32)),
                         rng.uniform(0, 8, m)])
    sp = np.concatenate([[2.0 ** -113, -2.0 ** -113, 2.0 ** 21, -2.0 ** 21], wide(rng, m, -113, 21), rng.uniform(0.01, 30, m)])
    ad = np.concatenate([[0.0, 1e-300, -1e-300, np.pi], rng.uniform(-np.pi, np.pi, m), wide(rng, m, -40, 2)])
    n = min(len(nc), len(sp), len(ad))
    nc, sp, ad = nc[:n], sp[:n], ad[:n]
    if zero_speed:
        z = f64([0.0, -0.0])
        a, b = np.meshgrid(f64([0.0, 1.0, 8.0]), z)
        nc = np.concatenate([a.ravel(), a.ravel(), nc])
        sp = np.concatenate([b.ravel(), b.ravel(), sp])
        ad = np.concatenate([np.full(6, 0.3), np.full(6, -0.3), ad])
    return f64(nc), f64(sp), f64(ad)


@functools.lru_cache(None)
def turn_angle_cases():
    """turn_angle<true>: any speed, zero included; reference: the host's nc / speed / 50"""
    nc, sp, ad = _turn_operands(np.random.default_rng(119), 30000, True)
    with np.errstate(all="ignore"):
        nad = nc / sp / 50
        nad = np.where(ad < 0, nad * -1, nad)
        rot = nad - ad
    return {"nc": nc, "speed": sp, "adiff": ad, "rot": rot}


@functools.lru_cache(None)
def turn_angle_rcp_cases():
    """turn_angle<false> and turn_angle_fast: |speed| in [2^-113, 2^21]; reference: the exact
    +-nc / (speed 50) (adiff's sign) and the exact rot = that - adiff"""
    nc, sp, ad = _turn_operands(np.random.default_rng(120), 10000, False)
    with mp.workprec(PREC):
        nad = [(mpf(float(a)) / (mpf(float(b)) * 50)) * (-1 if c < 0 else 1) for a, b, c in zip(nc, sp, ad)]
        rot = [v - mpf(float(c)) for v, c in zip(nad, ad)]
    return {"nc": nc, "speed": sp, "adiff": ad, "nad": nad, "rot": rot}


# ---- SpeedController ------------------------------------------------------------------------------------
SC_SET = (0.0, 2.0 ** -60, -2.0 ** -60, 2.0 ** 20, -2.0 ** 20, 0.5, 3.0, 10.0, 17.123, 22.2, -5.0, 21.987654321)
SC_TIMES = (0.0, 2.0 ** -60, -2.0 ** -60, 2.0 ** 20, -2.0 ** 20, 0.02, 0.5, 1.0, 2.56, 4.44, 0.3333333333333333)


@functools.lru_cache(None)
def sc_cases():
    """SC fields from speed_in_range's set, t = 0.02 k (k = 1..128), shifts on both sides of t, and an
    overriding speed. All operands lie in the unchecked variants' domain."""
    rng = np.random.default_rng(121)
    m = 60000
    start = rng.choice(SC_SET, m)
    target = rng.choice(SC_SET, m)
    ord_ = rng.random(m) < 0.4                       # ordinary ramps: ego speed -> a speed-grid target
    start = np.where(ord_, rng.uniform(0, 22.2, m), start)
    target = np.where(ord_, rng.uniform(0, 22.2, m), target)
    sel = rng.random(m)
    target = np.where(sel < 0.08, start, target)                                     # target == start
    target = np.where((sel >= 0.08) & (sel < 0.12), np.nextafter(start, np.inf), target)
    target = np.where((sel >= 0.12) & (sel < 0.16), np.nextafter(start, -np.inf), target)
    target = np.where((sel >= 0.16) & (sel < 0.2), start + 1e-5 * rng.choice([0.5, 1.0, 1.5, -0.999, -1.001], m), target)
    bad = ~in_speed_range(target)                    # (a neighbour of +0 or of 2^20 outside the set)
    target = np.where(bad, start, target)
    ttime = np.where(ord_ & (rng.random(m) < 0.8), rng.uniform(0.02, 5.0, m), rng.choice(SC_TIMES, m))
    k = rng.integers(1, 129, m).astype(np.float64)
    k[:128] = np.arange(1, 129)
    t = 0.02 * k
    ch = rng.integers(0, 8, m)
    shift = np.select([ch == 0, ch == 1, ch == 2, ch == 3, ch == 4, ch == 5, ch == 6],
                      [np.zeros(m), t, t - rng.uniform(0, 1, m), t + rng.uniform(0, 1, m), np.nextafter(t, 0.0),
                       np.nextafter(t, 10.0), t - ttime], rng.uniform(-3, 3, m))
    shift = np.where(np.isfinite(shift) & (np.abs(shift) < 2.0 ** 21), shift, 0.0)
    speed = np.where(rng.random(m) < 0.7, rng.uniform(0, 22.2, m), rng.choice(SC_SET, m))
    start, target, ttime, shift, speed = map(f64, (start, target, ttime, shift, speed))
    # the target == start rows again with a shift of +0: the in-range, in-ramp 0 / ttime and 0 / 0 cases
    with np.errstate(all="ignore"):
        te = np.maximum(t - shift, 0.0)                           # sc_get_speed's clamped time
        num = (target - start) * te
        q = num / ttime
        speed_ref = np.where(te > ttime, target, start + q)
        keep = (t > ttime) | (np.abs(target - start) < K_EPS)     # sc_override's early returns
        mt = ttime * (speed - start) / (target - start)
        shift_ref = np.where(keep, shift, t - mt)
    return {"start": start, "target": target, "ttime": ttime, "shift": shift, "k": k, "t": t, "speed": speed,
            "te": te, "past": te > ttime, "q": q, "speed_ref": f64(speed_ref), "keep": keep, "mt": f64(mt),
            "shift_ref": f64(shift_ref)}


def in_speed_range(x):
    """speed_in_range's definition: +0, or a magnitude in [2^-60, 2^20]"""
    x = f64(x)
    return np.where(x == 0, ~np.signbit(x), (np.abs(x) >= 2.0 ** -60) & (np.abs(x) <= 2.0 ** 20))


@functools.lru_cache(None)
def speed_in_range_cases():
    rng = np.random.default_rng(122)
    e = neighbours([2.0 ** -60, 2.0 ** 20], 2)
    x = f64(np.concatenate([e, -e, [0.0, -0.0, np.nan, np.inf, -np.inf, -1.0, -22.2, 22.2, 5e-324, -5e-324, DBL_MAX],
                            rng.uniform(-30, 30, 2000), wide(rng, 4000, -200, 200)]))
    return {"x": x, "r": in_speed_range(x).astype(np.float64)}
