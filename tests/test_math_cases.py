"""The harness of tests/test_math_primitives.py checked on its own (no GPU): ulp_err on hand-worked
values, every edge the primitives can go wrong at present in its corpus, every unchecked (_nc)
corpus inside its documented domain, and glibc's own sin, cos and atan2 under 1 ulp against the
mpmath reference on the same corpora — a bound the GPU must meet is one a known-good
implementation meets on these inputs."""
import math

import numpy as np
from mpmath import mp, mpf

import math_cases as mc
from math_cases import member, up1


def test_ulp_err_hand_worked():
    with mp.workprec(mc.PREC):
        one = mpf(1)
        assert mc.ulp_err(1.0, one) == 0.0
        assert mc.ulp_err(1.0 + 2.0 ** -52, one) == 1.0          # ulp(1) = 2^-52
        assert mc.ulp_err(1.0 - 2.0 ** -53, one) == 0.5          # the grid below 1 is twice as fine
        assert mc.ulp_err(1.0, one + mpf(2) ** -53) == 0.5       # a true value halfway between doubles
        assert mc.ulp_err(2.0, mpf(2) - mpf(2) ** -60) == 2.0 ** -8   # true value in [1, 2): ulp 2^-52
        assert mc.ulp_err(-3.0, mpf(3)) == 6 / 2.0 ** -51
        assert mc.ulp_err(5e-324, mpf(0)) == 1.0                 # subnormal grid: 2^-1074
        assert mc.ulp_err(5e-324, mpf(2) ** -1074 * 1.5) == 0.5
        assert mc.ulp_err(2.0 ** -1022 - 2.0 ** -1074, mpf(2) ** -1022) == 1.0
        assert mc.ulp_err(2.0 ** -1021, mpf(2) ** -1021 + mpf(2) ** -1073) == 1.0
        assert mc.ulp_err(math.inf, mpf(2) ** 1024) == 0.0       # overflows: IEEE gives the infinity
        assert mc.ulp_err(-math.inf, -mpf(2) ** 1030) == 0.0
        assert mc.ulp_err(mc.DBL_MAX, mpf(2) ** 1024) == math.inf
        assert mc.ulp_err(-math.inf, mpf(2) ** 1024) == math.inf
        assert mc.ulp_err(math.inf, mpf(mc.DBL_MAX)) == math.inf
        assert mc.ulp_err(math.nan, one) == math.inf
        assert mc.ulp_err(mc.DBL_MAX, mpf(mc.DBL_MAX) + mpf(2) ** 969) == 0.5 ** 2   # below the overflow threshold
        assert list(mc.ulp_errs([1.0, 2.0], [one, mpf(2) + mpf(2) ** -51])) == [0.0, 1.0]


def test_helpers():
    assert up1(1.0) == 1.0 + 2.0 ** -52 and up1(1.0, -1) == 1.0 - 2.0 ** -53 and up1(0.0) == 5e-324
    assert list(mc.neighbours(1.0, 1)) == [1.0 - 2.0 ** -53, 1.0, 1.0 + 2.0 ** -52]
    assert mc.same_bits([0.0, np.nan, 1.0, -0.0], [-0.0, np.nan, 1.0, -0.0]).tolist() == [False, True, True, True]
    assert member(np.array([0.0, np.nan]), 0.0, np.nan) and not member(np.array([0.0]), -0.0)
    assert 1 / 50.0 == 0.02                                      # div50's r is RN(1 / 50)
    with mp.workprec(mc.PREC):                                   # fmod_2pi's 2 y and 3 y are exact doubles
        assert mpf(2.0 * mc.TWO_PI) == 2 * mpf(mc.TWO_PI) and mpf(3.0 * mc.TWO_PI) == 3 * mpf(mc.TWO_PI)
    assert int(mc.hiword(mc.K_MEDIUM_MAX)[0]) < mc.SEAM_HI


def test_sqrt_corpus_edges():
    c = mc.sqrt_rd_cases()
    q = c["q"]
    lo, hi = 2.0 ** -900, 2.0 ** 900
    assert member(q, lo, hi, up1(lo), up1(lo, -1), up1(hi), up1(hi, -1), 0.0, -0.0, 5e-324, np.inf, np.nan, -1.0)
    assert member(q, *c["perfect"][:50]) and all(math.isqrt(int(v)) ** 2 == int(v) for v in c["perfect"][:50])
    for v in c["odd27_squares"][:50]:
        assert member(q, v, up1(v), up1(v, -1))
    e = np.floor(np.log2(q[(q >= lo) & (q < hi)])).astype(int)
    assert set(range(-900, 900)) <= set(e.tolist())              # every binade
    assert c["dok"].sum() > 80000 and (~c["dok"]).sum() > 500 and len(q) <= 2 ** 18


def _has_pair(a, b, va, vb):
    a, b = mc.f64(a), mc.f64(b)
    return bool((mc.same_bits(a, np.full_like(a, va)) & mc.same_bits(b, np.full_like(b, vb))).any())


def test_div_corpus_edges():
    c = mc.div_rcp_cases()
    n, d, r, q = c["n"], c["d"], c["r"], c["q"]
    lo, hi = 2.0 ** -900, 2.0 ** 900
    for v in (lo, hi, up1(lo), up1(lo, -1), up1(hi), up1(hi, -1), -lo, -hi):
        assert member(n, v) and member(d, v)
    assert _has_pair(n, d, hi, lo) and _has_pair(n, d, 1.3 * lo, 1.7 * 2.0 ** 150)       # the issue's two cases
    inr = lambda v: (np.abs(v) >= lo) & (np.abs(v) <= hi)
    both = inr(n) & inr(d)                                       # inside div_rcp's own range test
    assert (both & np.isinf(q)).sum() >= 5                       # overflowing quotients
    assert (both & (q != 0) & (np.abs(q) < 2.0 ** -1022)).sum() >= 10     # subnormal quotients
    assert (both & (q == 0)).sum() >= 1                          # underflow to zero
    assert _has_pair(n, d, 0.0, 1.0) and _has_pair(n, d, -0.0, 1.0) and _has_pair(n, d, -0.0, -1.0)
    assert _has_pair(d, r, 50.0, 0.02)
    for v in (np.inf, -np.inf, np.nan, 0.0, -0.0):
        assert member(n, v) and member(d, v)
    assert mc.same_bits(r, mc.hostdiv(1.0, d)).all() and len(n) <= 2 ** 18
    o = mc.div_off_cases()
    for key in ("checked", "nc"):
        k = o[key]
        r0 = mc.hostdiv(1.0, k["d"])
        for off in (-2, -1, 1, 2):
            s = k["off"] == off
            assert s.sum() > 1000 and mc.same_bits(k["r"][s], mc.up(r0[s], off)).all()
        assert len(k["n"]) <= 40000
    v = mc.div50_cases()["v"]
    assert member(v, 0.0, -0.0, np.inf, np.nan, 5e-324, lo, hi, up1(hi))


def test_nc_corpora_inside_their_domain():
    dl, dh = mc.NC_D
    nl, nh = mc.NC_N
    for c in (mc.div_rcp_nc_cases(), mc.div_nc_auto_cases(), mc.div_off_cases()["nc"]):
        n, d = c["n"], c["d"]
        assert ((np.abs(d) >= dl) & (np.abs(d) <= dh)).all()
        assert (((np.abs(n) >= nl) & (np.abs(n) <= nh)) | ((n == 0) & ~np.signbit(n))).all()
        for cn in (nl, nh):
            for cd in (dl, dh):
                assert _has_pair(n, d, cn, cd)                   # the four corners
        assert (n == 0).any()
    v = mc.div50_nc_cases()["v"]
    assert (((np.abs(v) >= dl) & (np.abs(v) <= dh)) | ((v == 0) & ~np.signbit(v))).all()
    assert member(v, 0.0, dl, dh, -dl, -dh)
    s = mc.sc_cases()
    for k in ("start", "target", "ttime"):
        assert mc.in_speed_range(s[k]).all(), k
    assert np.isfinite(s["shift"]).all() and mc.in_speed_range(s["speed"]).all()
    c = mc.div_sqrt_d_cases()
    assert ((c["q"] >= 2.0 ** -900) & (c["q"] <= 2.0 ** 900)).all() and (np.abs(c["n"]) <= c["d"] * 2.0 ** 15).all()
    assert member(c["n"], 0.0) and member(c["q"], 2.0 ** -900, 2.0 ** 900) and len(c["n"]) <= 40000
    nzq = np.abs(c["ieee"][c["n"] != 0])
    assert nzq.min() >= 2.0 ** -181 and nzq.max() <= 2.0 ** 15
    t = mc.turn_angle_rcp_cases()
    assert ((np.abs(t["speed"]) >= dl) & (np.abs(t["speed"]) <= dh)).all() and (t["nc"] >= 0).all()
    assert member(t["speed"], dl, dh, -dl, -dh)


def test_fmod_corpus_edges():
    c = mc.fmod_cases()
    a, y = c["a"], mc.TWO_PI
    for k in range(4):
        v = float(np.float64(k) * y)
        assert member(a, v, up1(v), up1(v, -1), -v, -up1(v), -up1(v, -1))
    assert member(a, -0.0, 0.0, np.inf, -np.inf, np.nan, 1e300, -1e300)
    assert (np.abs(a[np.isfinite(a)]) > 1e290).sum() <= 64 and len(a) <= 2 ** 18
    assert (a < 0).sum() > 10000
    s = mc.fmod_small_cases()
    b = s["a"]
    assert ((b >= 0) & (b < 3.0 * y) | np.isnan(b)).all() and np.isnan(b).any()
    assert member(b, 0.0, y, up1(y, -1), 2 * y, up1(2 * y, -1), s["top"]) and s["top"] < 3.0 * y


def test_asin_and_seam_corpus_edges():
    s = mc.asin_cases()["s"]
    m = mc.K_STEP_SIN_MAX
    assert (np.abs(s) <= m).all() and member(s, m, -m, up1(m, -1), -up1(m, -1), 0.0, -0.0, 2.0 ** -27)
    assert (np.abs(s) < 2.0 ** -27).sum() > 1000 and (np.abs(s) > m - 1e-6).sum() > 2000 and len(s) <= 40000
    c = mc.seam_cases()
    for j in range(-8, 9):
        assert member(c["cr"], up1(m, j) if j else m, -(up1(m, j) if j else m))
    assert np.allclose(c["cr"] ** 2 + c["dt"] ** 2, 1.0, rtol=0, atol=4e-16)


def test_atan2_corpus_edges():
    c = mc.atan2_cases()
    y, x = c["y"], c["x"]
    assert 30000 <= len(y) <= 42000 and np.isfinite(y).all() and np.isfinite(x).all() and not ((y == 0) & (x == 0)).any()
    for r in mc.ATAN_EDGES:
        for j in range(-4, 5):
            assert _has_pair(y, x, up1(r, j) if j else r, 1.0)
    gap = np.abs(np.frexp(y)[1].astype(int) - np.frexp(x)[1].astype(int))
    gap = np.where((y == 0) | (x == 0), 0, gap)
    assert all((gap == g).sum() >= 100 for g in (59, 60, 61, 62))
    with np.errstate(all="ignore"):
        unit = np.abs(y * y + x * x - 1.0) < 1e-15
    ang = np.arctan2(y[unit], x[unit])
    assert unit.sum() >= 12000 and np.histogram(ang, bins=64, range=(-np.pi, np.pi))[0].min() > 50     # every direction
    assert _has_pair(y, x, 0.0, -1.0) and _has_pair(y, x, -0.0, 1.0) and _has_pair(y, x, 1.0, -0.0)
    s = mc.atan2_special_cases()
    for p in ((0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (np.inf, np.inf), (-np.inf, -np.inf), (np.inf, -np.inf),
              (1.0, np.inf), (1.0, -np.inf), (-1.0, -np.inf), (np.inf, 1.0), (0.0, -1.0), (-0.0, -1.0), (1.0, 0.0), (-1.0, -0.0),
              (np.nan, 1.0), (1.0, np.nan)):
        assert _has_pair(s["y"], s["x"], *p), p
    assert mc.same_bits(s["r"][(s["y"] == 0) & np.signbit(s["y"]) & (s["x"] == -1.0)], [-math.pi]).all()


def test_sincos_corpus_edges():
    c = mc.sincos_cases()
    x = c["x"]
    assert len(x) <= 40000 and member(x, 0.0, -0.0, mc.PIO4, np.inf, -np.inf, np.nan, mc.K_MEDIUM_MAX)
    assert (np.abs(x) < 2.0 ** -27).sum() > 1000 and (np.abs(x) <= mc.PIO4).sum() > 6000
    with mp.workprec(mc.PREC):
        for k in (1, 2, 3, 4096, 2 ** 18, 2 ** 19 - 1, 2 ** 19, 2 ** 20 - 1, 2 ** 20):
            assert member(x, float(k * mp.pi / 2)), k
    assert c["ks"].max() == 2 ** 20 and (c["ks"] <= 2 ** 19).sum() > 7000
    # arguments that need the second and the third reduction round: |x - k pi/2| below 2^-16 and
    # 2^-49 of x's binade (sincos_pp's i > 16 and i > 49)
    kp = c["kpio2"]
    with mp.workprec(mc.PREC):
        red = np.array([float(abs(mpf(float(v)) - int(k) * mp.pi / 2)) for v, k in zip(kp[:4096], c["ks"][:4096])])
    drop = np.frexp(kp[:4096])[1] - np.frexp(red)[1]
    assert (drop > 17).all() and (drop > 51).sum() >= 1000
    hw = mc.hiword(x)
    assert (hw == mc.SEAM_HI).sum() >= 6 and (hw == mc.SEAM_HI + 1).sum() >= 2
    assert member(x, *c["seam"]) and int(mc.hiword(c["seam"][2])[0]) == mc.SEAM_HI and c["seam"][2] > mc.K_MEDIUM_MAX
    assert (~c["medium"] & c["finite"]).sum() > 200
    t = mc.turn_sincos_cases()
    tx = t["x"]
    assert (np.abs(tx) <= mc.K_MEDIUM_MAX).all() and member(tx, mc.PIO4, up1(mc.PIO4), up1(mc.PIO4, -1), -mc.PIO4,
                                                            mc.K_MEDIUM_MAX, -mc.K_MEDIUM_MAX)
    assert member(tx, *mc.up(t["kpio2"][:20], 2)) and member(tx, *mc.up(t["kpio2"][-5:], -2))
    assert (np.abs(t["beyond"][t["beyond_finite"]]) > mc.K_MEDIUM_MAX).all() and len(tx) <= 40000
    s = mc.sincos_small_cases()["x"]
    assert (np.abs(s) <= mc.SMALL_MAX).all() and member(s, mc.SMALL_MAX, -mc.SMALL_MAX, 0.0)


def test_sc_and_range_corpus_edges():
    c = mc.sc_cases()
    for k in ("start", "target", "ttime"):
        assert member(c[k], 0.0, 2.0 ** -60, -2.0 ** -60, 2.0 ** 20, -2.0 ** 20), k
    assert (c["target"] == c["start"]).sum() > 3000
    one = (c["target"] == np.nextafter(c["start"], np.inf)) | (c["target"] == np.nextafter(c["start"], -np.inf))
    assert one.sum() > 3000
    assert set(c["k"].tolist()) == set(float(k) for k in range(1, 129))
    assert mc.same_bits(c["t"], 0.02 * c["k"]).all()
    assert (c["shift"] < c["t"]).sum() > 10000 and (c["shift"] > c["t"]).sum() > 10000 and (c["shift"] == c["t"]).sum() > 1000
    assert (c["keep"] & (c["target"] == c["start"])).sum() > 3000 and (~c["keep"]).sum() > 5000
    assert (c["past"]).sum() > 5000 and (~c["past"]).sum() > 5000
    assert ((c["ttime"] == 0) & ~np.signbit(c["ttime"])).sum() > 1000
    near = np.abs(np.abs(c["target"] - c["start"]) - mc.K_EPS) < 1e-8
    assert near.sum() > 500                                       # both sides of kEps
    x = mc.speed_in_range_cases()["x"]
    for b in (2.0 ** -60, 2.0 ** 20):
        assert member(x, b, up1(b), up1(b, -1), -b, -up1(b), -up1(b, -1))
    assert member(x, 0.0, -0.0, np.nan, np.inf, -np.inf, -1.0)
    assert mc.in_speed_range([0.0, -0.0, 2.0 ** -60, up1(2.0 ** -60, -1), -2.0 ** 20, up1(2.0 ** 20), np.nan, np.inf]).tolist() == \
        [True, False, True, False, True, False, False, False]


def test_turn_angle_corpus_edges():
    c = mc.turn_angle_cases()
    assert _has_pair(c["nc"], c["speed"], 0.0, 0.0) and _has_pair(c["nc"], c["speed"], 8.0, -0.0)
    assert (c["adiff"] < 0).sum() > 10000 and member(c["adiff"], 0.0) and member(c["nc"], 0.0)
    assert np.isinf(c["rot"]).sum() >= 4 and np.isnan(c["rot"]).sum() >= 2


def test_glibc_meets_the_one_ulp_bounds():
    """The bounds the GPU primitives are held to, met by glibc's sin, cos and atan2 on the same
    corpora against the same mpmath references"""
    c = mc.sincos_cases()
    f = c["finite"]
    x = c["x"][f]
    es = mc.ulp_errs(np.sin(x), [e for e, k in zip(c["sin"], f) if k])
    ec = mc.ulp_errs(np.cos(x), [e for e, k in zip(c["cos"], f) if k])
    assert es.max() < 1.0 and ec.max() < 1.0, (es.max(), ec.max())
    a = mc.atan2_cases()
    nz = a["nonzero"]
    ea = mc.ulp_errs([math.atan2(p, q) for p, q in zip(a["y"][nz], a["x"][nz])], [e for e, k in zip(a["exact"], nz) if k])
    assert ea.max() < 1.0, ea.max()
    s = mc.asin_cases()
    assert mc.ulp_errs([math.asin(v) for v in s["s"]], s["exact"]).max() < 1.0
