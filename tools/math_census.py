"""Accuracy census of the candidate loop's FP64 primitives on the GPU: the corpora of
tests/math_cases.py through ppamd.math_eval, written to profiles/math_primitives.json. Per kind:
the input count and, where the claim is exactness, the number of inputs that differ from the host's
IEEE result; where it is an ulp bound, the maximum error in ulps of the exact (mpmath) value with the
input that produced it and, for the quotient kinds, the share of results that are not the correctly
rounded quotient. tests/test_math_primitives.py asserts the bounds; this records the figures.

Usage: python tools/math_census.py [out.json]   (needs the built library and a GPU)"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "carnd-path-planning-project_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import math_cases as mc  # noqa: E402
import ppamd  # noqa: E402
from mpmath import mp, mpf  # noqa: E402


def ev(kind, *arrays):
    import torch
    dev = torch.device("cuda", 0)
    out = ppamd.math_eval(kind, *[torch.from_numpy(mc.f64(a)).to(dev) for a in arrays], device=0)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def exact_rec(got, ref, mask=None):
    ok = mc.same_bits(got, ref)
    if mask is not None:
        ok = ok[mask]
    return {"n": int(len(ok)), "differ_from_ieee": int((~ok).sum())}


def ulp_rec(got, exact, inputs, rn=None, mask=None):
    if mask is not None:
        got, inputs = got[mask], [a[mask] for a in inputs]
        exact = [e for e, k in zip(exact, mask) if k]
        rn = rn[mask] if rn is not None else None
    e = mc.ulp_errs(got, exact)
    i = int(np.argmax(e))
    rec = {"n": int(len(e)), "max_ulp": float(e[i]), "at": [float(a[i]).hex() for a in inputs]}
    if rn is not None:
        rec["not_correctly_rounded_share"] = float((~mc.same_bits(got, rn)).mean())
    return rec


def abs_rec(got, exact, inputs, mask=None):
    if mask is not None:
        got, inputs = got[mask], [a[mask] for a in inputs]
        exact = [e for e, k in zip(exact, mask) if k]
    with mp.workprec(mc.PREC):
        e = np.array([abs(float(mpf(float(g)) - r)) for g, r in zip(got, exact)])
    i = int(np.argmax(e))
    return {"n": int(len(e)), "max_abs": float(e[i]), "at": [float(a[i]).hex() for a in inputs]}


def census():
    R = {}
    c = mc.sqrt_rd_cases()
    d, rd, dok = ev("sqrt_rd", c["q"])
    R["sqrt_rd.d"] = exact_rec(d, c["d"])
    R["sqrt_rd.dok"] = exact_rec(dok, c["dok"].astype(np.float64))
    R["sqrt_rd.rd_slow_path"] = exact_rec(rd, c["rd"], ~c["dok"])
    c = mc.div_rcp_cases()
    R["div_rcp(r=RN(1/d))"] = exact_rec(ev("div_rcp", c["n"], c["d"], c["r"])[0], c["q"])
    R["div_rcp(2^900, 2^-900, 2^900)"] = float(ev("div_rcp", [2.0 ** 900], [2.0 ** -900], [2.0 ** 900])[0][0])
    c = mc.div50_cases()
    R["div50"] = exact_rec(ev("div50", c["v"])[0], c["q"])
    c = mc.div50_nc_cases()
    R["div50_nc"] = exact_rec(ev("div50_nc", c["v"])[0], c["q"])
    c = mc.div_rcp_nc_cases()
    R["div_rcp_nc(r=RN(1/d))"] = exact_rec(ev("div_rcp_nc", c["n"], c["d"], c["r"])[0], c["q"], c["n"] != 0)
    c = mc.fmod_cases()
    R["fmod_2pi"] = exact_rec(ev("fmod_2pi", c["a"])[0], c["r"])
    c = mc.fmod_small_cases()
    R["fmod_2pi_small"] = exact_rec(ev("fmod_2pi_small", c["a"])[0], c["r"])
    c = mc.rcp_cases()
    R["rcp_nr"] = ulp_rec(ev("rcp_nr", c["d"])[0], c["exact"], [c["d"]], mc.hostdiv(1.0, c["d"]))
    c = mc.div_auto_cases()
    R["div_rcp_auto"] = ulp_rec(ev("div_rcp_auto", c["n"], c["d"])[0], c["exact"], [c["n"], c["d"]], c["q"])
    c = mc.div_nc_auto_cases()
    R["div_rcp_nc_auto"] = ulp_rec(ev("div_rcp_nc_auto", c["n"], c["d"])[0], c["exact"], [c["n"], c["d"]], c["q"], c["n"] != 0)
    o = mc.div_off_cases()
    for kind, c in (("div_rcp", o["checked"]), ("div_rcp_nc", o["nc"])):
        R[kind + "(r 1-2 ulps off)"] = ulp_rec(ev(kind, c["n"], c["d"], c["r"])[0], c["exact"], [c["n"], c["d"], c["r"]],
                                               mc.hostdiv(c["n"], c["d"]), c["n"] != 0)
    c = mc.div_sqrt_cases()
    ex = [e if e is not None else mpf(0) for e in c["exact"]]
    R["div_rcp_n"] = ulp_rec(ev("div_rcp_n", c["n"], c["q"])[0], ex, [c["n"], c["q"]], c["ieee"], c["dok"])
    c = mc.div_sqrt_d_cases()
    R["div_rcp_d"] = ulp_rec(ev("div_rcp_d", c["n"], c["q"])[0], c["exact"], [c["n"], c["q"]], c["ieee"])
    c = mc.asin_cases()
    R["asin_small"] = ulp_rec(ev("asin_small", c["s"])[0], c["exact"], [c["s"]])
    c = mc.atan2_cases()
    (f,) = ev("atan2_fast", c["y"], c["x"])
    (p,) = ev("atan2_pp", c["y"], c["x"])
    R["atan2_fast"] = ulp_rec(f, c["exact"], [c["y"], c["x"]], mask=c["nonzero"])
    R["atan2_unit"] = exact_rec(ev("atan2_unit", c["y"], c["x"])[0], f)
    R["atan2_pp(exponent gap > 60)"] = ulp_rec(p, c["exact"], [c["y"], c["x"]], mask=c["pp_reached"])
    R["atan2_pp(every finite nonzero pair; no caller)"] = ulp_rec(p, c["exact"], [c["y"], c["x"]], mask=c["nonzero"])
    c = mc.sincos_cases()
    s, co = ev("sincos", c["x"])
    big = ~c["medium"] & c["finite"]
    R["sincos_pp.sin"] = ulp_rec(s, c["sin"], [c["x"]], mask=c["medium"])
    R["sincos_pp.cos"] = ulp_rec(co, c["cos"], [c["x"]], mask=c["medium"])
    R["sincos_pp.sin(library range)"] = abs_rec(s, c["sin"], [c["x"]], big)
    R["sincos_pp.cos(library range)"] = abs_rec(co, c["cos"], [c["x"]], big)
    c = mc.turn_sincos_cases()
    s, co = ev("turn_sincos", c["x"])
    R["turn_sincos.sin"] = abs_rec(s, c["sin"], [c["x"]])
    R["turn_sincos.cos"] = abs_rec(co, c["cos"], [c["x"]])
    R["turn_sincos.sin(|x| <= pi/4)"] = ulp_rec(s, c["sin"], [c["x"]], mask=c["direct"])
    R["turn_sincos.cos(|x| <= pi/4)"] = ulp_rec(co, c["cos"], [c["x"]], mask=c["direct"])
    c = mc.sincos_small_cases()
    s, co = ev("sincos_small", c["x"])
    R["sincos_small.sin"] = abs_rec(s, c["sin"], [c["x"]])
    R["sincos_small.cos"] = abs_rec(co, c["cos"], [c["x"]])
    c = mc.turn_angle_cases()
    R["turn_angle"] = exact_rec(ev("turn_angle", c["nc"], c["speed"], c["adiff"])[0], c["rot"])
    c = mc.turn_angle_rcp_cases()
    for kind in ("turn_angle_nolarge", "turn_angle_fast"):
        # the error of nad = nc 0.02 r against the exact nc / (speed 50), in units of 2^-52 |nad|, after
        # taking off the final subtraction's half ulp of rot (what the reciprocal chain contributes)
        (r,) = ev(kind, c["nc"], c["speed"], c["adiff"])
        with mp.workprec(mc.PREC):
            e = np.array([float((abs(mpf(float(g)) - x) - mc.ulp_of(x) / 2) / (abs(n) * mpf(2) ** -52)) if n != 0 else 0.0
                          for g, x, n in zip(r, c["rot"], c["nad"])])
        i = int(np.argmax(e))
        R[kind] = {"n": int(len(e)), "max_nad_error_2m52_relative": float(e[i]),
                   "at": [float(a[i]).hex() for a in (c["nc"], c["speed"], c["adiff"])]}
    c = mc.sc_cases()
    d2, d3 = np.stack([c["shift"], c["k"]]), np.stack([c["shift"], c["k"], c["speed"]])
    for kind in ("sc_speed", "sc_speed_r", "sc_speed_r_nc"):
        R[kind] = exact_rec(ev(kind, c["start"], c["target"], c["ttime"], d2)[0], c["speed_ref"])
    for kind in ("sc_override", "sc_override_r", "sc_override_r_nc"):
        R[kind] = exact_rec(ev(kind, c["start"], c["target"], c["ttime"], d3)[0], c["shift_ref"])
    c = mc.speed_in_range_cases()
    R["speed_in_range"] = exact_rec(ev("speed_in_range", c["x"])[0], c["r"])
    return R


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "math_primitives.json")
    rec = {"tool": "tools/math_census.py", "library": ppamd.version(), "kinds": census()}
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec["kinds"], indent=1))
