"""Writes tests/golden/pt_golden.json: exact Student-t tails for tests/test_student_t_cpu.py and tests/test_gpu_student_t.py.

    python tests/golden/make_golden_pt.py

Every value is computed at 60 digits from the doubles (q, df) as they are: the upper tail of |q| is I_x(df/2, 1/2) / 2 with
x = df / (df + q^2) (mpmath.betainc); where that does not converge (the largest df), quadrature of the density over split
points takes its place, and on df >= 5, 1e-3 <= |q| <= 6.4 both run and must agree to 1e-25.  Records are [tail, q, df, value] with q, df as
repr() of the double and the value to 30 significant digits; tails below the smallest normal double go to "tiny".
"""
import json
import os

import mpmath as mp

mp.mp.dps = 60

DF = [0.05, 0.3, 0.5, 1, 2, 3, 3.7, 5.5, 10, 30, 47.25, 100, 1e3, 2e4, 1e6, 1e8]
AQ = [0, 1e-300, 1e-20, 1e-8, 1e-3, 0.1, 0.5, 1, 1.5, 2, 3, 4.5, 6, 6.4, 8, 12, 20, 37, 60, 200, 1e3, 1e5, 1e10, 1e50, 1e150,
      1e300]
DBL_MIN = mp.mpf(2.2250738585072014e-308)


def switch_points(df):
    """arguments on either side of the method's range switches (deseq2_amd/student_t.py): t = q^2 / df at 1 and at 1e100,
    |q| at 2"""
    import numpy as np
    out = []
    r = float(np.sqrt(df))
    for c in (r, r * 1e50, 2.0):
        out += [float(np.nextafter(c, 0.0)), c, float(np.nextafter(c, np.inf)), c * (1 - 1e-9), c * (1 + 1e-9)]
    return out


def by_beta(aq, df):
    x = df / (df + aq * aq)
    return mp.betainc(df / 2, mp.mpf(1) / 2, 0, x, regularized=True) / 2


def by_quad(aq, df):
    """the integral of the density over u = |q| e^s, s from 0 to infinity, with split points on the scale 1 / q^2 on which the
    integrand falls"""
    lc = mp.loggamma((df + 1) / 2) - mp.loggamma(df / 2) - mp.log(mp.pi * df) / 2

    def f(s):
        u = aq * mp.exp(s)
        return mp.exp(lc - (df + 1) / 2 * mp.log1p(u * u / df)) * u
    w = 1 / max(aq * aq, 1)
    return mp.quad(f, [0] + [w * s for s in (0.25, 1, 4, 16, 64, 256, 1024, 4096, 1e5, 1e7, 1e10)] + [mp.inf])


def upper_of_abs(aq, df, stats):
    aq, df = mp.mpf(aq), mp.mpf(df)
    if aq == 0:
        return mp.mpf(1) / 2
    b = None
    try:
        b = by_beta(aq, df)
    except mp.libmp.NoConvergence:
        stats["noconv"] += 1
    if b is None or (df >= 5 and 1e-3 <= aq <= 6.4):
        # the quadrature is good where the density falls like a Gaussian (moderate |q|, q^2 well below df); deep in a
        # power-law tail it is not, and there it is neither used as a check nor trusted as a stand-in
        qd = by_quad(aq, df)
        if b is not None:
            stats["checked"] += 1
            assert abs(qd - b) <= mp.mpf(10) ** -25 * b, (aq, df, qd, b)
        else:
            assert qd < mp.mpf(10) ** -1000 or (aq <= 12 and aq * aq * 1000 < df), (aq, df, qd)
            stats["fallback"].append((float(aq), float(df)))
            b = qd
    return b


def main():
    normal, tiny = [], []
    stats = {"noconv": 0, "checked": 0, "fallback": []}
    for df in DF:
        for aq in AQ + switch_points(df):
            half = upper_of_abs(aq, float(df), stats)
            for q in ((aq, -aq) if aq != 0 else (0.0,)):
                small, large = half, 1 - half                  # (never 1 - (1 - half): that would round the tail away)
                for tail, v in (("upper", small if q >= 0 else large), ("lower", large if q >= 0 else small)):
                    rec = [tail, repr(float(q)), repr(float(df)), mp.nstr(v, 30, min_fixed=0, max_fixed=0)]
                    (tiny if v < DBL_MIN else normal).append(rec)
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "pt_golden.json"), "w") as f:
        json.dump({"digits": 30, "normal": normal, "tiny": tiny}, f, indent=0)
    print("normal", len(normal), "tiny", len(tiny), stats)


if __name__ == "__main__":
    main()
