"""Input builders for the device-math tests (tests/test_gpu_math.py), in plain numpy and importable without a GPU;
tests/test_math_cases_cpu.py holds them to what they claim.  Not a test itself.

Three kinds of input per entry point of csrc/dsq_math.hpp:
  random   the ordinary range, log-uniform where the range spans decades;
  edges    every threshold a branch of the routine compares with, and its k nextafter neighbours on both sides;
  layouts  for the routines that take a branch once per WAVE (__any over 64 lanes): the same ordinary elements arranged so
           that no aligned block of 64 holds a lane that triggers the slow branch (`pure`), and so that every block holds
           one (`poisoned`).  The test hook evaluates element i in thread i, so block w of the input IS wave w.
The predicates that decide a trigger are restated here (is_*_trigger) for the CPU test of the builders."""
import numpy as np

DBL_MIN = 2.2250738585072014e-308
DBL_MAX = float(np.finfo(np.float64).max)
DENORM_MIN = 5e-324
WAVE = 64
PARTIAL_LENGTHS = (1, 63, 65, 64 * 5 + 1)        # lengths that leave a partial last wave


def _bits(u):
    return float(np.array([u], dtype=np.uint64).view(np.float64)[0])


def edges(thresholds, k=3):
    """every threshold and its k nextafter neighbours below and above"""
    out = []
    for t in thresholds:
        lo = hi = np.float64(t)
        out.append(lo)
        for _ in range(k):
            with np.errstate(over="ignore"):          # (DBL_MAX's upper neighbour is Inf)
                lo = np.nextafter(lo, -np.inf)
                hi = np.nextafter(hi, np.inf)
            out += [lo, hi]
    return np.array(out, dtype=np.float64)


def loguniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


# ---- thresholds, read off the branches of csrc/dsq_math.hpp ---------------------------------------------------------------
# dexp: overflow, underflow to zero, the first subnormal result (log DBL_MIN), the reduction's k = 0 / +-1 switch (ln 2 / 2)
EXP_THRESHOLDS = [709.782712893384, -745.1332191019412, -708.3964185322641, 0.0, 0.34657359027997264, -0.34657359027997264,
                  1.0, -1.0]
# dlog: the subnormal rescaling, the mantissa split of the reduction (high word 0x3fe6a09e, and the same one binade up),
# 1 (f = 0), the ends of the range
LOG_THRESHOLDS = [DBL_MIN, _bits(0x3fe6a09e00000000), _bits(0x3ff6a09e00000000), 0.5, 1.0, 2.0, DBL_MAX, 0.0]
# dlog1p: |x| < 2^-53 returns x, the central range (sqrt(1/2) - 1, sqrt 2 - 1), the correction term's k >= 2 and k >= 54
# switches (u = 1 + x at high word 0x4006a09e and 0x4346a09e), the pole
LOG1P_THRESHOLDS = [1.1102230246251565e-16, -1.1102230246251565e-16, -0.2928932188134524, 0.41421356237309503,
                    _bits(0x4006a09e00000000) - 1.0, _bits(0x4346a09e00000000), 9007199254740992.0, -1.0, 0.0]
# the gamma family: the ten shift points (one trip fewer from each on), the pole
GAMMA_THRESHOLDS = [float(i) for i in range(1, 11)] + [0.0, DBL_MIN]
# dstirlerr: the table at the half-integers up to 15, the four series ranges.  (Positive arguments only: the table is
# indexed by 2 n.)
STIRLERR_THRESHOLDS = [0.5 * i for i in range(1, 31)] + [35.0, 80.0, 500.0]
STIRLERR_N_THRESHOLDS = STIRLERR_THRESHOLDS + [1e100]
# dpnorm_both / dpnorm_upper2: the three range edges, the subnormal results, the constant numerator below eps / 4
PNORM_THRESHOLDS = [0.67448975, float(np.sqrt(32.0)), 37.5, 38.4, 38.5, 5.5511151231257827e-17, 0.0]


def exp_edges():
    return edges(EXP_THRESHOLDS)


def log_edges():
    """legal for dlog_full / dlog / sf_log: subnormals, zeros, DBL_MAX's upper neighbour (Inf) and negatives included"""
    return np.concatenate([edges(LOG_THRESHOLDS), [-0.0, DENORM_MIN, np.inf]])


def log_subnormals(rng, n=20000):
    """log-uniform over the subnormal range [2^-1074, 2^-1022)"""
    x = np.exp2(rng.uniform(-1074.0, -1022.0, n))     # rounded to the subnormal grid
    x = x[(x > 0) & (x < DBL_MIN)]
    return np.concatenate([x, [DENORM_MIN, np.nextafter(DBL_MIN, 0.0)]])


def positive_normal(x):
    x = np.asarray(x, np.float64)
    return x[(x >= DBL_MIN) & (x < np.inf)]


def log1p_edges():
    return edges(LOG1P_THRESHOLDS)


def gamma_edges():
    return edges(GAMMA_THRESHOLDS)


def stirlerr_edges(n_form=False):
    x = edges(STIRLERR_N_THRESHOLDS if n_form else STIRLERR_THRESHOLDS)
    return x[(x > 0) & (x < 1e100)] if n_form else x[x > 0]


def pnorm_edges():
    e = edges(PNORM_THRESHOLDS)
    return np.concatenate([e, -e, [np.inf, -np.inf, np.nan, -0.0]])


# ---- random sets -----------------------------------------------------------------------------------------------------------
def positive_random(rng, n=40000):
    return np.concatenate([np.exp(rng.uniform(-30, 30, n)), rng.uniform(0, 20, n), loguniform(rng, 1e-300, 1e300, n // 4)])


def stirlerr_random(rng, n=40000):
    return np.concatenate([loguniform(rng, 1e-10, 1e99, n), rng.uniform(0.01, 600.0, n), np.arange(1, 1300) * 0.5])


def pnorm_random(rng, n=40000):
    return np.concatenate([rng.uniform(-40, 40, n), rng.normal(0, 2, n), loguniform(rng, 1e-300, 1.0, n // 8),
                           -loguniform(rng, 1e-300, 1.0, n // 8)])


# ---- wave layouts ---------------------------------------------------------------------------------------------------------
def poison_plan(n, rng):
    """where the n ordinary elements and the trigger lanes go: (total, where, trig).  Every aligned 64-block of the
    `total` slots holds exactly one trigger slot, at a random lane; `where` lists the slots of the ordinary elements in order."""
    nb = -(-n // (WAVE - 1))
    total = n + nb
    last = total - WAVE * (nb - 1)
    lane = rng.integers(0, WAVE, nb)
    lane[-1] = rng.integers(0, last)
    trig = WAVE * np.arange(nb) + lane
    mask = np.ones(total, bool)
    mask[trig] = False
    return total, np.flatnonzero(mask), trig


def poisoned(ordinary, triggers, plan):
    """the ordinary elements at plan's `where`, the trigger values (cycled) at its trigger slots"""
    total, where, trig = plan
    out = np.empty(total)
    out[where] = ordinary
    out[trig] = np.resize(np.asarray(triggers, np.float64), trig.size)
    return out


def blocks_with_trigger(is_trigger):
    """per aligned 64-block: how many lanes trigger"""
    t = np.asarray(is_trigger, bool)
    pad = (-t.size) % WAVE
    return np.concatenate([t, np.zeros(pad, bool)]).reshape(-1, WAVE).sum(axis=1)


# dlog: special = !(x >= DBL_MIN && x < Inf)
LOG_TRIGGERS = [DENORM_MIN, 1e-310, 0.0, np.inf, np.nan, -1.0, -0.0]


def is_log_trigger(x):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return ~((x >= DBL_MIN) & (x < np.inf))


def log_layouts(rng, n=64 * 300 - 17):
    x = np.concatenate([loguniform(rng, DBL_MIN, DBL_MAX, n // 2), np.exp(rng.uniform(-3, 3, n - n // 2))])
    plan = poison_plan(n, rng)
    return x, poisoned(x, LOG_TRIGGERS, plan), plan[1]


# the gamma family: a lane below 10 keeps the whole wave in the shift loop
def is_gamma_trigger(x):
    return np.asarray(x, np.float64) < 10.0


def gamma_layouts(rng, n=64 * 300 - 17):
    """pure (all >= 10: no trip), poisoned (one lane at 1e-3 per block: ten trips), where, and a third arrangement mixed at
    random with as many lanes below 10, with the slots of the ordinary elements in it"""
    x = np.concatenate([loguniform(rng, 10.0, 1e8, n // 2), rng.uniform(10.0, 60.0, n - n // 2)])
    x[:16] = np.nextafter(10.0, 11.0)
    x[16:32] = 10.0
    plan = poison_plan(n, rng)
    small = np.concatenate([rng.uniform(0.0, 10.0, n - n // 4), loguniform(rng, 1e-8, 1.0, n // 4)])
    perm = rng.permutation(2 * n)
    mixed = np.concatenate([x, small])[perm]
    where_mixed = np.argsort(perm)[:n]                # mixed[where_mixed] == x
    return x, poisoned(x, [1e-3], plan), plan[1], mixed, where_mixed


# dbd0: in the series branch, ok = |ej| < 1e280 && |ej| > 1e-150 && v > 1e-10 with v = ((x - np) / (x + np))^2
def bd0_state(x, np_):
    """(in the series branch and past the subnormal return, ok) by the operations of dbd0"""
    x = np.asarray(x, np.float64)
    np_ = np.asarray(np_, np.float64)
    with np.errstate(all="ignore"):
        series = np.abs(x - np_) < 0.1 * (x + np_)
        v = (x - np_) / (x + np_)
        s = (x - np_) * v
        series &= ~(np.abs(s) < DBL_MIN)
        ej = 2.0 * x * v
        v = v * v
        ok = (np.abs(ej) < 1e280) & (np.abs(ej) > 1e-150) & (v > 1e-10)
    return series, ok


def is_bd0_trigger(x, np_):
    series, ok = bd0_state(x, np_)
    return series & ~ok


def _np_at(x, d):
    """np with (x - np) / (x + np) ~ d"""
    return x * (1.0 - d) / (1.0 + d)


def bd0_layouts(rng, n=64 * 150 - 17):
    """(x, np) pure, (x, np) poisoned, where.  Ordinary lanes: series branch, relative distance in [1e-4, 0.09], both signs;
    the poison: relative distance 1e-7 (v = 1e-14 fails ok)"""
    x = loguniform(rng, 1e-2, 1e6, n)
    d = loguniform(rng, 1.2e-4, 0.085, n) * rng.choice([-1.0, 1.0], n)
    npp = _np_at(x, d)
    plan = poison_plan(n, rng)
    xt = loguniform(rng, 1e-2, 1e6, plan[2].size)
    npt = _np_at(xt, 1e-7 * rng.choice([-1.0, 1.0], xt.size))
    return (x, npp), (poisoned(x, xt, plan), poisoned(npp, npt, plan)), plan[1]


def bd0_random(rng, n=20000):
    """around x = np at every distance (the series at all its lengths), and far from it (the logarithm form)"""
    x = np.exp(rng.uniform(-5, 12, n))
    npp = x * np.exp(rng.normal(0, 0.2, n))
    k = n // 4
    npp[:k] = _np_at(x[:k], loguniform(rng, 1e-9, 0.2, k) * rng.choice([-1.0, 1.0], k))
    npp[k:k + 64] = x[k:k + 64]                       # x == np: the zero
    return x, npp


def bd0_edges(fast=False):
    """the 0.1 (x + np) switch from both sides and both signs, the v > 1e-10 window (relative distance 1e-5), x == np; for
    the plain form also the |ej| window at 1e-150 and 1e280 (outside what the fast form's caller vouches for)"""
    xs, nps = [], []

    def add(x, centre):
        e = edges([centre], k=6)
        xs.extend([x] * e.size)
        nps.extend(e)
    for x in (0.5, 1.0, 7.0, 1234.5, 1e6, 3.0e-7, 1e40, 1e-40):
        for d in (0.1, -0.1, 1e-5, -1e-5, 0.0):
            add(x, _np_at(x, d))
    if not fast:
        for x, d in ((1e-147, 0.05), (1e-149, 0.09), (5e-151, 0.09), (1e281, 0.09), (5e280, 0.05), (1e282, 1e-3),
                     (1e-300, 0.01), (1e-160, 1e-7)):
            add(x, _np_at(x, d))
            add(x, _np_at(x, -d))
    return np.array(xs), np.array(nps)


# dnbinom_mu_log: the fast regime is taken when no lane fails
#   ok = size > 1e-60 && size < 1e60 && mu > 1e-60 && mu < 1e60 && x < 1e60     (among the lanes that reach the general regime)
def dnbinom_general(x, size, mu):
    """the lanes that reach the general regime of dnbinom_mu_log (past every early return)"""
    x, size, mu = (np.asarray(v, np.float64) for v in (x, size, mu))
    with np.errstate(invalid="ignore"):
        return (~(np.isnan(x) | np.isnan(size) | np.isnan(mu)) & ~((mu < 0) | (size < 0)) & ~((x < 0) | ~np.isfinite(x)) &
                np.isfinite(size) & (x != 0) & ~(x < 1e-10 * size))


def is_dnbinom_trigger(x, size, mu):
    x, size, mu = (np.asarray(v, np.float64) for v in (x, size, mu))
    ok = (size > 1e-60) & (size < 1e60) & (mu > 1e-60) & (mu < 1e60) & (x < 1e60)
    return dnbinom_general(x, size, mu) & ~ok


def dnbinom_layouts(rng, n=64 * 600 - 17):
    """(x, size, mu) pure, poisoned, where: ordinary lanes in the general regime and inside the guard; the poison has
    mu = 1e-61 with an ordinary x and size"""
    def draw(k):
        x = np.floor(loguniform(rng, 1.0, 5000.0, k))
        size = loguniform(rng, 1e-3, 1e9, k)
        return x, size
    x, size = draw(n)
    mu = loguniform(rng, 1e-6, 1e6, n)
    mu[:2000] = x[:2000] * (1 + rng.normal(0, 1e-3, 2000)) + 1e-9     # x ~ np: the series of bd0
    plan = poison_plan(n, rng)
    xt, st = draw(plan[2].size)
    return (x, size, mu), (poisoned(x, xt, plan), poisoned(size, st, plan), poisoned(mu, [1e-61], plan)), plan[1]


def dnbinom_random(rng, n=100000):
    """every regime in one set: zeros, x < 1e-10 size, the general regime inside and outside the guard, in random lanes"""
    x = np.floor(loguniform(rng, 1.0, 5000.0, n))
    x[rng.uniform(size=n) < 0.2] = 0.0
    size = loguniform(rng, 1e-3, 1e9, n)
    mu = loguniform(rng, 1e-6, 1e6, n)
    k = n // 2
    size[k:] = loguniform(rng, 1e-70, 1e70, n - k)
    mu[k:] = loguniform(rng, 1e-70, 1e70, n - k)
    big = rng.uniform(size=n) < 0.02
    x[big] = np.floor(loguniform(rng, 1.0, 1e62, int(big.sum())))
    return x, size, mu


def dnbinom_guard_corners():
    """size and mu from the nextafter neighbours of 1e-60 and 1e60 in all four corner pairings, x in {1, 1e3, 1e59} and
    around 1e60; and x just above and below 1e-10 size for the branch in front of the general regime (integer-valued x)"""
    lo, hi = edges([1e-60]), edges([1e60])
    xs, ss, ms = [], [], []
    for sv in (lo, hi):
        for mv in (lo, hi):
            for x in (1.0, 1e3, 1e59, float(np.nextafter(1e60, 0.0)), 1e60, float(np.nextafter(1e60, np.inf))):
                s, m = np.meshgrid(sv, mv, indexing="ij")
                xs.append(np.full(s.size, x)); ss.append(s.ravel()); ms.append(m.ravel())
    # x against 1e-10 size: x an integer, size on both sides of 1e10 x
    for x in (1.0, 3.0, 1000.0, 123456.0):
        s = edges([x * 1e10], k=4)
        for mu in (0.5, 1e4, 1e12, 1e-61):
            xs.append(np.full(s.size, x)); ss.append(s); ms.append(np.full(s.size, mu))
    return np.concatenate(xs), np.concatenate(ss), np.concatenate(ms)


# ---- ddiv_n / drcp_n -------------------------------------------------------------------------------------------------------
DIV_X_RANGE = (1e-200, 1e200)          # |divisor|
DIV_Q_RANGE = (1e-250, 1e250)          # |quotient|
DIV_A_MIN = 1e-250                     # |numerator|, or zero


def _mantissa(rng, n):
    """random 53-bit mantissas in [1, 2)"""
    return 1.0 + rng.integers(0, 1 << 52, n).astype(np.float64) * 2.0 ** -52


def div_operands(rng, n=60000):
    """(a, x): random over the whole range, a = +0, quotients next to rounding boundaries, extreme mantissas; both signs"""
    sgn = lambda k: rng.choice([-1.0, 1.0], k)
    x = loguniform(rng, *DIV_X_RANGE, n) * sgn(n)
    q = loguniform(rng, *DIV_Q_RANGE, n) * sgn(n)
    with np.errstate(all="ignore"):
        a = q * x
    keep = (np.abs(a) >= DIV_A_MIN) & np.isfinite(a)
    a, x = a[keep], x[keep]
    # hard rounding: a = RN(q x) and its neighbours put a / x next to q, a representable number, and next to the midpoints
    m = n // 3
    qh = _mantissa(rng, m) * np.ldexp(1.0, rng.integers(-300, 300, m)) * sgn(m)
    xh = _mantissa(rng, m) * np.ldexp(1.0, rng.integers(-300, 300, m)) * sgn(m)
    with np.errstate(all="ignore"):
        ah = qh * xh
    keep = (np.abs(ah) >= 1e-240) & (np.abs(ah) < 1e300)
    ah, xh = ah[keep], xh[keep]
    ah = np.concatenate([np.nextafter(ah, -np.inf), ah, np.nextafter(ah, np.inf)])
    xh = np.concatenate([xh, xh, xh])
    # mantissas of all ones and 1 + ulp (and 1, 1.5) at a spread of exponents
    mant = np.array([1.0, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52, 1.5, 1.0 + 2.0 ** -26])
    ex = np.array([-600, -300, -53, -1, 0, 1, 52, 300, 600])
    xa = (mant[:, None] * np.ldexp(1.0, ex)[None, :]).ravel()
    A, X = np.meshgrid(np.concatenate([xa, -xa]), np.concatenate([xa, -xa]), indexing="ij")
    A, X = A.ravel(), X.ravel()
    a_all = np.concatenate([a, ah, A, np.zeros(128)])                 # a = +0 over divisors of both signs
    x_all = np.concatenate([x, xh, X, np.abs(x[:64]), -np.abs(x[64:128])])
    return div_in_range(a_all, x_all)


def div_negative_zero(rng, n=128):
    """(a, x) with a = -0: outside what ddiv_n promises (its comment: the result is +0 whatever the divisor's sign, where
    IEEE division gives -0 over a positive divisor) and outside what any caller forms"""
    x = loguniform(rng, *DIV_X_RANGE, n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    return -np.zeros(n), x


def div_hard_cases(rng, n=4000, residues=(1, 3, 5, 255, 1023)):
    """(a, x) whose exact quotient lies next to the MIDPOINT of two neighbouring doubles, as close as a quotient of doubles
    can: for an odd 53-bit integer X and a small odd r, the odd 54-bit M with M X = -r (mod 2^54) gives the integer
    A = (M X + r) / 2^54 < 2^53 and A / X = M / 2^54 + r / (2^54 X) -- the midpoint M / 2^54 missed by a relative 2^-107 r,
    on the side of the sign of r.  A quotient whose error before the final rounding exceeds that lands on the wrong side:
    these separate a refined reciprocal from a nearly refined one, which random operands (and the operands next to
    REPRESENTABLE quotients above) do not.  Scaled by powers of two (exact) over the stated range, both signs."""
    two54 = 1 << 54
    a_out, x_out = [], []
    for X in (rng.integers(1 << 51, 1 << 52, n) * 2 + 1).tolist():
        inv = pow(X, -1, two54)
        for r in residues:
            for rr in (r, -r):
                M = (-rr * inv) % two54
                if M < (1 << 53):
                    continue
                A, rem = divmod(M * X + rr, two54)
                assert rem == 0 and 0 < A < (1 << 53)
                a_out.append(float(A))
                x_out.append(float(X))
    a = np.array(a_out)
    x = np.array(x_out)
    ea = rng.integers(-500, 400, a.size)
    ex = rng.integers(-600, 500, a.size)
    sgn = rng.choice([-1.0, 1.0], (2, a.size))
    return div_in_range(np.ldexp(a, ea) * sgn[0], np.ldexp(x, ex) * sgn[1])


def div_in_range(a, x):
    """the pairs inside the stated operand range: |x| in DIV_X_RANGE, a zero or |a| >= DIV_A_MIN, |a / x| in DIV_Q_RANGE"""
    with np.errstate(all="ignore"):
        q = np.abs(a / x)
    ok = (np.abs(x) >= DIV_X_RANGE[0]) & (np.abs(x) <= DIV_X_RANGE[1]) & \
         ((a == 0) | ((np.abs(a) >= DIV_A_MIN) & (q >= DIV_Q_RANGE[0]) & (q <= DIV_Q_RANGE[1])))
    return a[ok], x[ok]


# ---- the closed split of nbinomLogLike ------------------------------------------------------------------------------------
def nb_split_inputs(rng, n=100000):
    """(y, alpha, mu): y in {0} u [1, 1e9] (integers), alpha over 1e-12 .. e^10 and the values that are not `fast` (0, Inf,
    NaN, negative), mu over 1e-30 .. 1e30; samples outside the split (0 < y < 1e-10 / alpha) among them"""
    y = np.floor(loguniform(rng, 1.0, 1e9, n))
    y[rng.uniform(size=n) < 0.2] = 0.0
    y[:64] = 1e9
    alpha = loguniform(rng, 1e-12, np.exp(10.0), n)
    mu = loguniform(rng, 1e-30, 1e30, n)
    k = n // 4
    mu[:k] = np.maximum(y[:k], 0.3) * np.exp(rng.normal(0, 0.5, k))          # the workload's regime: mu near y
    out = slice(k, k + n // 10)                                               # outside the split: y < 1e-10 size
    alpha[out] = loguniform(rng, 1e-12, 1e-11, n // 10)
    y[out] = np.floor(rng.uniform(0, 1.0, n // 10) * 1e-10 / alpha[out])
    odd = np.array([0.0, np.inf, np.nan, -1.0, -1e-3, -np.inf, 1e-12, np.exp(10.0), 1e-8])
    at = rng.choice(n, 4000, replace=False)
    alpha[at] = np.resize(odd, at.size)
    return y, alpha, mu


def nb_split_outside(y, alpha):
    """samples that the split hands to the full density although alpha is `fast`"""
    with np.errstate(all="ignore"):
        size = 1.0 / alpha
        fast = (alpha > 0) & np.isfinite(alpha) & np.isfinite(size) & (size > 0)
        return fast & (y > 0) & (y < 1e-10 * size)


# ---- sf_log / sf_exp: the values at the edges of the domain, as a literal table ----------------------------------------------
SF_LOG_TABLE = [(0.0, -np.inf), (-0.0, -np.inf), (np.inf, np.inf), (-1.0, np.nan), (-DENORM_MIN, np.nan), (-np.inf, np.nan),
                (np.nan, np.nan), (1.0, 0.0)]
SF_EXP_TABLE = [(-np.inf, 0.0), (np.inf, np.inf), (np.nan, np.nan), (0.0, 1.0), (-0.0, 1.0), (710.0, np.inf), (-746.0, 0.0)]


def check_table(f, table, what):
    x = np.array([t[0] for t in table])
    want = np.array([t[1] for t in table])
    got = np.asarray(f(x))
    same = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), "%s: %r -> %r, want %r" % (what, x[~same], got[~same], want[~same])


# ---- order_key / order_unkey -----------------------------------------------------------------------------------------------
def order_inputs(rng, n=20000):
    """+-0, +-subnormals, +-DBL_MIN, +-DBL_MAX, +-Inf, random normals of both signs; no NaN (the callers keep it away)"""
    pos = np.concatenate([[0.0, DENORM_MIN, 1e-310, np.nextafter(DBL_MIN, 0.0), DBL_MIN, np.nextafter(DBL_MIN, 1.0), 1.0,
                           np.nextafter(DBL_MAX, 0.0), DBL_MAX, np.inf],
                          loguniform(rng, DBL_MIN, DBL_MAX, n), rng.normal(0, 1, n) ** 2 + 1e-3,
                          log_subnormals(rng, 500)])
    x = np.concatenate([pos, -pos])
    return x[rng.permutation(x.size)]


def order_key_np(x):
    """the bit trick restated: negative numbers complemented, the others with the sign bit set"""
    b = np.ascontiguousarray(x, np.float64).view(np.uint64)
    return np.where((b >> np.uint64(63)) != 0, ~b, b | np.uint64(1 << 63))


def order_unkey_np(k):
    k = np.ascontiguousarray(k, np.uint64)
    return np.where((k >> np.uint64(63)) != 0, k & np.uint64((1 << 63) - 1), ~k).astype(np.uint64).view(np.float64)


def check_order_properties(x, keys, back):
    """properties, not a restatement: x without NaN, keys its order keys as uint64, back the round trip
      1. sorting by key gives the numeric order, -0 before +0;
      2. distinct bit patterns have distinct keys;
      3. the round trip returns the input's bits."""
    x = np.ascontiguousarray(x, np.float64)
    keys = np.ascontiguousarray(keys).view(np.uint64)
    assert not np.isnan(x).any()
    by_key = x[np.argsort(keys, kind="stable")]
    want = x[np.lexsort((~np.signbit(x), x))]         # numeric order; among equals (the zeros) the negative sign first
    assert np.array_equal(np.sort(x), want)
    assert np.array_equal(by_key.view(np.uint64), want.view(np.uint64)), "order by key is not the numeric order"
    assert np.unique(keys).size == np.unique(x.view(np.uint64)).size, "keys of distinct bit patterns collide"
    assert np.array_equal(np.ascontiguousarray(back, np.float64).view(np.uint64), x.view(np.uint64)), "round trip changes bits"
