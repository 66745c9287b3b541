#!/usr/bin/env python
"""CPU study of the fitDisp line search's evaluator policy (csrc/fit_disp.hip, DSQ_DISP_PREDICT / DSQ_DISP_GAMMA).

The search (src/DESeq2.cpp:194-266) is restated here in numpy / scipy -- NOT bit-exact, statistics only: which proposals are
rejected, accepted-and-continued or final, and what a policy that sends some of them through the likelihood alone would cost.
Inputs are the bench's shapes at a few hundred genes (tests/helpers.make_case), mu-hat from the oracle's fitBeta; the MAP leg
starts where the gene-wise leg ended, with the parametric trend of the gene-wise estimates as prior mean.

  python tools/disp_search_sim.py --config C3 --genes 300 --seed 1 --size-factors lognormal --x 0.77 0.85

prints, per leg (gene-wise, MAP): proposals per gene and the share rejected, the outcome transition table, the cost of each
policy relative to today's all-fused search for every x (cost of a likelihood-only evaluation in fused evaluations; one that
turns out accepted-and-continued is followed by a fused evaluation at the same point, both charged), and per gamma the share
of proposals sent likelihood-only and the share of those that were not accepted-and-continued."""
import argparse
import os
import sys

import numpy as np
from scipy.special import digamma, gammaln

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"C2": dict(m=100, design="two_group", weights=False),
          "C3": dict(m=500, design="batch_condition", weights=False),
          "C4": dict(m=2000, design=("factor", 10), weights=False),
          "C5": dict(m=200, design="two_group", weights=True)}
GAMMAS = (0.75, 1.0, 1.25, 1.5, 2.0)
EPSILON = 1.0e-4


class Gene:
    """log_posterior / dlog_posterior of one gene (src/DESeq2.cpp:31-107)"""

    def __init__(self, y, x, mu, w, use_w, prior_mean, prior_var, use_prior, thr=1e-2):
        self.y, self.x, self.mu, self.w, self.use_w = y, x, mu, w, use_w
        self.pm, self.pv, self.use_prior = prior_mean, prior_var, use_prior
        if use_w:                   # design columns whose weights are all below the threshold drop out of the Cox-Reid matrix
            keep = [(w[x[:, c] != 0] > thr).any() for c in range(x.shape[1])]
            self.x = x[:, keep]

    def _b(self, wd):
        ww = self.w * wd if self.use_w else wd
        return self.x.T @ (ww[:, None] * self.x)

    def lp(self, la):
        a = np.exp(la); r = 1.0 / a
        t = gammaln(self.y + r) - gammaln(r) - self.y * np.log(self.mu + r) - r * np.log1p(self.mu * a)
        ll = (self.w * t).sum() if self.use_w else t.sum()
        sign, logdet = np.linalg.slogdet(self._b(1.0 / (1.0 / self.mu + a)))
        prior = -0.5 * (la - self.pm) ** 2 / self.pv if self.use_prior else 0.0
        return ll + prior - 0.5 * logdet

    def dlp(self, la):
        a = np.exp(la); r = 1.0 / a
        t = digamma(r) + np.log1p(self.mu * a) - self.mu * a / (1.0 + self.mu * a) - digamma(self.y + r) + self.y / (self.mu + r)
        ll = r * r * ((self.w * t).sum() if self.use_w else t.sum())
        wd = 1.0 / (1.0 / self.mu + a)
        cr = -0.5 * np.trace(np.linalg.solve(self._b(wd), self._b(-wd * wd)))
        prior = -(la - self.pm) / self.pv if self.use_prior else 0.0
        return (ll + cr) * a + prior


def search(G, a, min_log_alpha, kappa_0=1.0, tol=1e-6, maxit=100):
    """the search of fit_disp_kernel, MODE 0; returns log alpha and one record per proposal:
    (outcome 'R' rejected / 'A' accepted and continued / 'F' accepted and final, kappa used, kstar before the proposal)"""
    lp, dlp = G.lp(a), G.dlp(a)
    kappa, it_acc, kstar, rec = kappa_0, 0, 0.0, []
    for _ in range(maxit):
        prop = a + kappa * dlp
        if prop < -30.0:
            kappa = (-30.0 - a) / dlp
        if prop > 10.0:
            kappa = (10.0 - a) / dlp
        a_try = a + kappa * dlp
        lp_try = G.lp(a_try)
        if -lp_try <= -lp - kappa * EPSILON * dlp * dlp:
            it_acc += 1
            a = a_try
            change = lp_try - lp
            if change < tol or a < min_log_alpha:
                rec.append(("F", kappa, kstar))
                break
            rec.append(("A", kappa, kstar))
            lp, dlp = lp_try, G.dlp(a)
            kappa = min(kappa * 1.1, kappa_0)
            if it_acc % 5 == 0:
                kappa /= 2.0
        else:
            rec.append(("R", kappa, kstar))
            if np.isfinite(lp_try):
                s = kappa * dlp
                with np.errstate(all="ignore"):
                    c = 2.0 * (lp_try - lp - dlp * s) / (s * s)
                kstar = 2.0 * (1.0 - EPSILON) / -c if c < 0.0 else np.inf
            kappa /= 2.0
    return a, rec


def policies(recs, xs, gammas=GAMMAS):
    """recs: one list of proposal records per gene -> dict of the tables"""
    n_prop = sum(len(r) for r in recs)
    n_rej = sum(o == "R" for r in recs for o, _, _ in r)
    trans = {(p, o): 0 for p in "SRA" for o in "RAF"}
    for r in recs:
        prev = "S"                                     # S: the start of the search
        for o, _, _ in r:
            trans[(prev, o)] += 1
            prev = o

    def lik_only(policy, gamma, prev, t, kappa, kstar):
        if policy == "always":
            return True
        if policy == "after_reject":
            return t == 0 or prev == "R"
        return t == 0 or (prev == "R" and kappa > gamma * kstar)

    def tally(policy, gamma=1.0):
        sent = cont = 0
        for r in recs:
            prev = "S"
            for t, (o, kappa, kstar) in enumerate(r):
                if lik_only(policy, gamma, prev, t, kappa, kstar):
                    sent += 1
                    cont += o == "A"
                prev = o
        return sent, cont

    today = len(recs) + n_prop                          # the evaluation at the start value is fused under every policy
    cost = {}
    for x in xs:
        row = {}
        for name, (sent, cont) in [("always", tally("always")), ("after_reject", tally("after_reject"))] + \
                                  [("gamma=%g" % g, tally("bound", g)) for g in gammas]:
            row[name] = (len(recs) + (n_prop - sent) + x * sent + cont) / today
        sent_pf = sum(o != "A" for r in recs for o, _, _ in r)
        row["foresight"] = (len(recs) + (n_prop - sent_pf) + x * sent_pf) / today
        cost[x] = row
    share = {g: tally("bound", g) for g in gammas}
    return dict(genes=len(recs), proposals=n_prop, rejected=n_rej, trans=trans, cost=cost,
                share={g: (s / max(n_prop, 1), (s - c) / max(s, 1), c / max(s, 1)) for g, (s, c) in share.items()})


def study(config="C3", genes=300, seed=1, sf_random=True, xs=(0.77, 0.85), prior_var=None, m=None):
    """both legs on one input -> {"gene-wise": tables, "MAP": tables}"""
    from oracle import oracle
    from tests.helpers import make_case
    sh = SHAPES[config]
    d = make_case(genes, m or sh["m"], sh["design"], seed=seed, weights=sh["weights"], sf_random=sf_random)
    y = d["counts"].astype(np.float64); x = d["x"]; p = x.shape[1]; use_w = sh["weights"]
    w = np.maximum(d["weights"], 1e-6)
    lam = np.full(p, 1e-6) / np.log(2) ** 2
    fb = oracle.fitBeta(d["counts"], x, d["nf"], d["alpha_init"], np.r_[1.0, np.zeros(p - 1)], d["beta_init"], lam, d["weights"],
                        use_w, 1e-8, 100, True, 0.5)
    mu = np.maximum(d["nf"] * np.exp(fb["beta_mat"] @ x.T), 0.5)
    min_la = np.log(1e-8 / 10)
    la0 = np.log(d["alpha_init"])
    n = y.shape[0]
    rec1, la1 = [], np.zeros(n)
    for g in range(n):
        la1[g], r = search(Gene(y[g], x, mu[g], w[g], use_w, 0.0, 1.0, False), la0[g], min_la)
        rec1.append(r)
    # the MAP leg (R/core.R estimateDispersionsMAP): parametric trend of the gene-wise estimates as prior mean
    base_mean = (y / d["nf"]).mean(axis=1)
    est = np.exp(la1)
    use = est > 1e-7
    try:
        c = oracle.parametricDispersionFit(base_mean[use], est[use])
        fit = c[0] + c[1] / base_mean
    except RuntimeError:
        fit = np.full(n, oracle.trimmedMeanFit(est))
    resid = (np.log(est) - np.log(fit))[use]
    if prior_var is None:
        from scipy.special import polygamma
        mad = 1.4826 * np.median(np.abs(resid - np.median(resid)))
        prior_var = max(mad * mad - float(polygamma(1, (x.shape[0] - p) / 2.0)), 0.25)
    init = np.where(est > 0.1 * fit, est, fit)
    rec2 = []
    for g in range(n):
        rec2.append(search(Gene(y[g], x, mu[g], w[g], use_w, np.log(fit[g]), prior_var, True), np.log(init[g]), min_la)[1])
    return {"gene-wise": policies(rec1, xs), "MAP": policies(rec2, xs), "prior_var": prior_var}


def report(res, out=sys.stdout):
    for leg in ("gene-wise", "MAP"):
        t = res[leg]
        out.write("%s: %d genes, %.2f proposals per gene, %.1f %% rejected%s\n" % (
            leg, t["genes"], t["proposals"] / t["genes"], 100.0 * t["rejected"] / max(t["proposals"], 1),
            " (prior variance %.3f)" % res["prior_var"] if leg == "MAP" else ""))
        out.write("  after \\ outcome        R        A        F   rejected\n")
        for p, name in (("S", "start"), ("R", "rejection"), ("A", "acceptance")):
            row = [t["trans"][(p, o)] for o in "RAF"]
            out.write("  %-16s %8d %8d %8d   %5.1f %%\n" % (name, row[0], row[1], row[2], 100.0 * row[0] / max(sum(row), 1)))
        xs = sorted(t["cost"])
        out.write("  cost of the search / all-fused  " + "".join("   x = %.2f" % x for x in xs) + "\n")
        for name in t["cost"][xs[0]]:
            out.write("    %-28s  " % name + "".join("   %8.3f" % t["cost"][x][name] for x in xs) + "\n")
        out.write("  gamma   sent likelihood-only   of those not accepted-and-continued\n")
        for g, (s, prec, _) in sorted(t["share"].items()):
            out.write("  %5.2f   %17.1f %%   %17.1f %%\n" % (g, 100.0 * s, 100.0 * prec))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", choices=sorted(SHAPES), default="C3")
    ap.add_argument("--genes", type=int, default=300)
    ap.add_argument("--samples", type=int, default=0, help="override the shape's sample count")
    ap.add_argument("--seed", type=int, choices=(1, 2, 3), default=1)
    ap.add_argument("--size-factors", choices=("lognormal", "unit"), default="lognormal")
    ap.add_argument("--x", type=float, nargs="+", default=[0.77, 0.85], help="cost of a likelihood-only evaluation / a fused one")
    ap.add_argument("--prior-var", type=float, default=None, help="prior variance of the MAP leg (default: estimated, floor 0.25)")
    a = ap.parse_args()
    print("# %s, %d genes, seed %d, size factors %s" % (a.config, a.genes, a.seed, a.size_factors))
    report(study(a.config, a.genes, a.seed, a.size_factors == "lognormal", tuple(a.x), a.prior_var, a.samples or None))


if __name__ == "__main__":
    main()
