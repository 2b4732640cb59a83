"""The profile-likelihood interval of isoform usage (include/emsar_hip.h "profile-likelihood intervals of isoform usage"): its independent
reference in numpy, shared by test_profile_usage_gpu.py.  Cases, samples and genes are those of tests/compare_usage_problems.py (UP.CASES),
each of whose two samples is one one-sample problem here; nothing the device computes enters anything here.

D_ref(u) of one sample comes from UP.Sample: e0 = Sample.at(0, .) gives usage = theta_t / X and F_hat, and Sample.profile(u, e0) the pair
(dual, feas) with dual >= P(u) >= feas, so D(u) lies in [2 (F_hat - dual), 2 (F_hat - feas)]; the width of that bracket is the
reference's own error w_ref.  Recorded per case and sample:
    usage, parts, members
    D0, D1           the dual D at the shares 1e-9 and 1 - 1e-9, or inf by the host's rule: the member(s) the end takes out have reads only
                     they explain (a row of that transcript alone with R > 0 and E > 0)
    lower_ref, upper_ref   the root of the dual D(u) = q on each side of usage, q the chi2_1 cut of level 0.95, by a bracketed search
                     (bisection, with an Illinois step where it falls inside the bracket) to |D - q| <= 1e-9; 0.0 / 1.0 where D0 / D1 <= q
    slope_lower, slope_upper   dD/du = -2 lambda X there
    w_lower, w_upper the width of the bracket there
python -m tests.profile_usage_problems --write NAME [--sample A|B] [--out FILE] computes one case (one sample of it); every search is
a few dozen plain EMs per point, seconds for the small genes and hours for the large ones, so the references are recorded in
tests/golden/profile_usage_refs.json and never computed by a test."""
import json
import os

import numpy as np

from tests import compare_problems as CP
from tests import compare_usage_problems as UP

Q95 = 3.841458820694124          # erf(sqrt(q / 2)) = 0.95
END = 1e-9
ROOT_TOL = 1e-9
G_STOP = 1e-11
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "profile_usage_refs.json")
CASES = UP.CASES
_refs = {}


def sample_of(name, which):
    """-> (prob, R, den, members, t) of sample `which` ("A" or "B") of the case"""
    prob, RA, RB, den_a, den_b, members, t = UP.case(name)
    return (prob, RA, den_a, members, t) if which == "A" else (prob, RB, den_b, members, t)


def own_reads(prob, R, den, tids):
    """does one of tids (den > 0) have a row of its own -- the transcript alone, however often -- with reads?"""
    n_tx, rp, ci, _, E = prob
    rp = rp.astype(np.int64)
    for c in np.flatnonzero((R > 0) & (E > 0)):
        row = set(int(x) for x in ci[rp[c]:rp[c + 1]])
        if len(row) == 1 and next(iter(row)) in tids and den[next(iter(row))] > 0:
            return True
    return False


def reference(prob, R, den, members, t, q=Q95, log=None):
    """the interval of transcript t of the gene `members` in one sample -> dict, or None where nothing is searched (t outside, a single
    member, a gene sum of 0)"""
    members = np.asarray(sorted(int(m) for m in members))
    if not den[t] > 0:
        return None
    S = UP.Sample(prob, R, den, members, t)
    if S.members < 2:
        return None
    e0 = S.at(0.0, 0.5)
    if not e0["X"] > 0:
        return None
    usage, F_hat = e0["th"] / e0["X"], e0["F"]
    out = dict(usage=usage, F_hat=F_hat, parts=len(S.parts), members=S.members, q=q)

    def point(u):
        p = S.profile(u, e0, g_stop=G_STOP)
        d = dict(u=u, D=2.0 * (F_hat - p["dual"]), w=2.0 * (p["dual"] - p["feas"]), slope=-2.0 * p["lam"] * p["X"])
        if log:
            log(d)
        return d

    others = set(int(m) for m in members if int(m) != int(t))
    for side, key, end, essential in ((0, "lower", END, own_reads(prob, R, den, {int(t)})), (1, "upper", 1.0 - END, own_reads(prob, R, den, others))):
        at_end = usage == (1.0 if side else 0.0)
        if at_end:
            out["D%d" % side] = 0.0
        elif essential:
            out["D%d" % side] = float("inf")
        else:
            out["D%d" % side] = point(end)["D"]
        if out["D%d" % side] <= q:
            out.update({key + "_ref": float(side), "slope_" + key: 0.0, "w_" + key: 0.0})
            continue
        lo, h_lo, hi, h_hi, kept, n = usage, -q, end, float("inf"), 0, 0            # h = D - q; the end of the side is never evaluated again
        while True:
            u = 0.5 * (lo + hi)
            if np.isfinite(h_hi) and n % 3 != 2:
                us = lo - h_lo * (hi - lo) / (h_hi - h_lo)
                if min(lo, hi) < us < max(lo, hi):
                    u = us
            d = point(u)
            n += 1
            h = d["D"] - q
            if abs(h) <= ROOT_TOL or n >= 200:
                break
            if h < 0:
                lo, h_lo = u, h
                h_hi *= 0.5 if kept == 1 else 1.0
                kept = 1
            else:
                hi, h_hi = u, h
                h_lo *= 0.5 if kept == -1 else 1.0
                kept = -1
        out.update({key + "_ref": d["u"], "slope_" + key: d["slope"], "w_" + key: d["w"], "resid_" + key: h, "points_" + key: n})
    return out


def recorded():
    if "recorded" not in _refs:
        with open(GOLDEN) as f:
            _refs["recorded"] = json.load(f)
    return _refs["recorded"]


def tested_reference(name, which):
    """the recorded reference of sample `which` of a case"""
    return recorded()[name][which]


if __name__ == "__main__":
    import sys
    import time
    write = "--write" in sys.argv
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    only = sys.argv[sys.argv.index("--sample") + 1] if "--sample" in sys.argv else "AB"
    names = [a for a in sys.argv[1:] if a in CASES] or list(CASES)
    for name in names:
        for which in only:
            t0 = time.time()
            r = reference(*sample_of(name, which), log=lambda d: print("   ", name, which, d, flush=True))
            r = {k: (int(v) if k in ("parts", "members") or k.startswith("points_") else float(v)) for k, v in r.items()}
            print(name, which, r, "%.1f s" % (time.time() - t0), flush=True)
            if write:
                have = json.load(open(out)) if os.path.exists(out) else {}
                have.setdefault(name, {})[which] = r
                with open(out, "w") as f:
                    json.dump(have, f, indent=1, sort_keys=True)
                    f.write("\n")
