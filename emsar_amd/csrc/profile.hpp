// profile.hpp -- the profile-likelihood intervals behind include/emsar_hip.h: emsar_hip_profile (device) and emsar_hip_profile_cut_host (no
// HIP call).  Part of emsar_hip.hip's translation unit, included after presence.hpp: the first stages ARE the presence test's
// (PresenceRun: plan, classify, baseline, mark_absent, drop_and_reduce), so theta_hat and Lambda are its bits; k_profile_sets
// (kernels_profile.hpp) runs the searches, its items batched by the runner the presence test uses (set_items.hpp).
// One call = one ProfileRun:  plan .. drop    PresenceRun's stages on the same query: status, theta_hat, F per set, Lambda per candidate
//                             closed_form     one-transcript components: the same search on the host from F(x) = u log x - x den
//                             search          one item (set, t, side) per limit to find -- upper for every candidate of a resident
//                                             set, lower where Lambda > q or t is essential --, in batches across the three classes
//                             reduce          records -> limits, deviances, status;  copy_out in query order
// One workgroup runs one search of at most max_evals solves of at most max_iter passes each: max_evals * max_iter passes is the longest
// a workgroup can run.  The context's theta, weights and scales are not touched.

namespace {

enum ProfileStatus : int32_t {
    PROF_TWO_SIDED = EMSAR_PROFILE_TWO_SIDED, PROF_LOWER_ZERO = EMSAR_PROFILE_LOWER_ZERO, PROF_OUTSIDE = EMSAR_PROFILE_OUTSIDE,
    PROF_NOT_RESIDENT = EMSAR_PROFILE_NOT_RESIDENT, PROF_UNCONVERGED = EMSAR_PROFILE_UNCONVERGED
};

// q with erf(sqrt(q / 2)) = level: bisection on r = sqrt(q / 2) until the bracket cannot be halved
inline double profile_cut(double level) {
    double lo = 0.0, hi = 1.0;
    while (std::erf(hi) < level && hi < 64.0) hi *= 2.0;        // erf(6) rounds to 1: every level < 1 is bracketed
    for (;;) {
        const double mid = lo + 0.5 * (hi - lo);
        if (!(mid > lo && mid < hi)) break;
        if (std::erf(mid) < level) lo = mid; else hi = mid;
    }
    return 2.0 * hi * hi;
}

struct ProfileRun {
    // what the searches of one candidate (PresenceRun::cand, same index) left
    struct Limits {
        double lower = NAN, upper = NAN, dev_lower = NAN, dev_upper = NAN;
        int32_t evals = 0, status = PROF_NOT_RESIDENT;
        bool capped = false;             // a search or one of its solves hit its cap
    };
    emsar_hip_ctx *const ctx;
    PresenceRun pres;
    const int32_t nq;
    const int32_t *const query;
    const emsar_profile_outputs out;     // a copy: all NULL when the caller gave none
    ProfileSearchParams Q;
    std::vector<Limits> lim;
    SetItemRunner<ProfileItem, ProfileRec> runner;
    emsar_profile_stats st{};

    // the presence stages batch under the profile's variable too
    ProfileRun(emsar_hip_ctx *c, const emsar_em_params *p, const emsar_profile_params &pp, int32_t nq_, const int32_t *q, const emsar_profile_outputs *o)
        : ctx(c), pres(c, p, nq_, q, nullptr, "EMSAR_HIP_PROFILE_BATCH"), nq(nq_), query(q), out(o ? *o : emsar_profile_outputs{}),
          runner(c, "EMSAR_HIP_PROFILE_BATCH", "profile: an item lies outside its class's sets") {
        Q.q = profile_cut(pp.level);
        Q.dev_tol = pp.dev_tol > 0.0 ? pp.dev_tol : 1e-4;
        Q.max_evals = pp.max_evals > 0 ? pp.max_evals : 40;
        Q.reserved0 = 0;
        st.cut = Q.q;
    }

    bool found(double dev) const { return std::fabs(dev - Q.q) <= Q.dev_tol * Q.q; }

    // One limit of a one-transcript component with u > 0 reads: x(m) = u / (m den) maximises u log x - m den x; the search of the kernel
    void closed_limit(int side, double u, double den, double &x, double &dev, int32_t &evals, bool &capped) const {
        const double th = u / den, F_hat = u * std::log(th) - th * den;
        ProfileSearch S;
        S.start(side, th * den, Q.q);
        const double sqrt_q = std::sqrt(Q.q);
        for (int n = 0;;) {
            x = u / (std::exp(S.z) * den);
            const double raw = 2.0 * (F_hat - (u * std::log(x) - x * den));
            dev = raw > 0.0 ? raw : 0.0;
            evals++; n++;
            if (!(raw == raw)) { capped = true; return; }
            if (found(dev)) return;
            if (n >= Q.max_evals) { capped = true; return; }
            S.update(std::sqrt(dev) - sqrt_q);
        }
    }

    // the presence test's status of every candidate -> what the profile reports before any search; the closed form on the host
    void classify_and_closed_form() {
        lim.resize(pres.cand.size());
        for (size_t k = 0; k < pres.cand.size(); k++) {
            PresenceRun::Cand &c = pres.cand[k];
            Limits &l = lim[k];
            if (c.status == PRES_OUTSIDE) { l.status = PROF_OUTSIDE; continue; }
            if (c.status == PRES_NOT_RESIDENT) { l.status = PROF_NOT_RESIDENT; continue; }
            if (c.status == PRES_ABSENT) c.lambda = 0.0;
            if (c.status == PRES_ESSENTIAL) c.lambda = INFINITY;
            l.capped = c.status == PRES_UNCONVERGED;
            l.status = c.lambda > Q.q ? PROF_TWO_SIDED : PROF_LOWER_ZERO;
            if (l.status == PROF_LOWER_ZERO) { l.lower = 0.0; l.dev_lower = c.lambda; }
            if (c.set >= 0) continue;            // a resident set: the searches run on the device
            const double u = pres.h_usum[(size_t)c.lib], den = pres.h_den[(size_t)c.lib];
            if (!(u > 0.0)) { l.upper = Q.q / (2.0 * den); l.dev_upper = Q.q; continue; }
            closed_limit(0, u, den, l.lower, l.dev_lower, l.evals, l.capped);
            closed_limit(1, u, den, l.upper, l.dev_upper, l.evals, l.capped);
        }
    }

    // the searches of the resident candidates and what their records say
    int search_and_reduce() {
        if (!pres.use_sets) return EMSAR_HIP_OK;
        std::vector<ProfileItem> items[emsar::kSetClasses];
        std::vector<ProfileRec> recs[emsar::kSetClasses];
        std::vector<int32_t> who[emsar::kSetClasses];          // item -> cand
        for (size_t k = 0; k < pres.cand.size(); k++) {
            const PresenceRun::Cand &c = pres.cand[k];
            if (c.set < 0 || lim[k].status == PROF_OUTSIDE || lim[k].status == PROF_NOT_RESIDENT) continue;
            const double F_hat = pres.base_rec[c.cls][(size_t)pres.base_of_set[c.cls][(size_t)c.set]].F;
            for (int side = lim[k].status == PROF_TWO_SIDED ? 0 : 1; side < 2; side++) {
                items[c.cls].push_back(ProfileItem{c.set, c.loc, side, 0, c.theta_hat, F_hat});
                who[c.cls].push_back((int32_t)k);
            }
        }
        const SetsDev &D = ctx->sets;
        const SetSolveParams P = set_params(pres.p);
        HIPCHK(set_class_lds_attributes(kProfileSets));
        const int rc = runner.run(items, recs, st.search_ms, st.items_launched,
            [](const ProfileItem &it, const emsar::SetDesc &d) { return it.t >= 0 && it.t < (int32_t)d.n_t && (it.side == 0 || it.side == 1); },
            [&](int c, int threads, hipStream_t s, size_t cnt, const ProfileItem *d_items, ProfileRec *d_rec) {
                hipLaunchKernelGGL(kProfileSets[c], dim3((unsigned)cnt), dim3(threads), D.RS.max_lds[c], s, D.d_sdesc[c].get(), d_items, D.d_g_tid.get(),
                                   D.d_g_u.get(), D.d_row_w.get(), D.d_srp.get(), D.d_sent.get(), D.d_scp.get(), D.d_scrow.get(), ctx->vec.d_den.get(), d_rec, P, Q);
            });
        if (rc) return rc;
        for (int cls = 0; cls < emsar::kSetClasses; cls++)
            for (size_t i = 0; i < recs[cls].size(); i++) {
                Limits &l = lim[(size_t)who[cls][i]];
                const ProfileRec &r = recs[cls][i];
                const bool base_ok = pres.base_rec[cls][(size_t)pres.base_of_set[cls][(size_t)items[cls][i].set]].converged != 0;
                st.evals_sum += r.evals; st.passes_sum += r.passes;
                st.evals_max = std::max(st.evals_max, r.evals); st.passes_max = std::max(st.passes_max, r.passes);
                l.evals += r.evals;
                if (r.flags != (PROFILE_REC_SEARCH_OK | PROFILE_REC_SOLVES_OK) || !base_ok) l.capped = true;
                if (items[cls][i].side == 0) { l.lower = r.x; l.dev_lower = r.dev; }
                else { l.upper = r.x; l.dev_upper = r.dev; }
            }
        return EMSAR_HIP_OK;
    }

    int copy_out() {
        for (size_t k = 0; k < lim.size(); k++) {
            Limits &l = lim[k];
            PresenceRun::Cand &c = pres.cand[k];
            if (l.status == PROF_OUTSIDE || l.status == PROF_NOT_RESIDENT) c.lambda = c.theta_hat = NAN;
            else if (l.capped) l.status = PROF_UNCONVERGED;
            st.n_status[l.status]++;
        }
        for (int32_t i = 0; i < nq; i++) {
            const size_t k = (size_t)pres.cand_of_lib[(size_t)pres.lib_of(query ? query[i] : i)];
            const Limits &l = lim[k];
            if (out.lower) out.lower[i] = l.lower;
            if (out.upper) out.upper[i] = l.upper;
            if (out.dev_lower) out.dev_lower[i] = l.dev_lower;
            if (out.dev_upper) out.dev_upper[i] = l.dev_upper;
            if (out.lambda) out.lambda[i] = pres.cand[k].lambda;
            if (out.theta_hat) out.theta_hat[i] = pres.cand[k].theta_hat;
            if (out.status) out.status[i] = l.status;
            if (out.evals) out.evals[i] = l.evals;
        }
        return EMSAR_HIP_OK;
    }

    int run() {
        int rc;
        if ((rc = pres.plan()) || (rc = pres.classify()) || (rc = pres.baseline())) return rc;
        pres.mark_absent();
        if ((rc = pres.drop_and_reduce())) return rc;
        classify_and_closed_form();
        if ((rc = search_and_reduce())) return rc;
        st.items_launched += pres.st.items_launched;
        st.baseline_ms = pres.st.baseline_ms; st.drop_ms = pres.st.drop_ms;
        return copy_out();
    }
};

}  // namespace

extern "C" {

int emsar_hip_profile(emsar_hip_ctx *ctx, const emsar_em_params *p, const emsar_profile_params *pp, int32_t n_query, const int32_t *query_tids,
                      const emsar_profile_outputs *out, emsar_profile_stats *stats) {
    if (const int rc = query_ok(ctx, n_query, query_tids)) return rc;      // first: a context without a sample is a state error whatever pp says
    const emsar_profile_params prm = pp ? *pp : emsar_profile_params{0.95, 0.0, 0, 0};
    if (!(prm.level > 0.0 && prm.level < 1.0) || !std::isfinite(prm.dev_tol)) return EMSAR_HIP_ERR_ARG;
    return run_query_call<ProfileRun>(ctx, stats, p, prm, n_query, query_tids, out);
}

int emsar_hip_profile_cut_host(double level, double *cut_out) {
    if (!(level > 0.0 && level < 1.0) || !cut_out) return EMSAR_HIP_ERR_ARG;
    *cut_out = profile_cut(level);
    return EMSAR_HIP_OK;
}

}  // extern "C"
