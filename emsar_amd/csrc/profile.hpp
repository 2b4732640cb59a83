// profile.hpp -- the profile-likelihood intervals behind include/emsar_hip.h: emsar_hip_profile (device) and emsar_hip_profile_cut_host (no
// HIP call).  Part of emsar_hip.hip's translation unit, included after presence.hpp: the first stages ARE the presence test's
// (PresenceRun::test: locate, baseline, mark_absent, drop_and_reduce), so theta_hat and Lambda are its bits; k_profile_sets
// (kernels_profile.hpp) runs the searches, its items batched by the runner the presence test uses (set_items.hpp).
// One call = one ProfileRun:  test            PresenceRun's stages on the same query: status, theta_hat, F per set, Lambda per candidate
//                             closed_form     one-transcript components: the kernel's search (ProfileStep) on the host from
//                                             F(x) = u log x - x den
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
    // what one candidate (SetQuery::cand of the presence stages, same index) is given
    struct Limits {
        double lower = NAN, upper = NAN, dev_lower = NAN, dev_upper = NAN;
        double lambda = NAN, theta_hat = NAN;           // the presence stages' values; NaN outside the likelihood and where not resident
        int32_t evals = 0, status = PROF_NOT_RESIDENT;
        bool capped = false;             // a search or one of its solves hit its cap
    };
    emsar_hip_ctx *const ctx;
    PresenceRun pres;
    const emsar_profile_outputs out;     // a copy: all NULL when the caller gave none
    ProfileSearchParams Q;
    std::vector<Limits> lim;
    SetItemRunner<ProfileItem, ProfileRec> runner;
    emsar_profile_stats st{};

    ProfileRun(emsar_hip_ctx *c, const emsar_em_params *p, const emsar_profile_params &pp, int32_t nq, const int32_t *query, const emsar_profile_outputs *o)
        : ctx(c), pres(c, p, nq, query, nullptr), out(o ? *o : emsar_profile_outputs{}),
          runner(c, "EMSAR_HIP_PROFILE_BATCH", "profile: an item lies outside its class's sets") {
        pres.runner.batch_env = runner.batch_env;       // the presence stages batch under the profile's variable too
        Q.q = profile_cut(pp.level);
        Q.dev_tol = pp.dev_tol > 0.0 ? pp.dev_tol : 1e-4;
        Q.max_evals = pp.max_evals > 0 ? pp.max_evals : 40;
        Q.reserved0 = 0;
        st.cut = Q.q;
    }

    // One limit of a one-transcript component with u > 0 reads: x(m) = u / (m den) maximises u log x - m den x; the search of the kernel
    // (ProfileStep).  evals and capped gather both sides.
    void closed_limit(int side, double u, double den, double &x, double &dev, int32_t &evals, bool &capped) const {
        const double th = u / den, F_hat = u * std::log(th) - th * den, sqrt_q = std::sqrt(Q.q);
        ProfileStep T;
        T.start(side, th, den, F_hat, Q);
        do x = u / (T.scale() * den);
        while (T.step(x, u * std::log(x) - x * den, F_hat, sqrt_q, Q));
        dev = T.dev;
        evals += T.evals;
        if (!T.search_ok) capped = true;
    }

    // the presence test's status of every candidate -> what the profile reports before any search; the closed form on the host
    void classify_and_closed_form() {
        lim.resize(pres.cand.size());
        for (size_t k = 0; k < pres.cand.size(); k++) {
            const PresenceRun::Test &c = pres.cand[k];
            const SetQuery::Cand &w = pres.q.cand[k];
            Limits &l = lim[k];
            if (c.status == PRES_OUTSIDE) { l.status = PROF_OUTSIDE; continue; }
            if (c.status == PRES_NOT_RESIDENT) { l.status = PROF_NOT_RESIDENT; continue; }
            l.lambda = c.reported_lambda(); l.theta_hat = c.theta_hat;
            l.capped = c.status == PRES_UNCONVERGED;
            l.status = l.lambda > Q.q ? PROF_TWO_SIDED : PROF_LOWER_ZERO;
            if (l.status == PROF_LOWER_ZERO) { l.lower = 0.0; l.dev_lower = l.lambda; }
            if (w.set >= 0) continue;            // a resident set: the searches run on the device
            const double den = pres.q.h_den[(size_t)w.lib];
            if (!(w.u > 0.0)) { l.upper = Q.q / (2.0 * den); l.dev_upper = Q.q; continue; }
            closed_limit(0, w.u, den, l.lower, l.dev_lower, l.evals, l.capped);
            closed_limit(1, w.u, den, l.upper, l.dev_upper, l.evals, l.capped);
        }
    }

    // the searches of the resident candidates and what their records say
    int search_and_reduce() {
        if (!pres.q.use_sets) return EMSAR_HIP_OK;
        std::vector<ProfileItem> items[emsar::kSetClasses];
        std::vector<ProfileRec> recs[emsar::kSetClasses];
        std::vector<int32_t> who[emsar::kSetClasses];          // item -> cand
        for (size_t k = 0; k < lim.size(); k++) {
            const SetQuery::Cand &w = pres.q.cand[k];
            if (w.set < 0 || lim[k].status == PROF_OUTSIDE || lim[k].status == PROF_NOT_RESIDENT) continue;
            for (int side = lim[k].status == PROF_TWO_SIDED ? 0 : 1; side < 2; side++) {
                items[w.cls].push_back(ProfileItem{w.set, w.loc, side, 0, lim[k].theta_hat, pres.base_of(w).F});
                who[w.cls].push_back((int32_t)k);
            }
        }
        const SetsDev &D = ctx->sets;
        const SetSolveParams P = set_params(pres.q.p);
        HIPCHK(set_class_lds_attributes(kProfileSets));
        const int rc = runner.run(items, recs, st.search_ms, st.items_launched,
            [&](int c, const ProfileItem &it) {
                const emsar::SetDesc *d = set_desc(ctx, c, it.set);
                return d && it.t >= 0 && it.t < (int32_t)d->n_t && (it.side == 0 || it.side == 1);
            },
            [&](int c, int threads, hipStream_t s, size_t cnt, const ProfileItem *d_items, ProfileRec *d_rec) {
                hipLaunchKernelGGL(kProfileSets[c], dim3((unsigned)cnt), dim3(threads), D.RS.max_lds[c], s, D.d_sdesc[c].get(), d_items, D.d_g_tid.get(),
                                   D.d_g_u.get(), D.d_row_w.get(), D.d_srp.get(), D.d_sent.get(), D.d_scp.get(), D.d_scrow.get(), ctx->vec.d_den.get(), d_rec, P, Q);
            });
        if (rc) return rc;
        for (int cls = 0; cls < emsar::kSetClasses; cls++)
            for (size_t i = 0; i < recs[cls].size(); i++) {
                Limits &l = lim[(size_t)who[cls][i]];
                const ProfileRec &r = recs[cls][i];
                const bool base_ok = pres.base_of(pres.q.cand[(size_t)who[cls][i]]).converged != 0;
                add_search_stats(st, r);
                l.evals += r.evals;
                if (r.flags != (PROFILE_REC_SEARCH_OK | PROFILE_REC_SOLVES_OK) || !base_ok) l.capped = true;
                if (items[cls][i].side == 0) { l.lower = r.x; l.dev_lower = r.dev; }
                else { l.upper = r.x; l.dev_upper = r.dev; }
            }
        return EMSAR_HIP_OK;
    }

    int copy_out() {
        for (Limits &l : lim) {
            if (l.capped) l.status = PROF_UNCONVERGED;       // never set outside the likelihood or where not resident
            st.n_status[l.status]++;
        }
        for (int32_t i = 0; i < pres.q.nq; i++) {
            const Limits &l = lim[pres.q.cand_index(i)];
            if (out.lower) out.lower[i] = l.lower;
            if (out.upper) out.upper[i] = l.upper;
            if (out.dev_lower) out.dev_lower[i] = l.dev_lower;
            if (out.dev_upper) out.dev_upper[i] = l.dev_upper;
            if (out.lambda) out.lambda[i] = l.lambda;
            if (out.theta_hat) out.theta_hat[i] = l.theta_hat;
            if (out.status) out.status[i] = l.status;
            if (out.evals) out.evals[i] = l.evals;
        }
        return EMSAR_HIP_OK;
    }

    int run() {
        int rc;
        if ((rc = pres.test())) return rc;
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
