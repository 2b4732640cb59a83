// presence.hpp -- the presence test behind include/emsar_hip.h: emsar_hip_presence (device) and emsar_hip_presence_pvalue_host (no HIP
// call).  Part of emsar_hip.hip's translation unit, included at its end after fit.hpp: it uses the context, plan_solve and set_params
// (solve.hpp), the item runner and the locator (set_items.hpp) and k_solve_sets_drop (kernels_presence.hpp).
// One call = one PresenceRun:  locate      SetQuery (set_items.hpp): which solvers a solve would run, the sets found on first use; every
//                                          queried transcript outside / not resident / closed form / candidate of a resident set
//                              baseline    one item (set, -1) per set that holds a candidate -> theta_hat in a vector of the run, F per set
//                              mark_absent candidates with theta_hat == 0
//                              drop        one item (set, t) per remaining candidate, in batches
//                              reduce      records -> Lambda, heir, status;  p-values;  copy_out in query order
// The context's theta, weights and scales are not touched: a following solve returns the same bits.

namespace {

enum PresenceStatus : int32_t {
    PRES_TESTED = EMSAR_PRESENCE_TESTED, PRES_ABSENT = EMSAR_PRESENCE_ABSENT, PRES_ESSENTIAL = EMSAR_PRESENCE_ESSENTIAL,
    PRES_OUTSIDE = EMSAR_PRESENCE_OUTSIDE, PRES_NOT_RESIDENT = EMSAR_PRESENCE_NOT_RESIDENT, PRES_UNCONVERGED = EMSAR_PRESENCE_UNCONVERGED,
    PRES_PENDING = -1                    // a candidate whose drop solve is still to come
};

// p of the boundary mixture (1/2) chi2_0 + (1/2) chi2_1
inline double presence_pvalue(double lambda) {
    if (lambda != lambda) return lambda;
    if (!(lambda > 0.0)) return 1.0;
    if (std::isinf(lambda)) return 0.0;
    return 0.5 * std::erfc(std::sqrt(lambda / 2.0));
}

struct PresenceRun {
    // what the test gives one queried transcript (SetQuery::cand, same index)
    struct Test {
        int32_t status = PRES_PENDING, heir = -1;       // heir: library index
        double lambda = NAN, share = NAN, theta_hat = NAN;
        double reported_lambda() const { return status == PRES_ABSENT ? 0.0 : status == PRES_ESSENTIAL ? INFINITY : lambda; }
    };
    emsar_hip_ctx *const ctx;
    SetQuery q;                          // where every queried transcript stands
    const emsar_presence_outputs out;    // a copy: all NULL when the caller gave none
    const int n;
    std::vector<Test> cand;
    std::vector<double> h_theta;                           // [n] theta_hat
    std::vector<int32_t> base_of_set[emsar::kSetClasses];  // set of a class -> its baseline item, -1 = none
    std::vector<PresenceRec> base_rec[emsar::kSetClasses];
    DevBuf<double> d_theta;              // [n] theta_hat: closed form and the baselined sets, the rest 0
    SetItemRunner<PresenceItem, PresenceRec> runner;
    emsar_presence_stats st{};

    PresenceRun(emsar_hip_ctx *c, const emsar_em_params *pp, int32_t nq, const int32_t *query, const emsar_presence_outputs *o)
        : ctx(c), q(c, pp, nq, query), out(o ? *o : emsar_presence_outputs{}), n(c->n_tx),
          runner(c, "EMSAR_HIP_PRESENCE_BATCH", "presence: an item lies outside its class's sets") {}

    // the locator's plan and classify, and what each standing means to the test before anything is solved
    int locate() {
        int rc;
        if ((rc = q.plan()) || (rc = q.classify())) return rc;
        cand.resize(q.cand.size());
        for (size_t k = 0; k < cand.size(); k++) {
            const SetQuery::Cand &w = q.cand[k];
            cand[k].status = w.standing == SetQuery::OUTSIDE ? PRES_OUTSIDE : w.standing == SetQuery::NOT_RESIDENT ? PRES_NOT_RESIDENT
                           : w.standing == SetQuery::CLOSED ? (w.u > 0.0 ? PRES_ESSENTIAL : PRES_ABSENT)
                           : w.own_reads ? PRES_ESSENTIAL : PRES_PENDING;
        }
        return EMSAR_HIP_OK;
    }

    // items through k_solve_sets_drop (SetItemRunner); the baseline's and the drop stage's items differ in `drop` alone
    int solve_items(const std::vector<PresenceItem> (&items)[emsar::kSetClasses], std::vector<PresenceRec> (&recs)[emsar::kSetClasses], double &ms_acc) {
        const SetsDev &D = ctx->sets;
        const SetSolveParams P = set_params(q.p);
        HIPCHK(set_class_lds_attributes(kSolveSetsDrop));
        return runner.run(items, recs, ms_acc, st.items_launched,
            [&](int c, const PresenceItem &it) { const emsar::SetDesc *d = set_desc(ctx, c, it.set); return d && it.drop >= -1 && it.drop < (int32_t)d->n_t; },
            [&](int c, int threads, hipStream_t s, size_t cnt, const PresenceItem *d_items, PresenceRec *d_rec) {
                hipLaunchKernelGGL(kSolveSetsDrop[c], dim3((unsigned)cnt), dim3(threads), D.RS.max_lds[c], s, D.d_sdesc[c].get(), d_items, D.d_g_tid.get(),
                                   D.d_g_u.get(), D.d_row_w.get(), D.d_srp.get(), D.d_sent.get(), D.d_scp.get(), D.d_scrow.get(), ctx->vec.d_den.get(), d_theta.get(), d_rec, P);
            });
    }

    // theta_hat: the closed form, and every set that holds a queried transcript solved with nothing dropped
    int baseline() {
        if (!q.use_sets) return EMSAR_HIP_OK;
        const SetsDev &D = ctx->sets;
        HIPCHK(d_theta.alloc((size_t)n));
        HIPCHK(hipMemsetAsync(d_theta, 0, (size_t)std::max(n, 2) * 8, ctx->stream));
        if (n > 0) hipLaunchKernelGGL(k_closed_form, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, n, D.d_kind.get(), D.d_usum.get(), ctx->vec.d_den.get(), d_theta.get());
        HIPCHK(hipGetLastError());
        std::vector<PresenceItem> items[emsar::kSetClasses];
        for (int c = 0; c < emsar::kSetClasses; c++) base_of_set[c].assign(D.RS.desc[c].size(), -1);
        for (const auto &w : q.cand)
            if (w.set >= 0 && base_of_set[w.cls][(size_t)w.set] < 0) {
                base_of_set[w.cls][(size_t)w.set] = (int32_t)items[w.cls].size();
                items[w.cls].push_back(PresenceItem{w.set, -1});
            }
        if (const int rc = solve_items(items, base_rec, st.baseline_ms)) return rc;
        h_theta.resize((size_t)n);
        if (n > 0) HIPCHK(hipMemcpyAsync(h_theta.data(), d_theta, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (int c = 0; c < emsar::kSetClasses; c++)
            for (const PresenceRec &r : base_rec[c])
                if (!std::isfinite(r.F)) { ctx->err = "presence: non-finite likelihood at a baseline"; return EMSAR_HIP_ERR_NUMERIC; }
        return EMSAR_HIP_OK;
    }
    // the baseline record of the set that holds candidate w
    const PresenceRec &base_of(const SetQuery::Cand &w) const { return base_rec[w.cls][(size_t)base_of_set[w.cls][(size_t)w.set]]; }

    void mark_absent() {
        if (!q.use_sets) return;
        for (size_t k = 0; k < cand.size(); k++) {
            Test &c = cand[k];
            if (c.status != PRES_NOT_RESIDENT) c.theta_hat = h_theta[(size_t)q.cand[k].lib];
            if (c.status == PRES_PENDING && c.theta_hat == 0.0) c.status = PRES_ABSENT;
        }
    }

    // the drop solves and what their records say
    int drop_and_reduce() {
        if (!q.use_sets) return EMSAR_HIP_OK;
        const auto &S = ctx->sets.RS;
        std::vector<PresenceItem> items[emsar::kSetClasses];
        std::vector<PresenceRec> recs[emsar::kSetClasses];
        std::vector<int32_t> who[emsar::kSetClasses];          // item -> cand
        for (size_t k = 0; k < cand.size(); k++)
            if (cand[k].status == PRES_PENDING) {
                const SetQuery::Cand &w = q.cand[k];
                items[w.cls].push_back(PresenceItem{w.set, w.loc});
                who[w.cls].push_back((int32_t)k);
            }
        if (const int rc = solve_items(items, recs, st.drop_ms)) return rc;
        for (int cls = 0; cls < emsar::kSetClasses; cls++)
            for (size_t i = 0; i < recs[cls].size(); i++) {
                Test &c = cand[(size_t)who[cls][i]];
                const SetQuery::Cand &w = q.cand[(size_t)who[cls][i]];
                const PresenceRec &r = recs[cls][i], &b = base_of(w);
                st.drop_passes_max = std::max(st.drop_passes_max, r.passes);
                st.drop_passes_sum += r.passes;
                if (r.infeasible > 0) { c.status = PRES_ESSENTIAL; continue; }
                if (!std::isfinite(r.F)) { ctx->err = "presence: non-finite likelihood at a drop solve"; return EMSAR_HIP_ERR_NUMERIC; }
                const double raw = 2.0 * (b.F - r.F);
                if (raw < st.min_raw_lambda) st.min_raw_lambda = raw;
                c.lambda = raw > 0.0 ? raw : 0.0;
                c.status = (r.converged && b.converged) ? PRES_TESTED : PRES_UNCONVERGED;
                if (r.heir >= 0) {
                    c.heir = q.h_gtid[S.desc[cls][(size_t)w.set].tid_off + (size_t)r.heir];
                    c.share = r.gain / (c.theta_hat * q.h_den[(size_t)w.lib]);
                }
            }
        return EMSAR_HIP_OK;
    }

    // the stages the profile intervals run first
    int test() {
        int rc;
        if ((rc = locate()) || (rc = baseline())) return rc;
        mark_absent();
        return drop_and_reduce();
    }

    int copy_out() {
        const std::vector<int32_t> caller_of = caller_of_lib(ctx);
        for (const Test &c : cand) st.n_status[c.status]++;
        for (int32_t i = 0; i < q.nq; i++) {
            const Test &c = cand[q.cand_index(i)];
            if (out.lambda) out.lambda[i] = c.reported_lambda();
            if (out.pvalue) out.pvalue[i] = presence_pvalue(c.reported_lambda());
            if (out.heir) out.heir[i] = c.heir < 0 ? -1 : !caller_of.empty() ? caller_of[(size_t)c.heir] : c.heir;
            if (out.heir_share) out.heir_share[i] = c.share;
            if (out.status) out.status[i] = c.status;
            if (out.theta_hat) out.theta_hat[i] = c.theta_hat;
        }
        return EMSAR_HIP_OK;
    }

    int run() {
        if (const int rc = test()) return rc;
        return copy_out();
    }
};

}  // namespace

extern "C" {

int emsar_hip_presence(emsar_hip_ctx *ctx, const emsar_em_params *p, int32_t n_query, const int32_t *query_tids, const emsar_presence_outputs *out,
                       emsar_presence_stats *stats) {
    if (const int rc = query_ok(ctx, n_query, query_tids)) return rc;
    return run_query_call<PresenceRun>(ctx, stats, p, n_query, query_tids, out);
}

int emsar_hip_presence_pvalue_host(int64_t n, const double *lambda, double *p_out) {
    if (n < 0 || (n > 0 && (!lambda || !p_out))) return EMSAR_HIP_ERR_ARG;
    for (int64_t i = 0; i < n; i++) p_out[i] = presence_pvalue(lambda[i]);
    return EMSAR_HIP_OK;
}

}  // extern "C"
