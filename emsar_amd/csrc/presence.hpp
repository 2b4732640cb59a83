// presence.hpp -- the presence test behind include/emsar_hip.h: emsar_hip_presence (device) and emsar_hip_presence_pvalue_host (no HIP
// call).  Part of emsar_hip.hip's translation unit, included at its end after fit.hpp: it uses the context, plan_solve and set_params
// (solve.hpp), the item runner (set_items.hpp) and k_solve_sets_drop (kernels_presence.hpp).
// One call = one PresenceRun:  plan        which solvers a solve would run; the sets are found on first use (ensure_sets)
//                              classify    every queried transcript: outside / not resident / closed form / candidate of a resident set
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
    // one queried transcript (library index), once however often it is asked for
    struct Cand {
        int32_t lib, cls = -1, set = -1, loc = -1;      // resident: size class, set within the class, position in the set
        int32_t status = PRES_PENDING, heir = -1;       // heir: library index
        double lambda = NAN, share = NAN, theta_hat = NAN;
    };
    emsar_hip_ctx *const ctx;
    const emsar_em_params p;             // the caller's parameters with the defaults filled in
    const int32_t nq;
    const int32_t *const query;          // caller tids, null = all in order
    const emsar_presence_outputs out;    // a copy: all NULL when the caller gave none
    const int n;
    bool use_sets = false;
    std::vector<Cand> cand;
    std::vector<int32_t> cand_of_lib;    // [n] -> cand, -1 = not queried
    std::vector<double> h_den, h_usum, h_gu, h_theta;      // [n] [n] [resident tids] [n]: den, closed-form counts, folded counts, theta_hat
    std::vector<int32_t> h_gtid;                           // [resident tids]
    std::vector<int32_t> base_of_set[emsar::kSetClasses];  // set of a class -> its baseline item, -1 = none
    std::vector<PresenceRec> base_rec[emsar::kSetClasses];
    DevBuf<double> d_theta;              // [n] theta_hat: closed form and the baselined sets, the rest 0
    SetItemRunner<PresenceItem, PresenceRec> runner;
    emsar_presence_stats st{};

    // batch_env: the profile intervals run these stages under their own variable
    PresenceRun(emsar_hip_ctx *c, const emsar_em_params *pp, int32_t nq_, const int32_t *q, const emsar_presence_outputs *o,
                const char *batch_env = "EMSAR_HIP_PRESENCE_BATCH")
        : ctx(c), p(solve_params(pp)), nq(nq_), query(q), out(o ? *o : emsar_presence_outputs{}), n(c->n_tx),
          runner(c, batch_env, "presence: an item lies outside its class's sets") {}

    int32_t lib_of(int32_t tid) const { return renumbered(ctx) ? tid_map(ctx)[(size_t)tid] : tid; }

    int plan() {
        if (!(p.count_floor >= 0.0) || (p.set_mode != 0 && p.set_mode != 1)) return EMSAR_HIP_ERR_ARG;
        SolvePlan sp;
        if (const int rc = plan_solve(ctx, p.set_mode, sp)) return rc;
        use_sets = sp.use_sets;
        cand_of_lib.assign((size_t)n, -1);
        for (int32_t i = 0; i < nq; i++) {
            const int32_t l = lib_of(query ? query[i] : i);
            if (cand_of_lib[(size_t)l] >= 0) continue;
            cand_of_lib[(size_t)l] = (int32_t)cand.size();
            Cand c; c.lib = l;
            cand.push_back(c);
        }
        return EMSAR_HIP_OK;
    }

    // Where every queried transcript stands before anything is solved.  The packed sets' transcript lists and folded counts live on
    // the device only (ensure_sets frees the host copies): they are read back here, with den and the closed-form counts.
    int classify() {
        if (!use_sets) { for (auto &c : cand) c.status = PRES_NOT_RESIDENT; return EMSAR_HIP_OK; }
        const SetsDev &D = ctx->sets;
        const auto &S = D.RS;
        size_t n_gu = 0;
        for (int c = 0; c < emsar::kSetClasses; c++) for (const auto &d : S.desc[c]) n_gu = std::max<size_t>(n_gu, (size_t)d.tid_off + d.n_t);
        h_den.resize((size_t)n); h_usum.resize((size_t)n); h_gtid.resize(n_gu); h_gu.resize(n_gu);
        if (n > 0) {
            HIPCHK(hipMemcpyAsync(h_den.data(), ctx->vec.d_den, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(h_usum.data(), D.d_usum, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (n_gu > 0) {
            HIPCHK(hipMemcpyAsync(h_gtid.data(), D.d_g_tid, n_gu * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(h_gu.data(), D.d_g_u, n_gu * 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (int c = 0; c < emsar::kSetClasses; c++) {
            base_of_set[c].assign(S.desc[c].size(), -1);
            for (size_t s = 0; s < S.desc[c].size(); s++) {
                const emsar::SetDesc &d = S.desc[c][s];
                for (uint32_t i = 0; i < d.n_t; i++) {
                    const int32_t k = cand_of_lib[(size_t)h_gtid[d.tid_off + i]];
                    if (k >= 0) { cand[(size_t)k].cls = c; cand[(size_t)k].set = (int32_t)s; cand[(size_t)k].loc = (int32_t)i; }
                }
            }
        }
        for (auto &c : cand) {
            const uint8_t kind = S.kind[(size_t)c.lib];
            if (!(h_den[(size_t)c.lib] > 0.0)) c.status = PRES_OUTSIDE;
            else if (kind == emsar::KIND_STREAMED || kind == emsar::KIND_CLUSTER) c.status = PRES_NOT_RESIDENT;
            else if (kind == emsar::KIND_CLOSED) c.status = h_usum[(size_t)c.lib] > 0.0 ? PRES_ESSENTIAL : PRES_ABSENT;
            else if (c.set < 0) { ctx->err = "presence: a resident transcript is in no packed set"; return EMSAR_HIP_ERR_HIP; }
            else if (h_gu[S.desc[c.cls][(size_t)c.set].tid_off + (size_t)c.loc] > 0.0) c.status = PRES_ESSENTIAL;    // a single-transcript row with reads
        }
        return EMSAR_HIP_OK;
    }

    // items through k_solve_sets_drop (SetItemRunner); the baseline's and the drop stage's items differ in `drop` alone
    int solve_items(const std::vector<PresenceItem> (&items)[emsar::kSetClasses], std::vector<PresenceRec> (&recs)[emsar::kSetClasses], double &ms_acc) {
        const SetsDev &D = ctx->sets;
        const SetSolveParams P = set_params(p);
        HIPCHK(set_class_lds_attributes(kSolveSetsDrop));
        return runner.run(items, recs, ms_acc, st.items_launched,
            [](const PresenceItem &it, const emsar::SetDesc &d) { return it.drop >= -1 && it.drop < (int32_t)d.n_t; },
            [&](int c, int threads, hipStream_t s, size_t cnt, const PresenceItem *d_items, PresenceRec *d_rec) {
                hipLaunchKernelGGL(kSolveSetsDrop[c], dim3((unsigned)cnt), dim3(threads), D.RS.max_lds[c], s, D.d_sdesc[c].get(), d_items, D.d_g_tid.get(),
                                   D.d_g_u.get(), D.d_row_w.get(), D.d_srp.get(), D.d_sent.get(), D.d_scp.get(), D.d_scrow.get(), ctx->vec.d_den.get(), d_theta.get(), d_rec, P);
            });
    }

    // theta_hat: the closed form, and every set that holds a queried transcript solved with nothing dropped
    int baseline() {
        if (!use_sets) return EMSAR_HIP_OK;
        const SetsDev &D = ctx->sets;
        HIPCHK(d_theta.alloc((size_t)n));
        HIPCHK(hipMemsetAsync(d_theta, 0, (size_t)std::max(n, 2) * 8, ctx->stream));
        if (n > 0) hipLaunchKernelGGL(k_closed_form, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, n, D.d_kind.get(), D.d_usum.get(), ctx->vec.d_den.get(), d_theta.get());
        HIPCHK(hipGetLastError());
        std::vector<PresenceItem> items[emsar::kSetClasses];
        for (const auto &c : cand)
            if (c.set >= 0 && base_of_set[c.cls][(size_t)c.set] < 0) {
                base_of_set[c.cls][(size_t)c.set] = (int32_t)items[c.cls].size();
                items[c.cls].push_back(PresenceItem{c.set, -1});
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

    void mark_absent() {
        if (!use_sets) return;
        for (auto &c : cand) {
            if (c.status != PRES_NOT_RESIDENT) c.theta_hat = h_theta[(size_t)c.lib];
            if (c.status == PRES_PENDING && c.theta_hat == 0.0) c.status = PRES_ABSENT;
        }
    }

    // the drop solves and what their records say
    int drop_and_reduce() {
        if (!use_sets) return EMSAR_HIP_OK;
        const auto &S = ctx->sets.RS;
        std::vector<PresenceItem> items[emsar::kSetClasses];
        std::vector<PresenceRec> recs[emsar::kSetClasses];
        std::vector<int32_t> who[emsar::kSetClasses];          // item -> cand
        for (size_t k = 0; k < cand.size(); k++)
            if (cand[k].status == PRES_PENDING) {
                items[cand[k].cls].push_back(PresenceItem{cand[k].set, cand[k].loc});
                who[cand[k].cls].push_back((int32_t)k);
            }
        if (const int rc = solve_items(items, recs, st.drop_ms)) return rc;
        for (int cls = 0; cls < emsar::kSetClasses; cls++)
            for (size_t i = 0; i < recs[cls].size(); i++) {
                Cand &c = cand[(size_t)who[cls][i]];
                const PresenceRec &r = recs[cls][i], &b = base_rec[cls][(size_t)base_of_set[cls][(size_t)c.set]];
                st.drop_passes_max = std::max(st.drop_passes_max, r.passes);
                st.drop_passes_sum += r.passes;
                if (r.infeasible > 0) { c.status = PRES_ESSENTIAL; continue; }
                if (!std::isfinite(r.F)) { ctx->err = "presence: non-finite likelihood at a drop solve"; return EMSAR_HIP_ERR_NUMERIC; }
                const double raw = 2.0 * (b.F - r.F);
                if (raw < st.min_raw_lambda) st.min_raw_lambda = raw;
                c.lambda = raw > 0.0 ? raw : 0.0;
                c.status = (r.converged && b.converged) ? PRES_TESTED : PRES_UNCONVERGED;
                if (r.heir >= 0) {
                    const emsar::SetDesc &d = S.desc[cls][(size_t)c.set];
                    c.heir = h_gtid[d.tid_off + (size_t)r.heir];
                    c.share = r.gain / (c.theta_hat * h_den[(size_t)c.lib]);
                }
            }
        return EMSAR_HIP_OK;
    }

    int copy_out() {
        const std::vector<int32_t> caller_of = caller_of_lib(ctx);
        for (auto &c : cand) {
            if (c.status == PRES_ABSENT) c.lambda = 0.0;
            if (c.status == PRES_ESSENTIAL) c.lambda = INFINITY;
            st.n_status[c.status]++;
        }
        for (int32_t i = 0; i < nq; i++) {
            const Cand &c = cand[(size_t)cand_of_lib[(size_t)lib_of(query ? query[i] : i)]];
            if (out.lambda) out.lambda[i] = c.lambda;
            if (out.pvalue) out.pvalue[i] = presence_pvalue(c.lambda);
            if (out.heir) out.heir[i] = c.heir < 0 ? -1 : !caller_of.empty() ? caller_of[(size_t)c.heir] : c.heir;
            if (out.heir_share) out.heir_share[i] = c.share;
            if (out.status) out.status[i] = c.status;
            if (out.theta_hat) out.theta_hat[i] = c.theta_hat;
        }
        return EMSAR_HIP_OK;
    }

    int run() {
        int rc;
        if ((rc = plan()) || (rc = classify()) || (rc = baseline())) return rc;
        mark_absent();
        if ((rc = drop_and_reduce())) return rc;
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
