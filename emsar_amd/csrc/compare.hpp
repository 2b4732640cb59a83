// compare.hpp -- the two-sample likelihood-ratio test behind include/emsar_hip.h: emsar_hip_compare (device) and
// emsar_hip_compare_pvalue_host (no HIP call).  Part of emsar_hip.hip's translation unit, included after profile.hpp: the first stages of
// each sample ARE the presence test's (PresenceRun: plan, classify), k_compare_sets (kernels_compare.hpp) runs the searches.
// One call = one CompareRun:  plan, classify   PresenceRun's stages on the same query, once per context: the sets of both samples are found
//                                              on first use, every queried transcript is located in each
//                             pair             per transcript: outside / not resident / both closed form (searched on the host) / one item
//                                              in the launch class of the larger of its two sets
//                             search           the items in batches across the three launch classes (PairItemRunner)
//                             reduce           records -> Lambda, p, log2fc, status;  copy_out in query order
// One workgroup runs one search of at most max_evals evaluations of two solves of at most max_iter passes each.  Neither context's
// theta, weights or scales are touched.  The launches run on ctx_a's streams; ctx_b's stream is drained before.

namespace {

enum CompareStatus : int32_t {
    CMP_TESTED = EMSAR_COMPARE_TESTED, CMP_BOTH_ABSENT = EMSAR_COMPARE_BOTH_ABSENT, CMP_OUTSIDE = EMSAR_COMPARE_OUTSIDE,
    CMP_NOT_RESIDENT = EMSAR_COMPARE_NOT_RESIDENT, CMP_UNCONVERGED = EMSAR_COMPARE_UNCONVERGED
};

// p of chi2 with one degree of freedom
inline double compare_pvalue(double lambda) {
    if (lambda != lambda) return lambda;
    if (!(lambda > 0.0)) return 1.0;
    if (std::isinf(lambda)) return 0.0;
    return std::erfc(std::sqrt(lambda / 2.0));
}

// the search of k_compare_sets on a pair of one-transcript components: the same steps, the same stopping rule, the same record
inline CompareRec compare_closed_pair(double u_a, double den_a, double u_b, double den_b, const CompareSearchParams &Q) {
    const double r = Q.ratio;
    CompareSearch S;
    ComparePoint pt;
    pt.lambda = 0.0; pt.scale_a = 1.0; pt.scale_b = 1.0;
    bool up = false;
    int evals = 0, search_ok = 0;
    double x0_a = 0.0, x0_b = 0.0, F0_a = 0.0, F0_b = 0.0, x_a = 0.0, x_b = 0.0, F_a = 0.0, F_b = 0.0;
    for (;;) {
        compare_closed_form(u_a, den_a, pt.scale_a, x_a, F_a);
        compare_closed_form(u_b, den_b, pt.scale_b, x_b, F_b);
        evals++;
        const double g = x_a - r * x_b;
        if (evals == 1) {
            x0_a = x_a; x0_b = x_b; F0_a = F_a; F0_b = F_b;
            if (!(F_a - F_a == 0.0) || !(F_b - F_b == 0.0)) break;
            if (g == 0.0) { search_ok = 1; break; }
            up = g > 0.0;
        }
        if (!(g - g == 0.0) || !(F_a - F_a == 0.0) || !(F_b - F_b == 0.0)) break;
        if (evals > 1 && 2.0 * std::fabs(pt.lambda * g) <= Q.dev_tol) { search_ok = 1; break; }
        const double h = g / (x_a + r * x_b);
        if (evals == 1) S.start(h); else S.update(h);
        // the root lies in the bracket and L is convex with slope -g: the dual value cannot fall further than |g| times the bracket
        if (2.0 * std::fabs(g) * ((S.v_hi - S.v_lo) * ComparePoint::end(up, r, den_a, den_b)) <= Q.dev_tol) { search_ok = 1; break; }
        if (evals >= Q.max_evals) break;
        pt.at(S.v, up, r, den_a, den_b);
    }
    CompareRec o;
    o.lambda_mult = pt.lambda; o.x_a = x_a; o.x_b = x_b; o.x0_a = x0_a; o.x0_b = x0_b;
    o.FhatA = F0_a; o.FhatB = F0_b; o.FA = F_a; o.FB = F_b;
    o.evals = evals; o.passes = 0; o.flags = (search_ok ? COMPARE_REC_SEARCH_OK : 0) | COMPARE_REC_SOLVES_OK;
    o.infeasible = 0;
    return o;
}

// what one queried transcript is given
struct CompareResult {
    double lambda = NAN, raw = NAN, log2fc = NAN, theta_a = NAN, theta_b = NAN, theta_null = NAN, multiplier = NAN, gap = NAN;
    int32_t evals = 0, status = CMP_NOT_RESIDENT;
};

// a record -> the transcript's numbers; false for a non-finite F at lambda = 0
inline bool compare_reduce(const CompareRec &r, double ratio, CompareResult &o) {
    if (!std::isfinite(r.FhatA) || !std::isfinite(r.FhatB)) return false;
    const double g = r.x_a - ratio * r.x_b;
    const double dual = (r.FA + r.FB) - r.lambda_mult * g;
    o.raw = r.evals == 1 ? 0.0 : 2.0 * ((r.FhatA + r.FhatB) - dual);
    o.lambda = o.raw > 0.0 ? o.raw : 0.0;                       // a NaN raw value: 0, with UNCONVERGED below
    o.theta_a = r.x0_a; o.theta_b = r.x0_b; o.theta_null = r.x_a; o.multiplier = r.lambda_mult; o.gap = g;
    o.evals = r.evals;
    const bool no_a = r.x0_a == 0.0, no_b = r.x0_b == 0.0;
    o.log2fc = (no_a && no_b) ? NAN : no_a ? -INFINITY : no_b ? INFINITY : std::log2(r.x0_a / (ratio * r.x0_b));
    if (no_a && no_b) o.status = CMP_BOTH_ABSENT;
    else o.status = r.flags == (COMPARE_REC_SEARCH_OK | COMPARE_REC_SOLVES_OK) ? CMP_TESTED : CMP_UNCONVERGED;
    return true;
}

// SetItemRunner's sibling for items that name a set in each of two contexts: items[c] run in launch class c (the larger of the item's
// two size classes) on the streams of `ctx`, at most a batch per class and launch; recs[c][i] answers items[c][i].  Every item's two
// sets are checked against their own context's descriptors before anything is launched.
struct PairItemRunner {
    emsar_hip_ctx *const ctx;            // ctx_a: its streams and events carry the launches
    const emsar_hip_ctx *const other;    // ctx_b
    DevBuf<CompareItem> d_items[emsar::kSetClasses];
    DevBuf<CompareRec> d_rec[emsar::kSetClasses];
    hipEvent_t e[2] = {nullptr, nullptr};

    PairItemRunner(emsar_hip_ctx *a, const emsar_hip_ctx *b) : ctx(a), other(b) {}
    ~PairItemRunner() { for (hipEvent_t ev : e) if (ev) (void)hipEventDestroy(ev); }

    // a side of an item: a one-transcript component (set -1), or transcript t of set `set` of class cls <= the launch class
    static bool side_ok(const emsar_hip_ctx *c, int launch_cls, int32_t cls, int32_t set, int32_t t, double den) {
        if (!(den > 0.0)) return false;
        if (set == -1) return true;
        if (cls < 0 || cls > launch_cls || set < 0) return false;
        const auto &desc = c->sets.RS.desc[cls];
        return (size_t)set < desc.size() && t >= 0 && t < (int32_t)desc[(size_t)set].n_t;
    }

    template <class Launch>
    int run(const std::vector<CompareItem> (&items)[emsar::kSetClasses], std::vector<CompareRec> (&recs)[emsar::kSetClasses], double &ms_acc,
            int64_t &launched, const Launch &launch) {
        size_t most = 0;
        for (int c = 0; c < emsar::kSetClasses; c++) {
            for (const CompareItem &it : items[c])
                if (!side_ok(ctx, c, it.cls_a, it.set_a, it.t_a, it.den_a) || !side_ok(other, c, it.cls_b, it.set_b, it.t_b, it.den_b) ||
                    std::max(it.set_a < 0 ? -1 : it.cls_a, it.set_b < 0 ? -1 : it.cls_b) != c) {
                    ctx->err = "compare: an item lies outside its class's sets";
                    return EMSAR_HIP_ERR_HIP;
                }
            recs[c].resize(items[c].size());
            most = std::max(most, items[c].size());
        }
        if (most == 0) return EMSAR_HIP_OK;
        const size_t batch = (size_t)item_batch((int64_t)(emsar::kSetClasses * (sizeof(CompareItem) + sizeof(CompareRec))), "EMSAR_HIP_COMPARE_BATCH",
                                                (int64_t)most, (int64_t)1 << 20);
        for (int c = 0; c < emsar::kSetClasses; c++)
            if (!items[c].empty()) {
                const size_t cnt = std::min(batch, items[c].size());
                HIPCHK(d_items[c].alloc(cnt)); HIPCHK(d_rec[c].alloc(cnt));
            }
        for (hipEvent_t &ev : e) if (!ev) HIPCHK(hipEventCreate(&ev));
        const hipStream_t st[emsar::kSetClasses] = {ctx->stream, ctx->side[0], ctx->side[1]};
        for (size_t first = 0; first < most; first += batch) {
            size_t cnt[emsar::kSetClasses];
            for (int c = 0; c < emsar::kSetClasses; c++) {
                cnt[c] = items[c].size() > first ? std::min(batch, items[c].size() - first) : 0;
                if (cnt[c]) HIPCHK(hipMemcpyAsync(d_items[c], items[c].data() + first, cnt[c] * sizeof(CompareItem), hipMemcpyHostToDevice, ctx->stream));
            }
            HIPCHK(hipEventRecord(e[0], ctx->stream));
            if (const int rc = fork_side_streams(ctx, 2)) return rc;
            for (int c = emsar::kSetClasses - 1; c >= 0; c--) if (cnt[c]) launch(c, emsar::kSetThreads[c], st[c], cnt[c], d_items[c].get(), d_rec[c].get());
            for (int i = 0; i < 2; i++) {
                HIPCHK(hipEventRecord(ctx->ev_join[i], ctx->side[i]));
                HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_join[i], 0));
            }
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(e[1], ctx->stream));
            for (int c = 0; c < emsar::kSetClasses; c++)
                if (cnt[c]) HIPCHK(hipMemcpyAsync(recs[c].data() + first, d_rec[c], cnt[c] * sizeof(CompareRec), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, e[0], e[1]));
            ms_acc += ms;
            for (int c = 0; c < emsar::kSetClasses; c++) launched += (int64_t)cnt[c];
        }
        return EMSAR_HIP_OK;
    }
};

struct CompareRun {
    using Result = CompareResult;        // per queried transcript (PresenceRun::cand of both samples, same index)
    emsar_hip_ctx *const ctx;            // ctx_a
    emsar_hip_ctx *const ctx_b;
    PresenceRun pa, pb;
    const int32_t nq;
    const int32_t *const query;
    const emsar_compare_outputs out;     // a copy: all NULL when the caller gave none
    CompareSearchParams Q;
    std::vector<Result> res;
    PairItemRunner runner;
    emsar_compare_stats st{};

    CompareRun(emsar_hip_ctx *a, emsar_hip_ctx *b, const emsar_em_params *p, const emsar_compare_params &cp, int32_t nq_, const int32_t *q,
               const emsar_compare_outputs *o)
        : ctx(a), ctx_b(b), pa(a, p, nq_, q, nullptr, "EMSAR_HIP_COMPARE_BATCH"), pb(b, p, nq_, q, nullptr, "EMSAR_HIP_COMPARE_BATCH"), nq(nq_), query(q),
          out(o ? *o : emsar_compare_outputs{}), runner(a, b) {
        Q = CompareSearchParams{cp.ratio == 0.0 ? 1.0 : cp.ratio, cp.dev_tol > 0.0 ? cp.dev_tol : 1e-4, cp.max_evals > 0 ? cp.max_evals : 40, 0};
    }

    static CompareSide side_of(const emsar_hip_ctx *c) {
        const SetsDev &D = c->sets;
        return CompareSide{D.d_sdesc[0].get(), D.d_sdesc[1].get(), D.d_sdesc[2].get(), D.d_g_tid.get(), D.d_g_u.get(), D.d_row_w.get(),
                           D.d_srp.get(), D.d_sent.get(), D.d_scp.get(), D.d_scrow.get(), c->vec.d_den.get()};
    }

    int reduce(const CompareRec &r, CompareResult &o) {
        if (!compare_reduce(r, Q.ratio, o)) { ctx->err = "compare: non-finite likelihood at lambda = 0"; return EMSAR_HIP_ERR_NUMERIC; }
        if (o.raw < st.min_raw_lambda) st.min_raw_lambda = o.raw;
        return EMSAR_HIP_OK;
    }

    int pair_search_reduce() {
        res.resize(pa.cand.size());
        std::vector<CompareItem> items[emsar::kSetClasses];
        std::vector<CompareRec> recs[emsar::kSetClasses];
        std::vector<int32_t> who[emsar::kSetClasses];          // item -> cand
        for (size_t k = 0; k < pa.cand.size(); k++) {
            const PresenceRun::Cand &a = pa.cand[k], &b = pb.cand[k];
            Result &o = res[k];
            if (a.status == PRES_NOT_RESIDENT || b.status == PRES_NOT_RESIDENT) { o.status = CMP_NOT_RESIDENT; continue; }
            if (a.status == PRES_OUTSIDE || b.status == PRES_OUTSIDE) { o.status = CMP_OUTSIDE; continue; }
            const double den_a = pa.h_den[(size_t)a.lib], den_b = pb.h_den[(size_t)b.lib];
            const double u_a = a.set < 0 ? pa.h_usum[(size_t)a.lib] : 0.0, u_b = b.set < 0 ? pb.h_usum[(size_t)b.lib] : 0.0;
            if (a.set < 0 && b.set < 0) {
                if (const int rc = reduce(compare_closed_pair(u_a, den_a, u_b, den_b, Q), o)) return rc;
                continue;
            }
            const int cls = std::max(a.set < 0 ? -1 : a.cls, b.set < 0 ? -1 : b.cls);
            items[cls].push_back(CompareItem{a.set, a.loc, a.cls, b.set, b.loc, b.cls, u_a, den_a, u_b, den_b});
            who[cls].push_back((int32_t)k);
        }
        const SetSolveParams P = set_params(pa.p);
        const CompareSide GA = side_of(ctx), GB = side_of(ctx_b);
        const auto &SA = ctx->sets.RS, &SB = ctx_b->sets.RS;
        size_t lds[emsar::kSetClasses], most = 0;              // a launch class holds the sets of its own and of every smaller class
        for (int c = 0; c < emsar::kSetClasses; c++) lds[c] = most = std::max(most, std::max((size_t)SA.max_lds[c], (size_t)SB.max_lds[c]));
        HIPCHK(set_class_lds_attributes(kCompareSets));
        const int rc = runner.run(items, recs, st.device_ms, st.items_launched,
            [&](int c, int threads, hipStream_t s, size_t cnt, const CompareItem *d_items, CompareRec *d_rec) {
                hipLaunchKernelGGL(kCompareSets[c], dim3((unsigned)cnt), dim3(threads), lds[c], s, d_items, GA, GB, d_rec, P, Q);
            });
        if (rc) return rc;
        for (int cls = 0; cls < emsar::kSetClasses; cls++)
            for (size_t i = 0; i < recs[cls].size(); i++) {
                const CompareRec &r = recs[cls][i];
                st.evals_sum += r.evals; st.passes_sum += r.passes;
                st.evals_max = std::max(st.evals_max, r.evals); st.passes_max = std::max(st.passes_max, r.passes);
                if (const int rc2 = reduce(r, res[(size_t)who[cls][i]])) return rc2;
            }
        return EMSAR_HIP_OK;
    }

    int copy_out() {
        for (const Result &o : res) st.n_status[o.status]++;
        for (int32_t i = 0; i < nq; i++) {
            const Result &o = res[(size_t)pa.cand_of_lib[(size_t)pa.lib_of(query ? query[i] : i)]];
            if (out.lambda) out.lambda[i] = o.lambda;
            if (out.pvalue) out.pvalue[i] = compare_pvalue(o.lambda);
            if (out.log2fc) out.log2fc[i] = o.log2fc;
            if (out.theta_a) out.theta_a[i] = o.theta_a;
            if (out.theta_b) out.theta_b[i] = o.theta_b;
            if (out.theta_null) out.theta_null[i] = o.theta_null;
            if (out.multiplier) out.multiplier[i] = o.multiplier;
            if (out.gap) out.gap[i] = o.gap;
            if (out.raw_lambda) out.raw_lambda[i] = o.raw;
            if (out.status) out.status[i] = o.status;
            if (out.evals) out.evals[i] = o.evals;
        }
        return EMSAR_HIP_OK;
    }

    int run() {
        int rc;
        if ((rc = pa.plan()) || (rc = pa.classify())) return rc;
        if ((rc = pb.plan()) || (rc = pb.classify())) { ctx->err = ctx_b->err; return rc; }
        if ((rc = pair_search_reduce())) return rc;
        return copy_out();
    }
};

// the two contexts hold one structure: compared on what they keep on the host
inline bool same_structure(const emsar_hip_ctx *a, const emsar_hip_ctx *b) {
    return a->n_rows == b->n_rows && a->n_tx == b->n_tx && a->nnz == b->nnz && a->h_row_ptr == b->h_row_ptr && a->h_col == b->h_col;
}

}  // namespace

extern "C" {

int emsar_hip_compare(emsar_hip_ctx *ctx_a, emsar_hip_ctx *ctx_b, const emsar_em_params *p, const emsar_compare_params *cp, int32_t n_query,
                      const int32_t *query_tids, const emsar_compare_outputs *out, emsar_compare_stats *stats) {
    if (!ctx_a || !ctx_b || ctx_a == ctx_b) return EMSAR_HIP_ERR_ARG;
    if (!ctx_a->have_sample || !ctx_b->have_sample) return EMSAR_HIP_ERR_STATE;      // first: a state error whatever the other arguments say
    if (ctx_a->device != ctx_b->device || !same_structure(ctx_a, ctx_b)) return EMSAR_HIP_ERR_ARG;
    if (const int rc = query_ok(ctx_a, n_query, query_tids)) return rc;
    const emsar_compare_params prm = cp ? *cp : emsar_compare_params{1.0, 0.0, 0, 0};
    if (!std::isfinite(prm.ratio) || prm.ratio < 0.0 || !std::isfinite(prm.dev_tol)) return EMSAR_HIP_ERR_ARG;
    emsar_hip_ctx *const ctx = ctx_b;
    HIPCHK(hipSetDevice(ctx_b->device));
    HIPCHK(hipStreamSynchronize(ctx_b->stream));
    return run_query_call<CompareRun>(ctx_a, stats, ctx_b, p, prm, n_query, query_tids, out);
}

// Diagnostic only (not declared in the public header; needs no device): what emsar_hip_compare gives a transcript whose component is a
// one-transcript component in both samples (u reads, den each) -- the search the host runs for such pairs.  values[9]: lambda, pvalue,
// log2fc, theta_a, theta_b, theta_null, multiplier, gap, raw_lambda.
int emsar_hip_debug_compare_closed(double u_a, double den_a, double u_b, double den_b, const emsar_compare_params *cp, double *values,
                                   int32_t *status, int32_t *evals) {
    const emsar_compare_params prm = cp ? *cp : emsar_compare_params{1.0, 0.0, 0, 0};
    if (!values || !status || !evals || !(u_a >= 0.0) || !(u_b >= 0.0) || !(den_a > 0.0) || !(den_b > 0.0)) return EMSAR_HIP_ERR_ARG;
    if (!std::isfinite(prm.ratio) || prm.ratio < 0.0 || !std::isfinite(prm.dev_tol)) return EMSAR_HIP_ERR_ARG;
    const CompareSearchParams Q{prm.ratio == 0.0 ? 1.0 : prm.ratio, prm.dev_tol > 0.0 ? prm.dev_tol : 1e-4, prm.max_evals > 0 ? prm.max_evals : 40, 0};
    CompareResult o;
    if (!compare_reduce(compare_closed_pair(u_a, den_a, u_b, den_b, Q), Q.ratio, o)) return EMSAR_HIP_ERR_NUMERIC;
    const double v[9] = {o.lambda, compare_pvalue(o.lambda), o.log2fc, o.theta_a, o.theta_b, o.theta_null, o.multiplier, o.gap, o.raw};
    for (int i = 0; i < 9; i++) values[i] = v[i];
    *status = o.status; *evals = o.evals;
    return EMSAR_HIP_OK;
}

int emsar_hip_compare_pvalue_host(int64_t n, const double *lambda, double *p_out) {
    if (n < 0 || (n > 0 && (!lambda || !p_out))) return EMSAR_HIP_ERR_ARG;
    for (int64_t i = 0; i < n; i++) p_out[i] = compare_pvalue(lambda[i]);
    return EMSAR_HIP_OK;
}

}  // extern "C"
