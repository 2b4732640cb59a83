// compare.hpp -- the two-sample likelihood-ratio test behind include/emsar_hip.h: emsar_hip_compare (device) and
// emsar_hip_compare_pvalue_host (no HIP call).  Part of emsar_hip.hip's translation unit, included after profile.hpp: each sample's
// queried transcripts are located as the presence test's are (SetQuery, set_items.hpp), k_compare_sets (kernels_compare.hpp) runs the
// searches.
// One call = one CompareRun:  plan, classify   SetQuery's stages on the same query, once per context: the sets of both samples are found
//                                              on first use, every queried transcript is located in each
//                             pair             per transcript: outside / not resident / both closed form (searched on the host) / one item
//                                              in the launch class of the larger of its two sets
//                             search           the items in batches across the three launch classes (SetItemRunner)
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

// the search of k_compare_sets (CompareStep) on a pair of one-transcript components, compare_closed_form as its evaluation
inline CompareRec compare_closed_pair(double u_a, double den_a, double u_b, double den_b, const CompareSearchParams &Q) {
    CompareStep T;
    T.start();
    double x_a, F_a, x_b, F_b;
    do {
        compare_closed_form(u_a, den_a, T.pt.scale_a, x_a, F_a);
        compare_closed_form(u_b, den_b, T.pt.scale_b, x_b, F_b);
    } while (T.step(x_a, F_a, x_b, F_b, den_a, den_b, Q));
    return T.record(0, 1, 0);
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

struct CompareRun {
    using Result = CompareResult;        // per queried transcript (SetQuery::cand of both samples, same index)
    emsar_hip_ctx *const ctx;            // ctx_a: its streams and events carry the launches
    emsar_hip_ctx *const ctx_b;
    SetQuery qa, qb;                     // where every queried transcript stands in each sample
    const emsar_compare_outputs out;     // a copy: all NULL when the caller gave none
    CompareSearchParams Q;
    std::vector<Result> res;
    SetItemRunner<CompareItem, CompareRec> runner;
    emsar_compare_stats st{};

    CompareRun(emsar_hip_ctx *a, emsar_hip_ctx *b, const emsar_em_params *p, const emsar_compare_params &cp, int32_t nq, const int32_t *query,
               const emsar_compare_outputs *o)
        : ctx(a), ctx_b(b), qa(a, p, nq, query), qb(b, p, nq, query), out(o ? *o : emsar_compare_outputs{}),
          runner(a, "EMSAR_HIP_COMPARE_BATCH", "compare: an item lies outside its class's sets") {
        Q = CompareSearchParams{cp.ratio == 0.0 ? 1.0 : cp.ratio, cp.dev_tol > 0.0 ? cp.dev_tol : 1e-4, cp.max_evals > 0 ? cp.max_evals : 40, 0};
    }

    // a side of an item: a one-transcript component (set -1), or transcript t of set `set` of class cls <= the launch class, checked
    // against its own context's descriptors
    static bool side_ok(const emsar_hip_ctx *c, int launch_cls, int32_t cls, int32_t set, int32_t t, double den) {
        if (!(den > 0.0)) return false;
        if (set == -1) return true;
        const emsar::SetDesc *d = cls <= launch_cls ? set_desc(c, cls, set) : nullptr;
        return d && t >= 0 && t < (int32_t)d->n_t;
    }
    // the launch class of a pair: the larger of its two size classes, a one-transcript component counting as none
    static int launch_class(int32_t set_a, int32_t cls_a, int32_t set_b, int32_t cls_b) { return std::max(set_a < 0 ? -1 : cls_a, set_b < 0 ? -1 : cls_b); }

    int reduce(const CompareRec &r, CompareResult &o) {
        if (!compare_reduce(r, Q.ratio, o)) { ctx->err = "compare: non-finite likelihood at lambda = 0"; return EMSAR_HIP_ERR_NUMERIC; }
        if (o.raw < st.min_raw_lambda) st.min_raw_lambda = o.raw;
        return EMSAR_HIP_OK;
    }

    int pair_search_reduce() {
        res.resize(qa.cand.size());
        std::vector<CompareItem> items[emsar::kSetClasses];
        std::vector<CompareRec> recs[emsar::kSetClasses];
        std::vector<int32_t> who[emsar::kSetClasses];          // item -> cand
        for (size_t k = 0; k < qa.cand.size(); k++) {
            const SetQuery::Cand &a = qa.cand[k], &b = qb.cand[k];
            Result &o = res[k];
            if (a.standing == SetQuery::NOT_RESIDENT || b.standing == SetQuery::NOT_RESIDENT) { o.status = CMP_NOT_RESIDENT; continue; }
            if (a.standing == SetQuery::OUTSIDE || b.standing == SetQuery::OUTSIDE) { o.status = CMP_OUTSIDE; continue; }
            const double den_a = qa.h_den[(size_t)a.lib], den_b = qb.h_den[(size_t)b.lib];
            if (a.set < 0 && b.set < 0) {
                if (const int rc = reduce(compare_closed_pair(a.u, den_a, b.u, den_b, Q), o)) return rc;
                continue;
            }
            const int cls = launch_class(a.set, a.cls, b.set, b.cls);
            items[cls].push_back(CompareItem{a.set, a.loc, a.cls, b.set, b.loc, b.cls, a.u, den_a, b.u, den_b});
            who[cls].push_back((int32_t)k);
        }
        const SetSolveParams P = set_params(qa.p);
        const CompareSide GA = side_of(ctx), GB = side_of(ctx_b);
        size_t lds[emsar::kSetClasses];
        launch_class_lds(lds, ctx, ctx_b);
        HIPCHK(set_class_lds_attributes(kCompareSets));
        const int rc = runner.run(items, recs, st.device_ms, st.items_launched,
            [&](int c, const CompareItem &it) {
                return side_ok(ctx, c, it.cls_a, it.set_a, it.t_a, it.den_a) && side_ok(ctx_b, c, it.cls_b, it.set_b, it.t_b, it.den_b) &&
                       launch_class(it.set_a, it.cls_a, it.set_b, it.cls_b) == c;
            },
            [&](int c, int threads, hipStream_t s, size_t cnt, const CompareItem *d_items, CompareRec *d_rec) {
                hipLaunchKernelGGL(kCompareSets[c], dim3((unsigned)cnt), dim3(threads), lds[c], s, d_items, GA, GB, d_rec, P, Q);
            });
        if (rc) return rc;
        for (int cls = 0; cls < emsar::kSetClasses; cls++)
            for (size_t i = 0; i < recs[cls].size(); i++) {
                const CompareRec &r = recs[cls][i];
                add_search_stats(st, r);
                if (const int rc2 = reduce(r, res[(size_t)who[cls][i]])) return rc2;
            }
        return EMSAR_HIP_OK;
    }

    int copy_out() {
        for (const Result &o : res) st.n_status[o.status]++;
        for (int32_t i = 0; i < qa.nq; i++) {
            const Result &o = res[qa.cand_index(i)];
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
        if ((rc = qa.plan()) || (rc = qa.classify())) return rc;
        if ((rc = qb.plan()) || (rc = qb.classify())) { ctx->err = ctx_b->err; return rc; }
        if ((rc = pair_search_reduce())) return rc;
        return copy_out();
    }
};

}  // namespace

extern "C" {

int emsar_hip_compare(emsar_hip_ctx *ctx_a, emsar_hip_ctx *ctx_b, const emsar_em_params *p, const emsar_compare_params *cp, int32_t n_query,
                      const int32_t *query_tids, const emsar_compare_outputs *out, emsar_compare_stats *stats) {
    if (const int rc = two_samples_ok(ctx_a, ctx_b, false)) return rc;
    if (const int rc = query_ok(ctx_a, n_query, query_tids)) return rc;
    const emsar_compare_params prm = cp ? *cp : emsar_compare_params{1.0, 0.0, 0, 0};
    if (!std::isfinite(prm.ratio) || prm.ratio < 0.0 || !std::isfinite(prm.dev_tol)) return EMSAR_HIP_ERR_ARG;
    return run_two_sample_call<CompareRun>(ctx_a, ctx_b, stats, p, prm, n_query, query_tids, out);
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
