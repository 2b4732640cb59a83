// compare_usage.hpp -- the two-sample test of isoform usage behind include/emsar_hip.h: emsar_hip_compare_usage.  Part of
// emsar_hip.hip's translation unit, included after gene_parts.hpp: the members of the queried transcripts' genes are located and
// grouped into parts as the gene-level two-sample test does (SetQuery; GeneQueryMembers, GenePartLists: gene_parts.hpp),
// k_compare_usage_sets (kernels_compare_usage.hpp) runs the searches.
// One call = one CompareUsageRun:  plan, classify   SetQuery's stages on the union of the members of the queried transcripts' genes, once
//                                                   per context
//                                  group            per gene and sample: its parts (GeneSideParts), once however many of its transcripts
//                                                   are asked for; per distinct (gene, t): the host-only statuses, t's place and the
//                                                   smallest den of the others; a gene whose parts are all closed form is searched on the
//                                                   host, any other (gene, t) is one item in the launch class of the gene's largest set part
//                                  search           the items in batches across the three launch classes (SetItemRunner)
//                                  reduce           records -> Lambda, p, shares, status (usage_reduce);  copy_out in query order
// One workgroup runs one two-level search.  Neither context's theta, weights or scales are touched.  The launches run on ctx_a's
// streams; ctx_b's stream is drained before.

namespace {

enum UsageStatus : int32_t {
    USE_TESTED = EMSAR_USAGE_TESTED, USE_BOTH_ABSENT = EMSAR_USAGE_BOTH_ABSENT, USE_OUTSIDE = EMSAR_USAGE_OUTSIDE,
    USE_NOT_RESIDENT = EMSAR_USAGE_NOT_RESIDENT, USE_UNCONVERGED = EMSAR_USAGE_UNCONVERGED, USE_TOO_LARGE = EMSAR_USAGE_TOO_LARGE,
    USE_UNDEFINED = EMSAR_USAGE_UNDEFINED, USE_SINGLE = EMSAR_USAGE_SINGLE
};
inline UsageSearchParams usage_search_params(const emsar_usage_params &up) {
    return UsageSearchParams{up.dev_tol > 0.0 ? up.dev_tol : 1e-4, up.max_evals > 0 ? up.max_evals : 40, up.max_outer > 0 ? up.max_outer : 12};
}

// the search of k_compare_usage_sets on a gene whose parts are all closed form (ca: A's, cb: B's; tc_a, tc_b: t's place in each),
// gene_closed_sum as its evaluation
inline UsageRec compare_usage_closed_search(const CompareGeneClosed *ca, int na, int tc_a, const CompareGeneClosed *cb, int nb, int tc_b, double den_ta,
                                            double mn_a, double den_tb, double mn_b, const UsageSearchParams &Q) {
    const auto eval = [&](bool b, const GenePoint &pt, GeneSums &S) { gene_closed_sum(b ? cb : ca, b ? nb : na, pt, S); };
    return usage_search(den_ta, mn_a, tc_a, den_tb, mn_b, tc_b, Q, eval).record(GeneSolveCount());
}

// what one queried transcript is given
struct UsageResult {
    double lambda = NAN, raw = NAN, usage_a = NAN, usage_b = NAN, usage_null = NAN, dlogit = NAN, slope = NAN;
    int32_t outer = 0, evals = 0, parts = 0, status = USE_NOT_RESIDENT;
};

inline double usage_logit(double u) { return std::log(u / (1.0 - u)); }      // -inf at 0, +inf at 1

// a record -> the transcript's numbers; false for a non-finite F at lambda = 0
inline bool usage_reduce(const UsageRec &r, UsageResult &o) {
    if (!std::isfinite(r.F0_a) || !std::isfinite(r.F0_b)) return false;
    o.outer = r.outer; o.evals = r.evals;
    if (!(r.X0_a > 0.0) || !(r.X0_b > 0.0)) { o.status = USE_UNDEFINED; return true; }
    o.usage_a = r.t0_a / r.X0_a; o.usage_b = r.t0_b / r.X0_b;
    o.dlogit = usage_logit(o.usage_a) - usage_logit(o.usage_b);              // inf - inf = NaN: both shares at the same end
    o.raw = r.outer == 1 ? 0.0 : 2.0 * ((r.F0_a + r.F0_b) - r.best);
    o.lambda = o.raw > 0.0 ? o.raw : 0.0;                                     // a NaN raw value: 0, with UNCONVERGED below
    o.usage_null = r.best_u; o.slope = r.slope;
    if (r.t0_a == 0.0 && r.t0_b == 0.0) o.status = USE_BOTH_ABSENT;
    else o.status = r.flags == (USAGE_REC_OUTER_OK | USAGE_REC_SOLVES_OK | USAGE_REC_INNER_OK) ? USE_TESTED : USE_UNCONVERGED;
    return true;
}

struct CompareUsageRun : GeneQueryMembers {
    using Result = UsageResult;          // per distinct queried transcript
    emsar_hip_ctx *const ctx;            // ctx_a: its gene map, its streams and events
    emsar_hip_ctx *const ctx_b;
    const emsar_em_params *const p;
    const int32_t nq;
    const int32_t *const query;          // caller tids, null = all in order
    const emsar_usage_outputs out;
    UsageSearchParams Q;
    std::vector<int32_t> tids;           // the queried transcripts, each once
    std::vector<int32_t> slot_of_tid;    // [n_tx] -> tids / res, -1 = not queried
    std::vector<Result> res;
    GenePartLists lists;
    DevBuf<int32_t> d_gene_of_b;         // ctx_b's gene_of_lib when it has no map of its own
    SetItemRunner<UsageItem, UsageRec> runner;
    emsar_usage_stats st{};

    CompareUsageRun(emsar_hip_ctx *a, emsar_hip_ctx *b, const emsar_em_params *pp, const emsar_usage_params &up, int32_t nq_, const int32_t *q,
                    const emsar_usage_outputs *o)
        : ctx(a), ctx_b(b), p(pp), nq(nq_), query(q), out(o ? *o : emsar_usage_outputs{}), Q(usage_search_params(up)),
          runner(a, "EMSAR_HIP_COMPARE_USAGE_BATCH", "compare_usage: an item lies outside its class's sets") {}

    int32_t tid_of_query(int32_t i) const { return query ? query[i] : i; }

    int reduce(const UsageRec &r, Result &o) {
        if (!usage_reduce(r, o)) { ctx->err = "compare_usage: non-finite likelihood at lambda = 0"; return EMSAR_HIP_ERR_NUMERIC; }
        if (o.raw < st.min_raw_lambda) st.min_raw_lambda = o.raw;
        return EMSAR_HIP_OK;
    }

    // t in gene slot k of the sample of q, t taking part there: its place among the closed-form parts (-1: in a set part; the order is
    // side_parts') and the smallest den of the other members taking part (inf: none)
    void place_of(const SetQuery &q, size_t k, int32_t t, int32_t &tc, double &mn) const {
        tc = -1; mn = INFINITY;
        int32_t n_closed = 0;
        for (int64_t m = gp[k]; m < gp[k + 1]; m++) {
            const int32_t s = member_tids[(size_t)m];
            const SetQuery::Cand &c = q.cand[(size_t)q.cand_of_lib[(size_t)q.lib_of(s)]];
            if (c.standing == SetQuery::OUTSIDE || c.standing == SetQuery::NOT_RESIDENT) continue;
            if (s == t) { if (c.standing == SetQuery::CLOSED) tc = n_closed; }
            else mn = std::min(mn, q.h_den[(size_t)c.lib]);
            if (c.standing == SetQuery::CLOSED) n_closed++;
        }
    }

    int group_search_reduce(const SetQuery &qa, const SetQuery &qb) {
        res.resize(tids.size());
        std::vector<UsageItem> items[emsar::kSetClasses];
        std::vector<UsageRec> recs[emsar::kSetClasses];
        std::vector<int32_t> who[emsar::kSetClasses];          // item -> tids slot
        const std::vector<int32_t> &of_tx = ctx->genes.h_gene_of_tx;
        struct GeneSides { GeneSideParts a, b; GenePartLists::Offsets at{-1, -1}; bool made = false; };
        std::vector<GeneSides> sides(genes.size());
        for (size_t i = 0; i < tids.size(); i++) {
            const int32_t t = tids[i], g = of_tx[(size_t)t];
            Result &o = res[i];
            if (g < 0) { o.status = USE_OUTSIDE; continue; }
            if (!qa.use_sets || !qb.use_sets) { o.status = USE_NOT_RESIDENT; continue; }
            const size_t k = (size_t)slot_of_gene[(size_t)g];
            GeneSides &G = sides[k];
            if (!G.made) { G.a = side_parts(qa, k, 0); G.b = side_parts(qb, k, 1); G.made = true; }
            const SetQuery::Cand &ta = qa.cand[(size_t)qa.cand_of_lib[(size_t)qa.lib_of(t)]], &tb = qb.cand[(size_t)qb.cand_of_lib[(size_t)qb.lib_of(t)]];
            if (ta.standing == SetQuery::OUTSIDE || tb.standing == SetQuery::OUTSIDE) { o.status = USE_OUTSIDE; continue; }
            if (G.a.not_resident || G.b.not_resident) { o.status = USE_NOT_RESIDENT; continue; }
            if (G.a.members < 2 || G.b.members < 2) { o.status = USE_SINGLE; continue; }
            if (G.a.count() > kGeneMaxParts || G.b.count() > kGeneMaxParts) { o.status = USE_TOO_LARGE; continue; }
            o.parts = G.a.count() + G.b.count();
            st.parts_max = std::max(st.parts_max, o.parts);
            int32_t tc_a, tc_b;
            double mn_a, mn_b;
            place_of(qa, k, t, tc_a, mn_a);
            place_of(qb, k, t, tc_b, mn_b);
            const double den_ta = qa.h_den[(size_t)ta.lib], den_tb = qb.h_den[(size_t)tb.lib];
            if (G.a.sets.empty() && G.b.sets.empty()) {
                const UsageRec r = compare_usage_closed_search(G.a.closed.data(), (int)G.a.closed.size(), tc_a, G.b.closed.data(), (int)G.b.closed.size(),
                                                               tc_b, den_ta, mn_a, den_tb, mn_b, Q);
                if (const int rc = reduce(r, o)) return rc;
                continue;
            }
            if (G.at.part_off < 0) G.at = lists.append(G.a, &G.b);            // the gene's slices, once for all its transcripts
            const int cls = lists.launch_class(G.at.part_off, (int32_t)(G.a.sets.size() + G.b.sets.size()));
            items[cls].push_back(UsageItem{G.at.part_off, (int32_t)G.a.sets.size(), (int32_t)G.b.sets.size(), G.at.closed_off, (int32_t)G.a.closed.size(),
                                           (int32_t)G.b.closed.size(), g, ta.lib, tb.lib, tc_a, tc_b, 0, den_ta, den_tb, mn_a, mn_b});
            who[cls].push_back((int32_t)i);
        }
        const int32_t *gene_of_lib_b = nullptr;
        if (!lists.empty()) {
            if (const int rc = gene_of_lib_of(ctx, ctx_b, d_gene_of_b, gene_of_lib_b)) return rc;
            if (const int rc = lists.upload(ctx)) return rc;
        }
        const SetSolveParams P = set_params(qa.p);
        const CompareSide GA = side_of(ctx), GB = side_of(ctx_b);
        size_t lds[emsar::kSetClasses];
        launch_class_lds(lds, ctx, ctx_b);
        HIPCHK(set_class_lds_attributes(kCompareUsageSets));
        const int32_t n_tx = ctx->n_tx;
        const int rc = runner.run(items, recs, st.device_ms, st.items_launched,
            [&](int c, const UsageItem &it) {
                if (!(it.den_ta > 0.0) || !(it.den_tb > 0.0) || !(it.mn_a > 0.0) || !(it.mn_b > 0.0)) return false;
                if (it.t_a < 0 || it.t_a >= n_tx || it.t_b < 0 || it.t_b >= n_tx) return false;
                if (it.tc_a < -1 || it.tc_a >= it.n_closed_a || it.tc_b < -1 || it.tc_b >= it.n_closed_b) return false;
                return lists.slice_ok(c, it.part_off, it.closed_off, it.gene, {{ctx, it.n_parts_a, it.n_closed_a}, {ctx_b, it.n_parts_b, it.n_closed_b}});
            },
            [&](int c, int threads, hipStream_t s, size_t cnt, const UsageItem *d_items, UsageRec *d_rec) {
                hipLaunchKernelGGL(kCompareUsageSets[c], dim3((unsigned)cnt), dim3(threads), lds[c], s, d_items, lists.d_parts.get(), lists.d_closed.get(),
                                   GA, GB, (const int32_t *)ctx->genes.d_gene_of_lib, gene_of_lib_b, d_rec, P, Q);
            });
        if (rc) return rc;
        for (int cls = 0; cls < emsar::kSetClasses; cls++)
            for (size_t i = 0; i < recs[cls].size(); i++) {
                const UsageRec &r = recs[cls][i];
                add_search_stats(st, r);
                st.outer_sum += r.outer; st.outer_max = std::max(st.outer_max, r.outer);
                if (const int rc2 = reduce(r, res[(size_t)who[cls][i]])) return rc2;
            }
        return EMSAR_HIP_OK;
    }

    int copy_out() {
        for (const Result &o : res) st.n_status[o.status]++;
        for (int32_t i = 0; i < nq; i++) {
            const Result &o = res[(size_t)slot_of_tid[(size_t)tid_of_query(i)]];
            if (out.lambda) out.lambda[i] = o.lambda;
            if (out.raw_lambda) out.raw_lambda[i] = o.raw;
            if (out.pvalue) out.pvalue[i] = compare_pvalue(o.lambda);
            if (out.usage_a) out.usage_a[i] = o.usage_a;
            if (out.usage_b) out.usage_b[i] = o.usage_b;
            if (out.usage_null) out.usage_null[i] = o.usage_null;
            if (out.dlogit) out.dlogit[i] = o.dlogit;
            if (out.slope) out.slope[i] = o.slope;
            if (out.status) out.status[i] = o.status;
            if (out.outer_evals) out.outer_evals[i] = o.outer;
            if (out.evals) out.evals[i] = o.evals;
            if (out.parts) out.parts[i] = o.parts;
        }
        return EMSAR_HIP_OK;
    }

    int run() {
        const std::vector<int32_t> &of_tx = ctx->genes.h_gene_of_tx;
        slot_of_tid.assign((size_t)ctx->n_tx, -1);
        std::vector<int32_t> gene_query;                       // the genes of the queried transcripts, in query order
        for (int32_t i = 0; i < nq; i++) {
            const int32_t t = tid_of_query(i);
            if (slot_of_tid[(size_t)t] >= 0) continue;
            slot_of_tid[(size_t)t] = (int32_t)tids.size();
            tids.push_back(t);
            if (of_tx[(size_t)t] >= 0) gene_query.push_back(of_tx[(size_t)t]);
        }
        list_members(ctx->genes, (int32_t)gene_query.size(), gene_query.data());
        SetQuery qa(ctx, p, (int32_t)member_tids.size(), member_tids.data()), qb(ctx_b, p, (int32_t)member_tids.size(), member_tids.data());
        int rc;
        if ((rc = qa.plan()) || (rc = qa.classify())) return rc;
        if ((rc = qb.plan()) || (rc = qb.classify())) { ctx->err = ctx_b->err; return rc; }
        if ((rc = group_search_reduce(qa, qb))) return rc;
        return copy_out();
    }
};

}  // namespace

extern "C" {

int emsar_hip_compare_usage(emsar_hip_ctx *ctx_a, emsar_hip_ctx *ctx_b, const emsar_em_params *p, const emsar_usage_params *up, int32_t n_query,
                            const int32_t *query_tids, const emsar_usage_outputs *out, emsar_usage_stats *stats) {
    if (const int rc = two_samples_ok(ctx_a, ctx_b, true)) return rc;
    if (const int rc = query_ok(ctx_a, n_query, query_tids)) return rc;
    const emsar_usage_params prm = up ? *up : emsar_usage_params{0.0, 0, 0};
    if (!std::isfinite(prm.dev_tol)) return EMSAR_HIP_ERR_ARG;
    return run_two_sample_call<CompareUsageRun>(ctx_a, ctx_b, stats, p, prm, n_query, query_tids, out);
}

// Diagnostic only (not declared in the public header; makes no HIP call): what emsar_hip_compare_usage gives member t_a of A's list /
// t_b of B's list (the same transcript) of a gene whose members are all one-transcript components -- n_a of them in sample A (u_a[i]
// reads, den_a[i] each; den 0 = takes no part), n_b in B --: the host's statuses and the search the host runs for such genes.
// values[8]: lambda, raw_lambda, pvalue, usage_a, usage_b, usage_null, dlogit, slope.  counts[4]: status, outer_evals, evals, parts.
int emsar_hip_debug_compare_usage_closed(int32_t n_a, const double *u_a, const double *den_a, int32_t t_a, int32_t n_b, const double *u_b,
                                         const double *den_b, int32_t t_b, const emsar_usage_params *up, double *values, int32_t *counts) {
    const emsar_usage_params prm = up ? *up : emsar_usage_params{0.0, 0, 0};
    if (!values || !counts || n_a < 1 || n_b < 1 || !u_a || !den_a || !u_b || !den_b || t_a < 0 || t_a >= n_a || t_b < 0 || t_b >= n_b) return EMSAR_HIP_ERR_ARG;
    if (!std::isfinite(prm.dev_tol)) return EMSAR_HIP_ERR_ARG;
    try {
        std::vector<CompareGeneClosed> c[2];
        int32_t tc[2] = {-1, -1};
        double mn[2] = {INFINITY, INFINITY}, den_t[2] = {0.0, 0.0};
        for (int side = 0; side < 2; side++) {
            const int32_t n = side ? n_b : n_a, t = side ? t_b : t_a;
            const double *u = side ? u_b : u_a, *den = side ? den_b : den_a;
            for (int32_t i = 0; i < n; i++) {
                if (!(u[i] >= 0.0) || !(den[i] >= 0.0)) return EMSAR_HIP_ERR_ARG;
                if (i == t) den_t[side] = den[i];
                if (!(den[i] > 0.0)) continue;
                if (i == t) tc[side] = (int32_t)c[side].size(); else mn[side] = std::min(mn[side], den[i]);
                c[side].push_back(CompareGeneClosed{u[i], den[i]});
            }
        }
        UsageResult o;
        if (tc[0] < 0 || tc[1] < 0) o.status = USE_OUTSIDE;
        else if (c[0].size() < 2 || c[1].size() < 2) o.status = USE_SINGLE;
        else if (c[0].size() > kGeneMaxParts || c[1].size() > kGeneMaxParts) o.status = USE_TOO_LARGE;
        else {
            o.parts = (int32_t)(c[0].size() + c[1].size());
            const UsageRec r = compare_usage_closed_search(c[0].data(), (int)c[0].size(), tc[0], c[1].data(), (int)c[1].size(), tc[1], den_t[0], mn[0],
                                                           den_t[1], mn[1], usage_search_params(prm));
            if (!usage_reduce(r, o)) return EMSAR_HIP_ERR_NUMERIC;
        }
        const double v[8] = {o.lambda, o.raw, compare_pvalue(o.lambda), o.usage_a, o.usage_b, o.usage_null, o.dlogit, o.slope};
        for (int i = 0; i < 8; i++) values[i] = v[i];
        counts[0] = o.status; counts[1] = o.outer; counts[2] = o.evals; counts[3] = o.parts;
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    return EMSAR_HIP_OK;
}

}  // extern "C"
