// compare_genes.hpp -- the gene-level two-sample likelihood-ratio test behind include/emsar_hip.h: emsar_hip_compare_genes.  Part of
// emsar_hip.hip's translation unit, included after gene_parts.hpp: the members of the queried genes are located in each sample as the
// transcript test's queries are (SetQuery, set_items.hpp) and grouped into parts (GeneQueryMembers, GenePartLists: gene_parts.hpp),
// k_compare_gene_sets (kernels_compare_genes.hpp) runs the searches.
// One call = one CompareGenesRun:  plan, classify   SetQuery's stages on the union of the queried genes' members, once per context
//                                  group            per gene and sample: the members taking part (den > 0) by part -- the packed sets that
//                                                   hold one, the one-transcript components --, the smallest den; the host-only statuses;
//                                                   a gene whose parts are all closed form is searched on the host, any other is one item
//                                                   in the launch class of its largest set part
//                                  search           the items in batches across the three launch classes (SetItemRunner)
//                                  reduce           records -> Lambda, p, log2fc, status (compare_reduce);  copy_out in query order
// One workgroup runs one search of at most max_evals evaluations of at most 2 * 64 solves of at most max_iter passes each.  Neither
// context's theta, weights or scales are touched.  The launches run on ctx_a's streams; ctx_b's stream is drained before.

namespace {

enum { CMP_TOO_LARGE = EMSAR_GENE_COMPARE_TOO_LARGE };

// the search of k_compare_gene_sets on a gene whose parts are all closed form (ca: A's, cb: B's), gene_closed_sum as its evaluation
inline CompareRec compare_gene_closed_search(const CompareGeneClosed *ca, int na, const CompareGeneClosed *cb, int nb, double min_a, double min_b,
                                             const CompareSearchParams &Q) {
    const auto eval = [&](bool b, const GenePoint &pt, GeneSums &S) { gene_closed_sum(b ? cb : ca, b ? nb : na, pt, S); };
    return compare_gene_search(min_a, min_b, Q, eval).record(0, 1, 0);
}

inline CompareSearchParams compare_search_params(const emsar_compare_params &cp) {
    return CompareSearchParams{cp.ratio == 0.0 ? 1.0 : cp.ratio, cp.dev_tol > 0.0 ? cp.dev_tol : 1e-4, cp.max_evals > 0 ? cp.max_evals : 40, 0};
}

struct CompareGenesRun : GeneQueryMembers {
    struct Result : CompareResult { int32_t parts = 0; };      // per queried gene; theta_a / theta_b / theta_null hold the gene sums
    emsar_hip_ctx *const ctx;            // ctx_a: its gene map, its streams and events
    emsar_hip_ctx *const ctx_b;
    const emsar_em_params *const p;      // the caller's solver parameters (SetQuery fills in the defaults)
    const int32_t nq;
    const int32_t *const query;          // gene ids, null = all in order
    const emsar_compare_gene_outputs out;
    CompareSearchParams Q;
    std::vector<Result> res;
    GenePartLists lists;
    DevBuf<int32_t> d_gene_of_b;         // ctx_b's gene_of_lib when it has no map of its own
    SetItemRunner<CompareGeneItem, CompareRec> runner;
    emsar_compare_gene_stats st{};

    CompareGenesRun(emsar_hip_ctx *a, emsar_hip_ctx *b, const emsar_em_params *pp, const emsar_compare_params &cp, int32_t nq_, const int32_t *q,
                    const emsar_compare_gene_outputs *o)
        : ctx(a), ctx_b(b), p(pp), nq(nq_), query(q), out(o ? *o : emsar_compare_gene_outputs{}), Q(compare_search_params(cp)),
          runner(a, "EMSAR_HIP_COMPARE_GENES_BATCH", "compare_genes: an item lies outside its class's sets") {}

    int32_t gene_of_query(int32_t i) const { return query ? query[i] : i; }

    int reduce(const CompareRec &r, Result &o) {
        if (!compare_reduce(r, Q.ratio, o)) { ctx->err = "compare_genes: non-finite likelihood at lambda = 0"; return EMSAR_HIP_ERR_NUMERIC; }
        if (o.raw < st.min_raw_lambda) st.min_raw_lambda = o.raw;
        return EMSAR_HIP_OK;
    }

    int group_search_reduce(const SetQuery &qa, const SetQuery &qb) {
        res.resize(genes.size());
        std::vector<CompareGeneItem> items[emsar::kSetClasses];
        std::vector<CompareRec> recs[emsar::kSetClasses];
        std::vector<int32_t> who[emsar::kSetClasses];          // item -> gene slot
        for (size_t k = 0; k < genes.size(); k++) {
            Result &o = res[k];
            if (!qa.use_sets || !qb.use_sets) { o.status = CMP_NOT_RESIDENT; continue; }
            const GeneSideParts a = side_parts(qa, k, 0), b = side_parts(qb, k, 1);
            if (a.not_resident || b.not_resident) { o.status = CMP_NOT_RESIDENT; continue; }
            if (a.count() == 0 || b.count() == 0) { o.status = CMP_OUTSIDE; continue; }
            if (a.count() > kGeneMaxParts || b.count() > kGeneMaxParts) { o.status = CMP_TOO_LARGE; continue; }
            o.parts = a.count() + b.count();
            st.parts_max = std::max(st.parts_max, o.parts);
            if (a.sets.empty() && b.sets.empty()) {
                const CompareRec r = compare_gene_closed_search(a.closed.data(), (int)a.closed.size(), b.closed.data(), (int)b.closed.size(),
                                                                a.min_den, b.min_den, Q);
                if (const int rc = reduce(r, o)) return rc;
                continue;
            }
            const GenePartLists::Offsets at = lists.append(a, &b);
            const int cls = lists.launch_class(at.part_off, (int32_t)(a.sets.size() + b.sets.size()));
            items[cls].push_back(CompareGeneItem{at.part_off, (int32_t)a.sets.size(), (int32_t)b.sets.size(), at.closed_off, (int32_t)a.closed.size(),
                                                 (int32_t)b.closed.size(), genes[k], 0, a.min_den, b.min_den});
            who[cls].push_back((int32_t)k);
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
        HIPCHK(set_class_lds_attributes(kCompareGeneSets));
        const int rc = runner.run(items, recs, st.device_ms, st.items_launched,
            [&](int c, const CompareGeneItem &it) {
                return it.min_a > 0.0 && it.min_b > 0.0 &&
                       lists.slice_ok(c, it.part_off, it.closed_off, it.gene, {{ctx, it.n_parts_a, it.n_closed_a}, {ctx_b, it.n_parts_b, it.n_closed_b}});
            },
            [&](int c, int threads, hipStream_t s, size_t cnt, const CompareGeneItem *d_items, CompareRec *d_rec) {
                hipLaunchKernelGGL(kCompareGeneSets[c], dim3((unsigned)cnt), dim3(threads), lds[c], s, d_items, lists.d_parts.get(), lists.d_closed.get(),
                                   GA, GB, (const int32_t *)ctx->genes.d_gene_of_lib, gene_of_lib_b, d_rec, P, Q);
            });
        if (rc) return rc;
        for (int cls = 0; cls < emsar::kSetClasses; cls++)
            for (size_t i = 0; i < recs[cls].size(); i++) {
                add_search_stats(st, recs[cls][i]);
                if (const int rc2 = reduce(recs[cls][i], res[(size_t)who[cls][i]])) return rc2;
            }
        return EMSAR_HIP_OK;
    }

    int copy_out() {
        for (const Result &o : res) st.n_status[o.status]++;
        for (int32_t i = 0; i < nq; i++) {
            const Result &o = res[(size_t)slot_of_gene[(size_t)gene_of_query(i)]];
            if (out.lambda) out.lambda[i] = o.lambda;
            if (out.pvalue) out.pvalue[i] = compare_pvalue(o.lambda);
            if (out.log2fc) out.log2fc[i] = o.log2fc;
            if (out.gene_a) out.gene_a[i] = o.theta_a;
            if (out.gene_b) out.gene_b[i] = o.theta_b;
            if (out.gene_null) out.gene_null[i] = o.theta_null;
            if (out.multiplier) out.multiplier[i] = o.multiplier;
            if (out.gap) out.gap[i] = o.gap;
            if (out.raw_lambda) out.raw_lambda[i] = o.raw;
            if (out.status) out.status[i] = o.status;
            if (out.evals) out.evals[i] = o.evals;
            if (out.parts) out.parts[i] = o.parts;
        }
        return EMSAR_HIP_OK;
    }

    int run() {
        list_members(ctx->genes, nq, query);
        SetQuery qa(ctx, p, (int32_t)member_tids.size(), member_tids.data()), qb(ctx_b, p, (int32_t)member_tids.size(), member_tids.data());
        int rc;
        if ((rc = qa.plan()) || (rc = qa.classify())) return rc;
        if ((rc = qb.plan()) || (rc = qb.classify())) { ctx->err = ctx_b->err; return rc; }
        if ((rc = group_search_reduce(qa, qb))) return rc;
        return copy_out();
    }
};

inline bool compare_params_ok(const emsar_compare_params &prm) { return std::isfinite(prm.ratio) && prm.ratio >= 0.0 && std::isfinite(prm.dev_tol); }

}  // namespace

extern "C" {

int emsar_hip_compare_genes(emsar_hip_ctx *ctx_a, emsar_hip_ctx *ctx_b, const emsar_em_params *p, const emsar_compare_params *cp, int32_t n_query,
                            const int32_t *query_genes, const emsar_compare_gene_outputs *out, emsar_compare_gene_stats *stats) {
    if (const int rc = two_samples_ok(ctx_a, ctx_b, true)) return rc;
    if (const int rc = gene_query_ok(ctx_a, n_query, query_genes)) return rc;
    const emsar_compare_params prm = cp ? *cp : emsar_compare_params{1.0, 0.0, 0, 0};
    if (!compare_params_ok(prm)) return EMSAR_HIP_ERR_ARG;
    return run_two_sample_call<CompareGenesRun>(ctx_a, ctx_b, stats, p, prm, n_query, query_genes, out);
}

// Diagnostic only (not declared in the public header; needs no device): what emsar_hip_compare_genes gives a gene whose parts are all
// closed form -- n_a one-transcript components in sample A (u_a[i] reads, den_a[i] each), n_b in B --: the search the host runs for such
// genes.  values[9]: lambda, pvalue, log2fc, gene_a, gene_b, gene_null, multiplier, gap, raw_lambda.
int emsar_hip_debug_compare_genes_closed(int32_t n_a, const double *u_a, const double *den_a, int32_t n_b, const double *u_b, const double *den_b,
                                         const emsar_compare_params *cp, double *values, int32_t *status, int32_t *evals) {
    const emsar_compare_params prm = cp ? *cp : emsar_compare_params{1.0, 0.0, 0, 0};
    if (!values || !status || !evals || n_a < 1 || n_b < 1 || !u_a || !den_a || !u_b || !den_b || !compare_params_ok(prm)) return EMSAR_HIP_ERR_ARG;
    try {
        std::vector<CompareGeneClosed> ca((size_t)n_a), cb((size_t)n_b);
        double min_a = INFINITY, min_b = INFINITY;
        for (int32_t i = 0; i < n_a; i++) {
            if (!(u_a[i] >= 0.0) || !(den_a[i] > 0.0)) return EMSAR_HIP_ERR_ARG;
            ca[(size_t)i] = CompareGeneClosed{u_a[i], den_a[i]}; min_a = std::min(min_a, den_a[i]);
        }
        for (int32_t i = 0; i < n_b; i++) {
            if (!(u_b[i] >= 0.0) || !(den_b[i] > 0.0)) return EMSAR_HIP_ERR_ARG;
            cb[(size_t)i] = CompareGeneClosed{u_b[i], den_b[i]}; min_b = std::min(min_b, den_b[i]);
        }
        const CompareSearchParams Q = compare_search_params(prm);
        CompareResult o;
        if (!compare_reduce(compare_gene_closed_search(ca.data(), n_a, cb.data(), n_b, min_a, min_b, Q), Q.ratio, o)) return EMSAR_HIP_ERR_NUMERIC;
        const double v[9] = {o.lambda, compare_pvalue(o.lambda), o.log2fc, o.theta_a, o.theta_b, o.theta_null, o.multiplier, o.gap, o.raw};
        for (int i = 0; i < 9; i++) values[i] = v[i];
        *status = o.status; *evals = o.evals;
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    return EMSAR_HIP_OK;
}

}  // extern "C"
