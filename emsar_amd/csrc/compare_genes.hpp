// compare_genes.hpp -- the gene-level two-sample likelihood-ratio test behind include/emsar_hip.h: emsar_hip_compare_genes.  Part of
// emsar_hip.hip's translation unit, included after compare.hpp: the members of the queried genes are located in each sample as the
// transcript test's queries are (SetQuery, set_items.hpp), k_compare_gene_sets (kernels_compare_genes.hpp) runs the searches.
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

enum { CMP_TOO_LARGE = EMSAR_GENE_COMPARE_TOO_LARGE, kCompareGeneMaxParts = 64 };

// the search of k_compare_gene_sets on a gene whose parts are all closed form (ca: A's, cb: B's), compare_gene_closed_sum as its evaluation
inline CompareRec compare_gene_closed_search(const CompareGeneClosed *ca, int na, const CompareGeneClosed *cb, int nb, double min_a, double min_b,
                                             const CompareSearchParams &Q) {
    CompareStep T;
    T.start();
    double x_a, F_a, x_b, F_b;
    do {
        double shift_a, shift_b;
        compare_gene_shifts(T, Q.ratio, min_b, shift_a, shift_b);
        x_a = F_a = x_b = F_b = 0.0;
        compare_gene_closed_sum(ca, na, min_a, T.pt.scale_a, shift_a, x_a, F_a);
        compare_gene_closed_sum(cb, nb, min_b, T.pt.scale_b, shift_b, x_b, F_b);
    } while (T.step(x_a, F_a, x_b, F_b, min_a, min_b, Q));
    return T.record(0, 1, 0);
}

inline CompareSearchParams compare_search_params(const emsar_compare_params &cp) {
    return CompareSearchParams{cp.ratio == 0.0 ? 1.0 : cp.ratio, cp.dev_tol > 0.0 ? cp.dev_tol : 1e-4, cp.max_evals > 0 ? cp.max_evals : 40, 0};
}

// The members taking part (den > 0) of one gene in one sample, by part.  min_den_live = the smallest den of those that are not
// closed-form members without reads (the gene profile's end-of-range rule asks for it)
struct GeneSideParts {
    std::vector<CompareGenePart> sets;
    std::vector<CompareGeneClosed> closed;
    double min_den = INFINITY, min_den_live = INFINITY;
    int members = 0;
    bool not_resident = false, own_reads = false;      // own_reads: a member taking part has reads only it explains
    int count() const { return (int)(sets.size() + closed.size()); }
};

// The queried genes of a gene-level call and their members, and the grouping of a gene's members into parts (compare_genes.hpp,
// profile_genes.hpp)
struct GeneQueryMembers {
    std::vector<int32_t> genes;          // the queried genes, each once
    std::vector<int32_t> slot_of_gene;   // [n_genes] -> genes / res, -1 = not queried
    std::vector<int64_t> gp;             // genes[k]'s members: member_tids[gp[k] .. gp[k+1]), ascending caller tid
    std::vector<int32_t> member_tids;

    void list_members(const GeneMap &map, int32_t nq, const int32_t *query /* null = all in order */) {
        const int32_t ng = map.n_genes;
        const std::vector<int32_t> &of_tx = map.h_gene_of_tx;
        slot_of_gene.assign((size_t)ng, -1);
        for (int32_t i = 0; i < nq; i++) {
            const int32_t g = query ? query[i] : i;
            if (slot_of_gene[(size_t)g] < 0) { slot_of_gene[(size_t)g] = (int32_t)genes.size(); genes.push_back(g); }
        }
        gp.assign(genes.size() + 1, 0);
        for (int32_t g : of_tx) if (g >= 0 && slot_of_gene[(size_t)g] >= 0) gp[(size_t)slot_of_gene[(size_t)g] + 1]++;
        for (size_t k = 0; k < genes.size(); k++) gp[k + 1] += gp[k];
        member_tids.resize((size_t)gp[genes.size()]);
        std::vector<int64_t> fill(gp.begin(), gp.end() - 1);
        for (int32_t t = 0; t < (int32_t)of_tx.size(); t++) {
            const int32_t g = of_tx[(size_t)t];
            if (g >= 0 && slot_of_gene[(size_t)g] >= 0) member_tids[(size_t)fill[(size_t)slot_of_gene[(size_t)g]]++] = t;
        }
    }

    // gene slot k in the sample of q: the members with den > 0 there, ascending caller tid, so parts come by their smallest tid
    GeneSideParts side_parts(const SetQuery &q, size_t k, int32_t side) const {
        GeneSideParts s;
        for (int64_t m = gp[k]; m < gp[k + 1]; m++) {
            const SetQuery::Cand &c = q.cand[(size_t)q.cand_of_lib[(size_t)q.lib_of(member_tids[(size_t)m])]];
            if (c.standing == SetQuery::OUTSIDE) continue;             // den == 0: held at 0 in this sample
            if (c.standing == SetQuery::NOT_RESIDENT) { s.not_resident = true; continue; }
            const double den = q.h_den[(size_t)c.lib];
            s.min_den = std::min(s.min_den, den);
            s.members++;
            if (c.standing == SetQuery::CLOSED) {
                s.closed.push_back(CompareGeneClosed{c.u, den});
                if (c.u > 0.0) { s.min_den_live = std::min(s.min_den_live, den); s.own_reads = true; }
                continue;
            }
            s.min_den_live = std::min(s.min_den_live, den);
            s.own_reads |= c.own_reads;
            bool seen = false;
            for (const CompareGenePart &p : s.sets) seen |= p.set == c.set && p.cls == c.cls;
            if (!seen) s.sets.push_back(CompareGenePart{side, c.set, c.cls, 0});
        }
        return s;
    }
};

// ctx_b's gene_of_lib for a two-sample call whose map lives on ctx_a: ctx_b's own when it has the map, else ctx_a's map in ctx_b's
// library numbering, uploaded into `hold` (compare_genes.hpp, compare_usage.hpp)
inline int gene_of_lib_of_b(emsar_hip_ctx *ctx, emsar_hip_ctx *ctx_b, DevBuf<int32_t> &hold, const int32_t *&ptr) {
    if (ctx_b->genes.have_genes) { ptr = ctx_b->genes.d_gene_of_lib; return EMSAR_HIP_OK; }
    const std::vector<int32_t> &of_tx = ctx->genes.h_gene_of_tx;
    std::vector<int32_t> of_lib(of_tx.size());
    const bool remap = renumbered(ctx_b);
    for (size_t t = 0; t < of_tx.size(); t++) of_lib[remap ? (size_t)tid_map(ctx_b)[t] : t] = of_tx[t];
    HIPCHK(hold.upload(of_lib.data(), of_lib.size()));
    ptr = hold;
    return EMSAR_HIP_OK;
}

struct CompareGenesRun : GeneQueryMembers {
    struct Result : CompareResult { int32_t parts = 0; };      // per queried gene; theta_a / theta_b / theta_null hold the gene sums
    using SideParts = GeneSideParts;
    emsar_hip_ctx *const ctx;            // ctx_a: its gene map, its streams and events
    emsar_hip_ctx *const ctx_b;
    const emsar_em_params *const p;      // the caller's solver parameters (SetQuery fills in the defaults)
    const int32_t nq;
    const int32_t *const query;          // gene ids, null = all in order
    const emsar_compare_gene_outputs out;
    CompareSearchParams Q;
    std::vector<Result> res;
    std::vector<CompareGenePart> h_parts;
    std::vector<CompareGeneClosed> h_closed;
    DevBuf<CompareGenePart> d_parts;
    DevBuf<CompareGeneClosed> d_closed;
    DevBuf<int32_t> d_gene_of_b;         // ctx_b's gene_of_lib when it has no map of its own
    SetItemRunner<CompareGeneItem, CompareRec> runner;
    emsar_compare_gene_stats st{};

    CompareGenesRun(emsar_hip_ctx *a, emsar_hip_ctx *b, const emsar_em_params *pp, const emsar_compare_params &cp, int32_t nq_, const int32_t *q,
                    const emsar_compare_gene_outputs *o)
        : ctx(a), ctx_b(b), p(pp), nq(nq_), query(q), out(o ? *o : emsar_compare_gene_outputs{}), Q(compare_search_params(cp)),
          runner(a, "EMSAR_HIP_COMPARE_GENES_BATCH", "compare_genes: an item lies outside its class's sets") {}

    int32_t gene_of_query(int32_t i) const { return query ? query[i] : i; }

    static CompareSide side_of(const emsar_hip_ctx *c) { return CompareRun::side_of(c); }

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
            const SideParts a = side_parts(qa, k, 0), b = side_parts(qb, k, 1);
            if (a.not_resident || b.not_resident) { o.status = CMP_NOT_RESIDENT; continue; }
            if (a.count() == 0 || b.count() == 0) { o.status = CMP_OUTSIDE; continue; }
            if (a.count() > kCompareGeneMaxParts || b.count() > kCompareGeneMaxParts) { o.status = CMP_TOO_LARGE; continue; }
            o.parts = a.count() + b.count();
            st.parts_max = std::max(st.parts_max, o.parts);
            if (a.sets.empty() && b.sets.empty()) {
                const CompareRec r = compare_gene_closed_search(a.closed.data(), (int)a.closed.size(), b.closed.data(), (int)b.closed.size(),
                                                                a.min_den, b.min_den, Q);
                if (const int rc = reduce(r, o)) return rc;
                continue;
            }
            int cls = -1;
            for (const CompareGenePart &p : a.sets) cls = std::max(cls, (int)p.cls);
            for (const CompareGenePart &p : b.sets) cls = std::max(cls, (int)p.cls);
            items[cls].push_back(CompareGeneItem{(int32_t)h_parts.size(), (int32_t)a.sets.size(), (int32_t)b.sets.size(), (int32_t)h_closed.size(),
                                                 (int32_t)a.closed.size(), (int32_t)b.closed.size(), genes[k], 0, a.min_den, b.min_den});
            who[cls].push_back((int32_t)k);
            h_parts.insert(h_parts.end(), a.sets.begin(), a.sets.end());
            h_parts.insert(h_parts.end(), b.sets.begin(), b.sets.end());
            h_closed.insert(h_closed.end(), a.closed.begin(), a.closed.end());
            h_closed.insert(h_closed.end(), b.closed.begin(), b.closed.end());
        }
        const int32_t *gene_of_lib_b = nullptr;
        if (!h_parts.empty()) {
            if (const int rc = gene_of_lib_of_b(ctx, ctx_b, d_gene_of_b, gene_of_lib_b)) return rc;
            HIPCHK(d_parts.upload(h_parts.data(), h_parts.size()));
            HIPCHK(d_closed.upload(h_closed.data(), h_closed.size()));
        }
        const SetSolveParams P = set_params(qa.p);
        const CompareSide GA = side_of(ctx), GB = side_of(ctx_b);
        const auto &SA = ctx->sets.RS, &SB = ctx_b->sets.RS;
        size_t lds[emsar::kSetClasses], most = 0;              // a launch class holds the sets of its own and of every smaller class
        for (int c = 0; c < emsar::kSetClasses; c++) lds[c] = most = std::max(most, std::max((size_t)SA.max_lds[c], (size_t)SB.max_lds[c]));
        HIPCHK(set_class_lds_attributes(kCompareGeneSets));
        const int rc = runner.run(items, recs, st.device_ms, st.items_launched,
            [&](int c, const CompareGeneItem &it) {
                if (!(it.min_a > 0.0) || !(it.min_b > 0.0) || it.n_parts_a < 0 || it.n_parts_b < 0 || it.n_closed_a < 0 || it.n_closed_b < 0) return false;
                if (it.n_parts_a > kCompareGeneMaxParts || it.n_parts_b > kCompareGeneMaxParts || it.part_off < 0 || it.closed_off < 0) return false;
                if ((size_t)it.part_off + (size_t)(it.n_parts_a + it.n_parts_b) > h_parts.size()) return false;
                if ((size_t)it.closed_off + (size_t)(it.n_closed_a + it.n_closed_b) > h_closed.size()) return false;
                if (it.gene < 0 || it.gene >= ctx->genes.n_genes) return false;
                int top = -1;
                for (int32_t k = 0; k < it.n_parts_a + it.n_parts_b; k++) {
                    const CompareGenePart &p = h_parts[(size_t)it.part_off + (size_t)k];
                    if (p.side != (k < it.n_parts_a ? 0 : 1) || p.cls > c || !set_desc(p.side ? ctx_b : ctx, p.cls, p.set)) return false;
                    top = std::max(top, (int)p.cls);
                }
                return top == c;
            },
            [&](int c, int threads, hipStream_t s, size_t cnt, const CompareGeneItem *d_items, CompareRec *d_rec) {
                hipLaunchKernelGGL(kCompareGeneSets[c], dim3((unsigned)cnt), dim3(threads), lds[c], s, d_items, d_parts.get(), d_closed.get(), GA, GB,
                                   (const int32_t *)ctx->genes.d_gene_of_lib, gene_of_lib_b, d_rec, P, Q);
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
    if (!ctx_a || !ctx_b || ctx_a == ctx_b) return EMSAR_HIP_ERR_ARG;
    if (!ctx_a->have_sample || !ctx_b->have_sample) return EMSAR_HIP_ERR_STATE;      // first: a state error whatever the other arguments say
    if (ctx_a->device != ctx_b->device || !same_structure(ctx_a, ctx_b)) return EMSAR_HIP_ERR_ARG;
    if (!ctx_a->genes.have_genes) return EMSAR_HIP_ERR_STATE;
    const GeneMap &ga = ctx_a->genes, &gb = ctx_b->genes;
    if (gb.have_genes && (gb.n_genes != ga.n_genes || gb.h_gene_of_tx != ga.h_gene_of_tx)) return EMSAR_HIP_ERR_ARG;
    if (!query_genes) n_query = ga.n_genes;
    if (n_query < 0) return EMSAR_HIP_ERR_ARG;
    if (query_genes) for (int32_t i = 0; i < n_query; i++) if (query_genes[i] < 0 || query_genes[i] >= ga.n_genes) return EMSAR_HIP_ERR_ARG;
    const emsar_compare_params prm = cp ? *cp : emsar_compare_params{1.0, 0.0, 0, 0};
    if (!compare_params_ok(prm)) return EMSAR_HIP_ERR_ARG;
    emsar_hip_ctx *const ctx = ctx_b;
    HIPCHK(hipSetDevice(ctx_b->device));
    HIPCHK(hipStreamSynchronize(ctx_b->stream));
    return run_query_call<CompareGenesRun>(ctx_a, stats, ctx_b, p, prm, n_query, query_genes, out);
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
