// profile_genes.hpp -- the gene-level profile-likelihood intervals and the gene presence test behind include/emsar_hip.h:
// emsar_hip_profile_genes (device) and emsar_hip_gene_presence_pvalue_host (no HIP call).  Part of emsar_hip.hip's translation unit,
// included after gene_parts.hpp: the members of the queried genes are located and grouped into parts as the gene-level two-sample
// test does (SetQuery; GeneQueryMembers, GenePartLists: gene_parts.hpp), k_profile_gene_base and k_profile_gene_sets
// (kernels_profile_genes.hpp) do the solves.
// One call = one ProfileGenesRun:  plan, classify   SetQuery's stages on the union of the queried genes' members
//                                  group            per gene: its parts, mn, the end of the upper range; the host-only statuses; a gene
//                                                   whose parts are all closed form is finished on the host (profile_gene_closed)
//                                  baseline         one item per remaining gene: X_hat, F_hat, F_drop -> Lambda, status
//                                  search           one item per limit to find -- upper always, lower where Lambda > q --, in batches
//                                                   across the three launch classes (SetItemRunner)
//                                  reduce           records -> limits, deviances, status;  copy_out in query order
// One workgroup runs one search of at most max_evals evaluations of at most 64 solves of at most max_iter passes each.  The context's
// theta, weights and scales are not touched.

namespace {

enum { GPROF_TOO_LARGE = EMSAR_GENE_PROFILE_TOO_LARGE };

// P(chi2_k > lambda), x = lambda / 2: k even exp(-x) sum_{j < k/2} x^j / j!, k odd erfc(sqrt x) + exp(-x) sum_{j=1}^{(k-1)/2}
// x^(j-1/2) / Gamma(j+1/2).  The terms are built by their ratios; beyond x = 700, where exp(-x) underflows against terms that
// overflow, each term is exp(its logarithm).
inline double gene_presence_pvalue(double lambda, int32_t k) {
    if (!(lambda == lambda) || k < 1) return NAN;
    if (lambda <= 0.0) return 1.0;
    if (std::isinf(lambda)) return 0.0;
    const double x = 0.5 * lambda;
    const bool odd = (k & 1) != 0;
    const int n_terms = odd ? (k - 1) / 2 : k / 2;
    double sum = 0.0;
    if (x < 700.0) {
        double term = odd ? 2.0 * std::sqrt(x / M_PI) : 1.0;       // x^(1/2) / Gamma(3/2), or x^0 / 0!
        for (int j = 0; j < n_terms; j++) {
            sum += term;
            term *= odd ? x / ((double)j + 1.5) : x / (double)(j + 1);
        }
        sum *= std::exp(-x);
    } else {
        const double lx = std::log(x);
        for (int j = 0; j < n_terms; j++) {
            const double a = odd ? (double)j + 0.5 : (double)j;    // the term x^a / Gamma(a + 1)
            sum += std::exp(a * lx - std::lgamma(a + 1.0) - x);
        }
    }
    const double p = (odd ? std::erfc(std::sqrt(x)) : 0.0) + sum;
    return p > 1.0 ? 1.0 : p;
}

// what one queried gene is given
struct ProfileGeneResult {
    double lower = NAN, upper = NAN, dev_lower = NAN, dev_upper = NAN, lambda = NAN, gene_hat = NAN;
    int32_t evals = 0, evals_upper = 0, parts = 0, members = 0, status = PROF_NOT_RESIDENT;     // evals: both searches
    bool capped = false;                 // a search or a solve hit its cap
};

// The end of the upper range (ProfileGeneStep): mn0 = the smallest den of the closed-form members without reads; reachable when it lies
// strictly below the den of every other member taking part
inline bool profile_gene_end(const GeneSideParts &s, double &mn0) {
    mn0 = INFINITY;
    for (const CompareGeneClosed &c : s.closed) if (!(c.u > 0.0)) mn0 = std::min(mn0, c.den);
    return mn0 < s.min_den_live;
}

// Lambda and the status it decides, from the raw value (+inf for an essential gene)
inline void profile_gene_presence(double raw, double q, ProfileGeneResult &o) {
    o.lambda = raw > 0.0 ? raw : 0.0;
    o.status = o.lambda > q ? PROF_TWO_SIDED : PROF_LOWER_ZERO;
    if (o.status == PROF_LOWER_ZERO) { o.lower = 0.0; o.dev_lower = o.lambda; }
}

inline void profile_gene_take(const ProfileRec &r, int side, ProfileGeneResult &o) {
    o.evals += r.evals;
    if (r.flags != (PROFILE_REC_SEARCH_OK | PROFILE_REC_SOLVES_OK)) o.capped = true;
    if (side == 0) { o.lower = r.x; o.dev_lower = r.dev; }
    else { o.upper = r.x; o.dev_upper = r.dev; o.evals_upper = r.evals; }
}

// one limit of a gene whose parts are all closed form: k_profile_gene_sets' loop with gene_closed_sum as its evaluation
inline ProfileRec profile_gene_closed_limit(const CompareGeneClosed *c, int n, int side, int end, double mn, double mn0, double X_hat, double F_hat,
                                            const ProfileSearchParams &Q) {
    ProfileGeneStep T;
    T.start(side, end, X_hat, mn, F_hat, Q);
    const double sqrt_q = std::sqrt(Q.q);
    GeneSums S;
    do {
        const double s = T.scale();
        S = GeneSums{0.0, 0.0, 0.0};
        gene_closed_sum(c, n, GenePoint{mn, s, mn * (s - 1.0), -1, 0.0}, S);
    } while (T.step(S.X, S.F, F_hat, mn0, sqrt_q));
    return profile_gene_record(T, GeneSolveCount());
}

// A gene whose parts are all closed form (s.sets empty, s.closed not): baseline, Lambda and both limits on the host.  A member with
// reads makes the gene essential (only it explains them); without any the gene sum is 0, Lambda 0, and upper = q / (2 mn) as the
// transcript profile's closed form has it.  False for a non-finite F_hat.
inline bool profile_gene_closed(const GeneSideParts &s, const ProfileSearchParams &Q, ProfileGeneResult &o) {
    const CompareGeneClosed *c = s.closed.data();
    const int n = (int)s.closed.size();
    GeneSums hat{0.0, 0.0, 0.0};
    gene_closed_sum(c, n, GenePoint{s.min_den, 1.0, 0.0, -1, 0.0}, hat);
    const double X_hat = hat.X, F_hat = hat.F;
    double mn0;
    if (!std::isfinite(F_hat) || !std::isfinite(X_hat)) return false;
    o.gene_hat = X_hat;
    profile_gene_presence(s.own_reads ? INFINITY : 0.0, Q.q, o);
    if (!s.own_reads) { o.upper = Q.q / (2.0 * s.min_den); o.dev_upper = Q.q; return true; }
    const int end = profile_gene_end(s, mn0) ? 1 : 0;
    profile_gene_take(profile_gene_closed_limit(c, n, 0, 0, s.min_den, mn0, X_hat, F_hat, Q), 0, o);
    profile_gene_take(profile_gene_closed_limit(c, n, 1, end, s.min_den, mn0, X_hat, F_hat, Q), 1, o);
    return true;
}

inline ProfileSearchParams profile_search_params(const emsar_profile_params &pp) {
    return ProfileSearchParams{profile_cut(pp.level), pp.dev_tol > 0.0 ? pp.dev_tol : 1e-4, pp.max_evals > 0 ? pp.max_evals : 40, 0};
}
inline bool profile_params_ok(const emsar_profile_params &prm) { return prm.level > 0.0 && prm.level < 1.0 && std::isfinite(prm.dev_tol); }

struct ProfileGenesRun : GeneQueryMembers {
    // a gene that goes to the device: its slices of the lists and what its items share
    struct Pending { int32_t slot, cls, part_off, n_parts, closed_off, n_closed, end; double mn, mn0; bool own_reads; };
    emsar_hip_ctx *const ctx;
    const emsar_em_params *const p;      // the caller's solver parameters (SetQuery fills in the defaults)
    const int32_t nq;
    const int32_t *const query;          // gene ids, null = all in order
    const emsar_profile_gene_outputs out;
    ProfileSearchParams Q;
    std::vector<ProfileGeneResult> res;
    std::vector<Pending> pending;
    GenePartLists lists;
    SetItemRunner<ProfileGeneBaseItem, ProfileGeneBaseRec> base_runner;
    SetItemRunner<ProfileGeneItem, ProfileRec> runner;
    emsar_profile_gene_stats st{};

    ProfileGenesRun(emsar_hip_ctx *c, const emsar_em_params *pp, const emsar_profile_params &prm, int32_t nq_, const int32_t *q,
                    const emsar_profile_gene_outputs *o)
        : ctx(c), p(pp), nq(nq_), query(q), out(o ? *o : emsar_profile_gene_outputs{}), Q(profile_search_params(prm)),
          base_runner(c, "EMSAR_HIP_PROFILE_GENES_BATCH", "profile_genes: a baseline item lies outside its class's sets"),
          runner(c, "EMSAR_HIP_PROFILE_GENES_BATCH", "profile_genes: an item lies outside its class's sets") { st.cut = Q.q; }

    int numeric() { ctx->err = "profile_genes: non-finite likelihood at the baseline"; return EMSAR_HIP_ERR_NUMERIC; }

    int group(const SetQuery &q) {
        res.resize(genes.size());
        for (size_t k = 0; k < genes.size(); k++) {
            ProfileGeneResult &o = res[k];
            if (!q.use_sets) { o.status = PROF_NOT_RESIDENT; continue; }
            const GeneSideParts s = side_parts(q, k, 0);
            if (s.not_resident) { o.status = PROF_NOT_RESIDENT; continue; }
            if (s.count() == 0) { o.status = PROF_OUTSIDE; continue; }
            if (s.count() > kGeneMaxParts) { o.status = GPROF_TOO_LARGE; continue; }
            o.parts = s.count(); o.members = s.members;
            st.parts_max = std::max(st.parts_max, o.parts);
            if (s.sets.empty()) {
                if (!profile_gene_closed(s, Q, o)) return numeric();
                continue;
            }
            Pending g;
            const GenePartLists::Offsets at = lists.append(s);
            g.slot = (int32_t)k;
            g.part_off = at.part_off; g.n_parts = (int32_t)s.sets.size();
            g.closed_off = at.closed_off; g.n_closed = (int32_t)s.closed.size();
            g.cls = lists.launch_class(g.part_off, g.n_parts);
            g.end = profile_gene_end(s, g.mn0) ? 1 : 0;
            if (!g.end) g.mn0 = s.min_den;           // never used; keeps the item finite
            g.mn = s.min_den; g.own_reads = s.own_reads;
            pending.push_back(g);
        }
        return EMSAR_HIP_OK;
    }

    // what the two item kinds share: mn and the slices (GenePartLists::slice_ok)
    bool slices_ok(int c, int32_t part_off, int32_t n_parts, int32_t closed_off, int32_t n_closed, int32_t gene, double mn) const {
        return mn > 0.0 && lists.slice_ok(c, part_off, closed_off, gene, {{ctx, n_parts, n_closed}});
    }

    int solve_search_reduce(const SetQuery &q) {
        if (pending.empty()) return EMSAR_HIP_OK;
        if (const int urc = lists.upload(ctx)) return urc;
        const SetSolveParams P = set_params(q.p);
        const CompareSide G = side_of(ctx);
        const int32_t *gene_of = ctx->genes.d_gene_of_lib;
        size_t lds[emsar::kSetClasses];
        launch_class_lds(lds, ctx);

        // baseline and drop
        std::vector<ProfileGeneBaseItem> bitems[emsar::kSetClasses];
        std::vector<ProfileGeneBaseRec> brecs[emsar::kSetClasses];
        std::vector<int32_t> bwho[emsar::kSetClasses];         // item -> pending
        for (size_t i = 0; i < pending.size(); i++) {
            const Pending &g = pending[i];
            bitems[g.cls].push_back(ProfileGeneBaseItem{g.part_off, g.n_parts, g.closed_off, g.n_closed, genes[(size_t)g.slot], g.own_reads ? 1 : 0, g.mn});
            bwho[g.cls].push_back((int32_t)i);
        }
        HIPCHK(set_class_lds_attributes(kProfileGeneBase));
        int rc = base_runner.run(bitems, brecs, st.baseline_ms, st.items_launched,
            [&](int c, const ProfileGeneBaseItem &it) { return slices_ok(c, it.part_off, it.n_parts, it.closed_off, it.n_closed, it.gene, it.mn); },
            [&](int c, int threads, hipStream_t s, size_t cnt, const ProfileGeneBaseItem *d_items, ProfileGeneBaseRec *d_rec) {
                hipLaunchKernelGGL(kProfileGeneBase[c], dim3((unsigned)cnt), dim3(threads), lds[c], s, d_items, lists.d_parts.get(), lists.d_closed.get(),
                                   G, gene_of, d_rec, P);
            });
        if (rc) return rc;

        // Lambda, status, and the limits to search
        std::vector<ProfileGeneItem> items[emsar::kSetClasses];
        std::vector<ProfileRec> recs[emsar::kSetClasses];
        std::vector<int32_t> who[emsar::kSetClasses];          // item -> gene slot
        for (int cls = 0; cls < emsar::kSetClasses; cls++)
            for (size_t i = 0; i < brecs[cls].size(); i++) {
                const Pending &g = pending[(size_t)bwho[cls][i]];
                const ProfileGeneBaseRec &b = brecs[cls][i];
                ProfileGeneResult &o = res[(size_t)g.slot];
                if (!std::isfinite(b.F_hat) || !std::isfinite(b.X_hat)) return numeric();
                o.gene_hat = b.X_hat;
                if (!b.converged) o.capped = true;
                double raw = INFINITY;                          // essential: decided before the launch, or by the drop's epilogue
                if (b.X_hat == 0.0) raw = 0.0;                  // absent: the baseline IS the maximum under X = 0, as the presence test has it
                else if (!g.own_reads && b.infeasible == 0) {
                    raw = 2.0 * (b.F_hat - b.F_drop);
                    if (!(raw == raw)) return numeric();
                    if (raw < st.min_raw_lambda) st.min_raw_lambda = raw;
                }
                profile_gene_presence(raw, Q.q, o);
                for (int side = o.status == PROF_TWO_SIDED ? 0 : 1; side < 2; side++) {
                    items[cls].push_back(ProfileGeneItem{g.part_off, g.n_parts, g.closed_off, g.n_closed, genes[(size_t)g.slot], side,
                                                         side == 1 ? g.end : 0, 0, g.mn, g.mn0, b.X_hat, b.F_hat});
                    who[cls].push_back(g.slot);
                }
            }
        HIPCHK(set_class_lds_attributes(kProfileGeneSets));
        rc = runner.run(items, recs, st.search_ms, st.items_launched,
            [&](int c, const ProfileGeneItem &it) {
                return slices_ok(c, it.part_off, it.n_parts, it.closed_off, it.n_closed, it.gene, it.mn) && (it.side == 0 || it.side == 1) &&
                       (it.end == 0 || (it.side == 1 && it.mn0 > 0.0 && it.mn0 == it.mn));
            },
            [&](int c, int threads, hipStream_t s, size_t cnt, const ProfileGeneItem *d_items, ProfileRec *d_rec) {
                hipLaunchKernelGGL(kProfileGeneSets[c], dim3((unsigned)cnt), dim3(threads), lds[c], s, d_items, lists.d_parts.get(), lists.d_closed.get(),
                                   G, gene_of, d_rec, P, Q);
            });
        if (rc) return rc;
        for (int cls = 0; cls < emsar::kSetClasses; cls++)
            for (size_t i = 0; i < recs[cls].size(); i++) {
                add_search_stats(st, recs[cls][i]);
                profile_gene_take(recs[cls][i], items[cls][i].side, res[(size_t)who[cls][i]]);
            }
        return EMSAR_HIP_OK;
    }

    int copy_out() {
        for (ProfileGeneResult &o : res) {
            if (o.capped) o.status = PROF_UNCONVERGED;       // never set on a gene that was not searched
            st.n_status[o.status]++;
        }
        for (int32_t i = 0; i < nq; i++) {
            const ProfileGeneResult &o = res[(size_t)slot_of_gene[(size_t)(query ? query[i] : i)]];
            if (out.lower) out.lower[i] = o.lower;
            if (out.upper) out.upper[i] = o.upper;
            if (out.dev_lower) out.dev_lower[i] = o.dev_lower;
            if (out.dev_upper) out.dev_upper[i] = o.dev_upper;
            if (out.lambda) out.lambda[i] = o.lambda;
            if (out.pvalue) out.pvalue[i] = gene_presence_pvalue(o.lambda, o.members);
            if (out.gene_hat) out.gene_hat[i] = o.gene_hat;
            if (out.status) out.status[i] = o.status;
            if (out.evals) out.evals[i] = o.evals;
            if (out.parts) out.parts[i] = o.parts;
            if (out.members) out.members[i] = o.members;
        }
        return EMSAR_HIP_OK;
    }

    int run() {
        list_members(ctx->genes, nq, query);
        SetQuery q(ctx, p, (int32_t)member_tids.size(), member_tids.data());
        int rc;
        if ((rc = q.plan()) || (rc = q.classify()) || (rc = group(q)) || (rc = solve_search_reduce(q))) return rc;
        return copy_out();
    }
};

}  // namespace

extern "C" {

int emsar_hip_profile_genes(emsar_hip_ctx *ctx, const emsar_em_params *p, const emsar_profile_params *pp, int32_t n_query, const int32_t *query_genes,
                            const emsar_profile_gene_outputs *out, emsar_profile_gene_stats *stats) {
    if (!ctx) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample || !ctx->genes.have_genes) return EMSAR_HIP_ERR_STATE;      // first: a state error whatever the other arguments say
    if (const int rc = gene_query_ok(ctx, n_query, query_genes)) return rc;
    const emsar_profile_params prm = pp ? *pp : emsar_profile_params{0.95, 0.0, 0, 0};
    if (!profile_params_ok(prm)) return EMSAR_HIP_ERR_ARG;
    return run_query_call<ProfileGenesRun>(ctx, stats, p, prm, n_query, query_genes, out);
}

int emsar_hip_gene_presence_pvalue_host(int64_t n, const double *lambda, const int32_t *members, double *p_out) {
    if (n < 0 || (n > 0 && (!lambda || !members || !p_out))) return EMSAR_HIP_ERR_ARG;
    for (int64_t i = 0; i < n; i++) p_out[i] = gene_presence_pvalue(lambda[i], members[i]);
    return EMSAR_HIP_OK;
}

// Diagnostic only (not declared in the public header; needs no device): what emsar_hip_profile_genes gives a gene whose parts are all
// closed form -- n one-transcript components, u[i] reads and den[i] each --: what the host computes for such genes.
// values[8]: lower, upper, dev_lower, dev_upper, lambda, pvalue, gene_hat, and the evaluations of the upper search alone.
int emsar_hip_debug_profile_genes_closed(int32_t n, const double *u, const double *den, const emsar_profile_params *pp, double *values, int32_t *status,
                                         int32_t *evals) {
    const emsar_profile_params prm = pp ? *pp : emsar_profile_params{0.95, 0.0, 0, 0};
    if (!values || !status || !evals || n < 1 || !u || !den || !profile_params_ok(prm)) return EMSAR_HIP_ERR_ARG;
    try {
        GeneSideParts s;
        for (int32_t i = 0; i < n; i++) {
            if (!(u[i] >= 0.0) || !(den[i] > 0.0) || !std::isfinite(u[i]) || !std::isfinite(den[i])) return EMSAR_HIP_ERR_ARG;
            s.closed.push_back(CompareGeneClosed{u[i], den[i]});
            s.min_den = std::min(s.min_den, den[i]);
            if (u[i] > 0.0) { s.min_den_live = std::min(s.min_den_live, den[i]); s.own_reads = true; }
            s.members++;
        }
        ProfileGeneResult o;
        o.parts = o.members = s.members;
        if (!profile_gene_closed(s, profile_search_params(prm), o)) return EMSAR_HIP_ERR_NUMERIC;
        if (o.capped) o.status = PROF_UNCONVERGED;
        const double v[8] = {o.lower, o.upper, o.dev_lower, o.dev_upper, o.lambda, gene_presence_pvalue(o.lambda, o.members), o.gene_hat,
                             (double)o.evals_upper};
        for (int i = 0; i < 8; i++) values[i] = v[i];
        *status = o.status; *evals = o.evals;
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    return EMSAR_HIP_OK;
}

}  // extern "C"
