// profile_usage.hpp -- the profile-likelihood intervals of isoform usage behind include/emsar_hip.h: emsar_hip_profile_usage.  Part of
// emsar_hip.hip's translation unit, included after compare_usage.hpp and profile_genes.hpp: the members of the queried transcripts'
// genes are located and grouped into parts as the two-sample test of usage does (SetQuery; GeneQueryMembers, GenePartLists:
// gene_parts.hpp), k_profile_usage_base and k_profile_usage_sets (kernels_profile_usage.hpp) do the solves.
// One call = one ProfileUsageRun:  plan, classify   SetQuery's stages on the union of the members of the queried transcripts' genes
//                                  group            per gene: its parts, once however many of its transcripts are asked for; per
//                                                   distinct (gene, t): the host-only statuses, t's place, the smallest den of the
//                                                   others, the drops the host decides; a gene whose parts are all closed form is
//                                                   finished on the host (profile_usage_closed)
//                                  baseline         one item per remaining (gene, t): theta_hat_t, X_hat, F_hat, the two drops ->
//                                                   usage, lambda_zero, lambda_one, the limits that need no search
//                                  search           one item per limit to find, in batches across the three launch classes
//                                  reduce           records -> limits, deviances, status;  copy_out in query order
// The context's theta, weights and scales are not touched.

namespace {

enum ProfileUsageStatus : int32_t {
    UPROF_UPPER_ONE = EMSAR_UPROFILE_UPPER_ONE, UPROF_UNIT = EMSAR_UPROFILE_UNIT, UPROF_UNDEFINED = EMSAR_UPROFILE_UNDEFINED,
    UPROF_SINGLE = EMSAR_UPROFILE_SINGLE
};

inline ProfileUsageSearchParams profile_usage_search_params(const emsar_profile_params &pp) {
    return ProfileUsageSearchParams{profile_cut(pp.level), pp.dev_tol > 0.0 ? pp.dev_tol : 1e-4, pp.max_evals > 0 ? pp.max_evals : 40,
                                    pp.max_outer > 0 ? pp.max_outer : 24};
}

// what one queried transcript is given
struct ProfileUsageResult {
    double usage = NAN, lower = NAN, upper = NAN, dev_lower = NAN, dev_upper = NAN, lambda_zero = NAN, lambda_one = NAN;
    int32_t outer = 0, evals = 0, parts = 0, members = 0, status = PROF_NOT_RESIDENT;
    bool capped = false;                 // a search or a solve hit its cap
};

// The baseline and the raw deviances of the two ends (+inf: a dropped member is essential) -> usage, lambda_zero, lambda_one, the
// limits that need no search and the status so far; search[side] = that limit is to be found.  False for a non-finite baseline or raw
// value.  min_raw takes the most negative raw value.
inline bool profile_usage_ends(double t0, double X0, double F0, double raw_zero, double raw_one, double q, ProfileUsageResult &o, bool (&search)[2],
                               double &min_raw) {
    search[0] = search[1] = false;
    if (!std::isfinite(t0) || !std::isfinite(X0) || !std::isfinite(F0)) return false;
    if (!(X0 > 0.0)) { o.status = UPROF_UNDEFINED; return true; }
    o.usage = t0 / X0;
    if (o.usage == 0.0) raw_zero = 0.0;              // the baseline IS the maximum under theta_t = 0
    if (o.usage == 1.0) raw_one = 0.0;
    if (raw_zero != raw_zero || raw_one != raw_one) return false;
    if (raw_zero < min_raw) min_raw = raw_zero;
    if (raw_one < min_raw) min_raw = raw_one;
    o.lambda_zero = raw_zero > 0.0 ? raw_zero : 0.0;
    o.lambda_one = raw_one > 0.0 ? raw_one : 0.0;
    const bool zero = o.lambda_zero <= q, one = o.lambda_one <= q;
    if (zero) { o.lower = 0.0; o.dev_lower = o.lambda_zero; }
    if (one) { o.upper = 1.0; o.dev_upper = o.lambda_one; }
    search[0] = !zero; search[1] = !one;
    o.status = zero ? (one ? UPROF_UNIT : PROF_LOWER_ZERO) : (one ? UPROF_UPPER_ONE : PROF_TWO_SIDED);
    return true;
}

inline void profile_usage_take(const ProfileUsageRec &r, int side, ProfileUsageResult &o) {
    o.outer += r.outer; o.evals += r.evals;
    if (r.flags != (USAGE_REC_OUTER_OK | USAGE_REC_SOLVES_OK | USAGE_REC_INNER_OK)) o.capped = true;
    if (side == 0) { o.lower = r.u; o.dev_lower = r.dev; }
    else { o.upper = r.u; o.dev_upper = r.dev; }
}

// A (gene, t) whose gene's parts are all closed form (c[0 .. n), t at place tc): baseline, ends and both limits on the host, the
// search of k_profile_usage_sets with gene_closed_sum as its evaluation.  A closed-form member with reads is essential.
inline bool profile_usage_closed(const CompareGeneClosed *c, int n, int tc, double den_t, double mn, const ProfileUsageSearchParams &Q,
                                 ProfileUsageResult &o, double &min_raw) {
    GeneSums hat{0.0, 0.0, 0.0};
    gene_closed_sum(c, n, GenePoint{mn, 1.0, 0.0, tc, den_t}, hat);
    bool others_read = false, search[2];
    for (int k = 0; k < n; k++) if (k != tc && c[k].u > 0.0) others_read = true;
    if (!profile_usage_ends(hat.T, hat.X, hat.F, c[tc].u > 0.0 ? INFINITY : 0.0, others_read ? INFINITY : 0.0, Q.q, o, search, min_raw)) return false;
    for (int side = 0; side < 2; side++) {
        if (!search[side]) continue;
        const auto eval = [&](const UsagePoint &pt, GeneSums &S) { gene_closed_sum(c, n, GenePoint{mn, pt.scale, pt.shift, tc, pt.den_t}, S); };
        const ProfileUsageSearched R = profile_usage_search(side, hat.T, hat.X, hat.F, den_t, mn, side ? o.lambda_one : o.lambda_zero, Q, eval);
        profile_usage_take(R.record(GeneSolveCount()), side, o);
    }
    return true;
}

struct ProfileUsageRun : GeneQueryMembers {
    using Result = ProfileUsageResult;   // per distinct queried transcript
    // a (gene, t) that goes to the device: what its items share
    struct Pending { int32_t slot, cls, part_off, n_parts, closed_off, n_closed, gene, t, tc, skip; double den_t, mn; };
    emsar_hip_ctx *const ctx;
    const emsar_em_params *const p;
    const int32_t nq;
    const int32_t *const query;          // caller tids, null = all in order
    const emsar_profile_usage_outputs out;
    ProfileUsageSearchParams Q;
    std::vector<int32_t> tids;           // the queried transcripts, each once
    std::vector<int32_t> slot_of_tid;    // [n_tx] -> tids / res, -1 = not queried
    std::vector<Result> res;
    std::vector<Pending> pending;
    GenePartLists lists;
    SetItemRunner<ProfileUsageBaseItem, ProfileUsageBaseRec> base_runner;
    SetItemRunner<ProfileUsageItem, ProfileUsageRec> runner;
    emsar_profile_usage_stats st{};

    ProfileUsageRun(emsar_hip_ctx *c, const emsar_em_params *pp, const emsar_profile_params &prm, int32_t nq_, const int32_t *q,
                    const emsar_profile_usage_outputs *o)
        : ctx(c), p(pp), nq(nq_), query(q), out(o ? *o : emsar_profile_usage_outputs{}), Q(profile_usage_search_params(prm)),
          base_runner(c, "EMSAR_HIP_PROFILE_USAGE_BATCH", "profile_usage: a baseline item lies outside its class's sets"),
          runner(c, "EMSAR_HIP_PROFILE_USAGE_BATCH", "profile_usage: an item lies outside its class's sets") { st.cut = Q.q; }

    int32_t tid_of_query(int32_t i) const { return query ? query[i] : i; }
    int numeric() { ctx->err = "profile_usage: non-finite likelihood at the baseline"; return EMSAR_HIP_ERR_NUMERIC; }

    // t in gene slot k, t taking part: its place among the closed-form parts (-1: in a set part; the order is side_parts'), the
    // smallest den of the other members taking part (inf: none) and the drops the host decides
    void place_of(const SetQuery &q, size_t k, int32_t t, int32_t &tc, double &mn, int32_t &skip) const {
        tc = -1; mn = INFINITY; skip = 0;
        int32_t n_closed = 0;
        for (int64_t m = gp[k]; m < gp[k + 1]; m++) {
            const int32_t s = member_tids[(size_t)m];
            const SetQuery::Cand &c = q.cand[(size_t)q.cand_of_lib[(size_t)q.lib_of(s)]];
            if (c.standing == SetQuery::OUTSIDE || c.standing == SetQuery::NOT_RESIDENT) continue;
            const bool own = c.standing == SetQuery::CLOSED ? c.u > 0.0 : c.own_reads;
            if (s == t) { if (c.standing == SetQuery::CLOSED) tc = n_closed; }
            else mn = std::min(mn, q.h_den[(size_t)c.lib]);
            if (own) skip |= s == t ? PROFILE_USAGE_SKIP_T : PROFILE_USAGE_SKIP_OTHERS;
            if (c.standing == SetQuery::CLOSED) n_closed++;
        }
    }

    int group(const SetQuery &q) {
        res.resize(tids.size());
        const std::vector<int32_t> &of_tx = ctx->genes.h_gene_of_tx;
        struct GeneSide { GeneSideParts s; GenePartLists::Offsets at{-1, -1}; bool made = false; };
        std::vector<GeneSide> sides(genes.size());
        for (size_t i = 0; i < tids.size(); i++) {
            const int32_t t = tids[i], g = of_tx[(size_t)t];
            Result &o = res[i];
            if (g < 0) { o.status = PROF_OUTSIDE; continue; }
            if (!q.use_sets) { o.status = PROF_NOT_RESIDENT; continue; }
            const size_t k = (size_t)slot_of_gene[(size_t)g];
            GeneSide &G = sides[k];
            if (!G.made) { G.s = side_parts(q, k, 0); G.made = true; }
            const SetQuery::Cand &ct = q.cand[(size_t)q.cand_of_lib[(size_t)q.lib_of(t)]];
            if (ct.standing == SetQuery::OUTSIDE) { o.status = PROF_OUTSIDE; continue; }
            if (G.s.not_resident) { o.status = PROF_NOT_RESIDENT; continue; }
            if (G.s.members < 2) { o.status = UPROF_SINGLE; continue; }
            if (G.s.count() > kGeneMaxParts) { o.status = GPROF_TOO_LARGE; continue; }
            o.parts = G.s.count(); o.members = G.s.members;
            st.parts_max = std::max(st.parts_max, o.parts);
            int32_t tc, skip;
            double mn;
            place_of(q, k, t, tc, mn, skip);
            const double den_t = q.h_den[(size_t)ct.lib];
            if (G.s.sets.empty()) {
                if (!profile_usage_closed(G.s.closed.data(), (int)G.s.closed.size(), tc, den_t, mn, Q, o, st.min_raw_lambda)) return numeric();
                continue;
            }
            if (G.at.part_off < 0) G.at = lists.append(G.s);             // the gene's slices, once for all its transcripts
            Pending w;
            w.slot = (int32_t)i;
            w.part_off = G.at.part_off; w.n_parts = (int32_t)G.s.sets.size();
            w.closed_off = G.at.closed_off; w.n_closed = (int32_t)G.s.closed.size();
            w.cls = lists.launch_class(w.part_off, w.n_parts);
            w.gene = g; w.t = ct.lib; w.tc = tc; w.skip = skip; w.den_t = den_t; w.mn = mn;
            pending.push_back(w);
        }
        return EMSAR_HIP_OK;
    }

    // what the two item kinds share: den_t, mn, t, its place and the slices (GenePartLists::slice_ok)
    bool common_ok(int c, int32_t part_off, int32_t n_parts, int32_t closed_off, int32_t n_closed, int32_t gene, int32_t t, int32_t tc, double den_t,
                   double mn) const {
        return den_t > 0.0 && mn > 0.0 && t >= 0 && t < ctx->n_tx && tc >= -1 && tc < n_closed &&
               lists.slice_ok(c, part_off, closed_off, gene, {{ctx, n_parts, n_closed}});
    }

    int solve_search_reduce(const SetQuery &q) {
        if (pending.empty()) return EMSAR_HIP_OK;
        if (const int urc = lists.upload(ctx)) return urc;
        const SetSolveParams P = set_params(q.p);
        const CompareSide G = side_of(ctx);
        const int32_t *gene_of = ctx->genes.d_gene_of_lib;
        size_t lds[emsar::kSetClasses];
        launch_class_lds(lds, ctx);

        // baseline and drops
        std::vector<ProfileUsageBaseItem> bitems[emsar::kSetClasses];
        std::vector<ProfileUsageBaseRec> brecs[emsar::kSetClasses];
        std::vector<int32_t> bwho[emsar::kSetClasses];         // item -> pending
        for (size_t i = 0; i < pending.size(); i++) {
            const Pending &w = pending[i];
            bitems[w.cls].push_back(ProfileUsageBaseItem{w.part_off, w.n_parts, w.closed_off, w.n_closed, w.gene, w.t, w.tc, w.skip, w.den_t, w.mn});
            bwho[w.cls].push_back((int32_t)i);
        }
        HIPCHK(set_class_lds_attributes(kProfileUsageBase));
        int rc = base_runner.run(bitems, brecs, st.baseline_ms, st.items_launched,
            [&](int c, const ProfileUsageBaseItem &it) {
                return common_ok(c, it.part_off, it.n_parts, it.closed_off, it.n_closed, it.gene, it.t, it.tc, it.den_t, it.mn) && (it.skip & ~3) == 0;
            },
            [&](int c, int threads, hipStream_t s, size_t cnt, const ProfileUsageBaseItem *d_items, ProfileUsageBaseRec *d_rec) {
                hipLaunchKernelGGL(kProfileUsageBase[c], dim3((unsigned)cnt), dim3(threads), lds[c], s, d_items, lists.d_parts.get(), lists.d_closed.get(),
                                   G, gene_of, d_rec, P);
            });
        if (rc) return rc;

        // usage, the ends, and the limits to search
        std::vector<ProfileUsageItem> items[emsar::kSetClasses];
        std::vector<ProfileUsageRec> recs[emsar::kSetClasses];
        std::vector<int32_t> who[emsar::kSetClasses];          // item -> tids slot
        for (int cls = 0; cls < emsar::kSetClasses; cls++)
            for (size_t i = 0; i < brecs[cls].size(); i++) {
                const Pending &w = pending[(size_t)bwho[cls][i]];
                const ProfileUsageBaseRec &b = brecs[cls][i];
                Result &o = res[(size_t)w.slot];
                if (!b.converged) o.capped = true;
                // essential: decided before the launch, or by the drop's epilogue
                const double raw_zero = (w.skip & PROFILE_USAGE_SKIP_T) || b.infeasible_t ? INFINITY : 2.0 * (b.F0 - b.F_drop_t);
                const double raw_one = (w.skip & PROFILE_USAGE_SKIP_OTHERS) || b.infeasible_o ? INFINITY : 2.0 * (b.F0 - b.F_drop_o);
                bool search[2];
                if (!profile_usage_ends(b.t0, b.X0, b.F0, raw_zero, raw_one, Q.q, o, search, st.min_raw_lambda)) return numeric();
                for (int side = 0; side < 2; side++) {
                    if (!search[side]) continue;
                    items[cls].push_back(ProfileUsageItem{w.part_off, w.n_parts, w.closed_off, w.n_closed, w.gene, w.t, w.tc, side, w.den_t, w.mn,
                                                          b.t0, b.X0, b.F0, side ? o.lambda_one : o.lambda_zero});
                    who[cls].push_back(w.slot);
                }
            }
        HIPCHK(set_class_lds_attributes(kProfileUsageSets));
        rc = runner.run(items, recs, st.search_ms, st.items_launched,
            [&](int c, const ProfileUsageItem &it) {
                return common_ok(c, it.part_off, it.n_parts, it.closed_off, it.n_closed, it.gene, it.t, it.tc, it.den_t, it.mn) &&
                       (it.side == 0 || it.side == 1) && it.X0 > 0.0 && it.t0 >= 0.0 && it.D_end > Q.q;
            },
            [&](int c, int threads, hipStream_t s, size_t cnt, const ProfileUsageItem *d_items, ProfileUsageRec *d_rec) {
                hipLaunchKernelGGL(kProfileUsageSets[c], dim3((unsigned)cnt), dim3(threads), lds[c], s, d_items, lists.d_parts.get(), lists.d_closed.get(),
                                   G, gene_of, d_rec, P, Q);
            });
        if (rc) return rc;
        for (int cls = 0; cls < emsar::kSetClasses; cls++)
            for (size_t i = 0; i < recs[cls].size(); i++) {
                const ProfileUsageRec &r = recs[cls][i];
                add_search_stats(st, r);
                st.outer_sum += r.outer; st.outer_max = std::max(st.outer_max, r.outer);
                profile_usage_take(r, items[cls][i].side, res[(size_t)who[cls][i]]);
            }
        return EMSAR_HIP_OK;
    }

    int copy_out() {
        for (Result &o : res) {
            if (o.capped && o.status != UPROF_UNDEFINED) o.status = PROF_UNCONVERGED;       // UNDEFINED gives no values: it stays
            st.n_status[o.status]++;
        }
        for (int32_t i = 0; i < nq; i++) {
            const Result &o = res[(size_t)slot_of_tid[(size_t)tid_of_query(i)]];
            if (out.usage) out.usage[i] = o.usage;
            if (out.lower) out.lower[i] = o.lower;
            if (out.upper) out.upper[i] = o.upper;
            if (out.dev_lower) out.dev_lower[i] = o.dev_lower;
            if (out.dev_upper) out.dev_upper[i] = o.dev_upper;
            if (out.lambda_zero) out.lambda_zero[i] = o.lambda_zero;
            if (out.lambda_one) out.lambda_one[i] = o.lambda_one;
            if (out.status) out.status[i] = o.status;
            if (out.outer_evals) out.outer_evals[i] = o.outer;
            if (out.evals) out.evals[i] = o.evals;
            if (out.parts) out.parts[i] = o.parts;
            if (out.members) out.members[i] = o.members;
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
        SetQuery q(ctx, p, (int32_t)member_tids.size(), member_tids.data());
        int rc;
        if ((rc = q.plan()) || (rc = q.classify()) || (rc = group(q)) || (rc = solve_search_reduce(q))) return rc;
        return copy_out();
    }
};

}  // namespace

extern "C" {

int emsar_hip_profile_usage(emsar_hip_ctx *ctx, const emsar_em_params *p, const emsar_profile_params *pp, int32_t n_query, const int32_t *query_tids,
                            const emsar_profile_usage_outputs *out, emsar_profile_usage_stats *stats) {
    if (!ctx) return EMSAR_HIP_ERR_ARG;
    if (!ctx->have_sample || !ctx->genes.have_genes) return EMSAR_HIP_ERR_STATE;      // first: a state error whatever the other arguments say
    if (const int rc = query_ok(ctx, n_query, query_tids)) return rc;
    const emsar_profile_params prm = pp ? *pp : emsar_profile_params{0.95, 0.0, 0, 0};
    if (!profile_params_ok(prm)) return EMSAR_HIP_ERR_ARG;
    return run_query_call<ProfileUsageRun>(ctx, stats, p, prm, n_query, query_tids, out);
}

// Diagnostic only (not declared in the public header; makes no HIP call): what emsar_hip_profile_usage gives member t of a gene whose
// members are all one-transcript components -- n of them, u[i] reads and den[i] each; den 0 = takes no part --: the host's statuses
// and the searches the host runs for such genes.
// values[7]: usage, lower, upper, dev_lower, dev_upper, lambda_zero, lambda_one.  counts[5]: status, outer_evals, evals, parts, members.
int emsar_hip_debug_profile_usage_closed(int32_t n, const double *u, const double *den, int32_t t, const emsar_profile_params *pp, double *values,
                                         int32_t *counts) {
    const emsar_profile_params prm = pp ? *pp : emsar_profile_params{0.95, 0.0, 0, 0};
    if (!values || !counts || n < 1 || !u || !den || t < 0 || t >= n || !profile_params_ok(prm)) return EMSAR_HIP_ERR_ARG;
    try {
        std::vector<CompareGeneClosed> c;
        int32_t tc = -1;
        double mn = INFINITY;
        for (int32_t i = 0; i < n; i++) {
            if (!(u[i] >= 0.0) || !(den[i] >= 0.0) || !std::isfinite(u[i]) || !std::isfinite(den[i])) return EMSAR_HIP_ERR_ARG;
            if (!(den[i] > 0.0)) continue;
            if (i == t) tc = (int32_t)c.size(); else mn = std::min(mn, den[i]);
            c.push_back(CompareGeneClosed{u[i], den[i]});
        }
        ProfileUsageResult o;
        double min_raw = 0.0;
        if (tc < 0) o.status = PROF_OUTSIDE;
        else if (c.size() < 2) o.status = UPROF_SINGLE;
        else if (c.size() > kGeneMaxParts) o.status = GPROF_TOO_LARGE;
        else {
            o.parts = o.members = (int32_t)c.size();
            if (!profile_usage_closed(c.data(), (int)c.size(), tc, den[t], mn, profile_usage_search_params(prm), o, min_raw)) return EMSAR_HIP_ERR_NUMERIC;
            if (o.capped && o.status != UPROF_UNDEFINED) o.status = PROF_UNCONVERGED;
        }
        const double v[7] = {o.usage, o.lower, o.upper, o.dev_lower, o.dev_upper, o.lambda_zero, o.lambda_one};
        for (int i = 0; i < 7; i++) values[i] = v[i];
        counts[0] = o.status; counts[1] = o.outer; counts[2] = o.evals; counts[3] = o.parts; counts[4] = o.members;
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    return EMSAR_HIP_OK;
}

}  // extern "C"
