// compare_groups.hpp -- the K-sample test across replicate groups behind include/emsar_hip.h: emsar_hip_compare_groups (device) and
// emsar_hip_compare_groups_pvalue_host (no HIP call).  Part of emsar_hip.hip's translation unit, included after profile_genes.hpp
// (gene_presence_pvalue): every sample's queried transcripts are located as the presence test's are (SetQuery, set_items.hpp),
// k_compare_groups_sets (kernels_compare_groups.hpp) runs the searches.
// One call = one GroupsRun:  plan, classify   SetQuery's stages on the same query, once per context
//                            place            per transcript: outside / not resident / closed form in every sample (searched on the host) /
//                                             one item for all samples and one per group of two or more (a single group IS all samples:
//                                             one item), each in the launch class of the largest set among its samples; the locator
//                                             table [transcript][K] and the sample table [K] go to the device
//                            search           the items in batches across the three launch classes (SetItemRunner)
//                            reduce           records -> the two Lambdas, p, the common values, status;  copy_out in query order
// One workgroup runs one two-level search.  No context's theta, weights or scales are touched.  The launches run on the first context's
// streams; the others' streams are drained before.

namespace {

enum GroupsStatus : int32_t {
    GRP_TESTED = EMSAR_GROUPS_TESTED, GRP_ALL_ABSENT = EMSAR_GROUPS_ALL_ABSENT, GRP_OUTSIDE = EMSAR_GROUPS_OUTSIDE,
    GRP_NOT_RESIDENT = EMSAR_GROUPS_NOT_RESIDENT, GRP_UNCONVERGED = EMSAR_GROUPS_UNCONVERGED
};
constexpr int kGroupsMax = EMSAR_COMPARE_GROUPS_MAX;
static_assert(kGroupsMax == 32, "a sample mask is one 32-bit word");

inline GroupSearchParams groups_search_params(const emsar_groups_params &gp) {
    return GroupSearchParams{gp.dev_tol > 0.0 ? gp.dev_tol : 1e-4, gp.max_evals > 0 ? gp.max_evals : 40, gp.max_outer > 0 ? gp.max_outer : 12};
}
// P(chi2_df > lambda); df 0 is the point mass at 0
inline double groups_pvalue(double lambda, int32_t df) {
    if (df == 0) return lambda != lambda ? lambda : lambda > 0.0 ? 0.0 : 1.0;
    return gene_presence_pvalue(lambda, df);
}

// The groups of a call: the samples of each as a mask, in group order
struct GroupsLayout {
    int K = 0, G = 0;
    uint32_t all = 0;
    std::vector<uint32_t> mask;          // [G]
    std::vector<double> size;            // [K]
    // false: an id outside 0 .. G-1 (G = the largest id + 1), an empty group, or a size that is not finite and positive
    bool set(int K_, const int32_t *group_of, const double *size_) {
        K = K_; G = 0;
        for (int k = 0; k < K; k++) { if (group_of[k] < 0 || group_of[k] >= K) return false; G = std::max(G, group_of[k] + 1); }
        mask.assign((size_t)G, 0u); size.assign((size_t)K, 1.0);
        for (int k = 0; k < K; k++) mask[(size_t)group_of[k]] |= 1u << k;
        for (uint32_t m : mask) if (!m) return false;
        if (size_) for (int k = 0; k < K; k++) { if (!std::isfinite(size_[k]) || !(size_[k] > 0.0)) return false; size[(size_t)k] = size_[k]; }
        all = K == 32 ? 0xffffffffu : (1u << K) - 1u;
        return true;
    }
    static int count(uint32_t m) { return __builtin_popcount(m); }
    static int lowest(uint32_t m) { return __builtin_ctz(m); }
};

// what one queried transcript is given, next to its rows of theta_group [G] and theta_hat [K]
struct GroupsResult {
    double lambda_between = NAN, raw_between = NAN, lambda_within = NAN, raw_within = NAN, theta_common = NAN, slope = NAN;
    int32_t outer = 0, evals = 0, status = GRP_NOT_RESIDENT;
};

// The records of a transcript's items -> its numbers.  all: the all-samples item; group[g]: group g's item, null for a group of one
// sample (its C is that sample's F_hat) -- with one group, group[0] is `all` itself.  theta_hat, F_hat [K]: what the all-samples item
// left at lambda = 0.  With deficit(S) = sum_{k in S} F_hat^k - C(S) -- exactly 0 for an item that ended at outer point 0, every sum in
// ascending sample order -- Lambda_within = 2 sum_g deficit(S_g) and Lambda_between = 2 (deficit(all) - sum_g deficit(S_g)).
// false for a non-finite F at lambda = 0.
inline bool groups_reduce(const GroupsLayout &L, const GroupRec &all, const GroupRec *const *group, const double *theta_hat, const double *F_hat,
                          GroupsResult &o, double *theta_group) {
    bool absent = true;
    for (int k = 0; k < L.K; k++) { if (!std::isfinite(F_hat[k])) return false; absent = absent && theta_hat[k] == 0.0; }
    const auto deficit = [](const GroupRec &r) { return r.outer == 1 ? 0.0 : r.F0 - r.best; };
    const int ok = GROUP_REC_OUTER_OK | GROUP_REC_SOLVES_OK | GROUP_REC_INNER_OK;
    bool conv = all.flags == ok;
    double within = 0.0;
    o.evals = all.evals;
    for (int g = 0; g < L.G; g++) {
        const GroupRec *r = group[g];
        if (!r) { const int k = GroupsLayout::lowest(L.mask[(size_t)g]); theta_group[g] = theta_hat[k] / L.size[(size_t)k]; continue; }
        within += deficit(*r);
        theta_group[g] = r->best_x;
        if (r != &all) { o.evals += r->evals; conv = conv && r->flags == ok; }
    }
    o.raw_within = 2.0 * within;
    o.raw_between = L.G == 1 ? 0.0 : 2.0 * (deficit(all) - within);
    o.lambda_within = o.raw_within > 0.0 ? o.raw_within : 0.0;          // a NaN raw value: 0, with UNCONVERGED below
    o.lambda_between = o.raw_between > 0.0 ? o.raw_between : 0.0;
    o.theta_common = all.best_x; o.slope = all.slope; o.outer = all.outer;
    o.status = absent ? GRP_ALL_ABSENT : conv ? GRP_TESTED : GRP_UNCONVERGED;
    return true;
}

// Every search of one transcript or gene on the host, and their reduction: the all-samples search and one per group of two or more,
// each on a copy of E0 -- samples that keep th[k], Fh[k] of point 0 (put_hat) and evaluate without the device
template <class Samples>
inline bool groups_host_searches(const GroupsLayout &L, const Samples &E0, const GroupSearchParams &Q, GroupsResult &o, double *theta_group,
                                 double *theta_hat) {
    Samples E = E0;
    const GroupRec all = groups_search(L.K, L.all, Q, E).record(0, 1, 0);
    double F_hat[kGroupsMax];
    for (int k = 0; k < L.K; k++) { theta_hat[k] = E.th[k]; F_hat[k] = E.Fh[k]; }
    std::vector<GroupRec> recs((size_t)L.G);
    std::vector<const GroupRec *> group((size_t)L.G, nullptr);
    for (int g = 0; g < L.G; g++) {
        if (L.mask[(size_t)g] == L.all) { group[(size_t)g] = &all; continue; }
        if (GroupsLayout::count(L.mask[(size_t)g]) < 2) continue;
        Samples Eg = E0;
        recs[(size_t)g] = groups_search(L.K, L.mask[(size_t)g], Q, Eg).record(0, 1, 0);
        group[(size_t)g] = &recs[(size_t)g];
    }
    return groups_reduce(L, all, group.data(), theta_hat, F_hat, o, theta_group);
}

// K one-transcript components as groups_search's samples: compare_closed_form as the evaluation
struct GroupClosedSamples {
    const double *u, *den_, *size_;
    double th[kGroupsMax], Fh[kGroupsMax];
    double size(int k) const { return size_[k]; }
    double den(int k) const { return den_[k]; }
    double hat(int k) const { return th[k]; }
    void put_hat(int k, double x, double F) { th[k] = x; Fh[k] = F; }
    void eval(int k, double scale, double /* lambda */, double &x, double &F) const { compare_closed_form(u[k], den_[k], scale, x, F); }
};
// The searches of k_compare_groups_sets on a transcript that is a one-transcript component in every sample (u[k] reads, den[k]), and
// their reduction: what the host does for such transcripts
inline bool groups_closed_transcript(const GroupsLayout &L, const double *u, const double *den, const GroupSearchParams &Q, GroupsResult &o,
                                     double *theta_group, double *theta_hat) {
    return groups_host_searches(L, GroupClosedSamples{u, den, L.size.data(), {}, {}}, Q, o, theta_group, theta_hat);
}

struct GroupsRun {
    using Result = GroupsResult;
    emsar_hip_ctx *const ctx;            // the first sample's: its streams and events carry the launches
    emsar_hip_ctx *const *const ctxs;    // [K]
    GroupsLayout L;
    std::vector<std::unique_ptr<SetQuery>> q;      // [K] where every queried transcript stands in each sample
    const emsar_groups_outputs out;      // a copy: all NULL when the caller gave none
    const GroupSearchParams Q;
    std::vector<Result> res;             // per queried transcript (SetQuery::cand of every sample, same index)
    std::vector<double> res_group, res_hat;        // [cand][G], [cand][K]
    SetItemRunner<GroupItem, GroupRec> runner;
    emsar_groups_stats st{};

    GroupsRun(emsar_hip_ctx *c0, emsar_hip_ctx *const *cs, const GroupsLayout &lay, const emsar_em_params *p, const emsar_groups_params &gp,
              int32_t nq, const int32_t *query, const emsar_groups_outputs *o)
        : ctx(c0), ctxs(cs), L(lay), out(o ? *o : emsar_groups_outputs{}), Q(groups_search_params(gp)),
          runner(c0, "EMSAR_HIP_GROUPS_BATCH", "compare_groups: an item lies outside its class's sets") {
        for (int k = 0; k < L.K; k++) q.emplace_back(new SetQuery(cs[k], p, nq, query));
        st.df_between = L.G - 1; st.df_within = L.K - L.G;
    }

    int fail_numeric() { ctx->err = "compare_groups: non-finite likelihood at lambda = 0"; return EMSAR_HIP_ERR_NUMERIC; }
    void note_raw(const Result &o) {
        if (o.raw_between < st.min_raw_lambda) st.min_raw_lambda = o.raw_between;
        if (o.raw_within < st.min_raw_lambda) st.min_raw_lambda = o.raw_within;
    }

    int place_search_reduce() {
        const int K = L.K, G = L.G;
        const size_t n_cand = q[0]->cand.size();
        res.resize(n_cand);
        res_group.assign(n_cand * (size_t)G, NAN); res_hat.assign(n_cand * (size_t)K, NAN);
        std::vector<GroupLoc> locs(n_cand * (size_t)K, GroupLoc{-1, 0, 0, 0, 0.0, 0.0});
        std::vector<GroupItem> items[emsar::kSetClasses];
        std::vector<GroupRec> recs[emsar::kSetClasses];
        struct Where { int32_t cls = -1, idx = -1; };
        std::vector<Where> where(n_cand * (size_t)(G + 1));    // [cand][0] the all-samples item, [cand][1 + g] group g's
        std::vector<int32_t> row_of(n_cand, -1);
        int32_t n_rows = 0;
        for (size_t i = 0; i < n_cand; i++) {
            Result &o = res[i];
            bool outside = false, away = false, closed = true;
            for (int k = 0; k < K; k++) {
                const SetQuery::Cand &c = q[(size_t)k]->cand[i];
                away = away || c.standing == SetQuery::NOT_RESIDENT;
                outside = outside || c.standing == SetQuery::OUTSIDE;
                closed = closed && c.standing == SetQuery::CLOSED;
            }
            if (away) { o.status = GRP_NOT_RESIDENT; continue; }
            if (outside) { o.status = GRP_OUTSIDE; continue; }
            GroupLoc *row = &locs[i * (size_t)K];
            for (int k = 0; k < K; k++) {
                const SetQuery::Cand &c = q[(size_t)k]->cand[i];
                row[k] = GroupLoc{c.set, c.set < 0 ? 0 : c.loc, c.set < 0 ? 0 : c.cls, 0, c.u, q[(size_t)k]->h_den[(size_t)c.lib]};
            }
            if (closed) {
                double u[kGroupsMax], den[kGroupsMax];
                for (int k = 0; k < K; k++) { u[k] = row[k].u; den[k] = row[k].den; }
                if (!groups_closed_transcript(L, u, den, Q, o, &res_group[i * (size_t)G], &res_hat[i * (size_t)K])) return fail_numeric();
                note_raw(o);
                continue;
            }
            const auto add = [&](uint32_t mask, int32_t row_id, Where &w) {
                int cls = -1;
                for (int k = 0; k < K; k++) if ((mask >> k) & 1u) cls = std::max(cls, row[k].set < 0 ? -1 : row[k].cls);
                if (cls < 0) cls = 0;                                            // every sample of the subset closed form: the smallest launch
                w.cls = cls; w.idx = (int32_t)items[cls].size();
                items[cls].push_back(GroupItem{(int32_t)i, row_id, mask, 0});
            };
            row_of[i] = n_rows++;
            add(L.all, row_of[i], where[i * (size_t)(G + 1)]);
            for (int g = 0; g < G; g++)
                if (L.mask[(size_t)g] != L.all && GroupsLayout::count(L.mask[(size_t)g]) >= 2) add(L.mask[(size_t)g], -1, where[i * (size_t)(G + 1) + 1 + (size_t)g]);
        }
        std::vector<double> h_theta((size_t)n_rows * (size_t)K), h_F((size_t)n_rows * (size_t)K);
        if (n_rows > 0) {
            std::vector<GroupSample> samples((size_t)K);
            for (int k = 0; k < K; k++) samples[(size_t)k] = GroupSample{side_of(ctxs[k]), L.size[(size_t)k]};
            DevBuf<GroupSample> d_samples;
            DevBuf<GroupLoc> d_locs;
            DevBuf<double> d_theta, d_F;
            HIPCHK(d_samples.upload(samples.data(), samples.size()));
            HIPCHK(d_locs.upload(locs.data(), locs.size()));
            HIPCHK(d_theta.alloc(h_theta.size())); HIPCHK(d_F.alloc(h_F.size()));
            // the LDS of a launch class: the largest set of that class or a smaller one in any sample, then theta_hat^k, K doubles
            size_t lds[emsar::kSetClasses];
            launch_class_lds(lds, ctxs[0]);
            for (int k = 1; k < K; k++) {
                size_t l[emsar::kSetClasses];
                launch_class_lds(l, ctxs[k]);
                for (int c = 0; c < emsar::kSetClasses; c++) lds[c] = std::max(lds[c], l[c]);
            }
            int lds_limit = 0;
            HIPCHK(hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
            uint32_t hat_off[emsar::kSetClasses];
            for (int c = 0; c < emsar::kSetClasses; c++) {
                hat_off[c] = (uint32_t)((lds[c] + 7) / 8 * 8);
                lds[c] = hat_off[c] + (size_t)K * sizeof(double);
                if (!items[c].empty() && lds[c] > (size_t)lds_limit) { ctx->err = "compare_groups: a launch needs more LDS than the device has"; return EMSAR_HIP_ERR_HIP; }
                HIPCHK(hipFuncSetAttribute((const void *)kCompareGroupsSets[c], hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(emsar::kSetLdsCap[c] + 8 + kGroupsMax * sizeof(double))));
            }
            const SetSolveParams P = set_params(q[0]->p);
            const int rc = runner.run(items, recs, st.device_ms, st.items_launched,
                [&](int c, const GroupItem &it) {
                    if (it.q < 0 || (size_t)it.q >= n_cand || it.row < -1 || it.row >= n_rows || (it.mask & ~L.all) || GroupsLayout::count(it.mask) < 2) return false;
                    int cls = -1;
                    for (int k = 0; k < K; k++) {
                        if (!((it.mask >> k) & 1u)) continue;
                        const GroupLoc &l = locs[(size_t)it.q * (size_t)K + (size_t)k];
                        if (!CompareRun::side_ok(ctxs[k], c, l.cls, l.set, l.t, l.den)) return false;
                        cls = std::max(cls, l.set < 0 ? -1 : l.cls);
                    }
                    return std::max(cls, 0) == c;
                },
                [&](int c, int threads, hipStream_t s, size_t cnt, const GroupItem *d_items, GroupRec *d_rec) {
                    hipLaunchKernelGGL(kCompareGroupsSets[c], dim3((unsigned)cnt), dim3(threads), lds[c], s, d_items, d_samples.get(), d_locs.get(),
                                       d_theta.get(), d_F.get(), d_rec, K, hat_off[c], P, Q);
                });
            if (rc) return rc;
            HIPCHK(hipMemcpy(h_theta.data(), d_theta, h_theta.size() * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(h_F.data(), d_F, h_F.size() * sizeof(double), hipMemcpyDeviceToHost));
        }
        for (int cls = 0; cls < emsar::kSetClasses; cls++)
            for (const GroupRec &r : recs[cls]) {
                add_search_stats(st, r);
                st.outer_sum += r.outer; st.outer_max = std::max(st.outer_max, r.outer);
            }
        std::vector<const GroupRec *> group((size_t)G);
        for (size_t i = 0; i < n_cand; i++) {
            if (row_of[i] < 0) continue;
            const Where *w = &where[i * (size_t)(G + 1)];
            const GroupRec &all = recs[w[0].cls][(size_t)w[0].idx];
            for (int g = 0; g < G; g++)
                group[(size_t)g] = L.mask[(size_t)g] == L.all ? &all : w[1 + g].cls < 0 ? nullptr : &recs[w[1 + g].cls][(size_t)w[1 + g].idx];
            const double *th = &h_theta[(size_t)row_of[i] * (size_t)K], *Fh = &h_F[(size_t)row_of[i] * (size_t)K];
            if (!groups_reduce(L, all, group.data(), th, Fh, res[i], &res_group[i * (size_t)G])) return fail_numeric();
            std::copy(th, th + K, &res_hat[i * (size_t)K]);
            note_raw(res[i]);
        }
        return EMSAR_HIP_OK;
    }

    int copy_out() {
        const SetQuery &q0 = *q[0];
        const size_t K = (size_t)L.K, G = (size_t)L.G;
        for (const Result &o : res) st.n_status[o.status]++;
        for (int32_t i = 0; i < q0.nq; i++) {
            const size_t c = q0.cand_index(i);
            const Result &o = res[c];
            if (out.lambda_between) out.lambda_between[i] = o.lambda_between;
            if (out.p_between) out.p_between[i] = groups_pvalue(o.lambda_between, st.df_between);
            if (out.lambda_within) out.lambda_within[i] = o.lambda_within;
            if (out.p_within) out.p_within[i] = groups_pvalue(o.lambda_within, st.df_within);
            if (out.raw_between) out.raw_between[i] = o.raw_between;
            if (out.raw_within) out.raw_within[i] = o.raw_within;
            if (out.theta_common) out.theta_common[i] = o.theta_common;
            if (out.slope) out.slope[i] = o.slope;
            if (out.theta_group) std::copy(&res_group[c * G], &res_group[c * G] + G, out.theta_group + (size_t)i * G);
            if (out.theta_hat) std::copy(&res_hat[c * K], &res_hat[c * K] + K, out.theta_hat + (size_t)i * K);
            if (out.status) out.status[i] = o.status;
            if (out.outer) out.outer[i] = o.outer;
            if (out.evals) out.evals[i] = o.evals;
        }
        return EMSAR_HIP_OK;
    }

    int run() {
        for (int k = 0; k < L.K; k++) {
            int rc;
            if ((rc = q[(size_t)k]->plan()) || (rc = q[(size_t)k]->classify())) { if (k) ctx->err = ctxs[k]->err; return rc; }
        }
        if (const int rc = place_search_reduce()) return rc;
        return copy_out();
    }
};

// the launches run on the first context's streams: another context's own stream is drained before
inline int drain_stream(emsar_hip_ctx *ctx) {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return EMSAR_HIP_OK;
}
inline emsar_groups_params groups_params_or_default(const emsar_groups_params *gp) { return gp ? *gp : emsar_groups_params{0.0, 0, 0}; }

}  // namespace

extern "C" {

int emsar_hip_compare_groups(emsar_hip_ctx *const *ctxs, int32_t n_samples, const int32_t *group_of, const double *size, const emsar_em_params *p,
                             const emsar_groups_params *gp, int32_t n_query, const int32_t *query_tids, const emsar_groups_outputs *out,
                             emsar_groups_stats *stats) {
    if (!ctxs || n_samples < 2 || n_samples > kGroupsMax || !group_of) return EMSAR_HIP_ERR_ARG;
    for (int k = 0; k < n_samples; k++) {
        if (!ctxs[k]) return EMSAR_HIP_ERR_ARG;
        for (int j = 0; j < k; j++) if (ctxs[j] == ctxs[k]) return EMSAR_HIP_ERR_ARG;
    }
    for (int k = 0; k < n_samples; k++) if (!ctxs[k]->have_sample) return EMSAR_HIP_ERR_STATE;
    for (int k = 1; k < n_samples; k++) if (ctxs[k]->device != ctxs[0]->device || !same_structure(ctxs[0], ctxs[k])) return EMSAR_HIP_ERR_ARG;
    if (const int rc = query_ok(ctxs[0], n_query, query_tids)) return rc;
    const emsar_groups_params prm = groups_params_or_default(gp);
    if (!std::isfinite(prm.dev_tol)) return EMSAR_HIP_ERR_ARG;
    try {
        GroupsLayout L;
        if (!L.set(n_samples, group_of, size)) return EMSAR_HIP_ERR_ARG;
        for (int k = 1; k < n_samples; k++) if (const int rc = drain_stream(ctxs[k])) return rc;
        return run_query_call<GroupsRun>(ctxs[0], stats, ctxs, L, p, prm, n_query, query_tids, out);
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
}

// Diagnostic only (not declared in the public header; makes no HIP call): what emsar_hip_compare_groups gives a transcript that is a
// one-transcript component in each of the K samples (u[k] reads, den[k]) -- the searches the host runs for such transcripts.
// values[8]: lambda_between, p_between, lambda_within, p_within, raw_between, raw_within, theta_common, slope.  theta_group[G],
// theta_hat[K].  counts[3]: status, outer, evals.
int emsar_hip_debug_compare_groups_closed(int32_t n_samples, const double *u, const double *den, const int32_t *group_of, const double *size,
                                          const emsar_groups_params *gp, double *values, double *theta_group, double *theta_hat, int32_t *counts) {
    if (n_samples < 2 || n_samples > kGroupsMax || !u || !den || !group_of || !values || !theta_group || !theta_hat || !counts) return EMSAR_HIP_ERR_ARG;
    const emsar_groups_params prm = groups_params_or_default(gp);
    if (!std::isfinite(prm.dev_tol)) return EMSAR_HIP_ERR_ARG;
    for (int k = 0; k < n_samples; k++) if (!(u[k] >= 0.0) || !(den[k] > 0.0)) return EMSAR_HIP_ERR_ARG;
    try {
        GroupsLayout L;
        if (!L.set(n_samples, group_of, size)) return EMSAR_HIP_ERR_ARG;
        GroupsResult o;
        if (!groups_closed_transcript(L, u, den, groups_search_params(prm), o, theta_group, theta_hat)) return EMSAR_HIP_ERR_NUMERIC;
        const double v[8] = {o.lambda_between, groups_pvalue(o.lambda_between, L.G - 1), o.lambda_within, groups_pvalue(o.lambda_within, L.K - L.G),
                             o.raw_between, o.raw_within, o.theta_common, o.slope};
        for (int i = 0; i < 8; i++) values[i] = v[i];
        counts[0] = o.status; counts[1] = o.outer; counts[2] = o.evals;
    } catch (const std::bad_alloc &) { return EMSAR_HIP_ERR_OOM; }
    return EMSAR_HIP_OK;
}

int emsar_hip_compare_groups_pvalue_host(int64_t n, const double *lambda, const int32_t *df, double *p_out) {
    if (n < 0 || (n > 0 && (!lambda || !df || !p_out))) return EMSAR_HIP_ERR_ARG;
    for (int64_t i = 0; i < n; i++) p_out[i] = groups_pvalue(lambda[i], df[i]);
    return EMSAR_HIP_OK;
}

}  // extern "C"
